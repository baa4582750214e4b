"""A fixed-seed slice of the randomised sweep of the path extension (tests/tools/fuzz_extend.py): random genomes with repeats, ragged
read pairs with errors, a device graph of drawn K and filters, the pather's own paths; snk_dev_extend_paths without and with
SNK_EXT_BACK against the Python restatement (tests/extref.py)."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_extend_fuzz_slice(snk):
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "tools" / "fuzz_extend.py"), "8", "31"], capture_output=True, text=True, timeout=300)
    tail = "\n".join(r.stdout.splitlines()[-12:])
    assert r.returncode == 0, tail + "\n" + r.stderr[-2000:]
    assert "8 of 8 cases bit-exact" in r.stdout, tail
