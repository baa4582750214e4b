"""Two fixed-seed slices of the randomised read-pathing sweep (tests/tools/fuzz_paths.py): random genomes with long homopolymers and
short-period repeats, read pairs of up to 256 bases with planted duplicate groups, random K / filters / pathing variant, every read's
path, every pair's duplicate flag and the per-unitig barcode lists against the C oracle; and on every case's paths the four other stages that
run after the pather -- the paths index, the compressed paths and their unzip, the edge -> barcode lists on both sort paths -- against
their numpy restatements (a48ref.paths_index, a48xref.zip_paths, ebcxref.edge_barcodes)."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("seed", [21, 22])
def test_path_fuzz_slice(snk, seed):
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "tools" / "fuzz_paths.py"), "12", str(seed)], capture_output=True, text=True, timeout=600)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, tail + "\n" + r.stderr[-2000:]
    assert "12 of 12 cases bit-exact" in r.stdout, tail
