"""snk_dev_mow_lawn against the Python restatement (tests/mowref.py, pinned to the reference's MowLawn on tests/golden/mow/) on a hundred
seeds of tests/mowgen.py that no fixture holds: bubbles with tips, reads on both strands with substitutions, duplicates, filtered reads,
crowded tips.  dup is MarkDups as the project restates it."""
import numpy as np
import pytest

import mowgen
import mowref
from mowdev import Input

pytestmark = pytest.mark.gpu
SEEDS = tuple(range(1000, 1100))


def test_hundred_seeds(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    engine = Engine(0)
    total = dict.fromkeys(mowref.COUNTERS, 0)
    try:
        for seed in SEEDS:
            c = mowgen._from_hand(mowgen.fuzz(seed, 48 if seed % 4 else 60, n_motifs=6), None)
            dup = mowgen.dup_of(c)
            want_dels, want_scored, cnt = mowref.mow_entries(c.g, c.eb, c.inv, c.codes, c.lens, c.quals, *c.paths, dup)
            inp = Input(c)
            with inp.handle() as h:
                dels, scored, stats = engine.mow_lawn(inp.graph(h), *inp.reads(), inp.paths, dup)
            assert np.array_equal(dels, want_dels) and np.array_equal(scored, want_scored), seed
            assert {k: stats[k] for k in cnt} == cnt, (seed, stats)
            for k in cnt:
                total[k] += cnt[k]
    finally:
        engine.close()
    assert all(total[k] > 0 for k in total), total
