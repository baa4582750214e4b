"""CloseGap2 / CloseGap on the device (snk_dev_close_gaps) against the Python restatement (tests/closeref.py, pinned to the reference's
closures by test_closures_host.py and, on this distribution, by test_closures_fuzz_host.py) on the 160 seeded cases of tests/closegen.py:
both flags at max_width 400, CloseGap2 at a drawn width of 100, 150 or 1 200, with the paths index given and made inside, with every
placement on the host routine, at bod_budget 1 and at a budget drawn between the smallest and the largest 32-mer count a side of the
case's pairs has.  closure_off, bases and pair_first must be byte-equal and closeref.COUNTERS equal every time.

The budget: snk_dev_close_gaps hands a pair to the host routine when the larger of its two sides' 32-mer counts is ABOVE the budget
(`m > budget`, supernova_amd/csrc/snk_close.hip; include/snk.h: "a pair with a side over the budget"), so n_place_host must be the
number of pairs whose bod_max (closegen.expected) is greater than the budget, not greater or equal.

That the generation reaches every part of the stage, and that the expected answers move with every constant, is checked without a GPU
in test_closures_fuzz_host.py."""
import time

import numpy as np
import pytest

import closegen
import closeref

N_CASES, BLOCK = closegen.N_SEEDS, 20


def _engine():
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return Engine(0)


def _check(what, got, out, want, n_host=None):
    from test_gpu_closures import _counts, _equal
    assert _equal(got, want[:3]), (what, got[2].tolist(), want[2].tolist())
    assert _counts(out) == want[3], (what, _counts(out), want[3])
    if n_host is not None:
        assert int(out.n_place_host) == n_host, (what, int(out.n_place_host), n_host)


@pytest.mark.gpu
@pytest.mark.parametrize("block", range(N_CASES // BLOCK))
def test_fuzz_against_the_restatement(snk, block, tmp_path):
    from supernova_amd import graphio, lib as _lib
    from test_gpu_closures import _Case, _index, _raw
    e = _engine()
    made = split = 0
    t0, t_ref = time.perf_counter(), 0.0
    try:
        for seed in range(block * BLOCK, (block + 1) * BLOCK):
            c = closegen.make_case(seed)
            if c is None:
                continue
            made += 1
            t1 = time.perf_counter()
            want2, want1 = closegen.expected(c, True), closegen.expected(c, False)
            width, budget = closegen.drawn(c)
            want_w = closegen.expected(c, True, width)
            t_ref += time.perf_counter() - t1
            bod, n_pairs = want2[4], len(c.pairs)
            D = _Case(c)
            before = [t.clone() for t in D.tensors()]
            with graphio.hbv_handle(c.K, *D.u) as h:
                for cg1, want in ((False, want2), (True, want1)):
                    off, bases, first, stats = e.close_gaps(c.K, h, D.d_off, D.d_bases, D.inv, D.rows[:D.n], D.read_len, D.quals[:D.n], D.lens[:D.n], *D.paths, D.pairs[:D.n_pairs],
                                                            cg1=cg1)
                    assert all(np.array_equal(a, b) for a, b in zip((off, bases, first), want[:3])), (seed, cg1, first.tolist(), want[2].tolist())
                    assert {k: stats[k] for k in closeref.COUNTERS} == want[3] and stats["max_width"] == 400, (seed, cg1, stats, want[3])
                    graphio.write_closures(tmp_path / "closures.fastb", off, bases)
                    assert (tmp_path / "closures.fastb").read_bytes() == closeref.fastb_bytes(want[0], want[1]), (seed, cg1)
                    rc, msg, out, got = _raw(e, D, h, _lib.CLOSE_CG1 if cg1 else 0)
                    assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got, (off, bases, first))), (seed, cg1, "a second call", msg)
                    _check((seed, cg1, "a second call"), got, out, want, 0)
                rc, msg, out, got = _raw(e, D, h, 0, max_width=width)
                assert rc == 0 and out.max_width == width, msg
                _check((seed, "width", width), got, out, want_w, 0)
                px = _index(e, D)
                rc, msg, out, got = _raw(e, D, h, 0, px=px)
                assert rc == 0, msg
                _check((seed, "index given"), got, out, want2, 0)
                rc, msg, out, got = _raw(e, D, h, _lib.CLOSE_PLACE_HOST)
                assert rc == 0, msg
                _check((seed, "host"), got, out, want2, n_pairs)
                rc, msg, out, got = _raw(e, D, h, 0, budget=1)
                assert rc == 0 and out.bod_budget == 1, msg
                _check((seed, "budget 1"), got, out, want2, int((bod > 1).sum()))
                rc, msg, out, got = _raw(e, D, h, 0, budget=budget)
                assert rc == 0 and out.bod_budget == budget, msg
                _check((seed, "budget", budget), got, out, want2, int((bod > budget).sum()))
                split += 0 < int(out.n_place_host) < n_pairs
            for a, b in zip(before, D.tensors()):
                assert bool((a == b).all()), (seed, "an input changed")
    finally:
        e.close()
    t = time.perf_counter() - t0
    print(f"closures fuzz block {block}: {made} cases, {t:.1f} s, of which the restatement {t_ref:.1f} s; {split} cases with pairs on either side of the drawn budget")
    assert made >= 15 and split >= 1, (made, split)


@pytest.mark.gpu
def test_pinned_seeds_match_the_reference(snk):
    """the pinned seeds against the bytes the reference's own CloseGap2 / CloseGap wrote (tests/golden/closures/fuzz_<seed>.npz), at
    max_width 400 and 1 200"""
    from supernova_amd import graphio, lib as _lib
    from test_gpu_closures import _Case, _raw
    e = _engine()
    try:
        for seed in closeref.FUZZ:
            c, z = closegen.make_case(seed), closeref.load_fuzz(seed)
            assert z["input_digest"] == closeref.digest(c, c.reads), f"seed {seed}: the generator no longer makes the input the reference ran on"
            D = _Case(c)
            with graphio.hbv_handle(c.K, *D.u) as h:
                for flag in closeref.FLAGS:
                    for sfx, width in (("", closeref.MAX_WIDTH), ("_wide", closeref.WIDE)):
                        rc, msg, out, got = _raw(e, D, h, _lib.CLOSE_CG1 if flag == "cg1" else 0, max_width=width)
                        assert rc == 0, msg
                        assert closeref.fastb_bytes(got[0], got[1]) == z[f"fastb_{flag}{sfx}"] and np.array_equal(got[2], z[f"pair_first_{flag}{sfx}"]), (seed, flag, width)
    finally:
        e.close()
