"""CloseGap / CloseGap2 without a GPU: the Python restatement (tests/closeref.py) reproduces the closures the reference's own functions
wrote for every fixture under tests/golden/closures/ (tests/golden/make_closures_golden.py), both flags, and graphio.write_closures gives
the bytes of the reference's closures.fastb."""
import numpy as np
import pytest

import closeref


@pytest.mark.parametrize("name", closeref.ALL)
@pytest.mark.parametrize("flag", closeref.FLAGS)
def test_restatement_reproduces_the_reference(name, flag):
    c = closeref.load(name)
    off, bases, first, cnt, _ = closeref.close_gaps(c.I, c.pairs, flag == "cg2")
    assert np.array_equal(first, getattr(c, f"pair_first_{flag}")), (first.tolist(), getattr(c, f"pair_first_{flag}").tolist())
    assert np.array_equal(off, getattr(c, f"closure_off_{flag}")) and np.array_equal(bases, getattr(c, f"bases_{flag}"))
    assert cnt == getattr(c, f"counts_{flag}")
    assert cnt["n_pairs_0"] + cnt["n_pairs_1"] + cnt["n_pairs_2"] + cnt["n_pairs_many"] == len(c.pairs)
    assert int(first[-1]) == cnt["n_pairs_1"] + 2 * cnt["n_pairs_2"]
    if flag == "cg1":
        assert cnt["n_partners_tried"] == cnt["n_partners_placed"] == cnt["n_followers"] == 0


@pytest.mark.parametrize("name", closeref.WIDE_CASES)
@pytest.mark.parametrize("flag", closeref.FLAGS)
def test_restatement_reproduces_the_reference_at_another_width(name, flag):
    """max_width = 1 200: a consensus of 1000 columns or more gives no offsets"""
    c = closeref.load(name)
    off, bases, first, cnt, _ = closeref.close_gaps(c.I, c.pairs, flag == "cg2", closeref.WIDE)
    assert np.array_equal(first, getattr(c, f"pair_first_{flag}_wide")) and np.array_equal(off, getattr(c, f"closure_off_{flag}_wide"))
    assert np.array_equal(bases, getattr(c, f"bases_{flag}_wide")) and cnt == getattr(c, f"counts_{flag}_wide") and cnt["n_cons_too_long"] >= 1
    assert not np.array_equal(first, getattr(c, f"pair_first_{flag}"))


@pytest.mark.parametrize("name", closeref.HAND)
def test_hand_made_items_by_name(name):
    """the stated closures of every hand-made item, by name -- CloseGap2, CloseGap and max_width 1 200 -- in the reference's result (the
    fixture, which the restatement reproduces); the filters an item is there for remove an offset of its pair; only the long follower has more
    32-mers than the default bod_budget"""
    import handclose
    c = closeref.load(name)
    h = handclose.case(c.K)
    for flag, which, sfx, width in (("cg2", "closures", "", closeref.MAX_WIDTH), ("cg1", "closures_cg1", "", closeref.MAX_WIDTH), ("cg2", "closures_wide", "_wide", closeref.WIDE)):
        handclose.assert_items(h, c.edge_of, c.pairs, getattr(c, f"closure_off_{flag}{sfx}"), getattr(c, f"bases_{flag}{sfx}"), getattr(c, f"pair_first_{flag}{sfx}"),
                               f"the fixture ({flag})", which)           # (= the restatement's: test_restatement_reproduces_the_reference*)
    for it in h.items:
        w = {}
        closeref.close_gap(c.I, c.edge_of[it.pair[0]], c.edge_of[it.pair[1]], True, closeref.MAX_WIDTH, None, w)
        assert all(w[f] >= 1 for f in it.fires), (it.name, w)
        assert (w.get("bod_max", 0) > closeref.BOD_BUDGET) == (it.name == "long_follower"), (it.name, w)
    assert {i.name for i in h.items} >= {"two_offsets", "three_offsets", "invalidation", "big_near_small", "partner_placed_once", "partner_found_twice"}
    assert handclose.BOD_BUDGET == closeref.BOD_BUDGET
    # what the quality item is for: the seed consensus has A where the closure has T
    it = {i.name: i for i in h.items}["quality_columns"]
    locs, _ = closeref._locs(c.I, c.edge_of[it.pair[0]], False)
    con = closeref.seed_consensus(*closeref._stack(c.I, c.edge_of[it.pair[0]], locs, closeref.MAX_WIDTH, False))
    assert con[100:105].tolist() == [0] * 5 and it.closures[0][100:105] == "TTTTT"


def test_the_fixtures_are_not_vacuous():
    """some pair closes, some does not, and CloseGap2 places partners that CloseGap does not have"""
    tot = {f: {k: sum(getattr(closeref.load(n), f"counts_{f}")[k] for n in closeref.ALL) for k in closeref.COUNTERS} for f in closeref.FLAGS}
    assert all(tot[f][k] >= 1 for f in closeref.FLAGS for k in ("n_pairs_0", "n_pairs_1", "n_pairs_2", "n_pairs_many"))
    assert tot["cg2"]["n_partners_placed"] >= 1 and tot["cg2"]["n_followers"] >= 1
    assert tot["cg2"]["n_rows"] != tot["cg1"]["n_rows"], "the two flags differ nowhere"


@pytest.mark.parametrize("name", closeref.ALL)
def test_write_closures_gives_the_reference_bytes(snk, name, tmp_path):
    """closures.fastb = BinaryWriter::writeFile(vec<basevector>) is the layout snk_write_bv writes and snk_read_bv reads"""
    from supernova_amd import graphio
    c = closeref.load(name)
    for flag in closeref.FLAGS:
        want = getattr(c, f"fastb_{flag}")
        off, bases = getattr(c, f"closure_off_{flag}"), getattr(c, f"bases_{flag}")
        graphio.write_closures(tmp_path / "closures.fastb", off, bases)
        assert (tmp_path / "closures.fastb").read_bytes() == want
        assert closeref.fastb_bytes(off, bases) == want
        off2, bases2 = graphio.read_bv(str(tmp_path / "closures.fastb"))
        assert np.array_equal(np.asarray(off2, np.uint64), off) and np.array_equal(bases2, bases)


def test_restatement_bits_table_spot_values():
    """the RESTATEMENT's table only (the library's own is reached through the closures): spot values of PrecomputedBinomialSums<1000>(20, 0.75): log10 of exact binomial sums where the arithmetic is exact enough to say, 0.0
    where the reference never writes, -inf where pow(0.25, n) has underflowed"""
    from math import comb, log10
    t = closeref.bits_table()
    assert t.shape == (1000, 1000) and not t[:20].any() and t[20, 20] == 0.0 and t[999, 999] == 0.0
    for n, k in ((20, 0), (20, 5), (40, 10), (100, 30), (400, 250)):
        exact = sum(comb(n, i) * 3 ** i for i in range(k + 1)) / 4 ** n
        assert abs(t[n, k] - log10(exact)) < 1e-9, (n, k, t[n, k], log10(exact))
    assert np.isneginf(t[600, 0]) and np.isfinite(t[500, 0])
