"""snk_dev_mark_dups (csrc/snk_dups.hip) on hand-made paths (tests/handpaths.py) against the C oracle's MarkDups (oracle_lib.mark_dups,
pinned to the reference by tests/golden/a48/*.npz and dup_groups.npz): the widths of the sort key that no pather produces -- 10 bits,
the last width of the one-sort path (62, unplaced reads on bit 62), the first of the automatic two-sort fallback (63), 73 bits, 31-bit
edge ids and 32-bit offset ranges inside one sort -- with groups that only a high bit of the edge id or the sign bit of the offset keeps
apart, no read placed, every read in one group, both mates of a pair in one group, lens / bc NULL, and the refusals.  Every case runs
with dups_two_sorts unset and pinned to 1; test_handpaths_host.py checks on the CPU that the cases are what they are named for."""
import numpy as np
import pytest

import handpaths

pytestmark = pytest.mark.gpu
SNK_E_ARG = -1


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


def _expect(call, c):
    """every pair's flag and every counter of a good call == the oracle"""
    assert call.rc == 0, call.err.value
    o_dup, o_art, o_rate, o_nd, o_ni = c.oracle
    assert int(call.out.n_pairs) == len(o_dup)
    assert np.array_equal(call.dup, o_dup), np.nonzero(call.dup != o_dup)[0][:10]
    got, want = call.counters(), (o_nd, o_ni, int(o_dup.sum()), int(o_art.sum()), int((c.d.path_n > 0).sum()), o_rate)
    print(f"[dups_handmade] {c.name}: total_bits {c.bits}, counters {got}, snk_dev_mark_dups {call.out.ms:.3f} ms")
    assert got == want


@pytest.mark.parametrize("name", sorted(handpaths.DUPS_CASES))
def test_mark_dups_matches_the_oracle_on_both_sort_paths(engine, tune, name):
    c = handpaths.dups_case(name)
    assert handpaths.total_bits(c.d) == c.bits                      # the case takes the branch it is named for
    if handpaths.DUPS_CASES[name]["kind"] in handpaths.WIDE and len(c.d.bc) > 2:
        v = handpaths.group_view(c.d)
        by_edge, by_off, by_low = handpaths.high_bit_twins(v.groups, c.edge_bit)
        assert by_low >= 1 and (by_edge >= 1 or c.edge_bit < 19) and (by_off >= 1 or name.startswith("wide_edge")) and by_edge + by_off >= 1
    if name == "twins-2000":
        together = handpaths.group_view(c.d).mates_together
        assert any(decisive and tie for _, decisive, tie in together) and all(c.oracle[1][p] for p, _, tie in together if tie)
    assert engine.get_option("dups_two_sorts") is None
    kw = dict(null_lens=c.null_lens, null_bc=c.null_bc, pad_seed=c.pad_seed)
    auto = handpaths.DupsCall(engine, c.d, **kw)
    _expect(auto, c)
    tune("dups_two_sorts", 1)
    two = handpaths.DupsCall(engine, c.d, **kw)
    _expect(two, c)
    assert np.array_equal(auto.dup, two.dup) and auto.counters() == two.counters()
    if name.startswith(("empty", "unplaced")):
        assert not auto.dup.any() and auto.counters() == (0, 0, 0, 0, 0, 0.0)


def test_refusals_leave_out_zero_and_the_context_usable(engine):
    """A path table of another read count: SNK_E_ARG, *out all zero, and the next call on the same context equals the oracle."""
    c = handpaths.dups_case("narrow-129")
    n = len(c.d.path_n)
    for other in (n - 2, n + 2, 0):
        bad = handpaths.DupsCall(engine, c.d, paths_n_reads=other)
        assert bad.rc == SNK_E_ARG and f"paths of {other}".encode() in bad.err.value, (bad.rc, bad.err.value)
        assert bad.zeroed()
        _expect(handpaths.DupsCall(engine, c.d), c)
