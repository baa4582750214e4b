"""What the hand-made MarkDups cases of tests/handpaths.py (run on the device by test_gpu_dups_handmade.py) rest on, checked with the C
oracle alone: every case has the key width it is named for, every case with more than one pair has duplicate groups, quality-sum ties
and groups over several barcodes, and the cases made for one branch of the kernel hold what that branch needs.  A change to the generator
that empties a case of its point fails here, without a GPU."""
import numpy as np
import pytest

import handpaths


@pytest.mark.parametrize("name", sorted(handpaths.DUPS_CASES))
def test_case_is_what_it_is_named_for(name):
    c = handpaths.dups_case(name)
    d = c.d
    assert handpaths.total_bits(d) == c.bits
    assert d.codes.shape == (2 * handpaths.DUPS_CASES[name]["n_pairs"], c.L) and d.path_edges.min(initial=0) >= 0
    assert np.all(d.codes[np.arange(c.L)[None, :] >= d.lens[:, None]] == 0) and d.lens.min(initial=5) >= 5
    o_dup, o_art, o_rate, o_nd, o_ni = c.oracle
    v = handpaths.group_view(d, lens=c.lens, bc=np.zeros(len(d.bc), np.int32) if c.null_bc else d.bc)
    assert (v.n_dup_reads, v.n_interdup_reads) == (o_nd, o_ni)            # the groups as restated here are the oracle's
    n_pairs = len(d.bc) // 2
    if name.startswith(("empty", "unplaced")):
        assert not (d.path_n > 0).any() and o_nd == 0 and not o_dup.any() and not o_art.any()
    elif n_pairs > 1:
        assert len(v.groups) >= 1 and v.n_ties >= 1 and o_dup.any() and o_art.any()
        assert c.null_bc or (o_ni >= 1 and 0 < o_rate <= 1)
        assert 0 < (d.path_n == 0).sum() or name.startswith("one_group")      # a share of the reads has no path
        assert (d.lens < c.L).any() or name == "one_group-2000"
    if name.startswith("one_group"):
        assert len(v.groups) == 1 and len(v.groups[0][3]) == 2 * n_pairs
    if handpaths.DUPS_CASES[name]["kind"] in handpaths.WIDE and n_pairs > 1:
        by_edge, by_off, by_low = handpaths.high_bit_twins(v.groups, c.edge_bit)
        assert by_low >= 1
        assert by_edge >= 1 or c.edge_bit < 19            # (wide_off has three small edge ids)
        assert by_off >= 1 or name.startswith("wide_edge")
    if name == "twins-2000":
        assert any(decisive and tie for _, decisive, tie in v.mates_together)
        assert all(o_art[p] for p, _, tie in v.mates_together if tie)     # both mates in one group with a tie, identical: the pair is an artifact


def test_every_width_class_occurs():
    widths = {handpaths.dups_case(n).bits for n in handpaths.DUPS_CASES}
    assert {10, 62, 63, 73} <= widths and any(11 <= w <= 40 for w in widths)
    assert any(40 < w < 62 for w in widths)               # 31-bit edges and 32-bit offsets inside the one-sort path as well
