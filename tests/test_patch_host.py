"""Gap-patch insertion on the CPU: the Python restatement of StageInsertPatch (tests/patchref.py) against what the reference's own
functions made of every case (tests/golden/patch/*.npz, written by tests/golden/make_patch_golden.py).  The restatement builds the graph
the way the library does -- allx chopped into pieces of at most 256 bases that overlap by K, the C oracle's count with min_freq 1, the
K-base sequences added as one-k-mer unitigs, the library's host graph builder -- so equality with the reference's bytes shows that
chopping with overlap K gives the reference's graph and that the oracle's edge builder (kmers/ReadPather.h) agrees with the BigK one
on these inputs.  The host-only part of the C interface (snk_patch_plan_sizes) is checked here too."""
import ctypes as C

import numpy as np
import pytest

import a48xref
import patchref
from supernova_amd import graphio, lib as _lib


_res: dict = {}


def restated(key):
    if key not in _res:
        c = patchref.case(key)
        _res[key] = patchref.insert_patch(c.K, c.a_hbv, c.closures, c.offset, c.n_edges, c.edges)
    return _res[key]


@pytest.mark.parametrize("key", patchref.ALL)
def test_restatement_reproduces_the_reference(key):
    g, m = patchref.golden(key), restated(key)
    assert m.a_hbv == g.a_hbv, "patched a.hbv"
    assert m.a_inv == g.a_inv, "patched a.inv"
    off, ids = patchref.flat(m.to3)
    assert np.array_equal(off, g.to3_off) and np.array_equal(ids, g.to3), "to3"
    assert np.array_equal(m.left3, g.left3), "left3"
    assert np.array_equal(m.edge, g.edge) and np.array_equal(a48xref.wrap16(m.offset), g.offset), "translated paths"
    assert m.pathsx == g.pathsx, "a.pathsX bytes"
    assert sum(m.counters.values()) == int((patchref.case(key).n_edges > 0).sum())


@pytest.mark.parametrize("K", patchref.KS)
def test_what_the_cases_are_for(K):
    """The property every hand-made case exists for, read from the reference's result (so that a later edit of a generator cannot lose it)."""
    def G(name):
        key = f"{name}_k{K}"
        return patchref.case(key), patchref.golden(key), restated(key)
    c, g, m = G("none")
    assert g.a_hbv == c.a_hbv and g.a_inv == c.a_inv and not c.closures                     # the graph comes back byte for byte
    assert all(len(x) == 1 for x in m.to3) and not g.left3.any()
    c, g, m = G("bridge")
    n_old, n_new = a48xref.parse_hbv(c.a_hbv).E, m.g3.E
    assert n_new == n_old - 2 and (g.left3 != 0).sum() == 2                                  # two dead ends become one edge (and its reverse complement)
    assert G("bridge_rc")[1].a_hbv == g.a_hbv                                                # the closure reverse-complemented: the same graph
    c, g, m = G("mid_split")
    sizes = set(np.diff(g.to3_off.astype(np.int64)).tolist())
    assert {2, 3} <= sizes
    later = m.offset[(m.edge >= 0)]
    assert m.counters["n_later"] >= 3 and m.counters["n_cleared"] >= 1 and len(later)
    trims = set()
    for r in np.nonzero(c.n_edges == 1)[0]:                                                  # one-edge paths: which part of the split edge they land on
        e = int(c.edges[int(c.n_edges[:r].sum())])
        if m.edge[r] >= 0 and len(m.to3[e]) == 3:
            trims.add(m.to3[e].index(int(m.edge[r])))
    assert trims == {0, 1, 2}
    c, g, m = G("inside")
    assert g.a_hbv == c.a_hbv                                                                # the closure lies on the graph already
    c, g, m = G("twice")
    assert m.g3.E == 2                                                                        # duplicate and overlapping closures: one bridge
    c, g, m = G("short")
    lens = sorted(len(s) for s in m.unitigs)
    assert lens.count(K) == 3 and lens.count(K + 1) == 1 and [len(x) for x in c.closures].count(K - 1) == 1   # two novel K-mers + a palindrome, one (K+1)-mer; K-1 is skipped
    c, g, m = G("lonely_edge")
    assert sum(len(s) == K for s in c.old_unitigs) == 2 and sum(len(s) == K for s in m.unitigs) == 2          # isolated one-k-mer edges survive
    c, g, m = G("palindrome")
    assert any(len(s) == K and s == patchref.hu.rc(s) for s in m.unitigs)                    # the palindromic k-mer is an edge of its own
    c, g, m = G("circle")
    two = np.nonzero(c.n_edges == 2)[0]
    starts = np.concatenate([[0], np.cumsum(c.n_edges.astype(np.int64))])
    assert any(c.edges[starts[r]] == c.edges[starts[r] + 1] for r in two) and m.counters["n_later"] >= 1       # [e, e]: OverlapAppend overlaps
    assert any(m.g3.v_left[e] == m.g3.v_right[e] for e in range(m.g3.E))
    c, g, m = G("new_branch")
    assert np.diff(m.g3.from_off).max() == 4                                                 # a third and a fourth out-edge
    c, g, m = G("negative")
    assert (c.offset[c.n_edges > 0] < 0).all() and m.counters["n_first"] == int((c.n_edges > 0).sum())
    c, g, m = G("long_edge")
    assert max(len(s) for s in c.old_unitigs) > 256 + K and max(patchref.n_pieces(len(s), K) for s in c.old_unitigs) >= 3


def test_synth_case_has_bridges():
    c, g = patchref.case(patchref.SYNTH), patchref.golden(patchref.SYNTH)
    assert len(c.closures) == 20 and a48xref.parse_hbv(g.a_hbv).E > a48xref.parse_hbv(c.a_hbv).E and (g.edge >= 0).sum() >= 1900


def test_overlap_append_takes_the_longest_overlap():
    q = [1, 2, 3, 4, 3, 4]
    patchref.overlap_append(q, [3, 4, 3, 4, 5, 6])
    assert q == [1, 2, 3, 4, 3, 4, 5, 6]                                                     # Vec.h:584-591's own example
    q = [7, 7]
    patchref.overlap_append(q, [7, 7])
    assert q == [7, 7]
    q = [1, 2]
    patchref.overlap_append(q, [3])
    assert q == [1, 2, 3]


@pytest.mark.parametrize("key", patchref.ALL)
def test_plan_sizes(snk, key):
    """snk_patch_plan_sizes (host only) counts the rows the restatement's chopping makes."""
    c = patchref.case(key)
    g = a48xref.parse_hbv(c.a_hbv)
    off, bases = patchref.hu.to_arrays(c.old_unitigs)
    coff, _ = patchref.closures_arrays(c.closures)
    rows_u, _, lonely_u = patchref.pieces(c.old_unitigs, c.K)
    rows_c, _, lonely_c = patchref.pieces(c.closures, c.K)
    n_j = sum(int(g.to_off[v + 1] - g.to_off[v]) * int(g.from_off[v + 1] - g.from_off[v]) for v in range(g.N))
    plan = _lib.SnkPatchPlan()
    err = C.create_string_buffer(512)
    with graphio.hbv_handle(c.K, off, bases) as h:
        rc = snk.snk_patch_plan_sizes(c.K, len(c.old_unitigs), off.ctypes.data, C.byref(h), len(c.closures), coff.ctypes.data, C.byref(plan), err, 512)
        assert rc == 0, err.value
        assert (plan.n_unitig_pieces, plan.n_junctions, plan.n_closure_pieces, plan.n_lonely_max) == (len(rows_u), n_j, len(rows_c), len(lonely_u) + len(lonely_c))
        assert plan.n_pieces == len(rows_u) + n_j + len(rows_c)
        # refusals: offsets that do not ascend, a unitig below K bases; *out is zero afterwards
        bad = coff.copy()
        if len(bad) > 2:
            bad[1] = bad[2] + np.uint64(1)
            assert snk.snk_patch_plan_sizes(c.K, len(c.old_unitigs), off.ctypes.data, C.byref(h), len(c.closures), bad.ctypes.data, C.byref(plan), err, 512) == -1
            assert plan.n_pieces == 0
        short = off.copy()
        short[1:] -= np.uint64(int(off[1]) - c.K + 1)
        assert snk.snk_patch_plan_sizes(c.K, len(c.old_unitigs), short.ctypes.data, C.byref(h), 0, None, C.byref(plan), err, 512) == -1 and plan.n_pieces == 0
