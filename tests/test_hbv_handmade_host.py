"""The graph-from-unitigs step on hand-made unitig sets (tests/handunitigs.py), host side: snk_hbv_from_unitigs, snk_hbv_involution,
snk_write_hbv and snk_write_bv against what the reference's buildHBVFromEdges and writers made of the same sets (tests/golden/hbv/, written
by tests/golden/make_hbv_golden.py), and the oracle (sno_hbv_build, sno_write_bv) against the same fixtures: the GPU tests take their
expected values from it for the cases that are not kept.  Every comparison is exact.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import handunitigs as hu

SNK_E_ARG = -1
ALL = [(n, K) for n in hu.CASES for K in hu.KS]
KEPT = [(n, K) for n in hu.SAVED for K in hu.KS]


def _host(c):
    from supernova_amd import graphio
    return graphio.hbv_from_unitigs(c.K, c.off, c.bases)


@pytest.mark.parametrize("name,K", ALL)
def test_case_is_a_unitig_set_and_keeps_what_it_is_for(name, K):
    c = hu.case(name, K)                       # (check_valid runs inside)
    hu.check_valid(c.unitigs, K)
    assert c.unitigs == hu.bvcomp_sorted(c.unitigs)
    hu.check_facts(c)
    assert sorted(hu.orders(c)) == sorted(hu.ORDERS) and all(sorted(p) == list(range(len(c.unitigs))) for p in hu.orders(c).values())


def test_the_kept_cases_are_the_ones_named():
    assert set(hu.SAVED) | set(hu.UNSAVED) == set(hu.CASES) and set(hu.UNSAVED) == {"chain_1023", "chain_1024", "forest_255", "forest_256", "mixed_seed2", "mixed_seed3", "mixed_seed4"}
    assert all(hu.golden_path(n, K).exists() for n, K in KEPT)
    assert sorted(p.name for p in hu.golden_path("x", 48).parent.glob("*.npz")) == sorted(hu.golden_path(n, K).name for n, K in KEPT)


@pytest.mark.parametrize("name,K", ALL)
def test_host_builder_equals_oracle_and_the_facts(snk, name, K):
    c = hu.case(name, K)
    h, o = _host(c), hu.oracle_hbv(c)
    assert hu.same_graph(h, o) is None, hu.same_graph(h, o)
    f = c.facts
    assert (h["n_edges"], h["n_vertices"]) == (f["n_edges"], f["n_vertices"])
    assert int((h["v_left"] == h["v_right"]).sum()) == f["self_loops"]
    _, n = np.unique(np.stack([h["v_left"], h["v_right"]]), axis=1, return_counts=True)
    assert int((n * (n - 1) // 2).sum()) == f["parallel_pairs"]
    assert int(np.bincount(np.concatenate([h["v_left"], h["v_right"]])).max()) == f["max_ends"]


@pytest.mark.parametrize("name,K", KEPT)
def test_host_builder_and_writers_equal_the_reference(snk, tmp_path, name, K):
    from supernova_amd import graphio
    c = hu.case(name, K)
    g = hu.golden(c)                           # (compares the regenerated unitigs with the fixture's)
    h = _host(c)
    assert hu.same_graph(h, g.hbv) is None, hu.same_graph(h, g.hbv)
    assert np.array_equal(g.edge_lens, np.diff(c.off.astype(np.int64))[h["src"]])
    with graphio.hbv_handle(K, c.off, c.bases) as handle:
        inv = np.full(max(h["n_edges"], 1), -7, np.int32)
        err = C.create_string_buffer(512)
        assert snk.snk_hbv_involution(C.byref(handle), len(c.unitigs), inv.ctypes.data, err, 512) == 0, err.value
    assert g.a_inv[:8] == b"BINWRITE" and int.from_bytes(g.a_inv[8:16], "little") == h["n_edges"]
    assert np.array_equal(inv[:h["n_edges"]], np.frombuffer(g.a_inv[16:], "<i4"))
    graphio.write_hbv(tmp_path / "a.hbv", tmp_path / "a.inv", K, c.off, c.bases)
    assert (tmp_path / "a.hbv").read_bytes() == g.a_hbv
    assert (tmp_path / "a.inv").read_bytes() == g.a_inv
    graphio.write_bv(tmp_path / "edges.bv", c.off, c.bases)
    assert (tmp_path / "edges.bv").read_bytes() == g.edges_bv


@pytest.mark.parametrize("name,K", KEPT)
def test_oracle_equals_the_reference(name, K, tmp_path):
    """pins the oracle that the GPU tests use for the sizes that are not kept"""
    c = hu.case(name, K)
    g = hu.golden(c)
    assert hu.same_graph(hu.oracle_hbv(c), g.hbv) is None, hu.same_graph(hu.oracle_hbv(c), g.hbv)
    assert hu.oracle_bv(c, tmp_path / "oracle.bv") == g.edges_bv


def test_the_writer_cases_hold_self_loops_and_parallel_edges():
    """a.hbv lists a vertex's edges by upper-bound insertion in edge-id order: the order matters where a vertex has a self-loop or two edges
    to one neighbour.  The byte comparison above runs on such graphs."""
    for K in hu.KS:
        assert hu.case("circle", K).facts["self_loops"] == 2 and hu.case("bubble", K).facts["parallel_pairs"] == 2
        m = hu.case("mixed_seed1", K).facts
        assert m["self_loops"] >= 2 and m["parallel_pairs"] >= 2


@pytest.mark.parametrize("K", hu.KS)
def test_refusals(snk, K):
    from supernova_amd import lib as _lib
    c = hu.case("bubble", K)
    us = list(c.unitigs)
    us[2] = us[2][:K - 1]
    off, bases = hu.to_arrays(us)
    h = _lib.SnkHbv()
    C.memset(C.addressof(h), 0xA5, C.sizeof(h))
    err = C.create_string_buffer(512)
    assert snk.snk_hbv_from_unitigs(K, len(us), off.ctypes.data, bases.ctypes.data, C.byref(h), err, 512) == SNK_E_ARG and b"shorter than K" in err.value
    assert C.string_at(C.addressof(h), C.sizeof(h)) == bytes(C.sizeof(h))
    C.memset(C.addressof(h), 0xA5, C.sizeof(h))
    assert snk.snk_hbv_from_unitigs(K, 0, None, None, C.byref(h), err, 512) == 0
    assert (h.n_vertices, h.n_edges) == (0, 0) and C.string_at(C.addressof(h), C.sizeof(h)) == bytes(C.sizeof(h))
