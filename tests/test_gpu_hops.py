"""FindEdgePairs on the device (snk_dev_edge_pairs: 10X/Closomatic.cc:17-354).  Bar: the pairs equal what the reference's own function
wrote (tests/golden/hops/), the per-part counts and the counters equal those of the Python restatement that test_hops_host.py pins to
the same pairs, with the paths index given and made inside, with both flag settings, and wherever part 3's closures run."""
import ctypes as C

import numpy as np
import pytest

import goldens
import hopsref
import pathgen

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


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.array(a, dtype=dtype))).to(torch.device("cuda", 0))


class _Case:
    """a fixture's unitigs, paths, barcodes and flags on the device"""

    def __init__(self, c, paths=None):
        from supernova_amd import graphio
        self.c = c
        self.u = graphio.unitigs_to_arrays(c.unitigs)
        self.d_off, self.d_bases = _dev(self.u[0].astype(np.int64), np.int64), _dev(self.u[1], np.uint8)
        off, ne, edges = c.paths if paths is None else paths
        self.n, self.n_entries = len(ne), len(edges)
        self.paths = (_dev(off, np.int32), _dev(np.asarray(ne, np.uint32).view(np.int32), np.int32), _dev(edges if len(edges) else np.zeros(1, np.int32), np.int32)[:len(edges)])
        self.start = _dev(np.concatenate([[0], np.cumsum(np.asarray(ne, np.int64))]), np.int64)
        self.bc = _dev(c.bc[:self.n] if self.n else np.zeros(1, np.int32), np.int32)
        self.bad = _dev(c.bad[:self.n // 2] if self.n >= 2 else np.zeros(1, np.uint8), np.uint8)
        self.inv = np.ascontiguousarray(c.inv, dtype=np.int32)


_cases: dict = {}


def _case(name) -> _Case:
    if name not in _cases:
        _cases[name] = _Case(hopsref.load(name))
    return _cases[name]


def _raw(engine, D, h, flags=0, budget=0, px=None, inv=None, n_reads=None, n_total=None):
    """the C call itself -> (rc, message, SnkDevHops, pairs or None)"""
    from supernova_amd import lib as _lib
    import devcall
    p = _lib.SnkDevPaths()
    p.n_reads, p.n_edges_total = (D.n if n_reads is None else n_reads), (D.n_entries if n_total is None else n_total)
    p.offset, p.n_edges, p.edges, p.start = D.paths[0].data_ptr(), D.paths[1].data_ptr(), D.paths[2].data_ptr(), D.start.data_ptr()
    out = _lib.SnkDevHops()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    err = C.create_string_buffer(512)
    inv = D.inv if inv is None else inv
    rc = engine.lib.snk_dev_edge_pairs(engine._ctx, D.c.K, len(D.u[0]) - 1, D.d_off.data_ptr(), D.d_bases.data_ptr(), C.byref(h), inv.ctypes.data, C.byref(p),
                                       C.byref(px) if px is not None else None, D.bc.data_ptr(), D.bad.data_ptr(), flags, budget, C.byref(out), engine._stream(), err, 512)
    pairs = devcall.download(engine, out.pairs, 2 * int(out.n_pairs), np.int32).reshape(-1, 2) if rc == 0 else None
    return rc, err.value.decode(errors="replace"), out, pairs


def _index(engine, D):
    from supernova_amd import lib as _lib
    p = _lib.SnkDevPaths()
    p.n_reads, p.n_edges_total = D.n, D.n_entries
    p.offset, p.n_edges, p.edges, p.start = D.paths[0].data_ptr(), D.paths[1].data_ptr(), D.paths[2].data_ptr(), D.start.data_ptr()
    return engine._pidx(p, D.c.g.E, D.inv)


def _counts(out):
    return {k: int(getattr(out, k)) for k in hopsref.COUNTERS}


@pytest.mark.parametrize("name", hopsref.ALL)
def test_pairs_match_the_reference(engine, name):
    """Every fixture, both flag settings: Engine.edge_pairs (index made inside) and the C call with the index given return the
    reference's pairs and the restatement's counts; no closure needed the host at the default budget; a second call gives the same
    bytes; the inputs are untouched."""
    from supernova_amd import graphio, lib as _lib
    c, D = hopsref.load(name), _case(name)
    with graphio.hbv_handle(c.K, *D.u) as h:
        for og in (False, True):
            want = c.pairs_one_good if og else c.pairs
            cnt = c.counts_one_good if og else c.counts
            before = [t.clone() for t in (*D.paths, D.bc, D.bad, D.d_bases)]
            pairs, stats = engine.edge_pairs(c.K, h, D.d_off, D.d_bases, D.inv, *D.paths, D.bc, D.bad, one_good=og)
            assert pairs.dtype == np.int32 and np.array_equal(pairs, want), (og, len(pairs), len(want))
            assert {k: stats[k] for k in cnt} == cnt, (og, stats)
            assert stats["n_ext_host"] == 0 and stats["ext_budget"] == 128 and stats["ms"] > 0
            assert stats["n_two_class"] == stats["n_ext_round0"] + stats["n_ext_closure"] + stats["n_not_extended"]
            for a, b in zip(before, (*D.paths, D.bc, D.bad, D.d_bases)):
                assert bool((a == b).all()), "an input changed"
            px = _index(engine, D)
            flags = _lib.HOPS_ONE_GOOD if og else 0
            rc, msg, out, got = _raw(engine, D, h, flags, px=px)
            assert rc == 0 and np.array_equal(got, want) and _counts(out) == cnt and out.n_ext_host == 0, msg
            rc, msg, out2, again = _raw(engine, D, h, flags)
            assert rc == 0 and again.tobytes() == pairs.tobytes() and _counts(out2) == cnt, msg


@pytest.mark.parametrize("K", (48, 60))
def test_hand_made_items_by_name(engine, K):
    """the stated outcome of every hand-made item, by name, for both flag settings (a mutation of a threshold or of a filter shows here)"""
    import handhops
    from supernova_amd import graphio
    c, D = hopsref.load(f"hand_k{K}"), _case(f"hand_k{K}")
    with graphio.hbv_handle(K, *D.u) as h:
        got = {int(og): engine.edge_pairs(K, h, D.d_off, D.d_bases, D.inv, *D.paths, D.bc, D.bad, one_good=og)[0] for og in (False, True)}
    handhops.assert_items(handhops.case(K), handhops.edge_index(c.eb), c.inv, got, "the device")


@pytest.mark.parametrize("name", hopsref.ALL)
def test_no_result_depends_on_where_the_closures_run(engine, name):
    """SNK_HOPS_EXT_HOST: every residual edge goes through the host routine; ext_budget = 1: every edge whose set needs a second
    sequence does -- on every fixture where the closure extended an edge (n_ext_closure > 0: adversarial and the two hand-made ones) some
    must, because each of those edges has the sequence [e] AND a longer start in its set; a fixture whose sets all hold one sequence
    cannot overflow at any budget, so the bound is not asked of those.  Pairs and counts are the fixture's every time."""
    from supernova_amd import graphio, lib as _lib
    c, D = hopsref.load(name), _case(name)
    residual = c.counts["n_ext_closure"] + c.counts["n_not_extended"]
    with graphio.hbv_handle(c.K, *D.u) as h:
        rc, msg, out, got = _raw(engine, D, h, _lib.HOPS_EXT_HOST)
        assert rc == 0 and np.array_equal(got, c.pairs) and _counts(out) == c.counts, msg
        assert out.n_ext_host == residual and (residual == 0 or out.n_ext_host >= 1)
        rc, msg, out, got = _raw(engine, D, h, 0, budget=1)
        assert rc == 0 and np.array_equal(got, c.pairs) and _counts(out) == c.counts and out.ext_budget == 1, msg
        assert out.n_ext_host <= residual and (c.counts["n_ext_closure"] == 0 or out.n_ext_host >= 1), int(out.n_ext_host)
        rc, msg, out, got = _raw(engine, D, h, 0, budget=100000)
        assert rc == 0 and np.array_equal(got, c.pairs) and out.ext_budget == 128 and out.n_ext_host == 0, msg


def test_a_set_that_outgrows_its_slice_goes_to_the_host(engine):
    """The other hand-over: the set's 4 096 ints fill before it holds 128 sequences.  On the hand-made graph, e is followed by an edge of ONE
    k-mer that loops on its vertex, a read lies on [e loop] and its mate brings [loop loop]: the set grows by [e loop^k], k = 1 .. 99,
    (k + 2 ints each: 4 096 ints after 88 of them) until the 100th loop extends e.  At the default budget the device gives the edge to the
    host, and pairs and counts are the restatement's."""
    import handhops
    from types import SimpleNamespace
    from supernova_amd import graphio
    c, D0 = hopsref.load("hand_k48"), _case("hand_k48")
    it = {i.name: i for i in handhops.case(48).items}["part3_closure_loop_with_tail"]
    (e, loop), r = it.pairs[2][0], handhops.rc(it.pairs[0][1][0])
    rc = handhops.rc
    h = SimpleNamespace(items=[SimpleNamespace(pairs=[([e], [rc(r)], 1, 0), ([e], [rc(r)], 2, 0), ([e, loop], [rc(loop), rc(loop)], 1, 0)])])
    edge_of = handhops.edge_index(c.eb)
    paths, bc, bad = handhops.arrays(h, edge_of)
    how: dict = {}
    want, info = hopsref.find_edge_pairs(c.g, c.km, c.inv, paths[1], paths[2], bc, bad, False, how)
    assert how[edge_of[e]] == "closure" and c.km[edge_of[loop]] == 1
    D = _Case(SimpleNamespace(unitigs=c.unitigs, paths=paths, bc=bc, bad=bad, inv=c.inv, K=48, g=c.g))
    with graphio.hbv_handle(48, *D.u) as hh:
        pairs, stats = engine.edge_pairs(48, hh, D.d_off, D.d_bases, D.inv, *D.paths, D.bc, D.bad)
        assert np.array_equal(pairs, want) and {k: stats[k] for k in hopsref.COUNTERS} == {k: info[k] for k in hopsref.COUNTERS}, stats
        assert stats["ext_budget"] == 128 and stats["n_ext_host"] >= 1, stats
        # without the mate's [loop loop] nothing grows: the same edge stays on the device
        h.items[0].pairs[2] = ([e, loop], [rc(r)], 1, 0)
        paths, bc, bad = handhops.arrays(h, edge_of)
        want, info = hopsref.find_edge_pairs(c.g, c.km, c.inv, paths[1], paths[2], bc, bad, False)
        D = _Case(SimpleNamespace(unitigs=c.unitigs, paths=paths, bc=bc, bad=bad, inv=c.inv, K=48, g=c.g))
        pairs, stats = engine.edge_pairs(48, hh, D.d_off, D.d_bases, D.inv, *D.paths, D.bc, D.bad)
        assert np.array_equal(pairs, want) and len(want) >= 1 and stats["n_ext_host"] == 0, stats


def _all_zero(x) -> bool:
    return bytes(x) == bytes(C.sizeof(x))


def test_refusals(engine):
    """Every refusal returns SNK_E_ARG with *out all zero; the call after it works."""
    from supernova_amd import graphio, lib as _lib
    c, D = hopsref.load("adversarial"), _case("adversarial")
    off, ne, edges = c.paths
    start = np.concatenate([[0], np.cumsum(ne.astype(np.int64))])
    with graphio.hbv_handle(c.K, *D.u) as h:
        odd = _Case(c, (off[:-1], ne[:-1], edges[:start[-2]]))
        outside = _Case(c, (off, ne, np.where(np.arange(len(edges)) == 3, c.g.E, edges).astype(np.int32)))
        negative = _Case(c, (off, ne, np.where(np.arange(len(edges)) == 0, -1, edges).astype(np.int32)))
        not_inv = D.inv.copy()
        not_inv[0] = not_inv[1] if not_inv[1] != not_inv[0] else not_inv[2]
        px = _index(engine, D)
        px_edges, px_entries = _lib.SnkDevPidx.from_buffer_copy(px), _lib.SnkDevPidx.from_buffer_copy(px)
        px_edges.n_hbv_edges += 1
        px_entries.n_entries -= 1
        for what, case, kw in (("odd read count", odd, {}), ("edge id outside", outside, {}), ("negative edge id", negative, {}), ("inv", D, dict(inv=not_inv)),
                               ("px edges", D, dict(px=px_edges)), ("px entries", D, dict(px=px_entries)), ("flags", D, dict(flags=4)),
                               ("table", D, dict(n_total=D.n_entries - 1))):
            rc, msg, out, _ = _raw(engine, case, h, **kw)
            assert rc == SNK_E_ARG and msg and _all_zero(out), (what, rc, msg)
        rc, msg, out, got = _raw(engine, D, h, px=px)
        assert rc == 0 and np.array_equal(got, c.pairs), msg
        # no reads at all
        none = _Case(c, (off[:0], ne[:0], edges[:0]))
        rc, msg, out, got = _raw(engine, none, h)
        assert rc == 0 and out.n_pairs == 0 and len(got) == 0 and out.n_long_edges == c.counts["n_long_edges"], msg


def test_path_reads_gives_the_pairs_and_write_a48_the_file(engine, tmp_path):
    """count + graph + paths + MarkBads + index + FindEdgePairs in one path_reads call on the adversarial case (the device's paths ARE
    the reference's: test_gpu_paths.py): the pairs are the fixture's for both settings, write_a48 adds a.hops with the reference's
    bytes, and without bc the call is refused before anything runs.  Only this fixture can come out of path_reads: the hand-made ones
    have paths and no reads, `gapped` keeps its paths and not its reads, and the other golden cases either have one unitig and no pair
    or are cut to their first 10 000 reads (extref.golden_input), which path_reads would not reproduce."""
    from supernova_amd import graphio
    c, fx = goldens.load("adversarial"), hopsref.load("adversarial")
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    off, ne, edges, info = res.path_reads(rows, c.read_len, dq, lens=dl, bc=dbc, mark_dups=True, mark_bads="x", hops=True)
    assert np.array_equal(ne, fx.paths[1]) and np.array_equal(edges, fx.paths[2]) and np.array_equal(info["bads"]["bad"], fx.bad)
    assert info["hops"].dtype == np.int32 and np.array_equal(info["hops"], fx.pairs)
    assert {k: info["hops_stats"][k] for k in fx.counts} == fx.counts and "paths_index" in info
    u = graphio.unitigs_to_arrays(c.exp_unitigs)
    graphio.write_a48(tmp_path / "a.48", 48, *u, off, ne, edges, info)
    assert (tmp_path / "a.48" / "a.hops").read_bytes() == fx.hops
    _, _, _, info1 = res.path_reads(rows, c.read_len, dq, lens=dl, bc=dbc, mark_bads="x", hops="one_good")
    assert np.array_equal(info1["hops"], fx.pairs_one_good) and {k: info1["hops_stats"][k] for k in fx.counts_one_good} == fx.counts_one_good
    _, _, _, info2 = res.path_reads(rows, c.read_len, dq, lens=dl, bc=dbc, mark_bads="x", hops="one_good", download=False)
    assert "hops" not in info2 and info2["hops_stats"]["n_pairs"] == len(fx.pairs_one_good)
    with pytest.raises(ValueError):
        res.path_reads(rows, c.read_len, dq, lens=dl, hops=True)
