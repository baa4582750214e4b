"""Graph edits on the device (Engine.delete_edges: snk_dev_delete_edges; Engine.hanging_ends: snk_dev_hanging_ends;
Engine.trim_hanging_ends).  Bar: for every case the edited a.hbv / a.inv / a.hbx bytes, the per-read offsets and edges and their a.pathsX
bytes equal what the reference's own DeleteEdgesParallel + Cleanup made (tests/golden/edit/, see tests/golden/make_edit_golden.py);
edge_map / edge_koff and the counters equal the restatement's (tests/editref.py); the order of dels and duplicates in it do not matter,
two calls agree, the caller's arrays are left alone; the chained case goes through delete_edges twice; the paths index on the result
equals hopsref.paths_index of the fixture's paths; the refusals return SNK_E_ARG and leave *out zero; both histogram legs of
hanging_ends give the fixture's support and selection."""
import ctypes as C

import numpy as np
import pytest

import a48xref
import editref
import hopsref
from devcall import _zeroed

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


class _Input:
    """a case on the device: the unitigs (BVComp order), the paths; graph(h) is the tuple the engine takes"""

    def __init__(self, c):
        self.c = c
        self.off, bases = editref.hu.to_arrays(c.unitigs)
        self.bases_h = bases
        self.bases = _dev(bases, np.uint8)
        self.inv = c.inv.copy()
        self.paths = (_dev(c.offset, np.int32), _dev(c.n_edges.view(np.int32), np.int32), _dev(c.edges, np.int32))

    def graph(self, h):
        return (self.c.K, h, self.off, self.bases, self.inv)

    def tensors(self):
        return (self.bases, *self.paths)


def _handle(inp):
    from supernova_amd import graphio
    return graphio.hbv_handle(inp.c.K, inp.off, inp.bases_h)


def _everything(engine, out, tmp_path, tag):
    """what a result is compared by: file bytes, paths, a.pathsX bytes, maps, counters"""
    out.write(tmp_path / f"{tag}.hbv", tmp_path / f"{tag}.inv", tmp_path / f"{tag}.hbx")
    ne, start = out.n_edges.cpu().numpy().view(np.uint32), out.start.cpu().numpy()
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(ne.astype(np.int64))]))
    index, data, _ = engine.zip_paths(out.h, out.offset, out.n_edges, out.edges, out.start)
    return dict(a_hbv=(tmp_path / f"{tag}.hbv").read_bytes(), a_inv=(tmp_path / f"{tag}.inv").read_bytes(), a_hbx=(tmp_path / f"{tag}.hbx").read_bytes(),
                offset=out.offset.cpu().numpy().copy(), n_edges=ne.copy(), edges=out.edges.cpu().numpy().copy(), pathsx=a48xref.pathsx_bytes(index, data, len(ne)),
                inv=out.inv.copy(), edge_map=out.edge_map.copy(), edge_koff=out.edge_koff.copy(), counters=tuple(out.stats[k] for k in editref.COUNTERS))


def _same(a, b):
    return all((np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]) for k in a)


def _check(got, step, m, what):
    assert got["a_hbv"] == step.a_hbv, f"{what}: a.hbv"
    assert got["a_inv"] == step.a_inv and np.array_equal(got["inv"], np.frombuffer(step.a_inv, "<i4", offset=16)), f"{what}: a.inv"
    assert got["a_hbx"] == a48xref.hbx_bytes(a48xref.parse_hbv(step.a_hbv)), f"{what}: a.hbx"
    assert np.array_equal(got["offset"], step.offset), f"{what}: offsets"
    assert np.array_equal(got["n_edges"], step.n_edges) and np.array_equal(got["edges"], step.edges), f"{what}: edges"
    assert got["pathsx"] == step.pathsx, f"{what}: a.pathsX bytes"
    assert np.array_equal(got["edge_map"], m.edge_map) and np.array_equal(got["edge_koff"], m.edge_koff), f"{what}: edge_map / edge_koff"
    assert got["counters"] == tuple(m.counters[k] for k in editref.COUNTERS), f"{what}: counters"


@pytest.mark.parametrize("key", editref.ALL)
def test_matches_the_reference(engine, key, tmp_path):
    c, g, mine = editref.case(key), editref.golden(key), editref.restated(key)
    assert g.pinned
    inp = _Input(c)
    before = [t.clone() for t in inp.tensors()]
    with _handle(inp) as h:
        out = engine.delete_edges(inp.graph(h), inp.paths, c.dels)
        got = _everything(engine, out, tmp_path, "a")
        _check(got, g.steps[0], mine[0], "edit 0")
        # the paths index on the result
        E2 = int(out.h.n_edges)
        p, start = engine._paths_struct(out.offset, out.n_edges, out.edges, out.start)
        want = hopsref.paths_index(g.steps[0].n_edges, g.steps[0].edges, E2)
        ioff, ids = engine._pidx_info(engine._pidx(p, E2, out.inv), E2, out.inv, True)["paths_index"] if E2 else (np.zeros(1, np.uint64), np.zeros(0, np.uint64))
        assert all(np.array_equal(ids[int(ioff[e]):int(ioff[e + 1])].astype(np.int64), want[e]) for e in range(E2)), "paths index on the result"
        # the caller's arrays are left alone, a second call gives the same, and so does every order of dels without its duplicates
        assert all(bool((a == b).all()) for a, b in zip(before, inp.tensors())) and np.array_equal(inp.inv, c.inv), "an input array changed"
        assert _same(got, _everything(engine, engine.delete_edges(inp.graph(h), inp.paths, c.dels), tmp_path, "b")), "two calls differ"
        for tag, dels in (("u", np.unique(c.dels)), ("r", np.unique(c.dels)[::-1])):
            assert _same(got, _everything(engine, engine.delete_edges(inp.graph(h), inp.paths, dels), tmp_path, tag)), f"dels order {tag} gives another result"
        if c.second:                                   # the second edit takes the first result as it is
            d2 = editref.second_dels(mine[0], c.second)
            out2 = engine.delete_edges(out.graph, out.paths, d2)
            _check(_everything(engine, out2, tmp_path, "c"), g.steps[1], mine[1], "edit 1")


@pytest.mark.parametrize("key", editref.ALL)
def test_hanging_ends(engine, key):
    c, g = editref.case(key), editref.golden(key)
    inp = _Input(c)
    E = len(c.inv)
    with _handle(inp) as h:
        res = {leg: engine.hanging_ends(inp.graph(h), inp.paths, leg=leg) for leg in ((None, "lds", "sort") if E <= 16384 else (None, "sort"))}
    for leg, (support, dels, stats) in res.items():
        assert np.array_equal(support, g.support), f"support, leg {leg}"
        assert np.array_equal(dels, g.hang_dels), f"dels, leg {leg}"
        assert stats["leg"] == (leg or ("lds" if E <= 16384 else "sort")) and stats["n_unsupported"] == int((g.support == 0).sum())
    if c.hang_want is not None:
        assert np.array_equal(res[None][1], c.hang_want)


def test_hanging_ends_max_kmers(engine):
    """max_kmers is the bound: at 201 the longer tip goes too, at 199 neither"""
    c = editref.case("hang_k48")
    inp = _Input(c)
    with _handle(inp) as h:
        for mk in (199, 200, 201):
            _, dels, _ = engine.hanging_ends(inp.graph(h), inp.paths, max_kmers=mk)
            assert np.array_equal(dels, editref.hanging_ends(c.a_hbv, c.inv, c.n_edges, c.edges, mk)[1])
            assert len(dels) == {199: 3, 200: 5, 201: 7}[mk]


@pytest.mark.parametrize("key", ("hang_k48", "hang_k60", "run65_k48") + editref.G_SEQ)
def test_trim_hanging_ends(engine, key, tmp_path):
    """the two in a row equal the reference's edit with the selection: in the hang cases and in the golden graphs' sequences the first
    list of the fixture IS the selection; run65 has nothing that hangs and comes back as it is"""
    c, g = editref.case(key), editref.golden(key)
    inp = _Input(c)
    with _handle(inp) as h:
        out = engine.trim_hanging_ends(inp.graph(h), inp.paths)
        got = _everything(engine, out, tmp_path, "t")
    assert np.array_equal(out.dels, g.hang_dels) and np.array_equal(out.support, g.support)
    if key != "run65_k48":
        assert np.array_equal(np.unique(c.dels), g.hang_dels)
        _check(got, g.steps[0], editref.restated(key)[0], "trim")
    else:
        m = editref.delete_edges(c.a_hbv, c.inv, c.offset, c.n_edges, c.edges, g.hang_dels)
        assert len(g.hang_dels) == 0 and got["a_hbv"] == c.a_hbv and got["a_inv"] == c.a_inv, "nothing hangs: the graph comes back"
        assert got["a_hbv"] == m.a_hbv and np.array_equal(got["edges"], m.edges) and np.array_equal(got["offset"], m.offset)


def test_refusals(engine):
    """SNK_E_ARG and *out all zero"""
    from supernova_amd import lib as _lib
    c = editref.case("run3_k48")
    inp = _Input(c)
    err = C.create_string_buffer(512)
    lib = engine.lib
    off64 = _dev(inp.off.view(np.int64), np.int64)
    with _handle(inp) as h:
        E, U = int(h.n_edges), len(c.unitigs)
        g = a48xref.parse_hbv(c.a_hbv)

        def paths_struct(offset, n_edges, edges, start=None):
            st = np.concatenate([[0], np.cumsum(n_edges)]).astype(np.int64) if start is None else np.asarray(start, np.int64)
            d = [_dev(offset, np.int32), _dev(n_edges, np.int32), _dev(st, np.int64), _dev(edges, np.int32)]
            p = _lib.SnkDevPaths()
            p.n_reads, p.n_edges_total = len(n_edges), len(edges)
            p.offset, p.n_edges, p.start, p.edges = (t.data_ptr() for t in d)
            return p, d

        def delete(p, inv, dels, flags=0):
            out = _lib.SnkDevEdit()
            C.memset(C.byref(out), 0xFF, C.sizeof(out))
            inv, dels = np.ascontiguousarray(inv, np.int32), np.ascontiguousarray(dels, np.int32)
            rc = lib.snk_dev_delete_edges(engine._ctx, c.K, U, off64.data_ptr(), inp.bases.data_ptr(), C.byref(h), inv.ctypes.data, C.byref(p), dels.ctypes.data, len(dels),
                                          flags, C.byref(out), engine._stream(), err, 512)
            return rc, out

        def hanging(p, inv, flags=0):
            out = _lib.SnkDevHanging()
            C.memset(C.byref(out), 0xFF, C.sizeof(out))
            inv = np.ascontiguousarray(inv, np.int32)
            rc = lib.snk_dev_hanging_ends(engine._ctx, c.K, U, off64.data_ptr(), inp.bases.data_ptr(), C.byref(h), inv.ctypes.data, C.byref(p), 200, flags, C.byref(out),
                                          engine._stream(), err, 512)
            return rc, out

        e0 = 0
        ok, ok_arrays = paths_struct([0, 3], [1, 1], [0, 1])
        pair = [int(c.dels[0]), int(c.inv[c.dels[0]])]
        for dels, word in (([E], b"outside"), ([-1], b"outside"), ([pair[0]], b"inverse")):
            rc, out = delete(ok, c.inv, dels)
            assert rc == SNK_E_ARG and _zeroed(out) and word in err.value, dels
        bad_inv = c.inv.copy()
        bad_inv[0] = (c.inv[0] + 1) % E
        for fn in (lambda: delete(ok, bad_inv, pair), lambda: hanging(ok, bad_inv)):
            rc, out = fn()
            assert rc == SNK_E_ARG and _zeroed(out) and b"involution" in err.value
        rc, out = delete(ok, c.inv, pair, flags=1)
        assert rc == SNK_E_ARG and _zeroed(out)
        rc, out = hanging(ok, c.inv, flags=3)
        assert rc == SNK_E_ARG and _zeroed(out)
        for args, word in ((([0, 0], [1, 1], [0, E]), b"outside"), (([0, 0], [1, 1], [0, -1]), b"outside"), (([0, 0], [1, 1], [0, 1], [0, 2, 2]), b"add up"),
                           (([0, 0], [1, 2], [0, 1]), b"add up")):
            p, keep = paths_struct(*args)
            for fn in (lambda: delete(p, c.inv, pair), lambda: hanging(p, c.inv)):
                rc, out = fn()
                assert rc == SNK_E_ARG and _zeroed(out) and word in err.value, args
        # consecutive edges that do not meet at a vertex: an edge followed by itself (no loop in this graph)
        assert g.v_right[e0] != g.v_left[e0]
        p, keep = paths_struct([0], [2], [e0, e0])
        rc, out = delete(p, c.inv, pair)
        assert rc == SNK_E_ARG and _zeroed(out) and b"meet" in err.value
        # ... and the calls that are in order
        rc, out = delete(ok, c.inv, pair)
        assert rc == 0 and out.n_deleted == 2 and out.n_old_edges == E
        lib.snk_dev_edit_free(C.byref(out))
        rc, out = hanging(ok, c.inv)
        assert rc == 0 and out.n_hbv_edges == E and out.leg == _lib.HANG_LDS
        lib.snk_host_free(C.cast(out.dels, C.c_void_p))
