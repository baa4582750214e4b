"""MowLawn on the device (Engine.mow_lawn: snk_dev_mow_lawn; 10X/Lawnmower.cc:301-554).  Bar: on every fixture dels and scored equal what
the reference's own MowLawn gave (tests/golden/mow/) and the counters equal those of the Python restatement that test_mow_host.py pins
to the same fixtures; the inputs are untouched and a second call gives the same bytes; the refusals return SNK_E_ARG or
SNK_E_UNSUPPORTED and leave *out zero; an EditResult's graph and paths go in as they are."""
import ctypes as C

import numpy as np
import pytest

import a48xref
import extref
import mowgen
import mowref
from devcall import _zeroed
from mowdev import Input, dev

pytestmark = pytest.mark.gpu
SNK_E_ARG, SNK_E_UNSUPPORTED = -1, -6
NAMES = list(mowgen.HAND) + [mowgen.WIDE] + [f"fuzz_{s}" for s in mowgen.FUZZ_SEEDS] + list(mowgen.GOLDEN)


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", NAMES)
def test_matches_the_reference(engine, name):
    c = mowref.load(name)
    _, _, cnt = mowref.restated(name)
    inp = Input(c)
    before = [t.clone() for t in inp.tensors()]
    with inp.handle() as h:
        dels, scored, stats = engine.mow_lawn(inp.graph(h), *inp.reads(), inp.paths, c.dup)
        assert dels.dtype == np.int32 and np.array_equal(dels, c.dels), name
        assert scored.dtype == np.int32 and np.array_equal(scored, c.scored), name
        assert {k: stats[k] for k in cnt} == cnt, stats
        assert stats["n_dels"] == len(c.dels) and stats["n_scored"] == len(c.scored) and stats["ms"] > 0 and len(stats["phase_ms"]) == 6
        assert all(bool((a == b).all()) for a, b in zip(before, inp.tensors())) and np.array_equal(inp.inv, c.inv), "an input array changed"
        d2, s2, stats2 = engine.mow_lawn(inp.graph(h), *inp.reads(), inp.paths, dev(c.dup, np.uint8))
        assert d2.tobytes() == dels.tobytes() and s2.tobytes() == scored.tobytes() and {k: stats2[k] for k in cnt} == cnt, "two calls differ"


def test_window_test_runs_before_the_scores(engine):
    """wide_k48: thousands of entries on e1, few of them work items"""
    c = mowref.load(mowgen.WIDE)
    inp = Input(c)
    with inp.handle() as h:
        _, _, stats = engine.mow_lawn(inp.graph(h), *inp.reads(), inp.paths, c.dup, download=False)
    assert stats["n_entries_in_window"] < stats["n_entries_on_candidates"]
    assert stats["n_entries_on_candidates"] > 4000 and stats["n_candidates"] > 300


def test_edit_result_goes_in_as_it_is(engine, tmp_path):
    """delete what the rule picked, then ask again on the EditResult's graph and paths: the restatement on the edited graph agrees"""
    c = mowref.load("hand_k48")
    inp = Input(c)
    with inp.handle() as h:
        out = engine.delete_edges(inp.graph(h), inp.paths, c.dels)
        dels, scored, stats = engine.mow_lawn(out.graph, *inp.reads(), out.paths, c.dup)
    out.write(tmp_path / "a.hbv", tmp_path / "a.inv")
    g = a48xref.parse_hbv((tmp_path / "a.hbv").read_bytes())
    paths = (out.offset.cpu().numpy(), out.n_edges.cpu().numpy().view(np.uint32), out.edges.cpu().numpy())
    d, s, cnt = mowref.mow_entries(g, extref.edge_bases(g), out.inv, c.codes, c.lens, c.quals, *paths, c.dup)
    assert np.array_equal(dels, d) and np.array_equal(scored, s) and {k: stats[k] for k in cnt} == cnt
    assert cnt["n_candidates"] > 0 and len(s) > 0


def test_refusals(engine):
    """SNK_E_ARG / SNK_E_UNSUPPORTED and *out all zero"""
    from supernova_amd import lib as _lib
    from supernova_amd.engine import dev_reads
    c = mowref.load("hand_k48")
    inp = Input(c)
    err = C.create_string_buffer(512)
    lib = engine.lib
    g = c.g
    d_dup = dev(c.dup, np.uint8)
    n = len(c.lens)
    with inp.handle() as h:
        E, U = int(h.n_edges), len(c.unitigs)

        def paths_struct(offset, n_edges, edges):
            st = np.concatenate([[0], np.cumsum(np.asarray(n_edges, np.int64))]).astype(np.int64)
            d = [dev(offset, np.int32), dev(np.asarray(n_edges, np.uint32).view(np.int32), np.int32), dev(st, np.int64), dev(edges, np.int32)]
            p = _lib.SnkDevPaths()
            p.n_reads, p.n_edges_total = len(n_edges), len(edges)
            p.offset, p.n_edges, p.start, p.edges = (t.data_ptr() for t in d)
            return p, d

        def mow(p, n_reads=n, dup=d_dup.data_ptr(), flags=0, inv=inp.inv):
            out = _lib.SnkDevMow()
            C.memset(C.byref(out), 0xFF, C.sizeof(out))
            r = dev_reads(inp.rows[:n_reads], inp.L, inp.quals[:n_reads], inp.lens[:n_reads])
            inv = np.ascontiguousarray(inv, np.int32)
            rc = lib.snk_dev_mow_lawn(engine._ctx, c.K, U, inp.d_off.data_ptr(), inp.d_bases.data_ptr(), C.byref(h), inv.ctypes.data, C.byref(r), C.byref(p), dup, flags,
                                      C.byref(out), engine._stream(), err, 512)
            return rc, out

        off, ne, edges = (np.asarray(a).copy() for a in c.paths)
        ok, keep_ok = paths_struct(off, ne, edges)
        rc, out = mow(ok)
        assert rc == 0 and out.n_dels == len(c.dels) and out.n_scored == len(c.scored)
        lib.snk_host_free(C.cast(out.dels, C.c_void_p))
        # an odd read count, no dup, a flag
        odd, keep_odd = paths_struct(off[:n - 1], ne[:n - 1], edges[:int(ne[:n - 1].sum())])
        rc, out = mow(odd, n_reads=n - 1)
        assert rc == SNK_E_ARG and _zeroed(out) and b"pairs" in err.value
        rc, out = mow(ok, dup=None)
        assert rc == SNK_E_ARG and _zeroed(out) and b"d_dup" in err.value
        rc, out = mow(ok, flags=1)
        assert rc == SNK_E_ARG and _zeroed(out) and b"flags" in err.value
        bad_inv = inp.inv.copy()
        bad_inv[0] = (bad_inv[0] + 1) % E
        rc, out = mow(ok, inv=bad_inv)
        assert rc == SNK_E_ARG and _zeroed(out) and b"involution" in err.value
        # an edge id outside the graph
        first = int(np.nonzero(ne)[0][0])
        at = int(ne[:first].sum())
        for bad in (E, -1):
            e2 = edges.copy()
            e2[at] = bad
            p, keep = paths_struct(off, ne, e2)
            rc, out = mow(p)
            assert rc == SNK_E_ARG and _zeroed(out) and b"edge id" in err.value, bad
        # what snk_dev_paths_zip refuses or would not give back: a step to an edge that does not leave the vertex, a path of 256 edges
        e0 = int(edges[at])
        assert g.v_right[e0] != g.v_left[e0]
        ne2, e2 = ne.copy(), list(edges)
        ne2[first] += 1
        e2.insert(at, e0)
        p, keep = paths_struct(off, ne2, np.asarray(e2, np.int32))
        rc, out = mow(p)
        assert rc == SNK_E_ARG and _zeroed(out) and b"does not leave" in err.value
        loop = [e for e in range(E) if g.v_left[e] == g.v_right[e]]
        two = next(((a, int(b)) for a in range(E) for b in g.from_e[g.from_off[g.v_right[a]]:g.from_off[g.v_right[a] + 1]] if g.v_right[int(b)] == g.v_left[a]), None)
        assert loop or two, "the hand-made graph has a cycle (e1_twice)"
        cyc = [loop[0]] * 256 if loop else [two[0], two[1]] * 128
        ne3 = np.zeros(n, np.uint32)
        ne3[0] = 256
        p, keep = paths_struct(np.zeros(n, np.int32), ne3, np.asarray(cyc, np.int32))
        rc, out = mow(p)
        assert rc == SNK_E_UNSUPPORTED and _zeroed(out) and b"255" in err.value
        # ... and the call is in order afterwards
        rc, out = mow(ok)
        assert rc == 0 and out.n_dels == len(c.dels)
        lib.snk_host_free(C.cast(out.dels, C.c_void_p))
