"""Gap patches into the graph on the device (Engine.insert_patch: snk_dev_patch_pieces, snk_dev_count_graph, snk_dev_patch_merge,
snk_dev_hbv, snk_dev_patch_paths).  Bar: for every case the patched a.hbv / a.inv bytes, to3, left3, the translated paths and their
a.pathsX bytes equal what the reference's own StageInsertPatch steps made (tests/golden/patch/, see tests/golden/make_patch_golden.py);
the order of the closures does not matter, two calls agree, the caller's arrays are left alone; the refusals return their codes and
leave *out zero; StageExtension on the patched graph equals the reference's ExtendPathsNew on it."""
import ctypes as C

import numpy as np
import pytest

import a48xref
import patchref
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
    """a case on the device: the old unitigs (BVComp order), the closures in a given order, the paths"""

    def __init__(self, c, order=None):
        self.c = c
        self.off, bases = patchref.hu.to_arrays(c.old_unitigs)
        self.bases = _dev(bases, np.uint8)
        cl = list(c.closures) if order is None else [c.closures[int(i)] for i in order]
        self.coff, cb = patchref.closures_arrays(cl)
        self.cb = _dev(cb, np.uint8)
        self.paths = (_dev(c.offset, np.int32), _dev(c.n_edges.view(np.int32), np.int32), _dev(c.edges, np.int32))

    def tensors(self):
        return (self.bases, self.cb, *self.paths)


def _run(engine, inp):
    from supernova_amd import graphio
    with graphio.hbv_handle(inp.c.K, inp.off, inp.bases.cpu().numpy()) as h:
        return engine.insert_patch((inp.c.K, h, inp.off, inp.bases), (inp.coff, inp.cb), inp.paths)


def _everything(engine, out, tmp_path, tag):
    """what a result is compared by: file bytes, to3 / left3, per-read (edge, offset), a.pathsX bytes, counters"""
    out.write(tmp_path / f"{tag}.hbv", tmp_path / f"{tag}.inv")
    n = int(out.n_edges.shape[0])
    ne, off, edges, start = out.n_edges.cpu().numpy(), out.offset.cpu().numpy(), out.edges.cpu().numpy(), out.start.cpu().numpy()
    assert set(np.unique(ne).tolist()) <= {0, 1} and np.array_equal(start, np.concatenate([[0], np.cumsum(ne)]))       # at most ONE edge per read
    edge = np.full(n, -1, np.int32)
    edge[ne == 1] = edges
    index, data, _ = engine.zip_paths(out.h, out.offset, out.n_edges, out.edges, out.start)
    return dict(a_hbv=(tmp_path / f"{tag}.hbv").read_bytes(), a_inv=(tmp_path / f"{tag}.inv").read_bytes(), to3_off=out.to3_off.copy(), to3=out.to3.copy(),
                left3=out.left3.copy(), edge=edge, offset=off.copy(), pathsx=a48xref.pathsx_bytes(index, data, n), inv=out.inv.copy(),
                counters=(out.stats["n_first"], out.stats["n_later"], out.stats["n_cleared"]))


def _same(a, b):
    return all((np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]) for k in a)


@pytest.mark.parametrize("key", patchref.ALL)
def test_matches_the_reference(engine, key, tmp_path):
    c, g = patchref.case(key), patchref.golden(key)
    inp = _Input(c)
    before = [t.clone() for t in inp.tensors()]
    out = _run(engine, inp)
    got = _everything(engine, out, tmp_path, "a")
    assert got["a_hbv"] == g.a_hbv, "patched a.hbv"
    assert got["a_inv"] == g.a_inv and np.array_equal(got["inv"], np.frombuffer(g.a_inv, "<i4", offset=16)), "patched a.inv"
    assert np.array_equal(got["to3_off"], g.to3_off) and np.array_equal(got["to3"], g.to3), "to3"
    assert np.array_equal(got["left3"], g.left3), "left3"
    assert np.array_equal(got["edge"], g.edge), "translated paths: edges"
    assert np.array_equal(a48xref.wrap16(got["offset"]), g.offset), "translated paths: offsets"
    assert got["pathsx"] == g.pathsx, "a.pathsX bytes"
    placed = int((c.n_edges > 0).sum())
    assert sum(got["counters"]) == placed and got["counters"][0] + got["counters"][1] == int((g.edge >= 0).sum())
    if key.startswith("none_"):
        assert got["a_hbv"] == c.a_hbv and got["a_inv"] == c.a_inv                      # no closures: the input graph byte for byte
    # the caller's arrays are left alone, a second call gives the same, and so does every order of the closures
    assert all(bool((a == b).all()) for a, b in zip(before, inp.tensors())), "an input array changed"
    assert _same(got, _everything(engine, _run(engine, inp), tmp_path, "b")), "two calls differ"
    n = len(c.closures)
    for tag, order in (("r", np.arange(n)[::-1]), ("s", np.random.default_rng(n + c.K).permutation(n))):
        assert _same(got, _everything(engine, _run(engine, _Input(c, order)), tmp_path, tag)), f"closure order {tag} gives another result"


def test_offsets_are_int32(engine):
    """out->paths.offset is the int32 of TranslatePaths; only the zip wraps it (a path far down a long edge keeps its offset)."""
    c = patchref.case("long_edge_k48")
    m = patchref.insert_patch(c.K, c.a_hbv, c.closures, c.offset, c.n_edges, c.edges)
    out = _run(engine, _Input(c))
    assert np.array_equal(out.offset.cpu().numpy(), m.offset) and out.stats["n_first"] == m.counters["n_first"] and out.stats["n_later"] == m.counters["n_later"] \
        and out.stats["n_cleared"] == m.counters["n_cleared"]


def test_refusals(engine):
    """SNK_E_ARG and *out all zero: a closure base code above 3; an edge id outside the old graph; start / n_edges that do not add up."""
    import torch
    from supernova_amd import graphio, lib as _lib
    c = patchref.case("bridge_k48")
    inp = _Input(c)
    err = C.create_string_buffer(512)
    lib = engine.lib
    with graphio.hbv_handle(c.K, inp.off, inp.bases.cpu().numpy()) as h:
        plan = _lib.SnkPatchPlan()
        assert lib.snk_patch_plan_sizes(c.K, len(c.old_unitigs), inp.off.ctypes.data, C.byref(h), len(c.closures), inp.coff.ctypes.data, C.byref(plan), err, 512) == 0
        rows = torch.zeros((int(plan.n_pieces), 16), dtype=torch.int32, device="cuda")
        lens = torch.zeros((int(plan.n_pieces),), dtype=torch.int16, device="cuda")
        lonely = torch.zeros((max(int(plan.n_lonely_max), 1), 2), dtype=torch.int64, device="cuda")

        def pieces(cb, cap):
            pc = _lib.SnkDevPieces()
            C.memset(C.byref(pc), 0xFF, C.sizeof(pc))
            rc = lib.snk_dev_patch_pieces(engine._ctx, c.K, len(c.old_unitigs), inp.off.ctypes.data, inp.bases.data_ptr(), C.byref(h), len(c.closures), inp.coff.ctypes.data,
                                          cb.data_ptr(), cap, rows.data_ptr(), lens.data_ptr(), int(plan.n_lonely_max), lonely.data_ptr(), C.byref(pc), engine._stream(), err, 512)
            return rc, pc
        bad = inp.cb.clone()
        bad[len(bad) // 2] = 4
        rc, pc = pieces(bad, int(plan.n_pieces))
        assert rc == SNK_E_ARG and _zeroed(pc) and b"above 3" in err.value
        rc, pc = pieces(inp.cb, int(plan.n_pieces) - 1)                                   # buffers smaller than the plan
        assert rc == SNK_E_ARG and _zeroed(pc)
        rc, pc = pieces(inp.cb, int(plan.n_pieces))
        assert rc == 0 and pc.n_pieces == plan.n_pieces and int(lens.min()) >= c.K + 1 and int(lens.max()) <= 256

        E = int(h.n_edges)
        off64 = _dev(inp.off.view(np.int64), np.int64)

        def paths(offset, n_edges, edges, start=None):
            n = len(n_edges)
            st = np.concatenate([[0], np.cumsum(n_edges)]).astype(np.int64) if start is None else np.asarray(start, np.int64)
            d = [_dev(offset, np.int32), _dev(n_edges, np.int32), _dev(st, np.int64), _dev(edges, np.int32)]
            p = _lib.SnkDevPaths()
            p.n_reads, p.n_edges_total = n, len(edges)
            p.offset, p.n_edges, p.start, p.edges = (t.data_ptr() for t in d)
            px = _lib.SnkDevPatched()
            C.memset(C.byref(px), 0xFF, C.sizeof(px))
            rc = lib.snk_dev_patch_paths(engine._ctx, c.K, len(c.old_unitigs), off64.data_ptr(), inp.bases.data_ptr(), C.byref(h), len(c.old_unitigs), off64.data_ptr(),
                                         inp.bases.data_ptr(), C.byref(h), C.byref(p), C.byref(px), engine._stream(), err, 512)
            return rc, px
        rc, px = paths([0, 0], [1, 1], [0, E])
        assert rc == SNK_E_ARG and _zeroed(px) and b"outside" in err.value
        rc, px = paths([0, 0], [1, 1], [0, -1])
        assert rc == SNK_E_ARG and _zeroed(px)
        rc, px = paths([0, 0], [1, 1], [0, 1], start=[0, 2, 2])
        assert rc == SNK_E_ARG and _zeroed(px) and b"add up" in err.value
        rc, px = paths([0, 0], [1, 2], [0, 1])
        assert rc == SNK_E_ARG and _zeroed(px)
        rc, px = paths([0, 3], [1, 1], [0, 1])                                            # the old graph onto itself: every edge is its own image
        assert rc == 0 and px.n_first == 2 and px.n_to3 == E


def test_extension_on_the_patched_graph(engine):
    """The chain: snk_dev_extend_paths (without SNK_EXT_BACK) on what insert_patch returns equals the reference's ExtendPathsNew on the
    same graph and paths (tests/golden/patch/synth_2k_err_ext.npz, made through ext_driver)."""
    import goldens
    import pathgen
    key = patchref.SYNTH
    c, gc = patchref.case(key), goldens.load(key)
    want = bytes(np.load(patchref.PATCH / f"{key}_ext.npz")["pathsx0"])
    out = _run(engine, _Input(c))
    rows, quals, lens, _ = pathgen.to_device(gc.codes, gc.quals, gc.lens, np.zeros(len(gc.lens), np.int32))
    off, ne, edges, stats = engine.extend_paths(c.K, out.h, out.unitig_off, out.unitig_bases, rows, gc.codes.shape[1], quals, lens, out.offset, out.n_edges, out.edges,
                                                out.start, back=False)
    assert stats["n_quality_extended"] + stats["n_exact_extended"] >= 1
    index, data, _ = engine.zip_paths(out.h, _dev(off, np.int32), _dev(ne.view(np.int32), np.int32), _dev(edges, np.int32))
    assert a48xref.pathsx_bytes(index, data, len(ne)) == want
