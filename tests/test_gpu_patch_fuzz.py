"""Gap-patch insertion and the graph edit on the device (Engine.insert_patch, Engine.delete_edges / hanging_ends / trim_hanging_ends) against
the Python restatements (tests/patchref.py, tests/editref.py; pinned to the reference on this distribution by
tests/test_patch_fuzz_host.py) on the 120 seeded cases of tests/patchgen.py.

Per case: insert_patch -- the patched a.hbv / a.inv bytes, to3, left3, per read the edge and the int32 offset, the a.pathsX bytes and the
three counters; a second call, the caller's tensors, and on every second seed the closures reversed and in a seeded permutation.  Then,
on the graph insert_patch RETURNED (its handle, unitigs and involution as they are), delete_edges with the seed's own paths and deletion
list -- a.hbv / a.inv / a.hbx bytes, offsets, edges, a.pathsX bytes, edge_map, edge_koff and all seven counters; a second call, dels
without duplicates ascending and descending --, hanging_ends on all three legs, and on every fourth seed trim_hanging_ends against
delete_edges of that selection.  On the pinned seeds the device must also give the bytes the reference's own functions wrote
(tests/golden/patch/fuzz_<seed>.npz, tests/golden/edit/fuzz_<seed>.npz).

That the generation reaches every part of both stages, and that the expected answers move with every rule, is checked without a GPU in
test_patch_fuzz_host.py."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import a48xref
import editref
import patchgen
import patchref

pytestmark = pytest.mark.gpu
N_CASES, BLOCK = patchgen.N_SEEDS, 10


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


def _step(d):
    """a restated edit in the layout of a fixture's step"""
    idx, data, _ = a48xref.zip_paths(d.offset, d.n_edges, d.edges, a48xref.parse_hbv(d.a_hbv))
    return SimpleNamespace(a_hbv=d.a_hbv, a_inv=d.a_inv, offset=d.offset, n_edges=d.n_edges, edges=d.edges, pathsx=a48xref.pathsx_bytes(idx, data, len(d.n_edges)))


def _check_patch(seed, got, w, offset, counters=None):
    """w: the restatement's result, or a fixture (whose offsets are the int16 of the zip)"""
    to3_off, to3 = patchref.flat(w.to3) if isinstance(w.to3, list) else (w.to3_off, w.to3)
    assert got["a_hbv"] == w.a_hbv, (seed, "patched a.hbv")
    assert got["a_inv"] == w.a_inv and np.array_equal(got["inv"], np.frombuffer(w.a_inv, "<i4", offset=16)), (seed, "patched a.inv")
    assert np.array_equal(got["to3_off"], to3_off) and np.array_equal(got["to3"], to3), (seed, "to3")
    assert np.array_equal(got["left3"], w.left3), (seed, "left3")
    assert np.array_equal(got["edge"], w.edge), (seed, "translated paths: edges")
    assert np.array_equal(offset, w.offset), (seed, "translated paths: offsets")
    assert got["pathsx"] == w.pathsx, (seed, "a.pathsX bytes")
    if counters is not None:
        assert got["counters"] == counters, (seed, "counters", got["counters"], counters)


def _one(engine, seed, c, tmp_path) -> float:
    """every comparison of one case -> the seconds spent in the restatements"""
    import test_gpu_edit as E
    import test_gpu_patch as P
    t0 = time.perf_counter()
    m, ec = patchgen.patched(c), patchgen.edit_input(c)
    d, (support, hang) = patchgen.edited(c)
    trim = editref.delete_edges(ec.a_hbv, ec.inv, ec.offset, ec.n_edges, ec.edges, hang) if seed % 4 == 0 else None
    t_ref = time.perf_counter() - t0
    pinned = seed in patchgen.PINNED
    # ---- insert_patch
    inp = P._Input(c)
    before = [t.clone() for t in inp.tensors()]
    out = P._run(engine, inp)
    got = P._everything(engine, out, tmp_path, "a")
    _check_patch(seed, got, m, got["offset"], tuple(m.counters[k] for k in patchref.COUNTERS))
    if pinned:
        _check_patch((seed, "the reference"), got, patchref.golden(c.key), a48xref.wrap16(got["offset"]))
    assert all(bool((a == b).all()) for a, b in zip(before, inp.tensors())), (seed, "an input array of insert_patch changed")
    assert P._same(got, P._everything(engine, P._run(engine, inp), tmp_path, "b")), (seed, "two calls of insert_patch differ")
    if seed % 2 == 0:
        n = len(c.closures)
        for tag, order in (("r", np.arange(n)[::-1]), ("s", np.random.default_rng(n + c.K + seed).permutation(n))):
            assert P._same(got, P._everything(engine, P._run(engine, P._Input(c, order)), tmp_path, tag)), (seed, f"closure order {tag} gives another result")
    # ---- the edit, on the graph insert_patch returned
    graph = (c.K, out.h, out.unitig_off, out.unitig_bases, out.inv)
    paths = (P._dev(ec.offset, np.int32), P._dev(ec.n_edges.view(np.int32), np.int32), P._dev(ec.edges, np.int32))
    kept = [t.clone() for t in (out.unitig_off, out.unitig_bases, *paths)]
    inv_before = out.inv.copy()
    edit = lambda dels, tag: E._everything(engine, engine.delete_edges(graph, paths, dels), tmp_path, tag)
    egot = edit(ec.dels, "e")
    E._check(egot, _step(d), d, (seed, "edit"))
    if pinned:
        eg = editref.golden(c.key)
        assert eg.pinned
        E._check(egot, eg.steps[0], d, (seed, "edit, the reference"))
        assert np.array_equal(support, eg.support) and np.array_equal(hang, eg.hang_dels)
    assert E._same(egot, edit(ec.dels, "f")), (seed, "two calls of delete_edges differ")
    for tag, dels in (("u", np.unique(ec.dels)), ("v", np.unique(ec.dels)[::-1])):
        assert E._same(egot, edit(dels, tag)), (seed, f"dels order {tag} gives another result")
    # ---- the hanging-end selection on the patched graph
    E3 = len(out.inv)
    for leg in (None, "lds", "sort"):
        s, dl, stats = engine.hanging_ends(graph, paths, leg=leg)
        assert np.array_equal(s, support), (seed, "support", leg)
        assert np.array_equal(dl, hang), (seed, "hanging-end selection", leg, dl.tolist(), hang.tolist())
        assert stats["leg"] == (leg or ("lds" if E3 <= 16384 else "sort")) and stats["n_unsupported"] == int((support == 0).sum()), (seed, leg, stats)
    if trim is not None:
        t = engine.trim_hanging_ends(graph, paths)
        tgot = E._everything(engine, t, tmp_path, "t")
        assert np.array_equal(t.dels, hang) and np.array_equal(t.support, support), (seed, "trim: selection")
        E._check(tgot, _step(trim), trim, (seed, "trim"))
        assert E._same(tgot, edit(hang, "w")), (seed, "trim_hanging_ends is not delete_edges of its selection")
    assert all(bool((a == b).all()) for a, b in zip(kept, (out.unitig_off, out.unitig_bases, *paths))) and np.array_equal(out.inv, inv_before), (seed, "an input array of the edit changed")
    return t_ref


@pytest.mark.parametrize("block", range(N_CASES // BLOCK))
def test_fuzz_against_the_restatements(engine, block, tmp_path):
    made = 0
    t0, t_ref = time.perf_counter(), 0.0
    for seed in range(block * BLOCK, (block + 1) * BLOCK):
        t1 = time.perf_counter()
        c = patchgen.make_case(seed)
        t_ref += time.perf_counter() - t1
        if c is None:
            continue
        made += 1
        t_ref += _one(engine, seed, c, tmp_path)
    t = time.perf_counter() - t0
    print(f"patch fuzz block {block}: {made} cases, {t:.1f} s, of which the generator and the restatements {t_ref:.1f} s")
    assert made >= BLOCK - 1, made
