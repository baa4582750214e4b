"""snk_dev_hbv and snk_dev_bv_image (csrc/snk_hbv.hip, csrc/snk_host.hip) on hand-made unitig sets (tests/handunitigs.py): every case, K = 48
and 60, in three input orders, under the host flood and three device floods (hbv_strict: a device flood that gives up fails the call
instead of handing the graph to the host).  Expected values: the reference's (tests/golden/hbv/) where a fixture is kept, else the
oracle's, which tests/test_hbv_handmade_host.py pins to the reference.  Every comparison is exact; snk_ctx_last_hbv_flood has to confirm
the flood that was asked for and how many components went to device threads and to host threads."""
import ctypes as C

import numpy as np
import pytest

import handunitigs as hu
from devcall import _dev, _zeroed, download

pytestmark = pytest.mark.gpu
SNK_E_ARG = -1
FLOODS = {"host": dict(hbv_dev_min=1_000_000_000),                                # the sequential flood over the downloaded classes
          "device": dict(hbv_dev_min=0, hbv_strict=1),                            # one thread floods one component; above 1024 nodes the host's threads
          "device_big4": dict(hbv_dev_min=0, hbv_big=4, hbv_strict=1),            # above 4 nodes
          "device_big0": dict(hbv_dev_min=0, hbv_big=0, hbv_strict=1)}            # every component goes to the host's threads
BIG = {"device": 1024, "device_big4": 4, "device_big0": 0}


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


class _Unitigs:
    def __init__(self, off, bases):
        self.U = len(off) - 1
        self.d_off, self.d_bases = _dev(off.view(np.int64), np.int64), _dev(bases if len(bases) else np.zeros(1, np.uint8), np.uint8)


class HbvCall:
    """One call of snk_dev_hbv on unitigs uploaded as they are.  *out comes in full of 0xA5."""

    def __init__(self, engine, K, off, bases):
        from supernova_amd import lib as _lib
        self.u = _Unitigs(off, bases)
        out = self.out = _lib.SnkHbv()
        C.memset(C.addressof(out), 0xA5, C.sizeof(out))
        self.err = C.create_string_buffer(512)
        ms = C.c_float(0)
        self.rc = engine.lib.snk_dev_hbv(engine._ctx, K, self.u.U, self.u.d_off.data_ptr(), self.u.d_bases.data_ptr(), C.byref(out), C.byref(ms), engine._stream(), self.err, 512)
        dev, host = C.c_uint64(99), C.c_uint64(99)
        self.flood = (int(engine.lib.snk_ctx_last_hbv_flood(engine._ctx, C.byref(dev), C.byref(host))), int(dev.value), int(host.value))
        self.hbv = self.order = None
        if self.rc == 0:
            ne, nu = out.n_edges, self.u.U
            arr = lambda p, m, dt: np.array(np.ctypeslib.as_array(p, shape=(m,)), dtype=dt, copy=True) if m else np.zeros(0, dt)
            self.hbv = dict(n_vertices=out.n_vertices, n_edges=ne, v_left=arr(out.v_left, ne, np.int32), v_right=arr(out.v_right, ne, np.int32),
                            src=arr(out.src_unitig, ne, np.int32), is_rc=arr(out.is_rc, ne, np.uint8), fwd=arr(out.fwd_xlat, nu, np.int32), rev=arr(out.rev_xlat, nu, np.int32))
            self.order = arr(out.bvcomp_order, nu, np.int32)
            engine.lib.snk_hbv_free(C.byref(out))


def _good(call, c, perm, flood):
    assert call.rc == 0, call.err.value
    assert np.array_equal(call.order, np.argsort(perm)), "bvcomp_order"             # the input's unitig i is rank perm[i]
    exp = hu.expected(c)
    assert hu.same_graph(call.hbv, exp) is None, hu.same_graph(call.hbv, exp)
    n = len(c.facts["components"])
    want = (0, 0, n) if flood == "host" else (1,) + hu.flood_split(c.facts, BIG[flood])
    assert call.flood == want, (call.flood, want)


@pytest.mark.parametrize("flood", list(FLOODS))
@pytest.mark.parametrize("K", hu.KS)
@pytest.mark.parametrize("name", hu.CASES)
def test_dev_hbv(engine, tune, name, K, flood):
    for k, v in FLOODS[flood].items():
        tune(k, v)
    c = hu.case(name, K)
    first = None
    for oname, perm in hu.orders(c).items():
        call = HbvCall(engine, K, *hu.reordered(c, perm))
        _good(call, c, perm, flood)
        first = first or call
        assert hu.same_graph(call.hbv, first.hbv) is None, (oname, hu.same_graph(call.hbv, first.hbv))


@pytest.mark.parametrize("K", hu.KS)
def test_components_on_either_side_of_hbv_big(engine, tune, K):
    """a chain is one component of N nodes per strand: N = hbv_big is flooded by a device thread, N = hbv_big + 1 by a host thread"""
    tune("hbv_dev_min", 0)
    tune("hbv_strict", 1)
    for name, big, want in (("chain_1024", None, (1, 2, 0)), ("chain_1025", None, (1, 0, 2)), ("chain_1023", None, (1, 2, 0)),
                            ("chain_4", 4, (1, 2, 0)), ("chain_5", 4, (1, 0, 2)), ("chain_2", 4, (1, 2, 0))):
        if big is not None:
            tune("hbv_big", big)
        c = hu.case(name, K)
        assert c.facts["components"] == [c.facts["U"]] * 2
        call = HbvCall(engine, K, c.off, c.bases)
        assert call.rc == 0 and call.flood == want, (name, call.flood, call.err.value)
        assert hu.same_graph(call.hbv, hu.expected(c)) is None


def _image(engine, K, off, bases, by_first_kmer):
    u = _Unitigs(off, bases)
    d_img, nb = C.c_void_p(0), C.c_uint64(0)
    err = C.create_string_buffer(512)
    rc = engine.lib.snk_dev_bv_image(engine._ctx, K, u.U, u.d_off.data_ptr(), u.d_bases.data_ptr(), by_first_kmer, C.byref(d_img), C.byref(nb), engine._stream(), err, 512)
    assert rc == 0, err.value
    return download(engine, d_img.value, int(nb.value), np.uint8).tobytes()


@pytest.mark.parametrize("K", hu.KS)
@pytest.mark.parametrize("name", hu.CASES)
def test_dev_bv_image(engine, tmp_path, name, K):
    """by_first_kmer = 0 on the three input orders, by_first_kmer = 1 on the input sorted by its first K bases: the bytes of the reference's
    edges.bv (or of the oracle's writer)"""
    c = hu.case(name, K)
    want = hu.golden(c).edges_bv if name in hu.SAVED else hu.oracle_bv(c, tmp_path / "oracle.bv")
    for oname, perm in hu.orders(c).items():
        assert _image(engine, K, *hu.reordered(c, perm), 0) == want, oname
    by_first = np.array(sorted(range(len(c.unitigs)), key=lambda i: c.unitigs[i][:K]))
    assert name not in ("long", "forest_257", "mixed_seed1") or not np.array_equal(by_first, np.arange(len(c.unitigs)))         # (not BVComp order itself)
    assert _image(engine, K, *hu.reordered(c, by_first), 1) == want


@pytest.mark.parametrize("flood", ["host", "device"])
@pytest.mark.parametrize("short", ["K-1", "3"])
@pytest.mark.parametrize("K", hu.KS)
def test_result_rule_and_reuse(engine, tune, K, short, flood):
    """A unitig shorter than K in the middle: SNK_E_ARG, *out all zero, no flood reported; the next call on the context gives the right
    graph, and so does the one after it."""
    for k, v in FLOODS[flood].items():
        tune(k, v)
    c = hu.case("forest_257", K)
    us = list(c.unitigs)
    us[128] = us[128][:K - 1 if short == "K-1" else 3]
    bad = HbvCall(engine, K, *hu.to_arrays(us))
    assert bad.rc == SNK_E_ARG and b"shorter than K" in bad.err.value
    assert _zeroed(bad.out) and bad.flood == (0, 0, 0)
    perm = hu.orders(c)["shuffled"]
    a = HbvCall(engine, K, *hu.reordered(c, perm))
    _good(a, c, perm, flood)
    b = HbvCall(engine, K, *hu.reordered(c, perm))
    _good(b, c, perm, flood)
    assert hu.same_graph(a.hbv, b.hbv) is None and np.array_equal(a.order, b.order)
    none = HbvCall(engine, K, np.zeros(1, np.uint64), np.zeros(0, np.uint8))            # no unitigs: nothing, and no flood reported
    assert none.rc == 0 and (none.out.n_vertices, none.out.n_edges) == (0, 0) and none.flood == (0, 0, 0)
