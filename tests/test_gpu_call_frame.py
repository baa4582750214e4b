"""The call frame of the device stages that run after the graph (csrc/snk_call.h): after any refusal *out is all zero and the context
goes on working; snk_dev_hbv's refusal of a short unitig; the one largest-edge-id kernel at every alignment of its input."""
import ctypes as C

import numpy as np
import pytest

import a48ref
import a48xref
import goldens
import pathgen
from test_gpu_pathsx import _dev, _walks, _zip

pytestmark = pytest.mark.gpu
SNK_E_ARG, SNK_E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def adv(snk):
    from supernova_amd import graphio
    c = goldens.load("adversarial")
    return a48xref.parse_hbv(c.exp_ahbv), graphio.unitigs_to_arrays(c.exp_unitigs)


def _fill(s):
    C.memset(C.addressof(s), 0xA5, C.sizeof(s))
    return s


def _raw(s):
    return C.string_at(C.addressof(s), C.sizeof(s))


def _all_zero(s):
    return _raw(s) == bytes(C.sizeof(s))


# ---- snk_dev_hbv: a unitig shorter than K
def _hbv_fields(h, nu):
    ne = h.n_edges
    arr = lambda p, m: np.ctypeslib.as_array(p, shape=(m,)).copy()
    return dict(n_vertices=h.n_vertices, n_edges=ne, v_left=arr(h.v_left, ne), v_right=arr(h.v_right, ne), src_unitig=arr(h.src_unitig, ne),
                is_rc=arr(h.is_rc, ne), fwd_xlat=arr(h.fwd_xlat, nu), rev_xlat=arr(h.rev_xlat, nu))


@pytest.mark.parametrize("K,short,valid", [(48, (48, 47, 60), (100, 60, 48)), (60, (60, 59, 61), (100, 61, 60))])
def test_hbv_refuses_a_short_unitig_and_goes_on(engine, K, short, valid):
    """Lengths K, K - 1 and more: SNK_E_ARG, every field of *out zero (no event, no host array left behind); the same engine then builds
    the graph of three valid unitigs (given in BVComp order: longest first), equal field by field to snk_hbv_from_unitigs."""
    from supernova_amd import lib as _lib
    e = engine
    rng = np.random.default_rng(K)
    err = C.create_string_buffer(512)

    def call(lens):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        bases = rng.integers(0, 4, int(off[-1]), dtype=np.uint8)
        d_off, d_bases = _dev(off.view(np.int64), np.int64), _dev(bases, np.uint8)
        h, ms = _fill(_lib.SnkHbv()), C.c_float(7.0)
        rc = e.lib.snk_dev_hbv(e._ctx, K, len(lens), d_off.data_ptr(), d_bases.data_ptr(), C.byref(h), C.byref(ms), e._stream(), err, 512)
        return rc, h, off, bases

    rc, h, _, _ = call(short)
    assert rc == SNK_E_ARG and b"a unitig is shorter than K" in err.value
    assert _all_zero(h)
    rc, h, off, bases = call(valid)
    assert rc == 0, err.value
    try:
        got = _hbv_fields(h, 3)
        assert np.ctypeslib.as_array(h.bvcomp_order, shape=(3,)).tolist() == [0, 1, 2]
    finally:
        e.lib.snk_hbv_free(C.byref(h))
    h2 = _lib.SnkHbv()
    assert e.lib.snk_hbv_from_unitigs(K, 3, off.ctypes.data, bases.ctypes.data, C.byref(h2), err, 512) == 0, err.value
    try:
        want = _hbv_fields(h2, 3)
    finally:
        e.lib.snk_hbv_free(C.byref(h2))
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# ---- *out after a refusal, one case per entry point
@pytest.fixture(scope="module")
def world(engine, tmp_path_factory):
    """The adversarial case on the device; the arrays of one good run of every stage, checked once against the reference's files."""
    from supernova_amd import graphio
    c = goldens.load("adversarial")
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    off, ne, edges, info = res.path_reads(rows, c.read_len, dq, lens=dl, mark_dups=True, bc=dbc, paths_index=True, pathsx=True)
    assert np.array_equal(ne, c.exp_path_n) and np.array_equal(edges, c.exp_path_edges) and np.array_equal(info["dups"]["dup"], c.exp_dup)
    d = tmp_path_factory.mktemp("a48")
    graphio.write_a48(d, 48, *graphio.unitigs_to_arrays(res.unitigs()), off, ne, edges, info)
    f6, fx = a48ref.load("adversarial"), a48xref.load("adversarial")
    for f, b in {"a.paths.inv": f6["a.paths.inv"], "a.countsb": f6["a.countsb"], "a.dup": f6["a.dup"], "a.pathsX": fx["a.pathsX"]}.items():
        assert (d / f).read_bytes() == b, f
    return dict(c=c, rows=rows, dq=dq, dl=dl, dbc=dbc, res=res, off=off, ne=ne, edges=edges, info=info)


def _reads(w):
    from supernova_amd import lib as _lib
    r = _lib.SnkDevReads()
    r.n_reads, r.rows, r.row_words, r.read_len = w["rows"].shape[0], w["rows"].data_ptr(), w["rows"].shape[1], w["c"].read_len
    r.quals, r.qstride, r.lens, r.bc = w["dq"].data_ptr(), w["dq"].shape[1], w["dl"].data_ptr(), w["dbc"].data_ptr()
    return r


@pytest.mark.parametrize("entry", ["path_reads2", "mark_dups", "paths_index", "paths_zip", "paths_unzip", "check_graph"])
def test_out_is_zero_after_a_refusal(engine, world, adv, entry):
    """*out comes in full of 0xA5; after the refusal every byte is zero (the report keeps struct_size), and a good call of the same
    entry point on the same engine gives what the reference gives."""
    from supernova_amd import graphio, lib as _lib
    e, w, res, c = engine, world, world["res"], world["c"]
    err = C.create_string_buffer(512)
    st = e._stream()
    nu = res.n_unitigs
    r = _reads(w)
    if entry == "check_graph":
        ci = _lib.SnkCheckInput()
        ci.K, ci.min_freq, ci.n_kmers, ci.keys, ci.counts, ci.ctx = 47, 3, res.n_kmers, res.raw.keys, res.raw.counts, res.raw.ctx
        ci.n_unitigs, ci.unitig_off, ci.unitig_bases = nu, res.raw.unitig_off, res.raw.unitig_bases
        rep = _fill(_lib.SnkCheckReport())
        rep.struct_size = C.sizeof(rep)
        assert e.lib.snk_dev_check_graph(e._ctx, C.byref(ci), None, C.byref(rep), st, err, 512) == SNK_E_UNSUPPORTED and b"K=47" in err.value
        want = _lib.SnkCheckReport()
        want.struct_size = C.sizeof(want)
        assert _raw(rep) == _raw(want)
        assert res.check()["violations"] == 0
        return
    h, ms = _lib.SnkHbv(), C.c_float(0)
    assert e.lib.snk_dev_hbv(e._ctx, 48, nu, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(ms), st, err, 512) == 0, err.value
    try:
        p = _fill(_lib.SnkDevPaths())
        if entry == "path_reads2":
            r.read_len = 0
            assert e.lib.snk_dev_path_reads2(e._ctx, 48, C.byref(r), nu, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), 0, C.byref(p), st, err, 512) == SNK_E_ARG
            assert b"packed rows" in err.value and _all_zero(p)
            r.read_len = c.read_len
        assert e.lib.snk_dev_path_reads2(e._ctx, 48, C.byref(r), nu, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), 0, C.byref(p), st, err, 512) == 0, err.value
        n, tot = int(p.n_reads), int(p.n_edges_total)
        if entry == "path_reads2":
            assert np.array_equal(res._dl(p.n_edges, n * 4, np.uint32, (n,)), c.exp_path_n)
            assert np.array_equal(res._dl(p.edges, tot * 4, np.int32, (tot,)), c.exp_path_edges)
        elif entry == "mark_dups":
            dd = _fill(_lib.SnkDevDups())
            r.n_reads, p.n_reads = n - 1, n - 1
            assert e.lib.snk_dev_mark_dups(e._ctx, C.byref(r), C.byref(p), C.byref(dd), st, err, 512) == SNK_E_ARG and b"odd" in err.value
            assert _all_zero(dd)
            r.n_reads, p.n_reads = n, n
            assert e.lib.snk_dev_mark_dups(e._ctx, C.byref(r), C.byref(p), C.byref(dd), st, err, 512) == 0, err.value
            assert np.array_equal(res._dl(dd.dup, n // 2, np.uint8, (n // 2,)), c.exp_dup)
        elif entry == "paths_index":
            inv, E = w["info"]["inv"], len(w["info"]["inv"])
            assert E > 2
            bad = inv.copy()
            bad[0] = bad[1] = 2
            px = _fill(_lib.SnkDevPidx())
            assert e.lib.snk_dev_paths_index(e._ctx, C.byref(p), E, bad.ctypes.data, C.byref(px), st, err, 512) == SNK_E_ARG and b"involution" in err.value
            assert _all_zero(px)
            assert e.lib.snk_dev_paths_index(e._ctx, C.byref(p), E, inv.ctypes.data, C.byref(px), st, err, 512) == 0, err.value
            assert np.array_equal(res._dl(px.index_off, (E + 1) * 8, np.uint64, (E + 1,)), w["info"]["paths_index"][0])
            assert np.array_equal(res._dl(px.index_ids, int(px.n_entries) * 8, np.uint64, (int(px.n_entries),)), w["info"]["paths_index"][1])
            assert np.array_equal(res._dl(px.counts, E * 4, np.int32, (E,)), w["info"]["countsb"])
    finally:
        e.lib.snk_hbv_free(C.byref(h))
    g, u = adv
    if entry == "paths_zip":
        with graphio.hbv_handle(48, *u) as hh:
            long_p = _lib.SnkDevPaths()
            d_off, d_ne, d_edges = _dev(np.zeros(1), np.int32), _dev([256], np.int32), _dev(np.zeros(256), np.int32)
            d_start = _dev([0, 256], np.int64)
            long_p.n_reads, long_p.n_edges_total = 1, 256
            long_p.offset, long_p.n_edges, long_p.start, long_p.edges = d_off.data_ptr(), d_ne.data_ptr(), d_start.data_ptr(), d_edges.data_ptr()
            zx = _fill(_lib.SnkDevPathsx())
            assert e.lib.snk_dev_paths_zip(e._ctx, C.byref(long_p), C.byref(hh), C.byref(zx), st, err, 512) == SNK_E_UNSUPPORTED and b"255" in err.value
            assert _all_zero(zx)
            index, data, _ = _zip(e, hh, w["off"], w["ne"], w["edges"])
        assert np.array_equal(index, w["info"]["pathsx"][0]) and np.array_equal(data, w["info"]["pathsx"][1])
    elif entry == "paths_unzip":
        index, data = w["info"]["pathsx"]
        d_index, d_data = _dev(index, np.int64), _dev(data, np.uint8)
        with graphio.hbv_handle(48, *u) as hh:
            zx = _lib.SnkDevPathsx()
            zx.n_reads, zx.n_bytes, zx.n_index = len(w["ne"]), len(data), len(index) - 1
            zx.data, zx.index = d_data.data_ptr(), d_index.data_ptr()
            out = _fill(_lib.SnkDevPaths())
            assert e.lib.snk_dev_paths_unzip(e._ctx, C.byref(zx), C.byref(hh), C.byref(out), st, err, 512) == SNK_E_ARG and b"index entries" in err.value
            assert _all_zero(out)
            _, u_ne, u_edges, _ = e.unzip_paths(hh, d_index, d_data, len(w["ne"]))
        assert np.array_equal(u_ne, c.exp_path_n) and np.array_equal(u_edges, c.exp_path_edges)


# ---- the one largest-edge-id kernel: head peel, uint4 interior, tail peel
RANGE_N = [1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025]


class _NoJumps:
    """_walks' generator with its occasional random step switched off: only a dead end still makes one"""
    def __init__(self, rng):
        self.integers = rng.integers

    def random(self):
        return 1.0


@pytest.fixture(scope="module")
def range_cases(adv):
    """For every n, n path entries as walks of at most five edges (_walks); a walk that met a dead end is drawn again, so every step is
    one of the graph: the restatement reports n_steps_not_found == 0 for every in-range case, checked here on the CPU.  (The refused
    half never reaches the encoder.)"""
    g, _ = adv
    rng = _NoJumps(np.random.default_rng(77))
    out = {}
    for n in RANGE_N:
        ne = np.array([5] * (n // 5) + ([n % 5] if n % 5 else []), np.int64)
        walks = []
        for m in ne:
            for _ in range(1000):
                w = _walks(rng, g, [m])
                if a48xref.zip_paths(np.zeros(1, np.int32), np.array([m]), w, g)[2]["n_steps_not_found"] == 0:
                    break
            walks.append(w)
        edges, off = np.concatenate(walks), np.zeros(len(ne), np.int32)
        index, data, stats = a48xref.zip_paths(off, ne, edges, g)
        assert stats["n_steps_not_found"] == 0 and len(edges) == n
        out[n] = (off, ne, edges, index, data)
    return out


def _zip_at(engine, h, off, ne, edges, shift):
    """edges handed over as a slice whose first element sits `shift` words past a 16-byte boundary"""
    import torch
    buf = torch.zeros(len(edges) + 8, dtype=torch.int32, device=torch.device("cuda", 0))
    lead = (-(buf.data_ptr() // 4)) % 4 + shift
    view = buf[lead:lead + len(edges)]
    view.copy_(torch.from_numpy(np.asarray(edges, np.int32)))
    assert view.data_ptr() % 16 == 4 * shift
    return engine.zip_paths(h, _dev(off, np.int32), _dev(np.asarray(ne, np.uint32).view(np.int32), np.int32), view)


@pytest.mark.parametrize("n", RANGE_N)
def test_largest_edge_id_at_every_alignment(engine, adv, range_cases, n):
    from supernova_amd import graphio, lib as _lib
    g, u = adv
    off, ne, edges, x_index, x_data = range_cases[n]
    with graphio.hbv_handle(48, *u) as h:
        for shift in range(4):
            index, data, stats = _zip_at(engine, h, off, ne, edges, shift)
            assert np.array_equal(index, x_index) and np.array_equal(data, x_data) and stats["n_steps_not_found"] == 0
            for at in sorted({0, n // 2, n - 1}):
                bad = edges.copy()
                bad[at] = g.E
                with pytest.raises(_lib.SnkError) as ei:
                    _zip_at(engine, h, off, ne, bad, shift)
                assert ei.value.code == SNK_E_ARG and f"edge id {g.E}," in str(ei.value), (shift, at, str(ei.value))


@pytest.mark.parametrize("n", [1, 5, 1025])
def test_paths_index_refuses_the_bad_edge_id_wherever_it_sits(engine, adv, range_cases, n):
    from supernova_amd import lib as _lib
    g, _ = adv
    _, ne, edges, _, _ = range_cases[n]
    inv = np.arange(g.E, dtype=np.int32)                                      # (an involution; which one does not matter to the refusal)
    err = C.create_string_buffer(512)
    d_ne = _dev(ne, np.int32)
    d_start = _dev(np.concatenate([[0], np.cumsum(ne)]), np.int64)
    for at in sorted({0, n // 2, n - 1}) + [None]:
        a = edges.copy()
        if at is not None:
            a[at] = g.E
        d_edges = _dev(a, np.int32)
        assert d_edges.data_ptr() % 16 == 0
        p = _lib.SnkDevPaths()
        p.n_reads, p.n_edges_total, p.n_edges, p.start, p.edges = len(ne), n, d_ne.data_ptr(), d_start.data_ptr(), d_edges.data_ptr()
        px = _lib.SnkDevPidx()
        rc = engine.lib.snk_dev_paths_index(engine._ctx, C.byref(p), g.E, inv.ctypes.data, C.byref(px), engine._stream(), err, 512)
        if at is None:
            assert rc == 0 and int(px.n_entries) == n, err.value
        else:
            assert rc == SNK_E_ARG and f"edge id {g.E},".encode() in err.value, (at, err.value)
