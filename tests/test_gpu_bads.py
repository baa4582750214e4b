"""MarkBads on the device (snk_dev_mark_bads, snk_dev_mark_bads_df: 10X/SecretOps.cc:22-59, :70-107).  Bar: the pair flags equal what the
reference's own two overloads wrote (tests/golden/bads/), the counters equal those of the Python restatement that test_bads_host.py pins
to the same flags, and the form that decodes the stage's files again gives the resident form's bytes."""
import ctypes as C
import struct

import numpy as np
import pytest

import badsref
import goldens
import handbads
import pathgen

pytestmark = pytest.mark.gpu
SNK_E_ARG, SNK_E_UNSUPPORTED = -1, -6
MODES = (False, True)


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


class _Graph:
    """a case's unitigs on the device, and its reads"""

    def __init__(self, c, codes=None, quals=None, lens=None):
        from supernova_amd import graphio
        self.c = c
        self.u = graphio.unitigs_to_arrays(c.unitigs)
        self.d_off, self.d_bases = _dev(self.u[0].astype(np.int64), np.int64), _dev(self.u[1], np.uint8)
        codes, quals, lens = (c.codes if codes is None else codes), (c.quals if quals is None else quals), (c.lens if lens is None else lens)
        self.L = codes.shape[1]
        self.rows, self.quals, self.lens, _ = pathgen.to_device(codes, quals, lens, np.zeros(len(lens), np.int32))


_graphs: dict = {}


def _graph(name) -> _Graph:
    if name not in _graphs:
        _graphs[name] = _Graph(badsref.load(name))
    return _graphs[name]


def _dpaths(paths):
    off, ne, edges = paths
    return (_dev(off, np.int32), _dev(np.asarray(ne, np.uint32).view(np.int32), np.int32), _dev(edges if len(edges) else np.zeros(1, np.int32), np.int32)[:len(edges)])


def _take(paths, sel):
    """the paths of the reads `sel`, in that order"""
    off, ne, edges = paths
    start = np.concatenate([[0], np.cumsum(ne.astype(np.int64))])
    sel = np.asarray(sel, np.int64)
    e = np.concatenate([edges[start[r]:start[r + 1]] for r in sel]) if len(sel) else np.zeros(0, np.int32)
    return off[sel].astype(np.int32), ne[sel].astype(np.uint32), e.astype(np.int32)


def _modes(name):
    return (False,) if name in badsref.HAND_PLAIN else MODES


@pytest.mark.parametrize("name", badsref.ALL)
def test_flags_match_the_reference(engine, name):
    """Every fixture, both overloads: bad equals the reference's flags, the counters the restatement's; the inputs are untouched; a second
    call gives the same bytes."""
    from supernova_amd import graphio
    c, G = badsref.load(name), _graph(name)
    with graphio.hbv_handle(c.K, *G.u) as h:
        for x in _modes(name):
            want = c.bad_x if x else c.bad_plain
            cnt = badsref.restated(name, x)[1]
            d_in = _dpaths(c.paths)
            before = [t.clone() for t in (G.rows, G.quals, G.lens, G.d_off, G.d_bases)]
            bad, stats = engine.mark_bads(c.K, h, G.d_off, G.d_bases, G.rows, G.L, G.quals, G.lens, *d_in, x=x)
            assert bad.dtype == np.uint8 and np.array_equal(bad, want), (x, np.nonzero(bad != want)[0][:5])
            assert {k: stats[k] for k in cnt} == cnt, (x, stats)
            assert stats["n_pairs"] == len(want) and stats["n_slabs"] == 1 and stats["ms"] > 0
            for a, b in zip(d_in, c.paths):
                assert np.array_equal(a.cpu().numpy().view(b.dtype), b), "the input paths changed"
            for a, b in zip(before, (G.rows, G.quals, G.lens, G.d_off, G.d_bases)):
                assert bool((a == b).all()), "the reads or the unitigs changed"
            again, stats2 = engine.mark_bads(c.K, h, G.d_off, G.d_bases, G.rows, G.L, G.quals, G.lens, *d_in, x=x)
            assert again.tobytes() == bad.tobytes() and {k: stats2[k] for k in cnt} == cnt


@pytest.mark.parametrize("K", (48, 60))
def test_hand_made_pairs_by_name(engine, K):
    """the stated flag of every hand-made pair, by name, in both modes (a mutation of the threshold or of the junction shows here)"""
    from supernova_amd import graphio
    for name, modes in ((f"hand_k{K}", MODES), (f"handplain_k{K}", (False,))):
        c, G = badsref.load(name), _graph(name)
        with graphio.hbv_handle(K, *G.u) as h:
            for x in modes:
                bad, _ = engine.mark_bads(K, h, G.d_off, G.d_bases, G.rows, G.L, G.quals, G.lens, *_dpaths(c.paths), x=x)
                wrong = [p.name for i, p in enumerate(c.pairs) if bool(bad[i]) != (p.x if x else p.plain)]
                assert not wrong, (name, x, wrong)


def test_quality_255_on_a_fully_mismatching_read(engine):
    """256 bases, every one a mismatch at quality 255 (more than the reference's PQVec takes, so against the restatement): the sum is
    65 280 and nothing overflows; the same read at quality 0 is not bad."""
    from supernova_amd import graphio
    c = badsref.load("hand_k48")
    i = [p.name for p in c.pairs].index("all_mismatch_top_quality")
    sel = [2 * i, 2 * i + 1]
    for q, flag in ((255, 1), (0, 0)):
        quals = c.quals[sel].copy()
        quals[0, :] = q
        G = _Graph(c, c.codes[sel], quals, c.lens[sel])
        paths = _take(c.paths, sel)
        sums: list = []
        want, cnt = badsref.mark_bads(c.g, c.eb, c.codes[sel], c.lens[sel], quals, *paths, False, sums)
        assert sums[0] == 256 * q and want[0] == flag
        with graphio.hbv_handle(48, *G.u) as h:
            for x in MODES:
                bad, stats = engine.mark_bads(48, h, G.d_off, G.d_bases, G.rows, G.L, G.quals, G.lens, *_dpaths(paths), x=x)
                assert bad.tolist() == [flag] and {k: stats[k] for k in cnt} == cnt


@pytest.mark.parametrize("name,x", [("adversarial_cut", True), ("hand_k60", False), ("synth_4k_dups_cut", False)])
def test_pairs_are_independent(engine, name, x):
    """The pairs in a permuted order give the correspondingly permuted flags, and so does a slice that ends inside a workgroup's share."""
    from supernova_amd import graphio
    import torch
    c, G = badsref.load(name), _graph(name)
    want = c.bad_x if x else c.bad_plain
    n_pairs = len(want)
    rng = np.random.default_rng(11)
    with graphio.hbv_handle(c.K, *G.u) as h:
        for pp in (rng.permutation(n_pairs), np.arange(min(n_pairs, 33)), np.arange(1)):
            sel = np.stack([2 * pp, 2 * pp + 1], 1).reshape(-1)
            idx = torch.from_numpy(sel.astype(np.int64)).to(G.rows.device)
            bad, _ = engine.mark_bads(c.K, h, G.d_off, G.d_bases, G.rows[idx].contiguous(), G.L, G.quals[idx].contiguous(), G.lens[idx].contiguous(),
                                      *_dpaths(_take(c.paths, sel)), x=x)
            assert np.array_equal(bad, want[pp]), len(pp)


# ---- the form that decodes the stage's files again

def _triple(tmp_path, c):
    from supernova_amd import dfin, synth
    dfin.write_df(tmp_path / "reads", synth.pack_rows(c.codes), c.quals, bc=np.zeros(len(c.lens), np.int32), lens=c.lens)
    return dfin.DfFiles(tmp_path / "reads")


@pytest.mark.parametrize("name", ["adversarial_cut", "hand_k48"])
def test_df_form_gives_the_resident_bytes(engine, tmp_path, name):
    """On a triple written with snk_write_df: slab_reads 2 (the ring takes 16 at least), 64 and 0, a partial last slab, a range that starts
    behind read 0 -- every time the bytes and counters of the resident form on the same reads, in both modes."""
    from supernova_amd import graphio
    c, G = badsref.load(name), _graph(name)
    n = len(c.lens)
    assert c.quals.max() <= 63
    ranges = [(0, n, 0), (0, n, 64), (0, min(n, 2006), 2), (100, min(n, 2006) - 100 - 2, 64)] if n > 200 else [(0, n, 0), (0, n, 2), (0, n, 64), (10, n - 20, 2)]
    with _triple(tmp_path, c) as files, graphio.hbv_handle(c.K, *G.u) as h:
        assert files.n_reads == n
        for first, m, slab in ranges:
            assert first % 2 == 0 and m % 2 == 0 and (slab == 0 or m % max(slab, 16) != 0 or m == n)
            sel = np.arange(first, first + m)
            paths = _take(c.paths, sel)
            for x in MODES:
                res, st = engine.mark_bads(c.K, h, G.d_off, G.d_bases, G.rows[first:first + m].contiguous(), G.L, G.quals[first:first + m].contiguous(),
                                           G.lens[first:first + m].contiguous(), *_dpaths(paths), x=x)
                want = (c.bad_x if x else c.bad_plain)[first // 2:(first + m) // 2]
                assert np.array_equal(res, want)
                bad, sd = engine.mark_bads_df(c.K, h, G.d_off, G.d_bases, files, *_dpaths(paths), first=first, n=m, slab_reads=slab, x=x)
                assert bad.tobytes() == res.tobytes(), (first, m, slab, x, np.nonzero(bad != res)[0][:5])
                assert {k: sd[k] for k in badsref.COUNTERS} == {k: st[k] for k in badsref.COUNTERS}
                assert sd["n_slabs"] == -(-m // (max(slab, 16) if slab else 262144)) and sd["n_pairs"] == m // 2


# ---- refusals

def _raw(engine, G, h, paths, flags=0, start=None, n_total=None, quals=..., read_len=None, n_reads=None, p_reads=None):
    """the C call itself -> (rc, message, SnkDevBads)"""
    from supernova_amd import lib as _lib
    off, ne, edges = paths
    n = len(ne)
    d = (_dev(off, np.int32), _dev(np.asarray(ne, np.uint32).view(np.int32), np.int32), _dev(edges if len(edges) else np.zeros(1, np.int32), np.int32),
         _dev(np.concatenate([[0], np.cumsum(np.asarray(ne, np.int64))]) if start is None else start, np.int64))
    r = _lib.SnkDevReads()
    r.n_reads, r.rows, r.row_words, r.read_len = (n if n_reads is None else n_reads), G.rows.data_ptr(), G.rows.shape[1], G.L if read_len is None else read_len
    r.quals, r.qstride = (G.quals.data_ptr() if quals is ... else quals), G.quals.shape[1]
    r.lens = G.lens.data_ptr()
    p = _lib.SnkDevPaths()
    p.n_reads, p.n_edges_total = (n if p_reads is None else p_reads), len(edges) if n_total is None else n_total
    p.offset, p.n_edges, p.edges, p.start = d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr()
    b = _lib.SnkDevBads()
    C.memset(C.byref(b), 0xAB, C.sizeof(b))
    err = C.create_string_buffer(512)
    rc = engine.lib.snk_dev_mark_bads(engine._ctx, G.c.K, C.byref(r), len(G.u[0]) - 1, G.d_off.data_ptr(), G.d_bases.data_ptr(), C.byref(h), C.byref(p), flags,
                                      C.byref(b), engine._stream(), err, 512)
    return rc, err.value.decode(errors="replace"), b, d


def _all_zero(x) -> bool:
    return bytes(x) == bytes(C.sizeof(x))


def test_refusals(engine, tmp_path):
    """Every refusal returns its code with *out all zero; the call after it works."""
    from supernova_amd import graphio, lib as _lib
    c, G = badsref.load("hand_k48"), _graph("hand_k48")
    n = len(c.lens)
    bad_start = np.concatenate([[0], np.cumsum(c.paths[1].astype(np.int64))])
    bad_start[5] += 1
    with graphio.hbv_handle(48, *G.u) as h:
        cases = [
            ("odd n_reads", _take(c.paths, np.arange(n - 1)), {}, SNK_E_ARG),
            ("paths for other reads", c.paths, dict(p_reads=n - 2), SNK_E_ARG),
            ("edge id outside", (c.paths[0], c.paths[1], np.where(np.arange(len(c.paths[2])) == 3, c.g.E, c.paths[2]).astype(np.int32)), {}, SNK_E_ARG),
            ("negative edge id", (c.paths[0], c.paths[1], np.where(np.arange(len(c.paths[2])) == 0, -1, c.paths[2]).astype(np.int32)), {}, SNK_E_ARG),
            ("table", c.paths, dict(n_total=len(c.paths[2]) - 1), SNK_E_ARG),
            ("start with a gap", c.paths, dict(start=bad_start), SNK_E_ARG),
            ("quals NULL", c.paths, dict(quals=None), SNK_E_ARG),
            ("read_len", c.paths, dict(read_len=257), SNK_E_ARG),
            ("flags", c.paths, dict(flags=2), SNK_E_ARG),
        ]
        for what, paths, kw, code in cases:
            for flags in ((kw.get("flags"),) if "flags" in kw else (0, _lib.BADS_X)):
                rc, msg, b, _ = _raw(engine, G, h, paths, **dict(kw, flags=flags))
                assert rc == code and msg and _all_zero(b), (what, flags, rc, msg)
        rc, msg, b, _ = _raw(engine, G, h, c.paths, flags=_lib.BADS_X)
        assert rc == 0 and b.n_bad_pairs == int(c.bad_x.sum()) and b.n_pairs == n // 2, msg
        # no reads at all
        E = _Graph(c, c.codes[:0], c.quals[:0], c.lens[:0])
        rc, msg, b, _ = _raw(engine, E, h, (np.zeros(0, np.int32), np.zeros(0, np.uint32), np.zeros(0, np.int32)))
        assert rc == 0 and b.n_pairs == 0 and b.n_placed == 0, msg
    # what a ReadPathVecX cannot hold: refused with SNK_BADS_X only
    cp, hp = badsref.load("handplain_k48"), handbads.case(48, plain_only=True)
    with graphio.hbv_handle(48, *graphio.unitigs_to_arrays(cp.unitigs)) as h:
        for only, code in ((("nonadjacent_later_wins",), SNK_E_ARG), (("path_256_edges_151",), SNK_E_UNSUPPORTED)):
            codes, quals, lens, paths = handbads.arrays(hp, handbads.edge_index(cp.eb), only=only)
            Gp = _Graph(cp, codes, quals, lens)
            rc, msg, b, _ = _raw(engine, Gp, h, paths, flags=_lib.BADS_X)
            assert rc == code and msg and _all_zero(b), (only, rc, msg)
            rc, msg, b, _ = _raw(engine, Gp, h, paths)
            assert rc == 0 and b.n_pairs == 1, msg
    # the _df form: an odd first, an odd slab_reads, an odd n, unknown flags
    with _triple(tmp_path, c) as files, graphio.hbv_handle(48, *G.u) as h:
        for what, first, m, slab, x_flag in (("odd first", 1, 10, 64, 0), ("odd slab_reads", 0, 10, 63, 0), ("odd n", 0, 9, 64, 0), ("flags", 0, 10, 64, 2)):
            paths = _take(c.paths, np.arange(first, first + m))
            d = _dpaths(paths)
            p, _keep = engine._paths_struct(*d, None)
            b = _lib.SnkDevBads()
            C.memset(C.byref(b), 0xAB, C.sizeof(b))
            err = C.create_string_buffer(512)
            rc = engine.lib.snk_dev_mark_bads_df(engine._ctx, 48, files._h, first, m, 0, 0, slab, len(G.u[0]) - 1, G.d_off.data_ptr(), G.d_bases.data_ptr(), C.byref(h),
                                                 C.byref(p), x_flag, C.byref(b), err, 512)
            assert rc == SNK_E_ARG and err.value and _all_zero(b), (what, rc, err.value)


# ---- with the stages around it

def test_path_reads_result_stays_and_write_bad_gives_the_file(engine, tmp_path):
    """count + graph + paths + MarkBads in one path_reads call on the adversarial case (the device's paths ARE the reference's:
    test_gpu_paths.py): the flags are the fixture's; with download=False the flags stay on the device and write_bad after a download
    writes the fixture's bytes; the paths of the call are byte-unchanged by a MarkBads run over them."""
    from supernova_amd import graphio, lib as _lib
    import devcall
    c = goldens.load("adversarial")
    fx = badsref.load("adversarial")
    cut = badsref.load("adversarial_cut")
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    off, ne, edges, info = res.path_reads(rows, c.read_len, dq, lens=dl, mark_bads="x")
    assert np.array_equal(off, fx.paths[0]) and np.array_equal(ne, fx.paths[1]) and np.array_equal(edges, fx.paths[2])
    cnt = badsref.restated("adversarial", True)[1]
    assert np.array_equal(info["bads"]["bad"], fx.bad_x) and {k: info["bads"][k] for k in cnt} == cnt
    _, _, _, info0 = res.path_reads(rows, c.read_len, dq, lens=dl, mark_bads=True, download=False)
    assert "bad" not in info0["bads"] and {k: info0["bads"][k] for k in cnt} == badsref.restated("adversarial", False)[1]
    dev = info0["bads_dev"]
    graphio.write_bad(tmp_path / "a.bad", devcall.download(engine, dev.bad, int(dev.n_pairs), np.uint8))
    want = b"BINWRITE" + struct.pack("<Q", len(fx.bad_plain)) + fx.bad_plain.tobytes()
    assert (tmp_path / "a.bad").read_bytes() == want
    # Engine.mark_bads with download=False over the cut paths on the result's own unitigs: flags that are not all zero
    u = graphio.unitigs_to_arrays(c.exp_unitigs)
    with graphio.hbv_handle(48, *u) as h:
        d_off, d_bases = _dev(u[0].astype(np.int64), np.int64), _dev(u[1], np.uint8)
        d_in = _dpaths(cut.paths)
        b, stats = engine.mark_bads(48, h, d_off, d_bases, rows, c.read_len, dq, dl, *d_in, x=True, download=False)
        assert isinstance(b, _lib.SnkDevBads) and stats["n_bad_pairs"] == int(cut.bad_x.sum()) > 0
        graphio.write_bad(tmp_path / "cut.bad", devcall.download(engine, b.bad, int(b.n_pairs), np.uint8))
        assert (tmp_path / "cut.bad").read_bytes() == b"BINWRITE" + struct.pack("<Q", len(cut.bad_x)) + cut.bad_x.tobytes()
        for a, w in zip(d_in, cut.paths):
            assert np.array_equal(a.cpu().numpy().view(w.dtype), w)


def test_a_preceding_path_reads_result_is_unchanged(engine):
    """snk_dev_path_reads, then snk_dev_mark_bads on its device arrays: the paths read back before and after are the same bytes."""
    from supernova_amd import lib as _lib
    import devcall
    c = goldens.load("synth_4k_dups")
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    e = engine
    h, ms, err = _lib.SnkHbv(), C.c_float(0), C.create_string_buffer(512)
    assert e.lib.snk_dev_hbv(e._ctx, 48, res.n_unitigs, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(ms), e._stream(), err, 512) == 0, err.value
    try:
        r = _lib.SnkDevReads()
        r.n_reads, r.rows, r.row_words, r.read_len = rows.shape[0], rows.data_ptr(), rows.shape[1], c.read_len
        r.quals, r.qstride, r.lens = dq.data_ptr(), dq.shape[1], dl.data_ptr()
        out = _lib.SnkDevPaths()
        assert e.lib.snk_dev_path_reads(e._ctx, 48, C.byref(r), res.n_unitigs, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(out), e._stream(), err, 512) == 0, err.value
        n, tot = int(out.n_reads), int(out.n_edges_total)
        snap = lambda: [devcall.download(e, p, k, dt).tobytes() for p, k, dt in ((out.offset, n, np.int32), (out.n_edges, n, np.uint32), (out.start, n + 1, np.uint64),
                                                                                 (out.edges, tot, np.int32))]
        before = snap()
        unitigs_before = devcall.download(e, res.raw.unitig_bases, int(res.raw.unitig_total_bases), np.uint8).tobytes()
        for flags in (0, _lib.BADS_X):
            b = _lib.SnkDevBads()
            assert e.lib.snk_dev_mark_bads(e._ctx, 48, C.byref(r), res.n_unitigs, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(out), flags, C.byref(b),
                                           e._stream(), err, 512) == 0, err.value
            assert b.n_pairs == n // 2 and b.n_placed == int((np.frombuffer(before[1], np.uint32) > 0).sum())
            assert snap() == before
        assert devcall.download(e, res.raw.unitig_bases, int(res.raw.unitig_total_bases), np.uint8).tobytes() == unitigs_before
    finally:
        e.lib.snk_hbv_free(C.byref(h))
