"""Path extension on the device (snk_dev_extend_paths: ExtendPathsNew, 10X/Extend.cc:14-177).  Bar: the paths, and their a.pathsX bytes
through snk_dev_paths_zip, equal what the reference's own function wrote (tests/golden/ext/), for both flags; the counters equal those of
the Python restatement that test_extend_host.py pins to the same bytes."""
import ctypes as C

import numpy as np
import pytest

import a48xref
import extref
import goldens
import pathgen

pytestmark = pytest.mark.gpu
SNK_E_ARG, SNK_E_UNSUPPORTED = -1, -6
SLICES = (0, 1, 15, 16, 17, 255, 256, 257)


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

    def __init__(self, c):
        from supernova_amd import graphio
        self.c = c
        self.u = graphio.unitigs_to_arrays(c.unitigs)
        self.d_off, self.d_bases = _dev(self.u[0].astype(np.int64), np.int64), _dev(self.u[1], np.uint8)
        self.L = c.codes.shape[1]
        self.rows, self.quals, self.lens, _ = pathgen.to_device(c.codes, c.quals, c.lens, np.zeros(len(c.lens), np.int32))


_graphs: dict = {}


def _graph(name) -> _Graph:
    c = extref.load(name)
    key = name if name in extref.HAND else name.replace("_cut", "").replace("_first", "")
    if key not in _graphs:
        _graphs[key] = _Graph(extref.load(key))
    return _graphs[key]


def _extend(engine, G, paths, back, sel=None, download=True, h=None, lens=..., quals=..., read_len=None):
    """snk_dev_extend_paths over the reads `sel` (indices; None: all) of G with their paths"""
    import torch
    from supernova_amd import graphio
    off, ne, edges = paths
    rows, dq, dl = G.rows, G.quals, G.lens
    if sel is not None:
        idx = torch.from_numpy(np.asarray(sel, np.int64)).to(rows.device)
        rows, dq, dl = rows[idx].contiguous(), dq[idx].contiguous(), dl[idx].contiguous()
    args = (_dev(off, np.int32), _dev(np.asarray(ne, np.uint32).view(np.int32), np.int32), _dev(edges, np.int32))

    def call(hh):
        return engine.extend_paths(G.c.K, hh, G.d_off, G.d_bases, rows, G.L if read_len is None else read_len, dq if quals is ... else quals,
                                   dl if lens is ... else lens, *args, back=bool(back), download=download)
    if h is not None:
        return call(h)
    with graphio.hbv_handle(G.c.K, *G.u) as hh:
        return call(hh)


def _take(paths, sel):
    """the paths of the reads `sel`, in that order"""
    off, ne, edges = paths
    start = np.concatenate([[0], np.cumsum(ne.astype(np.int64))])
    sel = np.asarray(sel, np.int64)
    e = np.concatenate([edges[start[r]:start[r + 1]] for r in sel]) if len(sel) else np.zeros(0, np.int32)
    return off[sel].astype(np.int32), ne[sel].astype(np.uint32), e.astype(np.int32)


@pytest.mark.parametrize("name", extref.ALL)
def test_paths_and_bytes_match_the_reference(engine, name):
    """Every fixture, both flags: offset, n_edges and edges equal the fixture's unzipped paths; snk_dev_paths_zip of the result gives the
    reference's bytes; the counters equal the restatement's; the input paths are untouched; a second call gives identical arrays."""
    from supernova_amd import graphio
    c, G = extref.load(name), _graph(name)
    with graphio.hbv_handle(c.K, *G.u) as h:
        for back in (0, 1):
            x_idx, x_data, n_reads = a48xref.parse_pathsx(c.pathsx[back])
            want = a48xref.unzip_paths(x_idx, x_data, n_reads, c.g)
            d_in = (_dev(c.paths[0], np.int32), _dev(c.paths[1].view(np.int32), np.int32), _dev(c.paths[2], np.int32))
            off, ne, edges, stats = engine.extend_paths(c.K, h, G.d_off, G.d_bases, G.rows, G.L, G.quals, G.lens, *d_in, back=bool(back))
            assert off.dtype == np.int32 and ne.dtype == np.uint32 and edges.dtype == np.int32
            assert np.array_equal(ne, want[1]), np.nonzero(ne != want[1])[0][:5]
            assert np.array_equal(off, want[0]), np.nonzero(off != want[0])[0][:5]
            assert np.array_equal(edges, want[2])
            for a, b in zip(d_in, c.paths):
                assert np.array_equal(a.cpu().numpy().view(b.dtype), b), "the input paths changed"
            cnt = extref.restated(name, back)[3]
            assert {k: stats[k] for k in cnt} == cnt
            assert stats["n_reads"] == len(ne) and stats["n_edges_total"] == len(edges)
            assert stats["n_enumerated"] >= cnt["n_quality_extended"] + cnt["n_ambiguous"] + cnt["n_too_many"]
            index, data, _ = engine.zip_paths(h, _dev(off, np.int32), _dev(ne.view(np.int32), np.int32), _dev(edges, np.int32))
            assert a48xref.pathsx_bytes(index, data, len(ne)) == c.pathsx[back]
            again = engine.extend_paths(c.K, h, G.d_off, G.d_bases, G.rows, G.L, G.quals, G.lens, *d_in, back=bool(back))
            assert all(np.array_equal(a, b) for a, b in zip(again[:3], (off, ne, edges))) and {k: again[3][k] for k in cnt} == cnt


@pytest.mark.parametrize("name,back", [("adversarial_cut", 1), ("hand_k60", 1), ("adversarial", 0)])
def test_reads_are_independent(engine, name, back):
    """Slices of 0, 1, 15, 16, 17, 255, 256 and 257 reads give the corresponding slices of the full result, and so does a shuffled order."""
    c, G = extref.load(name), _graph(name)
    full = extref.restated(name, back)[:3]
    n = len(c.lens)
    rng = np.random.default_rng(7)
    picks = [np.arange(min(k, n)) + (0 if k >= n else int(rng.integers(0, n - k + 1))) for k in SLICES] + [rng.permutation(n)]
    for sel in picks:
        off, ne, edges, _ = _extend(engine, G, _take(c.paths, sel), back, sel=sel)
        want = _take(full, sel)
        assert np.array_equal(ne, want[1]) and np.array_equal(off, want[0]) and np.array_equal(edges, want[2]), len(sel)


def _raw(engine, G, h, paths, flags=0, start=None, n_total=None, quals=..., read_len=None, lens=...):
    """the C call itself -> (rc, message, SnkDevExtend)"""
    from supernova_amd import lib as _lib
    off, ne, edges = paths
    n = len(ne)
    d = (_dev(off, np.int32), _dev(np.asarray(ne, np.uint32).view(np.int32), np.int32), _dev(edges if len(edges) else np.zeros(1, np.int32), np.int32),
         _dev(np.concatenate([[0], np.cumsum(np.asarray(ne, np.int64))]) if start is None else start, np.int64))
    r = _lib.SnkDevReads()
    r.n_reads, r.rows, r.row_words, r.read_len = n, G.rows.data_ptr(), G.rows.shape[1], G.L if read_len is None else read_len
    r.quals, r.qstride = (G.quals.data_ptr() if quals is ... else quals), G.quals.shape[1]
    r.lens = G.lens.data_ptr() if lens is ... else lens.data_ptr()
    p = _lib.SnkDevPaths()
    p.n_reads, p.n_edges_total = n, len(edges) if n_total is None else n_total
    p.offset, p.n_edges, p.edges, p.start = d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr()
    x = _lib.SnkDevExtend()
    C.memset(C.byref(x), 0xAB, C.sizeof(x))
    err = C.create_string_buffer(512)
    rc = engine.lib.snk_dev_extend_paths(engine._ctx, G.c.K, C.byref(r), len(G.u[0]) - 1, G.d_off.data_ptr(), G.d_bases.data_ptr(), C.byref(h), C.byref(p), flags,
                                         C.byref(x), engine._stream(), err, 512)
    return rc, err.value.decode(errors="replace"), x, d


def _all_zero(x) -> bool:
    return bytes(x) == bytes(C.sizeof(x))


def test_refusals(engine):
    """Every refusal returns its code with *out all zero; the call after it works."""
    from supernova_amd import graphio, lib as _lib
    c, G = extref.load("hand_k48"), _graph("hand_k48")
    n = len(c.lens)
    names = [r.name for r in __import__("handext").case(48).reads]
    i_root, i_tail, i_empty = names.index("tree3_extended"), names.index("back_onto_root"), names.index("empty_path")
    start_of = np.concatenate([[0], np.cumsum(c.paths[1].astype(np.int64))])
    e_root = int(c.paths[2][start_of[i_root]])

    def with_offset(i, o):
        off = c.paths[0].copy()
        off[i] = o
        return off, c.paths[1], c.paths[2]

    with graphio.hbv_handle(48, *G.u) as h:
        L_root = int(c.lens[i_root])
        cases = [
            ("offset <= -len", with_offset(i_root, -L_root), {}, SNK_E_ARG),
            ("offset >= Bases", with_offset(i_root, len(c.eb[e_root])), {}, SNK_E_ARG),
            ("offset 32768", with_offset(i_root, 32768), {}, SNK_E_UNSUPPORTED),
            ("offset -32768", with_offset(i_root, -32768), {}, SNK_E_UNSUPPORTED),
            ("edge id outside", (c.paths[0], c.paths[1], np.where(np.arange(len(c.paths[2])) == 3, c.g.E, c.paths[2]).astype(np.int32)), {}, SNK_E_ARG),
            ("negative edge id", (c.paths[0], c.paths[1], np.where(np.arange(len(c.paths[2])) == 0, -1, c.paths[2]).astype(np.int32)), {}, SNK_E_ARG),
            ("table", c.paths, dict(n_total=len(c.paths[2]) - 1), SNK_E_ARG),
            ("quals NULL", c.paths, dict(quals=None), SNK_E_ARG),
            ("read_len", c.paths, dict(read_len=257), SNK_E_ARG),
            ("flags", c.paths, dict(flags=2), SNK_E_ARG),
        ]
        # a path on a read of length 0
        lens0 = G.lens.clone()
        lens0[i_root] = 0
        cases.append(("length 0", c.paths, dict(lens=lens0), SNK_E_ARG))
        # the backward leg on a read that ends inside the K - 1 bases its edge shares with the in-edges
        short = G.lens.clone()
        short[i_tail] = -int(c.paths[0][i_tail]) + 48 - 2
        cases.append(("back, short read", c.paths, dict(lens=short, flags=_lib.EXT_BACK), SNK_E_ARG))
        # a start table with a gap
        bad_start = np.concatenate([[0], np.cumsum(c.paths[1].astype(np.int64))])
        bad_start[5] += 1
        cases.append(("start with a gap", c.paths, dict(start=bad_start), SNK_E_ARG))
        # more than 255 edges
        ne_long = c.paths[1].copy()
        ne_long[i_root] = 256
        cases.append(("256 edges", (c.paths[0], ne_long, np.concatenate([c.paths[2][:start_of[i_root]], np.full(256, e_root, np.int32), c.paths[2][start_of[i_root] + 1:]])), {},
                      SNK_E_UNSUPPORTED))
        # a result of more than 255 edges: 255 given, one more in front from the backward leg (found after the result arrays exist)
        ne_255 = c.paths[1].copy()
        ne_255[i_tail] = 255
        e_tail = int(c.paths[2][start_of[i_tail]])
        p_255 = (c.paths[0], ne_255, np.concatenate([c.paths[2][:start_of[i_tail]], np.full(255, e_tail, np.int32), c.paths[2][start_of[i_tail] + 1:]]))
        cases.append(("255 edges and one in front", p_255, dict(flags=_lib.EXT_BACK), SNK_E_UNSUPPORTED))
        for what, paths, kw, code in cases:
            rc, msg, x, _ = _raw(engine, G, h, paths, **kw)
            assert rc == code and msg and _all_zero(x), (what, rc, msg)
        # the same short read is fine without the flag, and the same call with nothing wrong succeeds
        rc, msg, x, _ = _raw(engine, G, h, c.paths, lens=short)
        assert rc == 0 and x.paths.n_reads == n, msg
        rc, msg, x, _ = _raw(engine, G, h, c.paths, flags=_lib.EXT_BACK)
        assert rc == 0 and x.n_back_extended == extref.restated("hand_k48", 1)[3]["n_back_extended"], msg
        rc, msg, x, _ = _raw(engine, G, h, p_255)          # (255 edges without the backward leg: a path like any other)
        assert rc == 0 and x.paths.n_reads == n, msg
        # no reads at all
        rc, msg, x, _ = _raw(engine, _Empty(G), h, (np.zeros(0, np.int32), np.zeros(0, np.uint32), np.zeros(0, np.int32)))
        assert rc == 0 and x.paths.n_reads == 0 and x.paths.n_edges_total == 0, msg
    # a vertex with five out-edges: the list of continuations is sized for four
    v = "".join("ACGT"[i] for i in np.random.default_rng(5).integers(0, 4, 47))
    rnd = lambda k, s: "".join("ACGT"[i] for i in np.random.default_rng(s).integers(0, 4, k))
    five = sorted([rnd(30, 1) + v] + [v + b + rnd(20 + i, 10 + i) for i, b in enumerate("ACGT")] + [v + "A" + rnd(27, 20)], key=lambda s: (-len(s), s))
    G5 = _Five(G, five)
    with graphio.hbv_handle(48, *G5.u) as h5:
        rc, msg, x, _ = _raw(engine, G5, h5, (np.zeros(1, np.int32), np.zeros(1, np.uint32), np.zeros(0, np.int32)))
        assert rc == SNK_E_UNSUPPORTED and "four out-edges" in msg and _all_zero(x), (rc, msg)


class _Empty:
    """no reads on G's graph"""

    def __init__(self, G):
        self.c, self.u, self.d_off, self.d_bases, self.L = G.c, G.u, G.d_off, G.d_bases, G.L
        self.rows, self.quals, self.lens = G.rows[:0], G.quals[:0], G.lens[:0]


class _Five:
    """one read of G on another unitig set"""

    def __init__(self, G, unitigs):
        from supernova_amd import graphio
        self.c, self.L = G.c, G.L
        self.u = graphio.unitigs_to_arrays(unitigs)
        self.d_off, self.d_bases = _dev(self.u[0].astype(np.int64), np.int64), _dev(self.u[1], np.uint8)
        self.rows, self.quals, self.lens = G.rows[:1].contiguous(), G.quals[:1].contiguous(), G.lens[:1].contiguous()


def test_offsets_a_readpathvecx_cannot_hold_are_refused(engine):
    """The reference's own paths of synth_20k_err: a few reads lie beyond base 32767 of a 33 kb edge."""
    import a48ref
    from supernova_amd import graphio
    c = goldens.load("synth_20k_err")
    paths = a48xref.parse_paths(a48ref.load("synth_20k_err")["tmp.paths"])
    assert (paths[0] > 32767).any()
    G = _Graph(type("C", (), dict(K=48, unitigs=c.exp_unitigs, codes=c.codes, quals=c.quals, lens=c.lens)))
    with graphio.hbv_handle(48, *G.u) as h:
        rc, msg, x, _ = _raw(engine, G, h, paths)
    assert rc == SNK_E_UNSUPPORTED and "32767" in msg and _all_zero(x)


def test_end_to_end_path_reads_extend(engine):
    """count + graph + paths + extension + zip in one path_reads call on the adversarial case: the extended paths are what the reference's
    function makes of the reference's paths (the device's paths ARE those: test_gpu_paths.py), both as arrays and as a.pathsX bytes."""
    c = goldens.load("adversarial")
    fx = extref.load("adversarial")
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    off, ne, edges, info = res.path_reads(rows, c.read_len, dq, lens=dl, extend="back", pathsx=True)
    assert np.array_equal(off, fx.paths[0]) and np.array_equal(ne, fx.paths[1]) and np.array_equal(edges, fx.paths[2])
    want = extref.restated("adversarial", 1)
    x_off, x_ne, x_edges = info["extended"]
    assert np.array_equal(x_ne, want[1]) and np.array_equal(x_off, want[0]) and np.array_equal(x_edges, want[2])
    assert {k: info["extend_stats"][k] for k in want[3]} == want[3] and info["extend_stats"]["ms"] > 0
    index, data = info["extended_pathsx"]
    assert a48xref.pathsx_bytes(index, data, len(x_ne)) == fx.pathsx[1]
    # the zipped form of the paths as pathed is still there, and is not the extended one
    assert a48xref.pathsx_bytes(*info["pathsx"], len(ne)) == a48xref.load("adversarial")["a.pathsX"] != fx.pathsx[1]
    # flag 0, results left on the device
    _, _, _, info0 = res.path_reads(rows, c.read_len, dq, lens=dl, extend=True, download=False)
    want0 = extref.restated("adversarial", 0)[3]
    assert {k: info0["extend_stats"][k] for k in want0} == want0 and "extended" not in info0


def _special(kind, tmp_path, n_edges=1):
    import handext
    from supernova_amd import graphio
    s = handext.special(kind)
    u = graphio.unitigs_to_arrays(s.unitigs)
    graphio.write_hbv(tmp_path / "s.hbv", None, s.K, *u)
    g = a48xref.parse_hbv((tmp_path / "s.hbv").read_bytes())
    eb = extref.edge_bases(g)
    codes, quals, lens, paths = handext.special_arrays(s, handext.edge_index(eb), n_edges)
    return s, _Graph(type("C", (), dict(K=s.K, unitigs=s.unitigs, codes=codes, quals=quals, lens=lens))), g, eb, paths


def test_backward_leg_beyond_int16_is_refused(engine, tmp_path):
    """An in-edge of more than 32767 k-mers in front of a path at offset -30: with SNK_EXT_BACK the offset would become one a
    ReadPathVecX wraps (the reference zips the path between its legs), so the call is refused; without the flag it is an ordinary read."""
    from supernova_amd import graphio, lib as _lib
    s, G, g, eb, paths = _special("long_in_edge", tmp_path)
    with graphio.hbv_handle(s.K, *G.u) as h:
        rc, msg, x, _ = _raw(engine, G, h, paths, flags=_lib.EXT_BACK)
        assert rc == SNK_E_UNSUPPORTED and "32767" in msg and _all_zero(x), (rc, msg)
        rc, msg, x, _ = _raw(engine, G, h, paths)
        assert rc == 0 and x.paths.n_edges_total == 1 and x.n_back_extended == 0, msg


def test_leg_3_multi_match_is_refused(engine, tmp_path):
    """Two out-edges of one vertex with the same base at K-1, met by leg 3: the reference pushes both; refused, not reproduced."""
    from supernova_amd import graphio
    s, G, g, eb, paths = _special("multi_match", tmp_path)
    assert int(np.diff(g.from_off).max()) == 3
    with graphio.hbv_handle(s.K, *G.u) as h:
        rc, msg, x, _ = _raw(engine, G, h, paths)
        assert rc == SNK_E_UNSUPPORTED and "same base" in msg and _all_zero(x), (rc, msg)
        # the same read ending on its path's last base never reaches the vertex
        short = G.lens.clone()
        short[0] = len(s.seq) - 3
        rc, msg, x, _ = _raw(engine, G, h, paths, lens=short)
        assert rc == 0 and x.paths.n_edges_total == 1 and x.n_exact_extended == 0, msg
