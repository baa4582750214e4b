"""The compressed read paths on the device (snk_dev_paths_zip / snk_dev_paths_unzip: a.pathsX) and a.hbx through graphio.write_a48.
Bar: byte-equal to the files the reference's own code wrote (tests/golden/a48x/), and at sizes without fixtures equal to the numpy
restatement that test_a48x_files.py pins to those files."""
import numpy as np
import pytest

import a48ref
import a48xref
import goldens
import pathgen

pytestmark = pytest.mark.gpu
SNK_E_ARG, SNK_E_UNSUPPORTED = -1, -6
RETRIES = {"path_redo_cap": 1, "path_edge_cap": 1, "path_ubc_cap": 1, "path_redo_all": 1}       # as in test_gpu_paths_index.py


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
    """The adversarial case's graph: the restatement's view of it, and its unitig arrays."""
    from supernova_amd import graphio
    c = goldens.load("adversarial")
    return a48xref.parse_hbv(c.exp_ahbv), graphio.unitigs_to_arrays(c.exp_unitigs)


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype)).to(torch.device("cuda", 0))


def _zip(engine, h, off, ne, edges, start=None):
    return engine.zip_paths(h, _dev(off, np.int32), _dev(np.asarray(ne, np.uint32).view(np.int32), np.int32), _dev(edges, np.int32),
                            None if start is None else _dev(start, np.int64))


def _graph_of(res, K, tmp_path):
    """restatement's graph + unitig arrays of a device result (through the a.hbv the library writes for it)"""
    from supernova_amd import graphio
    u = graphio.unitigs_to_arrays(res.unitigs())
    graphio.write_hbv(tmp_path / "g.hbv", None, K, *u)
    return a48xref.parse_hbv((tmp_path / "g.hbv").read_bytes()), u


def _same_as_restatement(info, off, ne, edges, g):
    x_index, x_data, x_stats = a48xref.zip_paths(off, ne, edges, g)
    index, data = info["pathsx"]
    assert index.dtype == np.int64 and data.dtype == np.uint8
    assert np.array_equal(index, x_index), np.nonzero(index != x_index)[0][:5]
    assert len(data) == len(x_data) and np.array_equal(data, x_data), np.nonzero(data != x_data)[0][:5]
    s = info["pathsx_stats"]
    assert {k: s[k] for k in x_stats} == x_stats
    assert s["n_reads"] == len(ne) and s["n_bytes"] == len(data) and s["n_index"] == len(index)


@pytest.mark.parametrize("name", list(goldens.CASES) + ["long_unitig"])
def test_a48_files_match_the_reference(engine, name, tmp_path):
    """Count + graph + paths + duplicate marks + paths index + zip on the device, write_a48: a.hbx and a.pathsX byte-equal to the
    reference's, and the other six files still are."""
    from supernova_amd import graphio
    fx = a48xref.load(name)
    if name == "long_unitig":
        codes, quals, lens, bc = a48xref.long_unitig_reads()
        assert a48xref.reads_digest(codes, quals, lens, bc) == fx["reads_digest"], "the generator no longer makes the reads the fixture was made from"
        ign, L = 0, codes.shape[1]
        want = {f: fx[f] for f in a48xref.FILES if f != "tmp.paths"}
        want["a.paths"] = fx["tmp.paths"]
    else:
        c = goldens.load(name)
        codes, quals, lens, bc, ign, L = c.codes, c.quals, c.lens, c.bc, c.ign_bc_below, c.read_len
        f6 = a48ref.load(name)
        want = {"a.hbv": c.exp_ahbv, "a.inv": c.exp_ainv, "a.paths": f6["tmp.paths"], "a.paths.inv": f6["a.paths.inv"], "a.countsb": f6["a.countsb"],
                "a.dup": f6["a.dup"], "a.hbx": fx["a.hbx"], "a.pathsX": fx["a.pathsX"]}
    rows, dq, dl, dbc = pathgen.to_device(codes, quals, lens, bc)
    res = engine.count_graph(rows, L, quals=dq, bc=dbc, lens=dl, ign_bc_below=ign)
    off, ne, edges, info = res.path_reads(rows, L, dq, lens=dl, mark_dups=True, bc=dbc, paths_index=True, pathsx=True)
    u_off, u_bases = graphio.unitigs_to_arrays(res.unitigs())
    graphio.write_a48(tmp_path / "a.48", 48, u_off, u_bases, off, ne, edges, info)
    for f, b in want.items():
        got = (tmp_path / "a.48" / f).read_bytes()
        assert got == b, (f, len(got), len(b))
    _same_as_restatement(info, off, ne, edges, a48xref.parse_hbv(want["a.hbv"]))
    if name == "long_unitig":
        assert info["pathsx_stats"]["n_offsets_wrapped"] >= 1
    # without the key the file set is the six it was
    info.pop("pathsx")
    graphio.write_a48(tmp_path / "six", 48, u_off, u_bases, off, ne, edges, info)
    assert sorted(p.name for p in (tmp_path / "six").iterdir()) == ["a.countsb", "a.dup", "a.hbv", "a.inv", "a.paths", "a.paths.inv"]


def test_probe_paths_match_the_bytes_the_reference_wrote(engine, adv):
    """The hand-made paths of the probe fixture, uploaded as they are: the int16 wrap in both directions, a 255-edge path, steps that are
    no steps of the graph in the middle and at the end of a path, empty paths, 23 reads."""
    from supernova_amd import graphio
    g, u = adv
    fx = a48xref.load("probe_paths")
    off, ne, edges = a48xref.parse_paths(fx["tmp.paths"])
    with graphio.hbv_handle(48, *u) as h:
        index, data, stats = _zip(engine, h, off, ne, edges)
    x_index, x_data, n = a48xref.parse_pathsx(fx["a.pathsX"])
    assert n == len(ne) and np.array_equal(index, x_index) and np.array_equal(data, x_data)
    _, _, x_stats = a48xref.zip_paths(off, ne, edges, g)
    assert {k: stats[k] for k in x_stats} == x_stats and x_stats["n_steps_not_found"] == 2 and x_stats["n_offsets_wrapped"] == 2


def _walks(rng, g, sizes):
    """Paths of the given edge counts: walks over the graph; at an edge without out-edges, and now and then anywhere, the next edge is
    a random one (a step that may not be found)."""
    adj = [g.from_e[g.from_off[w]:g.from_off[w + 1]] for w in g.v_right]
    edges = []
    for n in sizes:
        e = int(rng.integers(0, g.E))
        for _ in range(int(n)):
            edges.append(e)
            a = adj[e]
            e = int(a[rng.integers(0, len(a))]) if len(a) and rng.random() > 0.02 else int(rng.integers(0, g.E))
    return np.asarray(edges, np.int32)


def _mixed_sizes(rng, n):
    """empty paths, 7-byte records (one edge) and records of 8 to 70 bytes in turn"""
    ne = np.zeros(n, np.int64)
    ne[1::3] = 1
    ne[2::3] = rng.integers(2, 253, len(ne[2::3]))
    if n > 5:
        ne[2], ne[5] = 2, 252                               # the ends of the range: 8 and 70 bytes
    return ne


@pytest.mark.parametrize("n_reads", [1, 9, 10, 11, 255, 256, 257, 2561])
def test_tile_and_index_edges(engine, adv, n_reads):
    """Read counts round the index step (10) and the tile (256 reads), several tiles; at 257 reads the first read's record is sized so that
    the second tile starts at every byte alignment of a 16-byte word in turn."""
    from supernova_amd import graphio
    g, u = adv
    rng = np.random.default_rng(1000 + n_reads)
    base = _mixed_sizes(rng, n_reads) if n_reads > 1 else np.array([137])
    seen = set()
    with graphio.hbv_handle(48, *u) as h:
        for want in (range(16) if n_reads == 257 else [None]):
            ne = base.copy()
            if want is not None:
                d = (want - int(a48xref.rec_bytes(ne[:256]).sum())) % 16          # bytes to add to read 0 (an empty path: one byte)
                d += 16 if 0 < d < 6 else 0
                ne[0] = 0 if d == 0 else 1 if d == 6 else 4 * (d - 6) - 2
            edges = _walks(rng, g, ne)
            off = rng.integers(-70000, 70000, n_reads).astype(np.int32)
            index, data, stats = _zip(engine, h, off, ne, edges)
            _same_as_restatement(dict(pathsx=(index, data), pathsx_stats=stats), off, ne, edges, g)
            rb = np.concatenate([[0], np.cumsum(a48xref.rec_bytes(ne))])
            assert int(rb[-1]) == len(data) and len(index) == (n_reads + 9) // 10
            if want is not None:
                seen.add(int(rb[256]) % 16)
    assert n_reads != 257 or seen == set(range(16))


@pytest.mark.parametrize("K", [48, 60])
def test_long_tandem_paths(engine, K, tmp_path):
    """The 250-base tandem-repeat reads of test_gpu_paths_index.py: paths of more than 64 edges that go round a loop of the graph."""
    from supernova_amd.engine import Params
    L = 250
    rng = np.random.default_rng(K * 1000 + L)
    gen = rng.integers(0, 4, 12000, dtype=np.uint8)
    gen[2000:2230] = 0
    gen[5000:5230] = np.resize(np.array([0, 2], np.uint8), 230)
    gen[8000:8230] = np.resize(np.array([0, 1, 3], np.uint8), 230)
    spots = [(2000, 230), (5000, 230), (8000, 230)]
    codes, quals, lens, bc = pathgen.pairs(rng, gen, int(len(gen) * 40 / L / 2), L, 0.002, 6, spots, spot_frac=0.5)
    rows, dq, dl, dbc = pathgen.to_device(codes, quals, lens, bc, pad_seed=K + L)
    res = engine.count_graph(rows, L, quals=dq, bc=dbc, lens=dl, params=Params(K=K))
    off, ne, edges, info = res.path_reads(rows, L, dq, lens=dl, pathsx=True)
    assert int(ne.max()) > 64
    g, _ = _graph_of(res, K, tmp_path)
    _same_as_restatement(info, off, ne, edges, g)


def test_refusals_leave_the_context_usable(engine, adv):
    """A path of 256 edges, an edge id equal to the number of edges, a start table that does not add up: each its error code, nothing
    handed back, and the next call works."""
    from supernova_amd import graphio, lib as _lib
    g, u = adv
    good = (np.array([5, 0], np.int32), np.array([2, 0], np.uint32), np.array([0, 0], np.int32))
    with graphio.hbv_handle(48, *u) as h:
        want = _zip(engine, h, *good)

        def refused(code, *paths, **kw):
            with pytest.raises(_lib.SnkError) as ei:
                _zip(engine, h, *paths, **kw)
            assert ei.value.code == code, str(ei.value)
            again = _zip(engine, h, *good)
            assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
            return str(ei.value)

        assert "255" in refused(SNK_E_UNSUPPORTED, np.zeros(1, np.int32), np.array([256], np.uint32), np.zeros(256, np.int32))
        assert "edge id" in refused(SNK_E_ARG, np.zeros(1, np.int32), np.array([2], np.uint32), np.array([0, g.E], np.int32))
        assert "add up" in refused(SNK_E_ARG, np.zeros(2, np.int32), np.array([1, 1], np.uint32), np.array([0, 0], np.int32), start=np.array([0, 2, 2], np.int64))
        # two reads on the same entry: every start lies inside the array, but the table is not the scan of n_edges
        assert "add up" in refused(SNK_E_ARG, np.zeros(2, np.int32), np.array([1, 1], np.uint32), np.array([0, 0], np.int32), start=np.array([0, 0, 2], np.int64))


def test_round_trip_200k_and_repeatable(engine, tune, tmp_path):
    """200 000 reads with 0.6 % errors: unzip(zip(p)) == p on every read whose steps are all steps of the graph, offsets compared after
    the int16 wrap; a second zip gives the same bytes, and so does one after the pather's lists were made to overflow and regrow."""
    from supernova_amd import graphio, synth
    sp = synth.synth_params(200_000, seed=0x5EED0C0D, sub_ppm=6000)
    rows, dq, dbc = engine.synth(sp)
    L = sp.read_len
    res = engine.count_graph(rows, L, quals=dq, bc=dbc)
    off, ne, edges, info = res.path_reads(rows, L, dq, pathsx=True)
    index, data = info["pathsx"]
    assert len(edges) > sp.n_reads // 2 and info["pathsx_stats"]["n_empty"] == int((ne == 0).sum())
    g, u = _graph_of(res, 48, tmp_path)
    whole = a48xref.all_steps_found(ne, edges, g)
    assert info["pathsx_stats"]["n_steps_not_found"] == 0 and whole.all()      # (pathReads only makes steps of the graph)
    with graphio.hbv_handle(48, *u) as h:
        u_off, u_ne, u_edges, _ = engine.unzip_paths(h, _dev(index, np.int64), _dev(data, np.uint8), len(ne))
    assert np.array_equal(u_ne, ne) and np.array_equal(u_edges, edges)
    assert np.array_equal(u_off, np.where(ne > 0, a48xref.wrap16(off), 0))
    _, _, _, again = res.path_reads(rows, L, dq, pathsx=True)
    assert np.array_equal(again["pathsx"][0], index) and np.array_equal(again["pathsx"][1], data)
    for o, v in RETRIES.items():
        tune(o, v)
    _, _, _, forced = res.path_reads(rows, L, dq, pathsx=True)
    assert forced["retries"] != 0
    assert np.array_equal(forced["pathsx"][0], index) and np.array_equal(forced["pathsx"][1], data)


def test_unzip_refuses_what_is_not_a_readpathvecx(engine, adv):
    """A data array cut one byte short; a branch id that points past the out-edges of its vertex; the whole array is accepted."""
    from supernova_amd import graphio, lib as _lib
    g, u = adv
    fx = a48xref.load("adversarial")
    index, data, n = a48xref.parse_pathsx(fx["a.pathsX"])
    c = goldens.load("adversarial")
    n_out = np.diff(g.from_off)[g.v_right]
    e = int(np.nonzero((n_out >= 1) & (n_out <= 3))[0][0])                    # an edge whose right vertex has fewer than four out-edges
    rec = np.array([2, 0, 0, e & 255, (e >> 8) & 255, (e >> 16) & 255, e >> 24, 3], np.uint8)
    with graphio.hbv_handle(48, *u) as h:
        u_off, u_ne, u_edges, _ = engine.unzip_paths(h, _dev(index, np.int64), _dev(data, np.uint8), n)
        assert np.array_equal(u_ne, c.exp_path_n) and np.array_equal(u_edges, c.exp_path_edges)
        with pytest.raises(_lib.SnkError) as ei:
            engine.unzip_paths(h, _dev(index, np.int64), _dev(data[:-1], np.uint8), n)
        assert ei.value.code == SNK_E_ARG and "n_bytes" in str(ei.value)
        with pytest.raises(_lib.SnkError) as ei:
            engine.unzip_paths(h, _dev(np.zeros(1, np.int64), np.int64), _dev(rec, np.uint8), 1)
        assert ei.value.code == SNK_E_ARG and "branch id" in str(ei.value)
        rec[7] = 0
        u_off, u_ne, u_edges, _ = engine.unzip_paths(h, _dev(np.zeros(1, np.int64), np.int64), _dev(rec, np.uint8), 1)
        assert u_ne.tolist() == [2] and u_edges.tolist() == [e, int(g.from_e[g.from_off[g.v_right[e]]])]
