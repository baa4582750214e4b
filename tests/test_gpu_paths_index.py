"""The paths index on the device (snk_dev_paths_index: a.paths.inv / a.countsb) and the a.48 file set from one result
(graphio.write_a48).  Bar: byte-equal to the files the reference's own code wrote for the golden cases (tests/golden/a48/), and at
sizes without fixtures equal to the numpy restatement that test_a48_files.py pins to those files."""
import tempfile
from pathlib import Path

import numpy as np
import pytest

import a48ref
import goldens
import pathgen
import refio

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


def _index(res, rows, L, dq, dl, dbc):
    off, ne, edges, info = res.path_reads(rows, L, dq, lens=dl, mark_dups=True, bc=dbc, paths_index=True)
    return off, ne, edges, info


def _check_restatement(ne, edges, info):
    """index, counts and counters == the restatement over the paths the same call returned"""
    inv = info["inv"]
    x_off, x_ids, x_counts = a48ref.paths_index(ne, edges, inv)
    g_off, g_ids = info["paths_index"]
    assert g_off.dtype == np.uint64 and g_ids.dtype == np.uint64 and info["countsb"].dtype == np.int32
    assert np.array_equal(g_off, x_off), np.nonzero(g_off != x_off)[0][:5]
    assert np.array_equal(g_ids, x_ids), np.nonzero(g_ids != x_ids)[0][:5]
    assert np.array_equal(info["countsb"], x_counts), np.nonzero(info["countsb"] != x_counts)[0][:5]
    p = info["pidx"]
    assert p["n_entries"] == len(edges) and p["n_hbv_edges"] == len(inv) and p["n_empty_edges"] == int((np.diff(x_off.astype(np.int64)) == 0).sum())
    assert (1 << p["key_bits"]) >= len(inv) and (p["key_bits"] == 0 or (1 << (p["key_bits"] - 1)) < len(inv))
    return x_off, x_ids, x_counts


@pytest.mark.parametrize("name", goldens.CASES)
def test_a48_files_match_the_reference(engine, name, tmp_path):
    """Count + graph + paths + duplicate marks + paths index on the device, write_a48: all six files byte-equal to the reference's."""
    from supernova_amd import graphio
    c = goldens.load(name)
    fx = a48ref.load(name)
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    off, ne, edges, info = _index(res, rows, c.read_len, dq, dl, dbc)
    u_off, u_bases = graphio.unitigs_to_arrays(res.unitigs())
    graphio.write_a48(tmp_path / "a.48", 48, u_off, u_bases, off, ne, edges, info)
    want = {"a.hbv": c.exp_ahbv, "a.inv": c.exp_ainv, "a.paths": fx["tmp.paths"], "a.paths.inv": fx["a.paths.inv"], "a.countsb": fx["a.countsb"],
            "a.dup": fx["a.dup"]}
    for f, b in want.items():
        got = (tmp_path / "a.48" / f).read_bytes()
        assert got == b, (f, len(got), len(b))
    _check_restatement(ne, edges, info)


def test_self_inverse_edge_keeps_its_own_count(engine):
    """counts rule (PathsIndex.cc:122-133) on the device: the adversarial case's palindrome edge is its own reverse complement."""
    c = goldens.load("adversarial")
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    off, ne, edges, info = _index(res, rows, c.read_len, dq, dl, dbc)
    inv = info["inv"]
    own = np.bincount(edges, minlength=len(inv))
    s = np.nonzero(inv == np.arange(len(inv)))[0]
    assert len(s) >= 1 and own[s].sum() > 0 and np.array_equal(info["countsb"][s], own[s])
    o = np.nonzero(inv != np.arange(len(inv)))[0]
    assert np.array_equal(info["countsb"][o], own[o] + own[inv[o]])
    assert np.array_equal(info["countsb"], a48ref.parse_countsb(a48ref.load("adversarial")["a.countsb"]))


@pytest.mark.parametrize("K", [48, 60])
def test_long_tandem_paths(engine, K):
    """Reads of 250 bases inside a homopolymer and period-2 / period-3 repeats: paths of more than 64 edges that visit an edge many
    times -- a read is in an edge's list as often as its path holds the edge."""
    from supernova_amd.engine import Params
    L = 250
    rng = np.random.default_rng(K * 1000 + L)
    g = rng.integers(0, 4, 12000, dtype=np.uint8)
    g[2000:2230] = 0
    g[5000:5230] = np.resize(np.array([0, 2], np.uint8), 230)
    g[8000:8230] = np.resize(np.array([0, 1, 3], np.uint8), 230)
    spots = [(2000, 230), (5000, 230), (8000, 230)]
    codes, quals, lens, bc = pathgen.pairs(rng, g, int(len(g) * 40 / L / 2), L, 0.002, 6, spots, spot_frac=0.5)
    rows, dq, dl, dbc = pathgen.to_device(codes, quals, lens, bc, pad_seed=K + L)
    res = engine.count_graph(rows, L, quals=dq, bc=dbc, lens=dl, params=Params(K=K))
    off, ne, edges, info = _index(res, rows, L, dq, dl, dbc)
    assert int(ne.max()) > 64
    x_off, x_ids, _ = _check_restatement(ne, edges, info)
    start = np.concatenate([[0], np.cumsum(ne.astype(np.int64))])
    r = int(np.argmax(ne))
    mine = edges[start[r]:start[r + 1]]
    e = int(np.bincount(mine).argmax())
    times = int((mine == e).sum())
    assert times > 1
    lst = x_ids[int(x_off[e]):int(x_off[e + 1])]
    g_off, g_ids = info["paths_index"]
    assert int((g_ids[int(g_off[e]):int(g_off[e + 1])] == r).sum()) == times == int((lst == r).sum())


RETRIES = {"path_redo_cap": 1, "path_edge_cap": 1, "path_ubc_cap": 1, "path_redo_all": 1}


@pytest.mark.parametrize("data", ["synth_200k_err", "synth_2m_clean"])
def test_large_index_is_the_restatement_and_repeatable(engine, data, tune):
    """Many edges (0.6 % errors) and few edges under heavy skew (clean reads: two edges hold everything): == restatement; a second call
    gives the same bytes; so do the minimiser-index look-ups and the pather's re-runs after its lists overflowed."""
    from supernova_amd import synth
    if data == "synth_200k_err":
        sp = synth.synth_params(200_000, seed=0x5EED0C0D, sub_ppm=6000)
    else:
        sp = synth.synth_params(2_000_000, seed=0x5EED0C0E, error_free=True)
    rows, dq, dbc = engine.synth(sp)
    L = sp.read_len
    res = engine.count_graph(rows, L, quals=dq, bc=dbc)

    def run():
        off, ne, edges, info = _index(res, rows, L, dq, None, dbc)
        return (off, ne, edges, info["paths_index"][0], info["paths_index"][1], info["countsb"], info["dups"]["dup"]), info

    base, info = run()
    _check_restatement(base[1], base[2], info)
    assert len(base[2]) > sp.n_reads // 2
    again, _ = run()
    for a, b in zip(again, base):
        assert np.array_equal(a, b)
    for lookup in (1, 0):
        tune("path_index", lookup)
        got, _ = run()
        for a, b in zip(got, base):
            assert np.array_equal(a, b)
    for o, v in RETRIES.items():
        tune(o, v)
    got, info2 = run()
    assert info2["retries"] != 0
    for a, b in zip(got, base):
        assert np.array_equal(a, b)


def test_a_paths_vs_a_fresh_reference_run_200k(engine, tmp_path):
    """200 000 reads with 0.6 % errors through the reference binary (where it is built): a.paths == the tmp.paths its pathReads wrote,
    and the index of those paths == the restatement."""
    from supernova_amd import graphio, synth
    import torch
    if not refio.REF_DRIVER.exists():
        pytest.skip("oracle/_ref/snref_driver is not built (the reference's sources are not on this machine)")
    n = 200_000
    sp = synth.synth_params(n, seed=0x5EED0A48, sub_ppm=6000)
    rows, quals, bc = synth.synth_host(sp)
    L = sp.read_len
    asc = synth.codes_to_ascii(synth.unpack_rows(rows, L))
    with tempfile.TemporaryDirectory() as td:
        refio.write_snkrd(Path(td) / "in.snkrd", np.full(n, L), asc, quals, bc)
        refio.run_ref(Path(td) / "in.snkrd", Path(td) / "out", threads=16)
        want = (Path(td) / "out" / "tmp.paths").read_bytes()
        want_inv = (Path(td) / "out" / "a.inv").read_bytes()
    dev = torch.device("cuda", 0)
    rows_d, quals_d, bc_d = torch.from_numpy(rows.view(np.int32)).to(dev), torch.from_numpy(quals).to(dev), torch.from_numpy(bc).to(dev)
    res = engine.count_graph(rows_d, L, quals=quals_d, bc=bc_d)
    off, ne, edges, info = _index(res, rows_d, L, quals_d, None, bc_d)
    u_off, u_bases = graphio.unitigs_to_arrays(res.unitigs())
    graphio.write_a48(tmp_path / "a.48", 48, u_off, u_bases, off, ne, edges, info)
    assert (tmp_path / "a.48" / "a.inv").read_bytes() == want_inv
    got = (tmp_path / "a.48" / "a.paths").read_bytes()
    assert got == want, (len(got), len(want))
    _check_restatement(ne, edges, info)


def test_paths_index_argument_checks(engine):
    """An involution of another graph (wrong length: edge ids fall outside it) and one that is not an involution are refused; the
    context is fine afterwards."""
    import ctypes as C
    from supernova_amd import lib as _lib
    c = goldens.load("adversarial")
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    off, ne, edges, info = _index(res, rows, c.read_len, dq, dl, dbc)
    inv = info["inv"]
    E = len(inv)
    # the paths struct of a fresh pathing call, kept on the device
    e = engine
    h = _lib.SnkHbv()
    ms = C.c_float(0)
    err = C.create_string_buffer(512)
    assert e.lib.snk_dev_hbv(e._ctx, 48, res.n_unitigs, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(ms), e._stream(), err, 512) == 0
    try:
        r = _lib.SnkDevReads()
        r.n_reads, r.rows, r.row_words, r.read_len = rows.shape[0], rows.data_ptr(), rows.shape[1], c.read_len
        r.quals, r.qstride, r.lens = dq.data_ptr(), dq.shape[1], dl.data_ptr()
        p = _lib.SnkDevPaths()
        assert e.lib.snk_dev_path_reads(e._ctx, 48, C.byref(r), res.n_unitigs, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(p), e._stream(), err, 512) == 0
    finally:
        e.lib.snk_hbv_free(C.byref(h))
    px = _lib.SnkDevPidx()
    emax = int(edges.max())
    small = np.arange(emax, dtype=np.int32)                   # identity on [0, emax): the largest edge id does not fit
    assert e.lib.snk_dev_paths_index(e._ctx, C.byref(p), emax, small.ctypes.data, C.byref(px), e._stream(), err, 512) == SNK_E_ARG
    assert b"edge id" in err.value and px.index_off is None
    bad = inv.copy()
    bad[0] = bad[1] = 2 if E > 2 else 0
    if E > 2:
        assert e.lib.snk_dev_paths_index(e._ctx, C.byref(p), E, bad.ctypes.data, C.byref(px), e._stream(), err, 512) == SNK_E_ARG
        assert b"involution" in err.value
    assert e.lib.snk_dev_paths_index(e._ctx, C.byref(p), E, inv.ctypes.data, C.byref(px), e._stream(), err, 512) == 0, err.value
    g_off = res._dl(px.index_off, (E + 1) * 8, np.uint64, (E + 1,))
    g_ids = res._dl(px.index_ids, int(px.n_entries) * 8, np.uint64, (int(px.n_entries),))
    assert np.array_equal(g_off, info["paths_index"][0]) and np.array_equal(g_ids, info["paths_index"][1])
