"""a.hbx and a.pathsX on the host (include/snk.h, "the compressed read paths"): the numpy restatement of a48xref.py and the writers
snk_write_hbx / snk_write_pathsx byte for byte against the files the reference's own code wrote (tests/golden/a48x/, made by
tests/golden/make_a48x_golden.py), snk_read_pathsx, and the bytes of snk_write_hbv, which now takes its From / To lists from the
function the other two share.  No GPU."""
import numpy as np
import pytest

import a48xref
import goldens


def _inputs(name):
    """-> (graph, offset, n_edges, edges, fixture) of a fixture case"""
    fx = a48xref.load(name)
    if name in goldens.CASES:
        c = goldens.load(name)
        return a48xref.parse_hbv(c.exp_ahbv), c.exp_path_off, c.exp_path_n, c.exp_path_edges, fx
    g = a48xref.parse_hbv(fx["a.hbv"] if name == "long_unitig" else goldens.load("adversarial").exp_ahbv)
    return (g, *a48xref.parse_paths(fx["tmp.paths"]), fx)


ALL = list(goldens.CASES) + list(a48xref.EXTRA)


@pytest.mark.parametrize("name", ALL)
def test_restatement_reproduces_the_reference_files(name):
    """zip + the a.pathsX layout == the reference's a.pathsX; the a.hbx layout over the lists of a.hbv == its a.hbx; unzip gives the paths
    back wherever the reference encoded every step."""
    g, off, ne, edges, fx = _inputs(name)
    index, data, stats = a48xref.zip_paths(off, ne, edges, g)
    assert a48xref.pathsx_bytes(index, data, len(ne)) == fx["a.pathsX"]
    if "a.hbx" in fx:
        assert a48xref.hbx_bytes(g) == fx["a.hbx"]
    r_index, r_data, n = a48xref.parse_pathsx(fx["a.pathsX"])
    assert n == len(ne) and np.array_equal(r_index, index)
    u_off, u_ne, u_edges = a48xref.unzip_paths(r_index, r_data, n, g, strict=False)
    assert np.array_equal(u_ne, ne) and np.array_equal(u_off, np.where(ne > 0, a48xref.wrap16(off), 0))
    whole = a48xref.all_steps_found(ne, edges, g)
    start = np.concatenate([[0], np.cumsum(ne.astype(np.int64))])
    keep = np.repeat(whole, ne.astype(np.int64))
    assert np.array_equal(u_edges[keep], edges[keep]) and start[-1] == len(u_edges)
    assert stats["n_empty"] == int((ne == 0).sum()) and (stats["n_steps_not_found"] == 0) == bool(whole.all())
    if name in goldens.CASES:
        assert stats["n_steps_not_found"] == 0              # (pathReads only makes paths whose steps are steps of the graph)


def test_the_extra_cases_hold_what_they_are_for():
    """long_unitig: offsets above 32767 whose stored form is negative; probe_paths: the wrap in both directions, a 255-edge path, two steps
    the reference did not encode, a read count that is no multiple of 10 -- all in bytes the reference wrote."""
    g, off, ne, edges, fx = _inputs("long_unitig")
    far = (ne > 0) & (off > 32767)
    assert far.sum() >= 1
    index, data, n = a48xref.parse_pathsx(fx["a.pathsX"])
    u_off, _, _ = a48xref.unzip_paths(index, data, n, g)
    assert np.all(u_off[far] == off[far] - 65536) and np.all(u_off[far] < 0)
    g, off, ne, edges, fx = _inputs("probe_paths")
    assert len(ne) % 10 != 0 and int(ne.max()) == 255 and (ne == 0).sum() >= 3
    assert {-40000, -1, 32767, 32768} <= set(off[ne == 1].tolist())
    _, _, stats = a48xref.zip_paths(off, ne, edges, g)
    assert stats["n_steps_not_found"] == 2 and stats["n_offsets_wrapped"] == 2
    index, data, n = a48xref.parse_pathsx(fx["a.pathsX"])
    assert len(data) == int(a48xref.rec_bytes(ne).sum()) and len(index) == 3
    r = int(np.nonzero((ne == 1) & (off == -40000))[0][0])
    at = int(np.concatenate([[0], np.cumsum(a48xref.rec_bytes(ne))])[r])
    assert int(np.frombuffer(data[at + 1:at + 3].tobytes(), "<i2")[0]) == 25536           # -40000 + 65536
    # a path with a step not found in the middle: its record keeps the size of 4 edges, and holds two ids, not three
    r = int(np.nonzero((ne == 4) & ~a48xref.all_steps_found(ne, edges, g))[0][0])
    at = int(np.concatenate([[0], np.cumsum(a48xref.rec_bytes(ne))])[r])
    assert int(data[at]) == 4 and int(data[at + 7]) < 16


@pytest.mark.parametrize("name", ALL)
def test_writers_match_the_reference_files(snk, tmp_path, name):
    """snk_write_pathsx from the parsed arrays == a.pathsX, and snk_read_pathsx reads it back; snk_write_hbx from the unitigs == a.hbx."""
    from supernova_amd import graphio
    fx = a48xref.load(name)
    index, data, n = a48xref.parse_pathsx(fx["a.pathsX"])
    graphio.write_pathsx(tmp_path / "a.pathsX", index, data, n)
    assert (tmp_path / "a.pathsX").read_bytes() == fx["a.pathsX"]
    r_index, r_data, r_n = graphio.read_pathsx(tmp_path / "a.pathsX")
    assert r_n == n and r_index.dtype == np.int64 and r_data.dtype == np.uint8 and np.array_equal(r_index, index) and np.array_equal(r_data, data)
    if name in goldens.CASES:
        c = goldens.load(name)
        u_off, u_bases = graphio.unitigs_to_arrays(c.exp_unitigs)
        graphio.write_hbx(tmp_path / "a.hbx", 48, u_off, u_bases)
        assert (tmp_path / "a.hbx").read_bytes() == fx["a.hbx"]


@pytest.mark.parametrize("name", goldens.CASES)
def test_write_hbv_bytes_are_what_they_were(snk, tmp_path, name):
    """a.hbv and a.inv from the shared From / To function == the reference's files."""
    from supernova_amd import graphio
    c = goldens.load(name)
    u_off, u_bases = graphio.unitigs_to_arrays(c.exp_unitigs)
    graphio.write_hbv(tmp_path / "a.hbv", tmp_path / "a.inv", 48, u_off, u_bases)
    assert (tmp_path / "a.hbv").read_bytes() == c.exp_ahbv and (tmp_path / "a.inv").read_bytes() == c.exp_ainv


def test_pathsx_files_at_the_edges(snk, tmp_path):
    """No reads; a count that does not fit the index; a file whose header and size disagree."""
    from supernova_amd import graphio, lib as _lib
    graphio.write_pathsx(tmp_path / "p0", np.zeros(0, np.int64), np.zeros(0, np.uint8), 0)
    assert (tmp_path / "p0").read_bytes() == a48xref.pathsx_bytes([], [], 0) and len((tmp_path / "p0").read_bytes()) == 40
    index, data, n = graphio.read_pathsx(tmp_path / "p0")
    assert n == 0 and len(index) == 0 and len(data) == 0
    with pytest.raises(_lib.SnkError):
        graphio.write_pathsx(tmp_path / "bad", np.zeros(1, np.int64), np.zeros(11, np.uint8), 11)
    b = a48xref.load("probe_paths")["a.pathsX"]
    (tmp_path / "short").write_bytes(b[:-1])
    with pytest.raises(_lib.SnkError):
        graphio.read_pathsx(tmp_path / "short")
    with pytest.raises(_lib.SnkError):
        graphio.read_pathsx(tmp_path / "missing")
