"""Host writers of the files DF leaves in a.48/ beside the graph -- a.paths, a.paths.inv, a.countsb, a.dup (include/snk.h, "the paths
index and the rest of a.48/") -- byte for byte against the files the reference's own code wrote for the golden cases
(tests/golden/a48/, made by tests/golden/make_a48_golden.py), and the numpy restatement of writePathsIndex pinned to those files.
No GPU."""
import numpy as np
import pytest

import a48ref
import goldens


def _case(name):
    c = goldens.load(name)
    return c, a48ref.load(name), a48ref.parse_inv(c.exp_ainv)


@pytest.mark.parametrize("name", goldens.CASES)
def test_writers_match_the_reference_files(snk, tmp_path, name):
    """snk_write_paths from the golden paths == tmp.paths (what DF renames to a.paths); snk_write_paths_index from the restated index ==
    a.paths.inv and a.countsb; snk_write_dup from the golden flags == a.dup."""
    from supernova_amd import graphio
    c, fx, inv = _case(name)
    graphio.write_paths(tmp_path / "a.paths", c.exp_path_off, c.exp_path_n, c.exp_path_edges)
    assert (tmp_path / "a.paths").read_bytes() == fx["tmp.paths"]
    start = np.zeros(len(c.exp_path_n) + 1, np.uint64)
    start[1:] = np.cumsum(c.exp_path_n.astype(np.int64))
    graphio.write_paths(tmp_path / "a.paths2", c.exp_path_off, c.exp_path_n, c.exp_path_edges, start=start)
    assert (tmp_path / "a.paths2").read_bytes() == fx["tmp.paths"]
    off, ids, counts = a48ref.paths_index(c.exp_path_n, c.exp_path_edges, inv)
    graphio.write_paths_index(tmp_path / "a.paths.inv", tmp_path / "a.countsb", off, ids, counts)
    assert (tmp_path / "a.paths.inv").read_bytes() == fx["a.paths.inv"]
    assert (tmp_path / "a.countsb").read_bytes() == fx["a.countsb"]
    graphio.write_dup(tmp_path / "a.dup", c.exp_dup)
    assert (tmp_path / "a.dup").read_bytes() == fx["a.dup"]


@pytest.mark.parametrize("name", goldens.CASES)
def test_restatement_decodes_to_the_reference_index(name):
    """order = argsort(edges, stable), ids = read_of_entry[order], off = cumsum(bincount(edges)) is exactly what a parser of the
    reference's a.paths.inv reads back; the counts rule gives its a.countsb -- the GPU tests may use the restatement at any size."""
    c, fx, inv = _case(name)
    off, ids, counts = a48ref.paths_index(c.exp_path_n, c.exp_path_edges, inv)
    r_off, r_ids = a48ref.parse_paths_inv(fx["a.paths.inv"])
    assert len(r_off) == len(inv) + 1 and int(r_off[-1]) == len(c.exp_path_edges) > 0
    assert np.array_equal(off, r_off) and np.array_equal(ids, r_ids)
    assert np.array_equal(counts, a48ref.parse_countsb(fx["a.countsb"]))
    # every edge's reads ascend, and a read is there as often as its path holds the edge
    e = int(np.argmax(np.diff(off.astype(np.int64))))
    mine = ids[int(off[e]):int(off[e + 1])].astype(np.int64)
    assert np.all(np.diff(mine) >= 0)
    read_of_entry = np.repeat(np.arange(len(c.exp_path_n)), c.exp_path_n.astype(np.int64))
    assert np.array_equal(np.bincount(mine, minlength=len(c.exp_path_n)), np.bincount(read_of_entry[c.exp_path_edges == e], minlength=len(c.exp_path_n)))


def test_self_inverse_edge_keeps_its_own_count():
    """The adversarial case plants a palindromic 48-mer: its edge is its own reverse complement and its support is not doubled."""
    c, fx, inv = _case("adversarial")
    self_inv = np.nonzero(inv == np.arange(len(inv)))[0]
    assert len(self_inv) >= 1
    own = np.bincount(c.exp_path_edges, minlength=len(inv))
    ref = a48ref.parse_countsb(fx["a.countsb"])
    assert np.array_equal(ref[self_inv], own[self_inv]) and own[self_inv].sum() > 0
    other = np.nonzero(inv != np.arange(len(inv)))[0]
    assert np.array_equal(ref[other], own[other] + own[inv[other]])


def test_empty_paths_and_unvisited_edges_write_valid_files(snk, tmp_path):
    """No reads at all, reads without a path, and edges nobody visits (the reference adds an empty entry, PathsIndex.cc:101-102)."""
    from supernova_amd import graphio
    z32, zu = np.zeros(0, np.int32), np.zeros(0, np.uint32)
    graphio.write_paths(tmp_path / "p0", z32, zu, z32)
    b = (tmp_path / "p0").read_bytes()
    assert len(b) == 32 and b[:4] == bytes(4) and b[4:8] == bytes([1, 0, 24, 4]) and np.array_equal(np.frombuffer(b[8:], "<u8"), [24, 32, 24])
    graphio.write_paths(tmp_path / "p3", np.array([5, 0, -2], np.int32), np.array([2, 0, 1], np.uint32), np.array([4, 1, 0], np.int32))
    b = (tmp_path / "p3").read_bytes()
    assert len(b) == 24 + 3 * 8 + 3 * 4 + 4 * 8
    assert np.array_equal(np.frombuffer(b[24:60], "<i4"), [5, 0, 4, 1, 0, 0, -2, 0, 0])
    assert np.array_equal(np.frombuffer(b[60:], "<u8"), [24, 40, 48, 60])
    inv = np.array([1, 0, 2, 4, 3], np.int32)
    off, ids, counts = a48ref.paths_index(np.array([2, 0, 1]), np.array([4, 1, 0]), inv)
    assert np.array_equal(off, [0, 1, 2, 2, 2, 3]) and np.array_equal(ids, [2, 0, 0]) and np.array_equal(counts, [2, 2, 0, 1, 1])
    graphio.write_paths_index(tmp_path / "i", tmp_path / "c", off, ids, counts)
    r_off, r_ids = a48ref.parse_paths_inv((tmp_path / "i").read_bytes())
    assert np.array_equal(r_off, off) and np.array_equal(r_ids, ids)
    assert np.array_equal(a48ref.parse_countsb((tmp_path / "c").read_bytes()), counts)
    off0, ids0, counts0 = a48ref.paths_index(zu, z32, inv)          # a graph, and no path entry at all
    graphio.write_paths_index(tmp_path / "i0", tmp_path / "c0", off0, ids0, counts0)
    r_off, r_ids = a48ref.parse_paths_inv((tmp_path / "i0").read_bytes())
    assert np.array_equal(r_off, np.zeros(6, np.uint64)) and len(r_ids) == 0
    assert np.array_equal(a48ref.parse_countsb((tmp_path / "c0").read_bytes()), np.zeros(5, np.int32))
    graphio.write_dup(tmp_path / "d0", np.zeros(0, np.uint8))
    assert (tmp_path / "d0").read_bytes() == b"BINWRITE" + bytes(8)
    with pytest.raises(Exception):
        graphio.write_paths_index(tmp_path / "bad", None, np.array([0, 2, 1], np.uint64), np.zeros(1, np.uint64), np.zeros(2, np.int32))
