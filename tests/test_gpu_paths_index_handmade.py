"""snk_dev_paths_index (csrc/snk_pidx.hip) on hand-made paths (tests/handpaths.py) against the numpy restatement of writePathsIndex
(a48ref.paths_index, pinned to the reference's a.paths.inv / a.countsb by test_a48_files.py), with ebcxref.toy_involution (an odd E has
a self-inverse last edge): graphs of 1 to 65537 edges -- every width of the sort key from 0 to 17 bits that these give -- entry
counts over every n % 4 and round the workgroup of the offsets kernel, runs of empty edges as long as the graph, and the refusals.

Not tested: the refusal of a read support above 2^31 - 1 (a.countsb holds int).  It needs 2^31 path entries, about 60 GB of arena."""
import numpy as np
import pytest

import a48ref
import ebcxref
import handpaths

pytestmark = pytest.mark.gpu
SNK_E_ARG = -1
E_ALL = [1, 2, 3, 255, 256, 257, 65536, 65537]
N_ALL = [0, 1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4099]           # every n % 4; (n + 3) / 4 work items: 256 a workgroup at 1024, 257 at 1025


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


def _key_bits(E):
    return int(E - 1).bit_length() if E > 1 else 0                 # ceil(log2 E)


def _reads(rng, n):
    """n path entries cut into reads of 0..5 edges, with empty reads in between and at both ends -> n_edges u32[]"""
    ne = [0]
    while sum(ne) < n:
        ne.append(min(int(rng.integers(0, 6)), n - sum(ne)))
    return np.array(ne + [0, 0], np.uint32)


def _expect(c, n_edges, edges, inv):
    """offsets, ids, counts and every counter of a good call against the restatement"""
    assert c.rc == 0, c.err.value
    E = len(inv)
    x_off, x_ids, x_counts = a48ref.paths_index(n_edges, edges, inv)
    assert np.array_equal(c.off, x_off), ("index_off", np.nonzero(c.off != x_off)[0][:5])
    assert np.array_equal(c.ids, x_ids), ("index_ids", np.nonzero(c.ids != x_ids)[0][:5])
    assert np.array_equal(c.counts, x_counts), ("counts", np.nonzero(c.counts != x_counts)[0][:5])
    o = c.out
    assert (int(o.n_entries), int(o.n_hbv_edges), int(o.n_empty_edges)) == (len(edges), E, int((np.diff(x_off.astype(np.int64)) == 0).sum()))
    assert int(o.key_bits) == _key_bits(E)


def _shapes(rng, E, n):
    """name -> edge ids of n entries"""
    kb = _key_bits(E)
    out = {"uniform": rng.integers(0, E, n), "all_on_0": np.zeros(n, np.int64), "all_on_last": np.full(n, E - 1)}
    top = 1 << (kb - 1) if kb else 0
    if top != E - 1:
        out["top_bit_and_last"] = np.where(rng.random(n) < 0.5, top, E - 1)
    if top >= 1:
        out["across_the_top_bit"] = np.where(rng.random(n) < 0.5, top, top - 1)      # in order only when the top key bit is looked at
    return out


@pytest.mark.parametrize("E", E_ALL)
def test_entry_counts_and_gaps(engine, E):
    inv = ebcxref.toy_involution(E)
    rng = np.random.default_rng(E)
    for n in N_ALL:
        ne = _reads(rng, n)
        for name, edges in _shapes(rng, E, n).items():
            try:
                _expect(handpaths.PidxCall(engine, ne, edges, inv), ne, edges, inv)
            except AssertionError as ex:
                raise AssertionError(f"E={E} n={n} {name}: {ex}") from ex


@pytest.mark.parametrize("E", E_ALL)
def test_a_read_that_holds_one_edge_200_times(engine, E):
    inv = ebcxref.toy_involution(E)
    rng = np.random.default_rng(200 + E)
    a = E // 2
    ne = np.array([0, 3, 200, 2, 0], np.uint32)
    edges = np.concatenate([rng.integers(0, E, 3), np.full(200, a), rng.integers(0, E, 2)])
    c = handpaths.PidxCall(engine, ne, edges, inv)
    _expect(c, ne, edges, inv)
    mine = c.ids[int(c.off[a]):int(c.off[a + 1])]
    assert int((mine == 2).sum()) == 200 and np.all(np.diff(mine.astype(np.int64)) >= 0)


@pytest.mark.parametrize("E", E_ALL)
def test_a_self_inverse_edge_keeps_its_own_count(engine, E):
    """Self-inverse edges next to pairs that share their sum: the last edge (and with an even E the one before it) is its own reverse
    complement."""
    inv = ebcxref.toy_involution(E)
    if E % 2 == 0:
        inv[E - 1], inv[E - 2] = E - 1, E - 2
    selfs = sorted({E - 1, E - 2 if E % 2 == 0 else E - 1})
    edges = [s for i, s in enumerate(selfs) for _ in range(4 + 3 * i)]
    if E >= 4:
        edges += [0] * 3 + [1] * 5 + [3] * 2                       # (0, 1) share 8; (2, 3) share 2, edge 2 has no entry of its own
    edges = np.random.default_rng(E).permutation(np.array(edges, np.int64))
    ne = _reads(np.random.default_rng(E + 1), len(edges))
    c = handpaths.PidxCall(engine, ne, edges, inv)
    _expect(c, ne, edges, inv)
    assert [int(c.counts[s]) for s in selfs] == [4 + 3 * i for i in range(len(selfs))]
    if E >= 4:
        assert c.counts[:4].tolist() == [8, 8, 2, 2] and int(c.off[3] - c.off[2]) == 0


def test_no_entries_and_no_edges(engine):
    c = handpaths.PidxCall(engine, [], [], np.zeros(0, np.int32))
    assert c.rc == 0 and c.off.tolist() == [0] and len(c.ids) == 0 and len(c.counts) == 0
    assert (int(c.out.n_entries), int(c.out.n_hbv_edges), int(c.out.n_empty_edges), int(c.out.key_bits)) == (0, 0, 0, 0)
    c = handpaths.PidxCall(engine, [0, 0, 0], [], np.zeros(0, np.int32))          # reads, none with a path
    assert c.rc == 0 and c.off.tolist() == [0]


def test_refusals_leave_out_zero_and_the_context_usable(engine):
    E, n = 257, 1025
    inv = ebcxref.toy_involution(E)
    rng = np.random.default_rng(7)
    ne, edges = _reads(rng, n), rng.integers(0, E, n)

    def refused(c, words):
        assert c.rc == SNK_E_ARG and words in c.err.value, (c.rc, c.err.value)
        assert c.zeroed()
        _expect(handpaths.PidxCall(engine, ne, edges, inv), ne, edges, inv)       # the same context goes on working

    for shift in (1, 2, 3):
        refused(handpaths.PidxCall(engine, ne, edges, inv, shift=shift), b"not 16-byte aligned")
    for at in (0, n // 2, n - 1):
        e = edges.copy()
        e[at] = E
        refused(handpaths.PidxCall(engine, ne, e, inv), f"edge id {E},".encode())
    e = edges.copy()
    e[n // 3] = -1
    refused(handpaths.PidxCall(engine, ne, e, inv), b"edge id -1,")
    long_ne = ne.copy()
    long_ne[-1] += 1                                               # the last read reaches past the entry table
    refused(handpaths.PidxCall(engine, long_ne, edges, inv, n_edges_total=n), b"do not add up")
    refused(handpaths.PidxCall(engine, ne, edges, inv, n_edges_total=n - 1), b"do not add up")
    start = np.concatenate([[0], np.cumsum(ne.astype(np.int64))])
    start[len(ne) // 2] = n + 1                                    # a start behind the table
    refused(handpaths.PidxCall(engine, ne, edges, inv, start=start), b"do not add up")
    refused(handpaths.PidxCall(engine, ne, np.zeros(n, np.int64), np.zeros(0, np.int32)), b"without edges")
