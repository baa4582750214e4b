"""snk_dev_edge_barcodes (csrc/snk_ebcx.hip): the edge -> barcode lists of computeEdgeToBarcodeX (10X/PathsIndex.cc:297-358) on the device
against the lists the reference's own code wrote (tests/golden/ebcx/), on both sort paths and in any read order; the edges of its kernels on
synthetic paths against the numpy restatement (tests/ebcxref.py); its refusals."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import ebcxref
import goldens
import pathgen

pytestmark = pytest.mark.gpu
SNK_E_ARG, SNK_E_UNSUPPORTED = -1, -6
GENERAL = 1                                     # SNK_EBC_GENERAL_SORT
TILE = 1024                                     # keys of a workgroup's tile in snk_ebcx.hip (256 threads, 4 keys each)


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
    return torch.from_numpy(np.array(a, dtype=dtype)).to(torch.device("cuda", 0))


def _dev_shifted(a, shift):
    """int32 values on the device, the first one `shift` words behind a 16-byte boundary"""
    import torch
    buf = torch.zeros(len(a) + 8, dtype=torch.int32, device=torch.device("cuda", 0))
    lead = (-(buf.data_ptr() // 4)) % 4 + shift
    view = buf[lead:lead + len(a)]
    view.copy_(torch.from_numpy(np.asarray(a, np.int32)))
    assert len(a) == 0 or view.data_ptr() % 16 == 4 * shift            # (an empty view has no address)
    return view


class Call:
    """One call of snk_dev_edge_barcodes on paths uploaded from host arrays.  *out comes in full of 0xA5."""

    def __init__(self, engine, n_edges, edges, bc, inv, flags=0, shift=0, n_edges_total=None, null_bc=False):
        from supernova_amd import lib as _lib
        self.ne = np.asarray(n_edges, np.uint32)
        self.edges = np.asarray(edges, np.int32)
        self.start = np.concatenate([[0], np.cumsum(self.ne.astype(np.int64))]).astype(np.int64)
        self.inv = np.ascontiguousarray(inv, dtype=np.int32)
        self.d_ne, self.d_start = _dev(self.ne.view(np.int32), np.int32), _dev(self.start, np.int64)
        self.d_edges, self.d_bc = _dev_shifted(self.edges, shift), _dev(np.asarray(bc, np.int32), np.int32)
        p = _lib.SnkDevPaths()
        p.n_reads, p.n_edges_total = len(self.ne), len(self.edges) if n_edges_total is None else n_edges_total
        p.n_edges, p.start, p.edges = self.d_ne.data_ptr(), self.d_start.data_ptr(), self.d_edges.data_ptr()
        self.out = _lib.SnkDevEbcx()
        C.memset(C.addressof(self.out), 0xA5, C.sizeof(self.out))
        self.err = C.create_string_buffer(512)
        E = len(self.inv)
        self.rc = engine.lib.snk_dev_edge_barcodes(engine._ctx, C.byref(p), None if null_bc else self.d_bc.data_ptr(), E, self.inv.ctypes.data if E else None, flags,
                                                   C.byref(self.out), engine._stream(), self.err, 512)
        self.off = self.bcs = None
        if self.rc == 0:
            o = self.out
            assert int(o.n_hbv_edges) == E
            self.off = _download(engine, o.ebc_off, (E + 1) * 8, np.uint64)
            self.bcs = _download(engine, o.ebc, int(o.n_ebc) * 4, np.int32)

    def zeroed(self):
        return C.string_at(C.addressof(self.out), C.sizeof(self.out)) == bytes(C.sizeof(self.out))

    def paths_untouched(self):
        return (np.array_equal(self.d_ne.cpu().numpy().view(np.uint32), self.ne) and np.array_equal(self.d_start.cpu().numpy(), self.start)
                and np.array_equal(self.d_edges.cpu().numpy(), self.edges))


def _download(engine, ptr, nbytes, dtype):
    host = np.zeros(max(nbytes, 1), np.uint8)
    if nbytes:
        engine._download(ptr, host.ctypes.data, nbytes)
    return host[:nbytes].view(dtype).copy()


def _expect(c, n_edges, edges, bc, inv, flags):
    """the lists and every statistic of a good call against the restatement"""
    assert c.rc == 0, c.err.value
    x_off, x_bcs = ebcxref.edge_barcodes(n_edges, edges, bc, inv)
    assert np.array_equal(c.off, x_off), "ebc_off"
    assert np.array_equal(c.bcs, x_bcs), "ebc"
    st = ebcxref.stats(x_off)
    o = c.out
    bc = np.asarray(bc, np.int64)
    pos = bc[bc > 0]
    is_sorted = int(np.all(np.diff(pos) >= 0))
    assert (int(o.n_ebc), int(o.n_empty_edges), int(o.max_list)) == (st["n_ebc"], st["n_empty_edges"], st["max_list"])
    assert int(o.n_keys) == 2 * int(np.asarray(n_edges, np.int64)[bc > 0].sum())
    assert int(o.bc_sorted) == is_sorted and int(o.general_sort) == int(bool(flags & GENERAL) or not is_sorted)
    assert int(o.key_bits) == max(0, int(np.ceil(np.log2(max(len(inv), 1)))))


# ---- 1. the reference's lists, on both sort paths
@pytest.mark.parametrize("name", ebcxref.CASES)
def test_fixture_parity_on_both_sort_paths(engine, tmp_path, name):
    from supernova_amd import graphio
    f = ebcxref.load(name)
    off, bcs = ebcxref.parse_ebcx(f.ebcx)
    for flags in (0, GENERAL):
        c = Call(engine, f.n_edges, f.edges, f.bc, f.inv, flags)
        assert c.rc == 0, c.err.value
        assert np.array_equal(c.off, off) and np.array_equal(c.bcs, bcs), flags
        graphio.write_ebcx(tmp_path / "a.ebcx", c.off, c.bcs)
        assert (tmp_path / "a.ebcx").read_bytes() == f.ebcx
        assert int(c.out.bc_sorted) == 1 and int(c.out.general_sort) == (1 if flags else 0)
        _expect(c, f.n_edges, f.edges, f.bc, f.inv, flags)


# ---- 2. the order of the reads does not matter
@pytest.mark.parametrize("name", ebcxref.CASES)
def test_shuffled_reads_give_the_same_lists(engine, name):
    f = ebcxref.load(name)
    off, bcs = ebcxref.parse_ebcx(f.ebcx)
    start = np.concatenate([[0], np.cumsum(f.n_edges.astype(np.int64))])
    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(len(f.n_edges))
        edges = np.concatenate([f.edges[start[r]:start[r + 1]] for r in perm])
        c = Call(engine, f.n_edges[perm], edges, f.bc[perm], f.inv, 0)
        assert c.rc == 0, c.err.value
        assert int(c.out.bc_sorted) == 0 and int(c.out.general_sort) == 1
        assert np.array_equal(c.off, off) and np.array_equal(c.bcs, bcs), seed


# ---- 3. from the reads, through Result.path_reads
@pytest.mark.parametrize("name", ["adversarial", "synth_20k_err"])
def test_end_to_end_from_the_reads(engine, name):
    import a48ref
    c = goldens.load(name)
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    inv = a48ref.parse_inv(c.exp_ainv)
    got = []
    for mode in (True, True, "general"):
        _, ne, edges, info = res.path_reads(rows, c.read_len, dq, lens=dl, bc=dbc, ebcx=mode)
        x_off, x_bcs = ebcxref.edge_barcodes(ne, edges, c.bc, inv)
        off, bcs = info["ebcx"]
        assert off.dtype == np.uint64 and bcs.dtype == np.int32
        assert np.array_equal(off, x_off) and np.array_equal(bcs, x_bcs)
        st = info["ebcx_stats"]
        assert st["n_ebc"] == len(bcs) and st["n_hbv_edges"] == len(inv) and st["n_keys"] == 2 * int(ne.astype(np.int64)[c.bc > 0].sum())
        got.append((off, bcs))
    assert all(np.array_equal(got[0][0], g[0]) and np.array_equal(got[0][1], g[1]) for g in got[1:])
    _, _, _, info = res.path_reads(rows, c.read_len, dq, lens=dl, bc=dbc, ebcx=True, download=False)
    assert "ebcx" not in info and info["ebcx_stats"]["n_ebc"] == len(got[0][1])
    with pytest.raises(ValueError):
        res.path_reads(rows, c.read_len, dq, lens=dl, ebcx=True)


# ---- 4. the edges of the kernels
N_PAIRS = sorted({0, 1, 3, 4, 255, 256, 257} | {TILE // 2 - 1, TILE // 2, TILE // 2 + 1, TILE + 1})     # key counts 2n: 16-byte tails and both tile boundaries


def _random_paths(rng, E, n):
    """n path entries in reads of 0..5 edges (the last may be cut), random edges, bc in -1 .. 6"""
    ne = []
    while sum(ne) < n:
        ne.append(min(int(rng.integers(0, 6)), n - sum(ne)))
    ne += [0, 0]
    ne = np.array(ne, np.uint32)
    return ne, rng.integers(0, E, n).astype(np.int32), rng.integers(-1, 7, len(ne)).astype(np.int32)


@pytest.mark.parametrize("E", [1, 2, 255, 256, 257, 4097])
def test_key_counts_round_the_tails_and_tiles(engine, E):
    inv = ebcxref.toy_involution(E)
    rng = np.random.default_rng(E)
    for n in N_PAIRS:
        ne, edges, bc = _random_paths(rng, E, n)
        bc[bc > 0] += 100                                          # every read with a barcode contributes: the key count is 2n when none is <= 0
        for which in ("all", "mixed"):
            b = np.where(bc > 0, bc, 1 + np.arange(len(bc)) % 3).astype(np.int32) if which == "all" else bc
            order = np.argsort(b, kind="stable")
            start = np.concatenate([[0], np.cumsum(ne.astype(np.int64))])
            s_edges = np.concatenate([edges[start[r]:start[r + 1]] for r in order]) if n else edges
            for shift in range(4):
                for flags in (0, GENERAL):
                    _expect(Call(engine, ne, edges, b, inv, flags, shift), ne, edges, b, inv, flags)                       # reads in any order
                    c = Call(engine, ne[order], s_edges, b[order], inv, flags, shift)                                       # ... and sorted by barcode
                    _expect(c, ne[order], s_edges, b[order], inv, flags)
                    if which == "all":
                        assert int(c.out.n_keys) == 2 * n


@pytest.mark.parametrize("E", [1, 2, 255, 256, 257, 4097])
def test_extreme_lists(engine, E):
    inv = ebcxref.toy_involution(E)
    rng = np.random.default_rng(100 + E)
    for flags in (0, GENERAL):
        # no read with a barcode: every list empty
        ne, edges, bc = _random_paths(rng, E, 300)
        c = Call(engine, ne, edges, np.minimum(bc, 0), inv, flags)
        _expect(c, ne, edges, np.minimum(bc, 0), inv, flags)
        assert int(c.out.n_empty_edges) == E and int(c.out.n_ebc) == 0 and int(c.out.n_keys) == 0 and not c.off.any()
        # no reads at all
        c = Call(engine, [], [], [], inv, flags)
        _expect(c, [], [], [], inv, flags)
        assert int(c.out.n_empty_edges) == E
        # one barcode on every edge
        ne, edges = np.full(E, 1, np.uint32), np.arange(E, dtype=np.int32)
        c = Call(engine, ne, edges, np.full(E, 7, np.int32), inv, flags)
        _expect(c, ne, edges, np.full(E, 7, np.int32), inv, flags)
        assert int(c.out.n_empty_edges) == 0 and int(c.out.max_list) == 1 and np.all(c.bcs == 7)
        # every read its own barcode on one edge: a list of 3000, over several tiles of the compaction
        a = E // 2
        ne, edges, bc = np.full(3000, 1, np.uint32), np.full(3000, a, np.int32), (1 + np.arange(3000)).astype(np.int32)
        c = Call(engine, ne, edges, bc, inv, flags)
        _expect(c, ne, edges, bc, inv, flags)
        assert int(c.out.max_list) == 3000 and np.array_equal(c.bcs[int(c.off[a]):int(c.off[a + 1])], bc)
        # only edge E - 1 is visited (by several reads of two barcodes): one long gap before it
        ne, edges, bc = np.full(5, 2, np.uint32), np.full(10, E - 1, np.int32), np.array([3, 3, 0, 9, 9], np.int32)
        c = Call(engine, ne, edges, bc, inv, flags)
        _expect(c, ne, edges, bc, inv, flags)
        assert c.bcs[int(c.off[E - 1]):].tolist() == [3, 9] and int(c.out.n_empty_edges) == E - len({E - 1, int(inv[E - 1])})
        # barcodes up to 2^31 - 1
        bc = np.array([1, 2**31 - 2, -(2**31), 2**31 - 1, 2**31 - 1], np.int32)
        _expect(Call(engine, ne, edges, bc, inv, flags), ne, edges, bc, inv, flags)


# ---- 5. refusals
def test_refusals_leave_out_zero_and_the_context_usable(engine):
    f = ebcxref.load("adversarial")
    E, n = f.E, len(f.edges)
    assert E > 2 and n > 10
    bad_inv = f.inv.copy()
    bad_inv[0] = bad_inv[1] = 2

    def refused(c, code, words):
        assert c.rc == code and words in c.err.value, (c.rc, c.err.value)
        assert c.zeroed()

    refused(Call(engine, f.n_edges, f.edges, f.bc, bad_inv), SNK_E_ARG, b"involution")
    for at in (0, n // 2, n - 1):
        e = f.edges.copy()
        e[at] = E
        for flags in (0, GENERAL):
            refused(Call(engine, f.n_edges, e, f.bc, f.inv, flags), SNK_E_ARG, f"edge id {E},".encode())
    e = f.edges.copy()
    e[n // 3] = -1
    refused(Call(engine, f.n_edges, e, f.bc, f.inv), SNK_E_ARG, b"edge id -1,")
    ne = f.n_edges.copy()
    ne[-1] += 1                                                    # the last read reaches past the entry table
    refused(Call(engine, ne, f.edges, f.bc, f.inv, n_edges_total=n), SNK_E_ARG, b"do not add up")
    refused(Call(engine, f.n_edges, f.edges, f.bc, f.inv, n_edges_total=n - 1), SNK_E_ARG, b"do not add up")
    refused(Call(engine, f.n_edges, f.edges, f.bc, f.inv, flags=2), SNK_E_ARG, b"flag")
    refused(Call(engine, f.n_edges, f.edges, f.bc, f.inv, flags=0x80000001), SNK_E_ARG, b"flag")
    refused(Call(engine, f.n_edges, f.edges, f.bc, f.inv, null_bc=True), SNK_E_ARG, b"NULL")
    refused(Call(engine, f.n_edges, f.edges, f.bc, f.inv, n_edges_total=2**31), SNK_E_UNSUPPORTED, b"2^31")
    c = Call(engine, f.n_edges, f.edges, f.bc, f.inv)             # the same context goes on working
    _expect(c, f.n_edges, f.edges, f.bc, f.inv, 0)
    assert np.array_equal(c.off, ebcxref.parse_ebcx(f.ebcx)[0])


# ---- 6. the paths are the caller's
@pytest.mark.parametrize("flags", [0, GENERAL])
def test_paths_are_untouched_and_calls_repeat(engine, flags):
    f = ebcxref.load("ebcx_probe")
    c = Call(engine, f.n_edges, f.edges, f.bc, f.inv, flags, shift=1)
    assert c.rc == 0 and c.paths_untouched() and np.array_equal(c.d_bc.cpu().numpy(), f.bc)
    digest = lambda c: hashlib.sha256(c.off.tobytes() + c.bcs.tobytes()).hexdigest()
    again = Call(engine, f.n_edges, f.edges, f.bc, f.inv, flags, shift=1)
    assert digest(c) == digest(again) and again.paths_untouched()
