"""Hand-made read paths for the stages that run after the pather -- test infrastructure (tests/test_gpu_dups_handmade.py,
tests/test_gpu_paths_index_handmade.py, tests/test_handpaths_host.py).

Two things: thin ctypes callers of snk_dev_mark_dups and snk_dev_paths_index on host arrays uploaded as they are (DupsCall, PidxCall, in
the style of Call in test_gpu_ebcx.py: *out comes in full of 0xA5; EbcxCall is that Call for the fuzz tool), and a generator of read pairs with paths for MarkDups whose first
edges and offsets come from small palettes, so that the width of the sort key (snk_dups.hip: bits(max edge) + bits(max offset - min
offset) + 10) is chosen by the test and not by a pather.  Nothing here needs a GPU until a caller is made.  (The upload and download helpers are tests/devcall.py's.)"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from devcall import _dev, _zeroed, download

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
HEADS = np.array([[0, 1, 2, 3, 0], [3, 3, 1, 0, 2], [0, 1, 2, 3, 1]], np.uint8)       # the first five bases of every read


# ---- the generator

def dup_pairs(rng, n_pairs, L, edges, offsets, n_heads=3, placed=0.8, short=0.2, twins=0.0, pins=()):
    """Read pairs (reads 2q, 2q+1) with paths.  Every read starts with one of HEADS[:n_heads], goes on with one of 3 bodies and has one of 3
    quality rows (two of them with the same sum, the third one larger), so identical reads and quality-sum ties are common; a share
    `short` of the reads has a length from 5 to L with base codes 0 behind it (the qualities behind it stay: garbage); a share `placed`
    has a path of 1-3 edges whose first edge and offset come from the palettes `edges` (>= 0) and `offsets`; bc per pair from {0, 1, 2}.
    twins: this share of the pairs has read 2q+1 identical to read 2q (bases, qualities, length) and placed like it.
    pins: [(edge, offset), ...] -- read i is placed there whatever was drawn (the extremes that fix the key's width).
    -> namespace(codes u8[n, L], quals u8[n, L], lens u16[n], bc i32[n], path_off i32[n], path_n u32[n], path_edges i32[sum])"""
    n = 2 * n_pairs
    edges, offsets = np.asarray(edges, np.int64), np.asarray(offsets, np.int64)
    assert L >= 8 and edges.min() >= 0 and edges.max() <= INT32_MAX and offsets.min() >= INT32_MIN and offsets.max() <= INT32_MAX
    bodies = rng.integers(0, 4, (3, L - 5), dtype=np.uint8)
    q0 = rng.integers(15, 41, L, dtype=np.uint8)
    q0[1], q0[2] = 20, 30
    q1, q2 = q0.copy(), q0.copy()
    q1[1], q1[2] = 30, 20                                          # the same sum at any length >= 5, other qualities
    q2[0] += 1                                                      # a larger sum
    qrows = np.stack([q0, q1, q2])
    codes = np.concatenate([HEADS[rng.integers(0, n_heads, n)], bodies[rng.integers(0, 3, n)]], axis=1)
    quals = qrows[rng.integers(0, 3, n)]
    lens = np.where(rng.random(n) < short, rng.integers(5, L + 1, n), L).astype(np.uint16)
    has = rng.random(n) < placed
    first = edges[rng.integers(0, len(edges), n)]
    off = offsets[rng.integers(0, len(offsets), n)]
    tw = np.nonzero(rng.random(n_pairs) < twins)[0]
    for a in (codes, quals, lens, first, off):
        a[2 * tw + 1] = a[2 * tw]
    has[2 * tw] = has[2 * tw + 1] = True
    for i, (e, o) in enumerate(pins[:n]):
        has[i], first[i], off[i] = True, e, o
    codes[np.arange(L)[None, :] >= lens[:, None]] = 0
    path_n = np.where(has, rng.integers(1, 4, n), 0).astype(np.uint32)
    start = np.concatenate([[0], np.cumsum(path_n.astype(np.int64))])
    path_edges = edges[rng.integers(0, len(edges), int(start[-1]))]
    path_edges[start[:-1][has]] = first[has]
    bc = np.repeat(rng.integers(0, 3, n_pairs), 2).astype(np.int32)
    return SimpleNamespace(codes=codes, quals=np.ascontiguousarray(quals), lens=lens, bc=bc, path_off=np.where(has, off, 0).astype(np.int32),
                           path_n=path_n, path_edges=path_edges.astype(np.int32))


def bits_of(v: int) -> int:
    return int(v).bit_length()


def total_bits(d) -> int:
    """the width snk_dups.hip derives from the placed reads: bits(max first edge) + bits(max offset - min offset) + 10 head bits"""
    has = d.path_n > 0
    if not has.any():
        return 10
    start = np.concatenate([[0], np.cumsum(d.path_n.astype(np.int64))])[:-1]
    first, off = d.path_edges[start[has]].astype(np.int64), d.path_off[has].astype(np.int64)
    return bits_of(first.max()) + bits_of(off.max() - off.min()) + 10


def group_view(d, lens=None, bc=None):
    """MarkDups' groups, restated from its definition (include/snk.h): the placed reads ordered by (first edge, offset, head of the MATE,
    read id), cut where one of the first three changes.  -> namespace(groups = [(edge, offset, head, ids ascending)] of the groups with
    more than one read, and over them: n_dup_reads, n_interdup_reads (a group's barcode is its first member's, or while that is 0 the
    next member's), n_ties (groups in which a member's quality sum over both mates equals the running maximum of the walk),
    mates_together = [(pair, decisive, tie)] for every group that holds both reads of a pair with the two identical; decisive: no earlier
    member of the group is identical to them, so only the look at the next member finds the copy; tie: the group has a tie, so the
    artifact check runs on it)."""
    n = len(d.path_n)
    lens = np.asarray(d.lens if lens is None else lens, np.int64)
    bc = np.asarray(d.bc if bc is None else bc, np.int64)
    has = np.nonzero(d.path_n > 0)[0]
    start = np.concatenate([[0], np.cumsum(d.path_n.astype(np.int64))])[:-1]
    first, off = d.path_edges[start[has]].astype(np.int64), d.path_off[has].astype(np.int64)
    head = (d.codes[has ^ 1, :5].astype(np.int64) * np.array([256, 64, 16, 4, 1])).sum(axis=1) if len(has) else np.zeros(0, np.int64)
    order = np.lexsort((has, head, off, first))
    ids, first, off, head = has[order], first[order], off[order], head[order]
    cut = np.concatenate([[True], (first[1:] != first[:-1]) | (off[1:] != off[:-1]) | (head[1:] != head[:-1]), [True]]) if len(ids) else np.array([True])
    at = np.nonzero(cut)[0]
    inside = np.arange(d.codes.shape[1])[None, :] < lens[:, None]
    qs = (d.quals.astype(np.int64) * inside).sum(axis=1)
    qsum = qs + qs[np.arange(n) ^ 1] if n else qs
    same = lambda x, y: lens[x] == lens[y] and np.array_equal(d.codes[x, :lens[x]], d.codes[y, :lens[y]]) and np.array_equal(d.quals[x, :lens[x]], d.quals[y, :lens[y]])
    v = SimpleNamespace(groups=[], n_dup_reads=0, n_interdup_reads=0, n_ties=0, mates_together=[])
    for a, b in zip(at[:-1], at[1:]):
        if b - a < 2:
            continue
        g = ids[a:b]
        v.groups.append((int(first[a]), int(off[a]), int(head[a]), g))
        v.n_dup_reads += len(g) - 1
        code, inter = int(bc[g[0]]), False
        for r in g[1:]:
            if code == 0:
                code = int(bc[r])
            elif int(bc[r]) != code:
                inter = True
        v.n_interdup_reads += (len(g) - 1) if inter else 0
        q, tie = int(qsum[g[0]]), False
        for r in g[1:]:
            tie |= int(qsum[r]) == q
            q = max(q, int(qsum[r]))
        v.n_ties += int(tie)
        for i in np.nonzero((g[1:] == g[:-1] + 1) & (g[:-1] % 2 == 0))[0]:
            if same(g[i], g[i + 1]):
                v.mates_together.append((int(g[i]) // 2, not any(same(g[i], y) for y in g[:i]), tie))
    return v


def high_bit_twins(groups, edge_bit):
    """-> (pairs of multi-read groups with the same offset and head whose edges differ in bit `edge_bit` only, pairs with the same edge and
    head whose offsets differ in bit 31 only, pairs whose edges or offsets differ in bit 0 only)"""
    keys = {(e, o, h) for e, o, h, _ in groups}
    def flip(o, bit):                                               # bit `bit` of an int32, flipped
        u = (o & 0xFFFFFFFF) ^ (1 << bit)
        return u - (1 << 32) if u >= 1 << 31 else u
    by_edge = sum((e ^ (1 << edge_bit), o, h) in keys for e, o, h in keys) // 2 if edge_bit >= 0 else 0
    by_off = sum((e, flip(o, 31), h) in keys for e, o, h in keys) // 2
    by_low = (sum((e ^ 1, o, h) in keys for e, o, h in keys) + sum((e, flip(o, 0), h) in keys for e, o, h in keys)) // 2
    return by_edge, by_off, by_low


# ---- the MarkDups cases (shared by the GPU test and the host test that checks what they rest on)

_WIDE_OFF = [INT32_MIN, INT32_MAX, 12345, 12345 - 2**31, 12344, 0]            # o and o - 2^31 differ in bit 31 only (so do 0 and -2^31); 12345 / 12344 in bit 0
_E31 = [2**31 - 1, 2**30 - 1, 2**31 - 2, 0, 1]                                # 2^31 - 1 and 2^30 - 1 differ in bit 30 only
# kind -> (first edges, offsets, heads, total_bits, the top bit of an edge id, pins: the reads that carry the extremes)
KINDS = {
    "tb10": ([0], [7], 3, 10, -1, [(0, 7)]),
    "narrow": ([0, 1, 2], [-3, 0, 5], 3, 16, 1, [(2, -3), (0, 5)]),
    "tb62": ([2**20 - 1, 2**19 - 1, 2**20 - 2, 0, 5], _WIDE_OFF, 1, 62, 19, [(2**20 - 1, INT32_MIN), (2**19 - 1, INT32_MAX)]),      # the last width of one sort
    "tb63": ([2**20, 0, 2**20 - 1, 2**20 - 2, 5], _WIDE_OFF, 1, 63, 20, [(2**20, INT32_MIN), (0, INT32_MAX)]),                      # the first of the fallback
    "tb73": (_E31, _WIDE_OFF, 1, 73, 30, [(2**31 - 1, INT32_MIN), (2**30 - 1, INT32_MAX)]),
    "wide_edge": (_E31, [-3, 0, 5, 4], 1, 45, 30, [(2**31 - 1, -3), (2**30 - 1, 5)]),            # 31-bit edges inside ONE sort
    "wide_off": ([0, 1, 2], _WIDE_OFF, 1, 44, 1, [(2, INT32_MIN), (0, INT32_MAX)]),              # 32-bit offsets inside one sort
    "wide_edge_3heads": (_E31, [-3, 0, 5, 4], 3, 45, 30, [(2**31 - 1, -3), (2**30 - 1, 5)]),
    "tb73_3heads": (_E31, _WIDE_OFF, 3, 73, 30, [(2**31 - 1, INT32_MIN), (2**30 - 1, INT32_MAX)]),
    "one_group": ([3], [-7], 1, 12, -1, []),
    "twins": (list(range(64)), list(range(-32, 32)), 3, 22, 5, [(63, -32), (0, 31)]),
}
WIDE = ("tb62", "tb63", "tb73", "wide_edge", "wide_off")
SIZES = (1, 127, 128, 129, 2000)              # pairs: round the 256-read workgroup, and several workgroups


def _cases():
    out = {}
    for kind in ("tb10", "narrow") + WIDE:
        for n in SIZES:
            out[f"{kind}-{n}"] = dict(kind=kind, n_pairs=n)
    out["wide_edge_3heads-2000"] = dict(kind="wide_edge_3heads", n_pairs=2000)
    out["tb73_3heads-2000"] = dict(kind="tb73_3heads", n_pairs=2000)
    out["empty-0"] = dict(kind="narrow", n_pairs=0, bits=10)
    out["unplaced-129"] = dict(kind="narrow", n_pairs=129, placed=0.0, pins=[], bits=10)
    for n in (1, 129):
        out[f"one_group-{n}"] = dict(kind="one_group", n_pairs=n, placed=1.0)
    out["one_group-2000"] = dict(kind="one_group", n_pairs=2000, placed=1.0, short=0.0)       # (one thread walks the group: full-length reads find their copy at once)
    out["twins-2000"] = dict(kind="twins", n_pairs=2000, twins=0.5)
    out["narrow-129-L151"] = dict(kind="narrow", n_pairs=129, L=151, pad_seed=151)
    for which in ("lens", "bc", "lens_bc"):
        out[f"narrow-129-null_{which}"] = dict(kind="narrow", n_pairs=129, null=which)
    return out


DUPS_CASES = _cases()
_made: dict = {}


def dups_case(name):
    """-> namespace(d: the reads and paths, bits: the key width the case is named for, edge_bit, null_lens, null_bc, pad_seed, lens / bc
    as the oracle has to see them, oracle: (dup, art, rate, n_dup_reads, n_interdup_reads) of oracle_lib.mark_dups).  Made once."""
    if name in _made:
        return _made[name]
    import zlib
    import oracle_lib
    s = DUPS_CASES[name]
    edges, offsets, n_heads, bits, edge_bit, pins = KINDS[s["kind"]]
    L = s.get("L", 24)
    d = dup_pairs(np.random.default_rng(zlib.crc32(name.encode())), s["n_pairs"], L, edges, offsets, n_heads, placed=s.get("placed", 0.8),
                  short=s.get("short", 0.2), twins=s.get("twins", 0.0), pins=s.get("pins", pins))
    null = s.get("null", "")
    c = SimpleNamespace(name=name, d=d, L=L, bits=s.get("bits", bits), edge_bit=edge_bit, null_lens="lens" in null, null_bc="bc" in null, pad_seed=s.get("pad_seed"))
    c.lens = np.full(len(d.lens), L, np.uint16) if c.null_lens else d.lens
    c.bc = None if c.null_bc else d.bc
    c.oracle = oracle_lib.mark_dups(d.codes, d.quals, c.lens, d.path_off, d.path_n.astype(np.int64), d.path_edges, bc=c.bc)
    _made[name] = c
    return c


# ---- the callers

def dev_shifted(a, shift):
    """int32 values on the device, the first one `shift` words behind a 16-byte boundary"""
    import torch
    buf = torch.zeros(len(a) + 8, dtype=torch.int32, device=torch.device("cuda", 0))
    lead = (-(buf.data_ptr() // 4)) % 4 + shift
    view = buf[lead:lead + len(a)]
    view.copy_(torch.from_numpy(np.asarray(a, np.int32)))
    assert len(a) == 0 or view.data_ptr() % 16 == 4 * shift            # (an empty view has no address)
    return view


class _Paths:
    """snk_dev_paths over host arrays: n_edges u32, start (their exclusive scan unless given), edges, offset"""

    def __init__(self, n_edges, edges, offset=None, shift=0, n_edges_total=None, n_reads=None, start=None):
        from supernova_amd import lib as _lib
        self.ne = np.asarray(n_edges, np.uint32)
        self.edges = np.asarray(edges, np.int32)
        self.start = np.concatenate([[0], np.cumsum(self.ne.astype(np.int64))]).astype(np.int64) if start is None else np.asarray(start, np.int64)
        self.d_ne, self.d_start, self.d_edges = _dev(self.ne.view(np.int32), np.int32), _dev(self.start, np.int64), dev_shifted(self.edges, shift)
        self.d_off = _dev(np.zeros(len(self.ne), np.int32) if offset is None else offset, np.int32)
        p = self.struct = _lib.SnkDevPaths()
        p.n_reads = len(self.ne) if n_reads is None else n_reads
        p.n_edges_total = len(self.edges) if n_edges_total is None else n_edges_total
        p.offset, p.n_edges, p.start, p.edges = self.d_off.data_ptr(), self.d_ne.data_ptr(), self.d_start.data_ptr(), self.d_edges.data_ptr()


class DupsCall:
    """One call of snk_dev_mark_dups on the reads and paths of dup_pairs.  *out comes in full of 0xA5."""

    def __init__(self, engine, d, null_lens=False, null_bc=False, pad_seed=None, paths_n_reads=None):
        import pathgen
        from supernova_amd import lib as _lib
        n, L = d.codes.shape
        self.dev = pathgen.to_device(d.codes, d.quals, d.lens, d.bc, pad_seed=pad_seed)
        rows, dq, dl, dbc = self.dev
        r = _lib.SnkDevReads()
        r.n_reads, r.rows, r.row_words, r.read_len = n, rows.data_ptr(), rows.shape[1], L
        r.quals, r.qstride = dq.data_ptr(), dq.shape[1]
        r.lens = None if null_lens else dl.data_ptr()
        r.bc = None if null_bc else dbc.data_ptr()
        self.paths = _Paths(d.path_n, d.path_edges, d.path_off, n_reads=paths_n_reads)
        self.out = _lib.SnkDevDups()
        C.memset(C.addressof(self.out), 0xA5, C.sizeof(self.out))
        self.err = C.create_string_buffer(512)
        self.rc = engine.lib.snk_dev_mark_dups(engine._ctx, C.byref(r), C.byref(self.paths.struct), C.byref(self.out), engine._stream(), self.err, 512)
        self.dup = download(engine, self.out.dup, int(self.out.n_pairs), np.uint8) if self.rc == 0 else None

    def zeroed(self):
        return _zeroed(self.out)

    def counters(self):
        o = self.out
        return (int(o.n_dup_reads), int(o.n_interdup_reads), int(o.n_dup_pairs), int(o.n_art_pairs), int(o.n_placed), float(o.interdup_rate))


class PidxCall:
    """One call of snk_dev_paths_index on paths uploaded from host arrays.  *out comes in full of 0xA5."""

    def __init__(self, engine, n_edges, edges, inv, shift=0, n_edges_total=None, start=None):
        from supernova_amd import lib as _lib
        self.inv = np.ascontiguousarray(inv, dtype=np.int32)
        E = len(self.inv)
        self.paths = _Paths(n_edges, edges, shift=shift, n_edges_total=n_edges_total, start=start)
        self.out = _lib.SnkDevPidx()
        C.memset(C.addressof(self.out), 0xA5, C.sizeof(self.out))
        self.err = C.create_string_buffer(512)
        self.rc = engine.lib.snk_dev_paths_index(engine._ctx, C.byref(self.paths.struct), E, self.inv.ctypes.data if E else None, C.byref(self.out),
                                                 engine._stream(), self.err, 512)
        self.off = self.ids = self.counts = None
        if self.rc == 0:
            o = self.out
            assert int(o.n_hbv_edges) == E
            self.off = download(engine, o.index_off, E + 1, np.uint64)
            self.ids = download(engine, o.index_ids, int(o.n_entries), np.uint64)
            self.counts = download(engine, o.counts, E, np.int32)

    def zeroed(self):
        return _zeroed(self.out)


class EbcxCall:
    """One call of snk_dev_edge_barcodes on paths uploaded from host arrays (tests/tools/fuzz_paths.py: the general sort, reads reordered)."""

    def __init__(self, engine, n_edges, edges, bc, inv, flags=0):
        from supernova_amd import lib as _lib
        self.inv = np.ascontiguousarray(inv, dtype=np.int32)
        E = len(self.inv)
        self.paths = _Paths(n_edges, edges)
        self.d_bc = _dev(bc, np.int32)
        self.out = _lib.SnkDevEbcx()
        C.memset(C.addressof(self.out), 0xA5, C.sizeof(self.out))
        self.err = C.create_string_buffer(512)
        self.rc = engine.lib.snk_dev_edge_barcodes(engine._ctx, C.byref(self.paths.struct), self.d_bc.data_ptr(), E, self.inv.ctypes.data if E else None, flags,
                                                   C.byref(self.out), engine._stream(), self.err, 512)
        self.off = self.bcs = None
        if self.rc == 0:
            self.off = download(engine, self.out.ebc_off, E + 1, np.uint64)
            self.bcs = download(engine, self.out.ebc, int(self.out.n_ebc), np.int32)
