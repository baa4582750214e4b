"""The a.48 fixtures of the compressed forms (tests/golden/a48x/*.npz: bytes the reference's own code wrote, see
tests/golden/make_a48x_golden.py) and a numpy restatement of what produced them: ReadPathVecX zip / unzip
(10X/paths/ReadPathParser.cc:18-51,106-132,184-198), the a.pathsX layout (10X/paths/ReadPathVecX.cc:976-996) and the a.hbx layout
(paths/HyperBasevector.cc:133-137, graph/DigraphTemplate.h:3107-3113).  test_a48x_files.py pins the restatement to the fixtures; the
GPU tests use it at sizes without fixtures."""
from __future__ import annotations

import hashlib
import struct
from pathlib import Path

import numpy as np

A48X = Path(__file__).resolve().parent / "golden" / "a48x"
SKIP = 10
EXTRA = ("long_unitig", "probe_paths")          # the cases beside goldens.CASES


FILES = ("a.hbx", "a.pathsX", "a.hbv", "a.inv", "tmp.paths", "a.paths.inv", "a.countsb", "a.dup")


def load(name: str) -> dict:
    """-> {file name: bytes} for the files the fixture holds (a golden case: a.hbx and a.pathsX; long_unitig: all eight; probe_paths:
    tmp.paths and a.pathsX), 'ref_summary', and for long_unitig 'reads_digest'."""
    z = np.load(A48X / f"{name}.npz")
    out = {f: bytes(z[f.replace(".", "_")]) for f in FILES if f.replace(".", "_") in z.files}
    for k in ("ref_summary", "reads_digest"):
        if k in z.files:
            out[k] = bytes(z[k])
    return out


# ---- the graph

class Graph:
    """From / To lists (CSR, in file order) and what follows from them."""

    def __init__(self, K, from_off, from_v, from_e, to_off, to_e, edges_blob, n_edges):
        self.K, self.N, self.E = K, len(from_off) - 1, n_edges
        self.from_off, self.from_v, self.from_e, self.to_off, self.to_e = from_off, from_v, from_e, to_off, to_e
        self.edges_blob = edges_blob                     # the edges_ section as a.hbv has it: u64 E, per edge u32 bases + 2-bit bytes
        self.v_left = np.zeros(n_edges, np.int32)
        self.v_right = np.zeros(n_edges, np.int32)
        self.from_pos = np.zeros(n_edges, np.int64)
        self.v_left[from_e] = np.repeat(np.arange(self.N, dtype=np.int32), np.diff(from_off))
        self.v_right[to_e] = np.repeat(np.arange(self.N, dtype=np.int32), np.diff(to_off))
        self.from_pos[from_e] = np.arange(len(from_e)) - np.repeat(from_off[:-1], np.diff(from_off))
        self.to_v = self.v_left[to_e]


def _lists(b: bytes, at: int, count_fmt: str):
    """vec<vec<int>> (u64 counts) or VecIntVec (u32 counts) -> (off i64[n+1], values i32[], position behind)."""
    n = struct.unpack_from("<Q", b, at)[0]
    at += 8
    w = struct.calcsize(count_fmt)
    off, vals = np.zeros(n + 1, np.int64), []
    for v in range(n):
        m = struct.unpack_from(count_fmt, b, at)[0]
        at += w
        vals.append(np.frombuffer(b, "<i4", m, at))
        at += 4 * m
        off[v + 1] = off[v] + m
    return off, (np.concatenate(vals) if vals else np.zeros(0, np.int32)).astype(np.int32), at


def parse_hbv(b: bytes) -> Graph:
    """a.hbv: "BINWRITE", int K, from_, from_edge_obj_, to_edge_obj_ (vec<vec<int>>), edges_."""
    assert b[:8] == b"BINWRITE"
    K = struct.unpack_from("<i", b, 8)[0]
    from_off, from_v, at = _lists(b, 12, "<Q")
    off2, from_e, at = _lists(b, at, "<Q")
    to_off, to_e, at = _lists(b, at, "<Q")
    assert np.array_equal(from_off, off2)
    E = struct.unpack_from("<Q", b, at)[0]
    assert E == len(from_e) == len(to_e)
    return Graph(K, from_off, from_v, from_e, to_off, to_e, b[at:], E)


def hbx_bytes(g: Graph) -> bytes:
    """a.hbx: "BINWRITE", int K, from_, to_, from_edge_obj_, to_edge_obj_ (VecIntVec: u64 count, per vertex u32 count + ints), edges_ (as in
    a.hbv), to_left_, to_right_ (vec<int>: u64 count + ints)."""
    def lists(off, vals):
        out = [struct.pack("<Q", len(off) - 1)]
        for v in range(len(off) - 1):
            out.append(struct.pack("<I", off[v + 1] - off[v]))
            out.append(vals[off[v]:off[v + 1]].astype("<i4").tobytes())
        return b"".join(out)
    vec = lambda a: struct.pack("<Q", len(a)) + a.astype("<i4").tobytes()
    return (b"BINWRITE" + struct.pack("<i", g.K) + lists(g.from_off, g.from_v) + lists(g.to_off, g.to_v) + lists(g.from_off, g.from_e)
            + lists(g.to_off, g.to_e) + g.edges_blob + vec(g.v_left) + vec(g.v_right))


# ---- the paths

def parse_paths(b: bytes):
    """a.paths / tmp.paths (feudal MasterVec<ReadPath>) -> (offset i32[n], n_edges u32[n], edges i32[])."""
    n32, flags, sz_fixed, sz_x, sz_a, var, fixed = struct.unpack("<IBBBBQQ", b[:24])
    tab = np.frombuffer(b[var:fixed], dtype="<u8").astype(np.int64)
    n = len(tab) - 1
    assert n == n32 and tab[0] == 24 and tab[-1] == var
    words = np.frombuffer(b[24:var], dtype="<i4")
    at = (tab[:-1] - 24) // 4
    ne = ((np.diff(tab) - 8) // 4).astype(np.uint32)
    keep = np.ones(len(words), bool)
    keep[at] = keep[at + 1] = False
    return words[at].astype(np.int32), ne, words[keep].astype(np.int32)


def rec_bytes(n):
    n = np.asarray(n, dtype=np.int64)
    return np.where(n > 0, 7 + (n + 2) // 4, 1)


def zip_paths(offset, n_edges, edges, g: Graph):
    """-> (index i64[ceil(n / 10)], data u8[], dict of the three counters).  A step e -> e' is found iff v_left[e'] == v_right[e]; its id
    is the position of e' in From(v_left[e']); a step not found writes nothing and does not move the bit cursor."""
    ne = np.asarray(n_edges, dtype=np.int64)
    offset = np.asarray(offset, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.int64)
    n = len(ne)
    assert ne.max(initial=0) <= 255 and g.from_pos.max(initial=0) <= 3
    start = np.concatenate([[0], np.cumsum(ne)])
    off = np.concatenate([[0], np.cumsum(rec_bytes(ne))])
    data = np.zeros(off[-1], np.uint8)
    data[off[:-1]] = ne
    has = ne > 0
    o16 = offset[has].astype(np.int16).view(np.uint16).astype(np.int64)       # astype wraps like static_cast<int16_t>
    first = edges[start[:-1][has]]
    p = off[:-1][has]
    data[p + 1], data[p + 2] = o16 & 255, o16 >> 8
    for k in range(4):
        data[p + 3 + k] = (first >> (8 * k)) & 255
    # the steps: entry i of `edges` that is not a read's first
    read_of = np.repeat(np.arange(n), ne)
    is_step = np.ones(len(edges), bool)
    is_step[start[:-1][has]] = False
    i = np.nonzero(is_step)[0]
    found = g.v_left[edges[i]] == g.v_right[edges[i - 1]]
    cum = np.concatenate([[0], np.cumsum(found)])
    first_step = np.searchsorted(i, start[:-1])                              # per read: the place of its first step in i
    rank = cum[:-1] - cum[first_step[read_of[i]]]                            # found steps of the same read before this one
    at = off[read_of[i]] + 7 + rank // 4
    np.add.at(data, at[found], (g.from_pos[edges[i]][found] << (2 * (rank[found] % 4))).astype(np.uint8))
    stats = dict(n_empty=int((~has).sum()), n_steps_not_found=int((~found).sum()), n_offsets_wrapped=int((has & ((offset < -32768) | (offset > 32767))).sum()))
    return off[:-1][::SKIP].astype(np.int64), data, stats


def unzip_paths(index, data, n_reads, g: Graph, strict: bool = True):
    """-> (offset i32[n], n_edges u32[n], edges i32[]); the records are walked from the index, group by group, and must end at len(data).
    A branch id that addresses no out-edge is an error; strict=False: the rest of that path is -1 (a record whose steps the reference did
    not all encode decodes to something else than it was made from)."""
    offset, ne, edges = np.zeros(n_reads, np.int32), np.zeros(n_reads, np.uint32), []
    assert len(index) == (n_reads + SKIP - 1) // SKIP
    at = 0
    for r in range(n_reads):
        if r % SKIP == 0:
            assert at == index[r // SKIP]
        n = int(data[at])
        ne[r] = n
        if n:
            offset[r] = int(np.frombuffer(data[at + 1:at + 3].tobytes(), "<i2")[0])
            e = int(np.frombuffer(data[at + 3:at + 7].tobytes(), "<u4")[0])
            edges.append(e)
            for j in range(n - 1):
                bid = (int(data[at + 7 + j // 4]) >> (2 * (j % 4))) & 3
                w = g.v_right[e] if e >= 0 else 0
                if e < 0 or bid >= g.from_off[w + 1] - g.from_off[w]:
                    assert not strict, (r, j, bid)
                    e = -1
                else:
                    e = int(g.from_e[g.from_off[w] + bid])
                edges.append(e)
        at += int(rec_bytes(n))
    assert at == len(data)
    return offset, ne, np.asarray(edges, dtype=np.int32)


def wrap16(offset):
    return np.asarray(offset).astype(np.int16).astype(np.int32)


def all_steps_found(n_edges, edges, g: Graph) -> np.ndarray:
    """bool per read: every step of its path goes to an out-edge of the vertex it arrives at (unzip gives such a path back)."""
    ne = np.asarray(n_edges, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(ne)])
    is_step = np.ones(len(edges), bool)
    is_step[start[:-1][ne > 0]] = False
    i = np.nonzero(is_step)[0]
    bad = g.v_left[edges[i]] != g.v_right[edges[i - 1]]
    return np.bincount(np.repeat(np.arange(len(ne)), ne)[i][bad], minlength=len(ne)) == 0


def pathsx_bytes(index, data, n_reads: int) -> bytes:
    """a.pathsX: skip, start_rid, next_start_rid, index size, data size (int64 each), the index, the data."""
    return struct.pack("<5q", SKIP, 0, n_reads, len(index), len(data)) + np.asarray(index, "<i8").tobytes() + np.asarray(data, np.uint8).tobytes()


def parse_pathsx(b: bytes):
    skip, s0, n_reads, ni, nb = struct.unpack_from("<5q", b, 0)
    assert skip == SKIP and s0 == 0 and len(b) == 40 + 8 * ni + nb
    return np.frombuffer(b, "<i8", ni, 40), np.frombuffer(b, np.uint8, nb, 40 + 8 * ni), n_reads


# ---- the reads of the long_unitig case (made again wherever they are needed: they are too large for a fixture; the fixture holds their digest)

def long_unitig_reads():
    """Error-free pairs over one random 40 kb genome at about 30x: reads far down a 40 kb edge have offsets above 32767.
    -> (codes u8[n, L], quals u8[n, L], lens u16[n], bc i32[n])."""
    L, G = 150, 40000
    rng = np.random.default_rng(0xA48C0DE)
    g = rng.integers(0, 4, G, dtype=np.uint8)
    n_pairs = G * 30 // L // 2
    codes = np.zeros((2 * n_pairs, L), np.uint8)
    for q in range(n_pairs):
        F = int(rng.integers(2 * L, 4 * L))
        s = int(rng.integers(0, G - F + 1))
        frag = g[s:s + F]
        if rng.random() < 0.5:
            frag = (3 - frag[::-1]).astype(np.uint8)
        codes[2 * q] = frag[:L]
        codes[2 * q + 1] = (3 - frag[::-1])[:L]
    quals = np.full((2 * n_pairs, L), 30, np.uint8)
    lens = np.full(2 * n_pairs, L, np.uint16)
    bc = np.repeat(1 + np.arange(n_pairs, dtype=np.int32) % 8, 2).astype(np.int32)
    return codes, quals, lens, bc


def reads_digest(codes, quals, lens, bc) -> bytes:
    h = hashlib.sha256()
    for a in (codes, quals, lens, bc):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest().encode()
