"""A plain Python restatement of the reference's path extension -- ExtendPathsNew (10X/Extend.cc:14-177) with the HyperBasevectorX
overload of ExtendPath (paths/long/large/GapToyTools4.cc:477-555, min_gain 5, mode 1) -- and the fixtures under tests/golden/ext/
(bytes the reference's own function wrote, see tests/golden/make_ext_golden.py, which asserts that this restatement reproduces them
before it saves a case).  Three legs per read, each on the result of the one before:
  1 backward (only with back=True; :25-61)   while offset < 0 and To(ToLeft(p[0])) is not empty: the first in-edge, in To-list order,
      whose bases agree with the read wherever they overlap it goes in front; offset += Kmers(edge)
  2 quality-aware (:63-95)                   the path is cut to its first edge, then ExtendPath: breadth-first enumeration of the
      continuations in From-list order (entry 101 reached = too many), those that cover the read scored by the summed quality of
      their mismatches, the best taken iff it is alone or beats the runner-up by 5
  3 exact (:97-177)                          a path that matches the read to its last base and ends inside the read goes on base by
      base; at an edge's end EVERY out-edge whose base K-1 equals the read's base is pushed (the loop has no break) and the last
      one becomes current
Only the first edge of a path and its offset reach the result: leg 1 looks at nothing else, and leg 2 drops the rest.
"""
from __future__ import annotations

import struct
from pathlib import Path

import numpy as np

import a48xref

EXT = Path(__file__).resolve().parent / "golden" / "ext"
MIN_GAIN, MAX_EXTS = 5, 100
COUNTERS = ("n_back_extended", "n_cut_to_first", "n_quality_extended", "n_ambiguous", "n_too_many", "n_exact_extended")


class Refused(ValueError):
    """An input the reference would read outside a read or an edge with (`code` 'arg'), or whose result its record cannot hold
    ('unsupported')."""

    def __init__(self, code: str, msg: str):
        super().__init__(msg)
        self.code = code


def edge_bases(g: a48xref.Graph) -> list[np.ndarray]:
    """The edges_ section of a.hbv (u64 E, per edge u32 bases + 2-bit bytes, base j at bits 2 (j % 4) of byte j / 4) -> codes per edge."""
    b = g.edges_blob
    E = struct.unpack_from("<Q", b, 0)[0]
    at, out = 8, []
    for _ in range(E):
        nb = struct.unpack_from("<I", b, at)[0]
        at += 4
        raw = np.frombuffer(b, np.uint8, (nb + 3) // 4, at)
        at += (nb + 3) // 4
        out.append(((raw[:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[:nb].astype(np.uint8))
    return out


def _extend_path(g, eb, K, e0, start, read, qual):
    """ExtendPath on the one-edge path [e0] at offset start -> (edges appended, 'extended' | 'ambiguous' | 'too_many' | None)."""
    if start < 0:
        return [], None
    ext = len(read) - (len(eb[e0]) - start)
    if ext <= 0:
        return [], None
    v = int(g.v_right[e0])
    if g.from_off[v + 1] == g.from_off[v]:
        return [], None
    exts, exts_len = [[]], [0]
    j = 0
    while j < len(exts):
        if j > MAX_EXTS:
            return [], "too_many"
        if exts_len[j] < ext:
            y = int(g.v_right[exts[j][-1]]) if exts[j] else v
            for l in range(int(g.from_off[y]), int(g.from_off[y + 1])):
                n = int(g.from_e[l])
                exts.append(exts[j] + [n])
                exts_len.append(exts_len[j] + len(eb[n]) - (K - 1))
        j += 1
    keep = [x for x, ln in zip(exts, exts_len) if ln >= ext]
    if not keep:
        return [], None
    n = len(read)
    r = read[n - ext:]
    q = qual[n - ext:n].astype(np.int64)
    qsum = []
    for x in keep:
        b = np.concatenate([eb[e][K - 1:] for e in x])[:ext]
        qsum.append(int(q[r != b].sum()))
    order = sorted(range(len(keep)), key=lambda i: qsum[i])         # (ties never decide: a tie at the top is declined)
    if len(keep) >= 2 and qsum[order[1]] - qsum[order[0]] < MIN_GAIN:
        return [], "ambiguous"
    return list(keep[order[0]]), "extended"


def extend_read(g, eb, K, read, qual, offset, path, back):
    """One read: (offset, list of edges) -> (offset, list of edges, set of counter names)."""
    hit = set()
    if len(path) == 0:
        return 0, [], hit
    n = len(read)
    p = [int(path[0])]
    n_in = len(path)
    if n == 0:
        raise Refused("arg", "a path on a read of length 0")
    if offset < -32767 or offset > 32767:
        raise Refused("unsupported", "offset outside +-32767")
    if offset <= -n or offset >= len(eb[p[0]]):
        raise Refused("arg", "offset outside the read or the first edge")
    # ---- leg 1
    n_back = 0
    if back:
        v = int(g.v_left[p[0]])
        if offset < 0 and g.to_off[v + 1] > g.to_off[v] and n < -offset + K - 1:
            raise Refused("arg", "the read ends inside the overlap of the first edge with its in-edges")
        while offset < 0:
            v = int(g.v_left[p[0]])
            if g.to_off[v + 1] == g.to_off[v]:
                break
            extended = False
            for j in range(int(g.to_off[v]), int(g.to_off[v + 1])):
                e = int(g.to_e[j])
                o, km = eb[e], len(eb[e]) - (K - 1)
                l0 = max(0, offset + km)
                if np.array_equal(o[l0:], read[l0 - offset - km:len(o) - offset - km]):
                    extended = True
                    p.insert(0, e)
                    offset += km
                    n_back += 1
                    break
            if not extended:
                break
        if n_back:
            hit.add("n_back_extended")
        if n_in + n_back > 255:
            raise Refused("unsupported", "a path of more than 255 edges")
        if offset > 32767:
            raise Refused("unsupported", "the backward leg moves the offset beyond 32767 (the path is zipped between the legs)")
    # ---- leg 2
    more, what = _extend_path(g, eb, K, p[0], offset, read, qual)
    if n_in + n_back >= 2 and not more:
        hit.add("n_cut_to_first")
    if what:
        hit.add({"extended": "n_quality_extended", "ambiguous": "n_ambiguous", "too_many": "n_too_many"}[what])
    p = [p[0]] + more
    # ---- leg 3
    pp, e = 0, p[0]
    rpos, epos = (-offset, 0) if offset < 0 else (0, offset)
    mismatch = False
    while True:
        if read[rpos] != eb[e][epos]:
            mismatch = True
            break
        rpos += 1
        if rpos == n:
            break
        epos += 1
        if epos == len(eb[e]):
            pp += 1
            if pp == len(p):
                break
            e = p[pp]
            epos = K - 1
    if not mismatch and rpos != n:
        np0 = len(p)
        while True:
            if epos < len(eb[e]):
                if read[rpos] != eb[e][epos]:
                    break
            else:
                v = int(g.v_right[e])
                ext = False
                for j in range(int(g.from_off[v]), int(g.from_off[v + 1])):
                    f = int(g.from_e[j])
                    if read[rpos] == eb[f][K - 1]:
                        e, epos, ext = f, K - 1, True
                        p.append(f)
                if not ext:
                    break
            rpos += 1
            epos += 1
            if rpos == n:
                break
        if len(p) > np0:
            hit.add("n_exact_extended")
    if len(p) > 255:
        raise Refused("unsupported", "a path of more than 255 edges")
    return offset, p, hit


def extend(g: a48xref.Graph, codes, lens, quals, offset, n_edges, edges, back: bool, eb=None, per_read: list | None = None):
    """-> (offset i32[n], n_edges u32[n], edges i32[], {counter: reads}).  codes / quals: one row per read, lens their lengths.
    per_read: a list that receives every read's set of counters."""
    eb = edge_bases(g) if eb is None else eb
    ne = np.asarray(n_edges, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(ne)])
    o_out, n_out, e_out = np.zeros(len(ne), np.int32), np.zeros(len(ne), np.uint32), []
    counters = dict.fromkeys(COUNTERS, 0)
    for r in range(len(ne)):
        L = int(lens[r])
        o, p, hit = extend_read(g, eb, g.K, np.asarray(codes[r][:L], np.uint8), np.asarray(quals[r][:L], np.uint8), int(offset[r]),
                                edges[start[r]:start[r + 1]], back)
        o_out[r], n_out[r] = o, len(p)
        e_out.extend(p)
        for k in hit:
            counters[k] += 1
        if per_read is not None:
            per_read.append(frozenset(hit))
    return o_out, n_out, np.asarray(e_out, dtype=np.int32), counters


def refused_reads(g, codes, lens, quals, offset, n_edges, edges, eb=None) -> np.ndarray:
    """bool per read: extend_read refuses it, without or with the backward leg (the call refuses its whole input for one such read, so a
    sweep over arbitrary paths takes them out first -- by this, not by a copy of the rules)"""
    eb = edge_bases(g) if eb is None else eb
    ne = np.asarray(n_edges, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(ne)])
    out = np.zeros(len(ne), bool)
    for r in range(len(ne)):
        L = int(lens[r])
        for back in (False, True):
            try:
                extend_read(g, eb, g.K, np.asarray(codes[r][:L], np.uint8), np.asarray(quals[r][:L], np.uint8), int(offset[r]), edges[start[r]:start[r + 1]], back)
            except Refused:
                out[r] = True
                break
    return out


# ---- the derived inputs of the fixtures

def cut_first_edge(g, eb, offset, n_edges, edges):
    """`*_cut`: the first edge of every path of two or more edges dropped (offset -= its k-mers)."""
    ne = np.asarray(n_edges, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(ne)])
    off = np.array(offset, dtype=np.int32)
    keep = np.ones(len(edges), bool)
    for r in np.nonzero(ne >= 2)[0]:
        off[r] -= len(eb[int(edges[start[r]])]) - (g.K - 1)
        keep[start[r]] = False
    return off, np.where(ne >= 2, ne - 1, ne).astype(np.uint32), np.asarray(edges)[keep].astype(np.int32)


def first_edge_only(offset, n_edges, edges):
    """`*_first`: every path cut to its first edge."""
    ne = np.asarray(n_edges, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(ne)])[:-1]
    return np.array(offset, dtype=np.int32), (ne > 0).astype(np.uint32), np.asarray(edges)[start[ne > 0]].astype(np.int32)


MAX_READS = 10000


def golden_input(paths):
    """The reference's own paths of a golden case as the fixtures use them: the first MAX_READS reads (the size limit of a fixture), and no
    path for a read whose offset lies outside +-32767 (a ReadPathVecX cannot hold it: the reference would wrap it and read outside the read)."""
    offset, ne, edges = paths
    n = min(len(ne), MAX_READS)
    ne64 = np.asarray(ne[:n], dtype=np.int64)
    edges = np.asarray(edges)[:int(ne64.sum())]
    far = (ne64 > 0) & ((offset[:n] < -32767) | (offset[:n] > 32767))
    keep = ~np.repeat(far, ne64)
    return np.where(far, 0, offset[:n]).astype(np.int32), np.where(far, 0, ne64).astype(np.uint32), edges[keep].astype(np.int32)


def names() -> list[str]:
    return sorted(p.stem for p in EXT.glob("*.npz"))


# ---- the fixtures

HAND = {"hand_k48": 48, "hand_k60": 60}
GOLDEN = ("synth_2k_err", "synth_6k_clean", "synth_20k_err", "adversarial", "synth_4k_dups")          # = goldens.CASES
BRANCHED = ("synth_20k_err", "adversarial", "synth_4k_dups")          # the golden cases with a path of two or more edges: they have _cut and _first
ALL = tuple(n + t for n in GOLDEN for t in (("", "_cut", "_first") if n in BRANCHED else ("",))) + tuple(HAND)
_cases: dict = {}
_restated: dict = {}


def load(name: str):
    """-> namespace(name, K, g, eb, codes, quals, lens, unitigs (BVComp order), in_paths (bytes), paths = (offset, n_edges, edges),
    pathsx = {0: bytes, 1: bytes}, ref_summary).  Loaded once per process and left unchanged."""
    if name in _cases:
        return _cases[name]
    from types import SimpleNamespace
    z = np.load(EXT / f"{name}.npz")
    c = SimpleNamespace(name=name, in_paths=bytes(z["in_paths"]), pathsx={0: bytes(z["pathsx0"]), 1: bytes(z["pathsx1"])}, ref_summary=bytes(z["ref_summary"]).decode())
    if name in HAND:
        import handext
        h = handext.case(HAND[name])
        c.a_hbv = bytes(z["a_hbv"])
        c.g = a48xref.parse_hbv(c.a_hbv)
        c.eb = edge_bases(c.g)
        c.codes, c.quals, c.lens, _ = handext.arrays(h, handext.edge_index(c.eb))
        c.unitigs = h.unitigs
    else:
        import goldens
        base = name[:-4] if name.endswith("_cut") else name[:-6] if name.endswith("_first") else name
        gc = goldens.load(base)
        if base != name:
            b = load(base)
            c.g, c.eb = b.g, b.eb
        else:
            c.g = a48xref.parse_hbv(gc.exp_ahbv)
            c.eb = edge_bases(c.g)
        c.unitigs = gc.exp_unitigs
    c.K = c.g.K
    c.paths = a48xref.parse_paths(c.in_paths)
    if name not in HAND:
        n = len(c.paths[1])
        c.codes, c.quals, c.lens = gc.codes[:n], gc.quals[:n], gc.lens[:n]
    _cases[name] = c
    return c


def restated(name: str, back) -> tuple:
    """extend() over a fixture's input, computed once per process: (offset, n_edges, edges, counters)"""
    k = (name, bool(back))
    if k not in _restated:
        c = load(name)
        _restated[k] = extend(c.g, c.codes, c.lens, c.quals, *c.paths, bool(back), c.eb)
    return _restated[k]
