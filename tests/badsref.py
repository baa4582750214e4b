"""A plain numpy restatement of the reference's MarkBads -- lib/assembly/src/10X/SecretOps.cc:70-107 (ReadPath: the path's int offset) and
:22-59 (ReadPathVecX: the path has been through zip / unzip, so the offset is static_cast<int16_t>(offset)) -- and the fixtures under
tests/golden/bads/ (flags the reference's own two overloads wrote, see tests/golden/make_bads_golden.py, which asserts that this
restatement reproduces them before it saves a case).

For a read with a path p:  m = hb.Cat(p) (paths/HyperBasevector.cc:631-635), a chain of TrimCat (feudal/BaseVec.h:550-558): what is there
loses its last K-1 bases and the next edge is appended whole, adjacent or not -- the later edge's bases stand in the K-1 bases two
edges would share;  badsum = the raw quality summed over the read positions l with 0 <= offset + l < |m| and read[l] != m[offset + l];
bad[id / 2] iff badsum > 150 for either mate.  m is made here literally, by concatenation.
"""
from __future__ import annotations

from pathlib import Path
from types import SimpleNamespace

import numpy as np

import a48xref

BADS = Path(__file__).resolve().parent / "golden" / "bads"
MAX_BAD_SUM = 150
COUNTERS = ("n_placed", "n_mismatch_reads", "n_bad_reads", "n_bad_pairs", "n_offsets_wrapped")


class Refused(ValueError):
    """X mode on paths a ReadPathVecX cannot hold ('unsupported': more than 255 edges) or would not give back ('arg': a step e -> e' with e'
    not in From(ToRight(e)))."""

    def __init__(self, code: str, msg: str):
        super().__init__(msg)
        self.code = code


def cat(eb, K, path) -> np.ndarray:
    """hb.Cat(path): TrimCat does not look at adjacency."""
    m = eb[int(path[0])]
    for e in path[1:]:
        m = np.concatenate([m[:len(m) - (K - 1)], eb[int(e)]])
    return m


def badsum(m: np.ndarray, read: np.ndarray, qual: np.ndarray, offset: int) -> tuple[int, int]:
    """-> (badsum, mismatches inside m)"""
    epos = offset + np.arange(len(read), dtype=np.int64)
    ok = (epos >= 0) & (epos < len(m))
    mis = read[ok] != m[epos[ok]]
    return int(qual[ok][mis].astype(np.int64).sum()), int(mis.sum())


def mark_bads(g: a48xref.Graph, eb, codes, lens, quals, offset, n_edges, edges, x: bool = False, per_read: list | None = None):
    """-> (bad u8[n / 2], {counter: value}).  codes / quals: one row per read, lens their lengths.  per_read receives every read's badsum
    (None: no path)."""
    ne = np.asarray(n_edges, dtype=np.int64)
    n = len(ne)
    assert n % 2 == 0 and len(codes) == n, "reads 2q and 2q + 1 are mates"
    edges = np.asarray(edges, dtype=np.int64)
    offset = np.asarray(offset, dtype=np.int64)
    if x:
        if ne.max(initial=0) > 255:
            raise Refused("unsupported", "a path of more than 255 edges")
        if g.from_pos.max(initial=0) > 3:
            raise Refused("unsupported", "a vertex with more than four out-edges")
        if not a48xref.all_steps_found(ne, edges, g).all():
            raise Refused("arg", "a step to an edge that does not leave the vertex its predecessor ends in")
    start = np.concatenate([[0], np.cumsum(ne)])
    off = a48xref.wrap16(offset).astype(np.int64) if x else offset
    bad = np.zeros(n // 2, np.uint8)
    cnt = dict.fromkeys(COUNTERS, 0)
    cats: dict = {}
    for r in range(n):
        if not ne[r]:
            if per_read is not None:
                per_read.append(None)
            continue
        p = edges[start[r]:start[r + 1]]
        key = p.tobytes()
        if key not in cats:
            cats[key] = cat(eb, g.K, p)
        L = int(lens[r])
        s, nm = badsum(cats[key], np.asarray(codes[r][:L], np.uint8), np.asarray(quals[r][:L], np.uint8), int(off[r]))
        cnt["n_placed"] += 1
        cnt["n_mismatch_reads"] += nm > 0
        cnt["n_offsets_wrapped"] += int(offset[r]) != int(a48xref.wrap16(offset[r]))
        if s > MAX_BAD_SUM:
            cnt["n_bad_reads"] += 1
            bad[r // 2] = 1
        if per_read is not None:
            per_read.append(s)
    cnt["n_bad_pairs"] = int(bad.sum())
    return bad, {k: int(v) for k, v in cnt.items()}


# ---- the fixtures

GOLDEN = ("synth_2k_err", "synth_6k_clean", "synth_20k_err", "adversarial", "synth_4k_dups")          # = goldens.CASES
FAR = "synth_20k_err_far"
HAND = {"hand_k48": 48, "hand_k60": 60}                   # tests/handbads.py: the pairs both modes take
HAND_PLAIN = {"handplain_k48": 48, "handplain_k60": 60}   # ... and the ones SNK_BADS_X refuses (bad_x is empty)
ALL = tuple(n + t for n in GOLDEN for t in ("", "_cut")) + (FAR,) + tuple(HAND) + tuple(HAND_PLAIN)
_cases: dict = {}


def far_input(paths, n_total: int):
    """synth_20k_err_far: the pairs of which a read's offset lies outside +-32767 (exactly the reads extref.golden_input takes out), mates
    and paths kept.  -> (read ids, (offset, n_edges, edges))"""
    offset, ne, edges = paths
    ne64 = np.asarray(ne, dtype=np.int64)
    far = (ne64 > 0) & ((offset < -32767) | (offset > 32767))
    pairs = np.unique(np.nonzero(far)[0] // 2)
    ids = np.stack([2 * pairs, 2 * pairs + 1], 1).reshape(-1)
    start = np.concatenate([[0], np.cumsum(ne64)])
    keep = np.concatenate([np.arange(start[r], start[r + 1]) for r in ids]) if len(ids) else np.zeros(0, np.int64)
    return ids, (np.asarray(offset)[ids].astype(np.int32), ne64[ids].astype(np.uint32), np.asarray(edges)[keep].astype(np.int32))


def cut_input(g, eb, offset, n_edges, edges):
    """`*_cut`: the first edge of every path of two or more edges dropped while the offset STAYS: the read is then compared
    Kmers(first edge) bases away from where it lies."""
    ne = np.asarray(n_edges, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(ne)])
    keep = np.ones(len(edges), bool)
    keep[start[:-1][ne >= 2]] = False
    return np.array(offset, dtype=np.int32), np.where(ne >= 2, ne - 1, ne).astype(np.uint32), np.asarray(edges)[keep].astype(np.int32)


def load(name: str):
    """-> namespace(name, K, g, eb, codes, quals, lens, unitigs (BVComp order), paths = (offset, n_edges, edges), bad_plain, bad_x (None
    for a plain-only case), ref_summary, expect (hand-made: per pair (plain, x))).  Loaded once per process and left unchanged."""
    if name in _cases:
        return _cases[name]
    import extref
    z = np.load(BADS / f"{name}.npz")
    c = SimpleNamespace(name=name, bad_plain=z["bad_plain"].copy(), bad_x=z["bad_x"].copy() if name not in HAND_PLAIN else None,
                        ref_summary=bytes(z["ref_summary"]).decode())
    if name in HAND or name in HAND_PLAIN:
        import handbads
        h = handbads.case({**HAND, **HAND_PLAIN}[name], plain_only=name in HAND_PLAIN)
        c.a_hbv = bytes(z["a_hbv"])
        c.g = a48xref.parse_hbv(c.a_hbv)
        c.eb = extref.edge_bases(c.g)
        c.codes, c.quals, c.lens, c.paths = handbads.arrays(h, handbads.edge_index(c.eb))
        c.unitigs, c.expect, c.pairs = h.unitigs, [(p.plain, p.x) for p in h.pairs], h.pairs
    else:
        import a48ref
        import goldens
        base = FAR[:-4] if name == FAR else name[:-4] if name.endswith("_cut") else name
        gc = goldens.load(base)
        c.g = a48xref.parse_hbv(gc.exp_ahbv)
        c.eb = extref.edge_bases(c.g)
        c.unitigs = gc.exp_unitigs
        raw = a48xref.parse_paths(a48ref.load(base)["tmp.paths"])
        if name == FAR:
            ids, c.paths = far_input(raw, len(raw[1]))
        else:
            c.paths = extref.golden_input(raw)
            ids = np.arange(len(c.paths[1]))
            if name.endswith("_cut"):
                c.paths = cut_input(c.g, c.eb, *c.paths)
        c.ids = ids
        c.codes, c.quals, c.lens = gc.codes[ids], gc.quals[ids], gc.lens[ids]
    c.K = c.g.K
    assert bytes(z["input_digest"]).decode() == digest(c), f"{name}: the fixture was made from another input"
    _cases[name] = c
    return c


def digest(c) -> str:
    """what identifies a fixture's input: reads, paths and graph"""
    import hashlib
    h = hashlib.sha256()
    for a, dt in ((c.codes, np.uint8), (c.quals, np.uint8), (c.lens, np.uint16), (c.paths[0], np.int32), (c.paths[1], np.uint32), (c.paths[2], np.int32)):
        h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
    h.update(c.g.edges_blob)
    return h.hexdigest()


_restated: dict = {}


def restated(name: str, x: bool):
    k = (name, bool(x))
    if k not in _restated:
        c = load(name)
        _restated[k] = mark_bads(c.g, c.eb, c.codes, c.lens, c.quals, *c.paths, bool(x))
    return _restated[k]
