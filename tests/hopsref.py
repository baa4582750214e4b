"""A plain numpy / Python restatement of the reference's FindEdgePairs -- lib/assembly/src/10X/Closomatic.cc:17-354, the second step of
StageFindPatch, whose result DF keeps as a.hops -- and the fixtures under tests/golden/hops/ (pairs and file bytes the reference's own
function wrote, see tests/golden/make_hops_golden.py, which asserts that this restatement reproduces them before it saves a case).

Unlike the reference it also says which of the three parts gave a pair, and counts what the device code counts.  X and the sets of
sequences are made literally, as lists and sets of tuples; the closure keeps every sequence it has reached (the reference keeps one
round's: only whether 100 k-mers are reached matters, and the reachable set is the same).
"""
from __future__ import annotations

from pathlib import Path
from types import SimpleNamespace

import numpy as np

import a48xref

HOPS = Path(__file__).resolve().parent / "golden" / "hops"
MAX_DIST_TO_END, MIN_LANDING, GOOD_EXT, MIN_RIGHT = 120, 100, 100, 40
COUNTERS = ("n_part1", "n_part2", "n_part3", "n_sink_edges", "n_long_edges", "n_two_class", "n_ext_round0", "n_ext_closure", "n_not_extended")


def kmers_of(g: a48xref.Graph, eb) -> np.ndarray:
    return np.array([len(b) - g.K + 1 for b in eb], dtype=np.int64)


def involution(a_inv: bytes) -> np.ndarray:
    """a.inv = BinaryWriter::writeFile(vec<int>)"""
    assert a_inv[:8] == b"BINWRITE"
    n = int(np.frombuffer(a_inv, "<u8", 1, 8)[0])
    return np.frombuffer(a_inv, "<i4", n, 16).astype(np.int64)


def paths_index(n_edges, edges, E: int):
    """per edge the ascending ids of the reads whose path holds it, a read as often as it does (10X/PathsIndex.cc)"""
    ne = np.asarray(n_edges, dtype=np.int64)
    rid = np.repeat(np.arange(len(ne)), ne)
    order = np.argsort(np.asarray(edges, dtype=np.int64), kind="stable")
    srt = np.asarray(edges, dtype=np.int64)[order]
    off = np.searchsorted(srt, np.arange(E + 1))
    ids = rid[order]
    return [ids[off[e]:off[e + 1]] for e in range(E)]


def _sink(g, km, e) -> bool:                          # Closomatic.cc:43-53
    v = g.v_right[e]
    for l in range(g.from_off[v], g.from_off[v + 1]):
        w = g.from_v[l]
        if g.from_off[w + 1] - g.from_off[w] > 0 or g.to_off[w + 1] - g.to_off[w] > 1 or km[g.from_e[l]] > MAX_DIST_TO_END:
            return False
    return True


def _source(g, km, e) -> bool:                        # :84-94
    v = g.v_left[e]
    for l in range(g.to_off[v], g.to_off[v + 1]):
        w = g.to_v[l]
        if g.to_off[w + 1] - g.to_off[w] > 0 or g.from_off[w + 1] - g.from_off[w] > 1 or km[g.to_e[l]] > MAX_DIST_TO_END:
            return False
    return True


def _extends(x: tuple, y: tuple, l: int) -> bool:      # :269-276
    for m in range(len(y)):
        n = m + len(x) - 1 - l
        if 0 <= n < len(x) and x[n] != y[m]:
            return False
    return True


def find_edge_pairs(g: a48xref.Graph, km, inv, n_edges, edges, bc, bad, one_good: bool = False, per_edge: dict | None = None):
    """-> (pairs i32[n, 2] ascending, info).  info: the COUNTERS and 'parts' = (set, set, set) of the pairs each part gave.  per_edge receives
    for every edge part 3 looked at beyond the two-class test 'round0', 'closure' or 'not_extended'."""
    ne = np.asarray(n_edges, dtype=np.int64)
    n, E = len(ne), g.E
    assert n % 2 == 0
    start = np.concatenate([[0], np.cumsum(ne)])
    edges = np.asarray(edges, dtype=np.int64)
    P = [tuple(int(e) for e in edges[start[r]:start[r + 1]]) for r in range(n)]
    inv = [int(x) for x in inv]
    km = [int(x) for x in km]
    cls = [int(x) for x in bc]
    pidx = paths_index(ne, edges, E)
    sink = [_sink(g, km, e) for e in range(E)]
    cnt = dict.fromkeys(COUNTERS, 0)
    cnt["n_sink_edges"] = sum(sink)

    def e2s(e1):                                      # :57-74
        out = set()
        for r in pidx[e1]:
            p2 = P[r ^ 1]
            if e1 in P[r] and p2:
                e2 = inv[p2[-1]]
                if e2 != e1:
                    out.add((e2, cls[r]))
        return out

    def two_class(pairs):
        by = {}
        for f, b in pairs:
            by.setdefault(f, set()).add(b)
        return sorted(f for f, bs in by.items() if len(bs) >= 2)

    part1, part2, part3 = set(), set(), set()
    for e1 in range(E):
        if sink[e1]:
            for e2 in two_class(e2s(e1)):
                if one_good or _source(g, km, e2):
                    part1.add((e1, e2))
    seen = {a for a, _ in part1}
    for e1 in range(E):                               # :109-165
        if sink[e1] and e1 not in seen:
            for e2 in two_class(e2s(e1)):
                if km[e2] >= MIN_LANDING and e2 != e1 and g.v_right[e1] != g.v_left[e2]:
                    part2.add((e1, e2))
    for e in range(E):                                # :177-337
        if km[e] < g.K + 1:
            continue
        cnt["n_long_edges"] += 1
        re = inv[e]
        X, bs = set(), set()
        for r in pidx[e]:
            bs.add(cls[r])
            p1, p2 = P[r], P[r ^ 1]
            for j in range(len(p1)):
                if p1[j] == e:
                    X.add(p1[j:])
            if p2:
                X.add(tuple(inv[f] for f in reversed(p2)))
        for r in pidx[re]:
            bs.add(cls[r])
            p = P[r]
            for j in range(len(p)):
                if p[j] == re:
                    X.add(tuple(inv[f] for f in reversed(p[:j + 1])))
        if len(bs) < 2:
            continue
        cnt["n_two_class"] += 1
        tail = lambda x: sum(km[f] for f in x[1:])
        exts = {x for x in X if x[0] == e}
        if any(tail(x) >= GOOD_EXT for x in exts):
            cnt["n_ext_round0"] += 1
            if per_edge is not None:
                per_edge[e] = "round0"
            continue
        reached, work, extended = set(exts), list(exts), False
        while work and not extended:
            x = work.pop()
            for y in X:
                for l in range(len(y) - 1):
                    if y[l] == x[-1] and _extends(x, y, l):
                        x2 = x + y[l + 1:]
                        if tail(x2) >= GOOD_EXT:
                            extended = True
                        elif x2 not in reached:
                            reached.add(x2)
                            work.append(x2)
        if per_edge is not None:
            per_edge[e] = "closure" if extended else "not_extended"
        if extended:
            cnt["n_ext_closure"] += 1
            continue
        cnt["n_not_extended"] += 1
        right = lambda f: km[f] >= MIN_RIGHT and f != e and f != re
        too_easy, can = set(), set()
        for r in pidx[e]:                             # :290-312
            if bad[r // 2]:
                continue
            p1, p2 = P[r], P[r ^ 1]
            for j in range(len(p1)):
                if p1[j] == e:
                    too_easy.update(f for f in p1[j + 1:] if right(f))
            can.update((inv[f], cls[r]) for f in p2 if right(inv[f]))
        for r in pidx[re]:                            # :313-326
            if bad[r // 2]:
                continue
            p = P[r]
            for j in range(len(p)):
                if p[j] == re:
                    can.update((inv[f], cls[r]) for f in p[:j + 1] if right(inv[f]))
        for f in two_class(can):
            if f not in too_easy:
                part3.add((e, f))
    cnt["n_part1"], cnt["n_part2"], cnt["n_part3"] = len(part1), len(part2), len(part3)
    allp = sorted(part1 | part2 | part3)
    pairs = np.array(allp, dtype=np.int32).reshape(-1, 2)
    return pairs, dict(cnt, parts=(part1, part2, part3))


def hops_bytes(pairs) -> bytes:
    """a.hops = BinaryWriter::writeFile(vec<pair<int,int>>): "BINWRITE", u64 count, two i32 per pair"""
    pairs = np.ascontiguousarray(pairs, dtype="<i4").reshape(-1, 2)
    return b"BINWRITE" + np.uint64(len(pairs)).tobytes() + pairs.tobytes()


def only_part(info, k: int) -> set:
    """the pairs that part k (0, 1, 2) gave and no other part did"""
    others = set().union(*(p for i, p in enumerate(info["parts"]) if i != k))
    return info["parts"][k] - others


# ---- the fixtures

GOLDEN = ("synth_2k_err", "synth_6k_clean", "synth_20k_err", "adversarial", "synth_4k_dups")          # = goldens.CASES
GENERATED = ("gapped",)
HAND = {"hand_k48": 48, "hand_k60": 60}                   # tests/handhops.py
ALL = GOLDEN + GENERATED + tuple(HAND)
_cases: dict = {}


def digest(c) -> str:
    """what identifies a fixture's input: graph, involution, paths, barcodes and flags"""
    import hashlib
    h = hashlib.sha256()
    for a, dt in ((c.paths[0], np.int32), (c.paths[1], np.uint32), (c.paths[2], np.int32), (c.bc, np.int32), (c.bad, np.uint8), (c.inv, np.int32)):
        h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
    h.update(c.g.edges_blob)
    return h.hexdigest()


def golden_input(name: str):
    """A golden K=48 case on the reference's own paths, cut to extref.golden_input, bad = the bad_x of tests/golden/bads/.
    -> namespace(g, eb, km, inv, unitigs, paths, bc, bad)"""
    import a48ref
    import badsref
    import extref
    import goldens
    gc = goldens.load(name)
    c = SimpleNamespace(name=name, g=a48xref.parse_hbv(gc.exp_ahbv), a_hbv=gc.exp_ahbv, a_inv=gc.exp_ainv, unitigs=gc.exp_unitigs)
    c.eb = extref.edge_bases(c.g)
    c.paths = extref.golden_input(a48xref.parse_paths(a48ref.load(name)["tmp.paths"]))
    n = len(c.paths[1])
    c.bc = np.asarray(gc.bc[:n], dtype=np.int32)
    c.bad = badsref.load(name).bad_x.copy()
    assert len(c.bad) == n // 2
    return _finish(c)


def _finish(c):
    c.K = c.g.K
    c.km = kmers_of(c.g, c.eb)
    c.inv = involution(c.a_inv)
    return c


def load(name: str):
    """-> namespace(name, K, g, eb, km, inv, unitigs (BVComp order), paths = (offset, n_edges, edges), bc, bad, pairs (the reference's),
    hops (the file's bytes), pairs_one_good, hops_one_good, counts / counts_one_good (dict of COUNTERS), ref_summary; hand-made: items).
    Loaded once per process and left unchanged."""
    if name in _cases:
        return _cases[name]
    z = np.load(HOPS / f"{name}.npz")
    if name in GOLDEN:
        c = golden_input(name)
    else:
        import extref
        if name in HAND:
            import handhops
            h = handhops.case(HAND[name])
            c = SimpleNamespace(name=name, a_hbv=bytes(z["a_hbv"]), a_inv=bytes(z["a_inv"]), unitigs=h.unitigs, items=h.items)
            c.g = a48xref.parse_hbv(c.a_hbv)
            c.eb = extref.edge_bases(c.g)
            c.paths, c.bc, c.bad = handhops.arrays(h, handhops.edge_index(c.eb))
        else:
            c = SimpleNamespace(name=name, a_hbv=bytes(z["a_hbv"]), a_inv=bytes(z["a_inv"]), unitigs=bytes(z["unitigs"]).decode().split("\n"))
            c.g = a48xref.parse_hbv(c.a_hbv)
            c.eb = extref.edge_bases(c.g)
            c.paths = (z["path_offset"].copy(), z["path_n_edges"].copy(), z["path_edges"].copy())
            c.bc, c.bad = z["bc"].copy(), z["bad"].copy()
        _finish(c)
    c.pairs, c.pairs_one_good = z["pairs"].copy().reshape(-1, 2), z["pairs_one_good"].copy().reshape(-1, 2)
    c.hops, c.hops_one_good = bytes(z["hops"]), bytes(z["hops_one_good"])
    c.counts = dict(zip(COUNTERS, (int(v) for v in z["counts"])))
    c.counts_one_good = dict(zip(COUNTERS, (int(v) for v in z["counts_one_good"])))
    c.only = tuple(int(v) for v in z["only"])            # pairs that part 1 / 2 / 3 alone gave (flags 0)
    c.ref_summary = bytes(z["ref_summary"]).decode()
    assert bytes(z["input_digest"]).decode() == digest(c), f"{name}: the fixture was made from another input"
    _cases[name] = c
    return c


_restated: dict = {}


def restated(name: str, one_good: bool):
    k = (name, bool(one_good))
    if k not in _restated:
        c = load(name)
        _restated[k] = find_edge_pairs(c.g, c.km, c.inv, c.paths[1], c.paths[2], c.bc, c.bad, bool(one_good))
    return _restated[k]
