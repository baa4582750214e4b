"""A plain Python restatement of the reference's graph edit -- hbv.DeleteEdgesParallel(dels) followed by Cleanup
(paths/long/large/GapToyTools.cc:1287-1302: the path truncation, RemoveUnneededVertices2 of GapToyTools3.cc:487-667, CleanupCore of
GapToyTools.cc:1253-1285) -- and of the hanging-end selection of StageTrim (10X/runstages/RunStages.cc:91-146), their hand-made cases, and
the fixtures under tests/golden/edit/ (what the reference's own functions made of the cases: tests/golden/edit_driver.cc and
make_edit_golden.py).

The restatement keeps the From / To lists the way the reference does -- AddEdge inserts by upper_bound (graph/DigraphTemplate.h:2572-2582),
deletions erase in place, RemoveDeadEdgeObjects and RemoveEdgelessVertices renumber -- and writes a.hbv from those lists, so it does not
lean on the library's derivation of the list order.  The hanging-end rule is inline in StageTrim and cannot be called alone: it is pinned
by this restatement and by the edges each case names by hand (Case.hang_want).  The fuzz_<seed> fixtures (the edit step of the seeds of
tests/patchgen.py) add reference-made evidence for the edit on irregular graphs, none for that rule: their support and selection are
this restatement's too.
"""
from __future__ import annotations

import struct
import zlib
from bisect import bisect_right
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import a48xref
import handunitigs as hu
import patchref

EDIT = Path(__file__).resolve().parent / "golden" / "edit"
COUNTERS = ("n_deleted", "n_runs", "n_absorbed", "max_run", "n_truncated", "n_emptied", "n_collapsed")
MAX_PATHS = 5000


# ---- the graph as the reference holds it

class HB:
    """HyperBasevector: per vertex from_ / from_edge_obj_ / to_ / to_edge_obj_, and the edge objects (strings)"""

    def __init__(self, K, N, v_left, v_right, seqs, lists=None):
        self.K, self.edges = K, list(seqs)
        if lists is not None:
            self.frm, self.frm_e, self.to, self.to_e = lists
            return
        self.frm, self.frm_e, self.to, self.to_e = ([[] for _ in range(N)] for _ in range(4))
        for e, (v, w) in enumerate(zip(v_left, v_right)):
            self._insert(int(v), int(w), e)

    @classmethod
    def from_file(cls, a_hbv: bytes):
        g = a48xref.parse_hbv(a_hbv)
        cut = lambda off, vals: [[int(x) for x in vals[off[v]:off[v + 1]]] for v in range(g.N)]
        return cls(g.K, g.N, None, None, patchref.edge_strings(g), lists=(cut(g.from_off, g.from_v), cut(g.from_off, g.from_e), cut(g.to_off, g.to_v), cut(g.to_off, g.to_e)))

    @property
    def N(self):
        return len(self.frm)

    def _insert(self, v, w, e):
        i = bisect_right(self.frm[v], w)
        self.frm[v].insert(i, w)
        self.frm_e[v].insert(i, e)
        j = bisect_right(self.to[w], v)
        self.to[w].insert(j, v)
        self.to_e[w].insert(j, e)

    def add_edge(self, v, w, s):
        self.edges.append(s)
        self._insert(v, w, len(self.edges) - 1)
        return len(self.edges) - 1

    def delete_edges(self, dead):
        for v in range(self.N):
            for vs, es in ((self.frm[v], self.frm_e[v]), (self.to[v], self.to_e[v])):
                for j in range(len(es) - 1, -1, -1):
                    if dead[es[j]]:
                        del vs[j], es[j]

    def used(self):
        u = [False] * len(self.edges)
        for es in self.frm_e:
            for e in es:
                u[e] = True
        return u

    def to_left_right(self):
        l, r = [-1] * len(self.edges), [-1] * len(self.edges)
        for v in range(self.N):
            for e in self.frm_e[v]:
                l[e] = v
            for e in self.to_e[v]:
                r[e] = v
        return l, r

    def kmers(self, e):
        return len(self.edges[e]) - self.K + 1

    def remove_dead_edge_objects(self):
        used = self.used()
        to_new, count = [-1] * len(self.edges), 0
        for i, u in enumerate(used):
            if u:
                to_new[i] = count
                count += 1
        self.edges = [s for s, u in zip(self.edges, used) if u]
        self.frm_e = [[to_new[e] for e in es] for es in self.frm_e]
        self.to_e = [[to_new[e] for e in es] for es in self.to_e]
        return to_new

    def remove_edgeless_vertices(self):
        keep = [bool(self.frm[v] or self.to[v]) for v in range(self.N)]
        new_id, n = [-1] * self.N, 0
        for v, k in enumerate(keep):
            if k:
                new_id[v] = n
                n += 1
        pick = lambda ls: [l for l, k in zip(ls, keep) if k]
        self.frm, self.frm_e, self.to, self.to_e = pick(self.frm), pick(self.frm_e), pick(self.to), pick(self.to_e)
        self.frm = [[new_id[w] for w in ws] for ws in self.frm]
        self.to = [[new_id[w] for w in ws] for ws in self.to]

    def hbv_bytes(self) -> bytes:
        """BinaryWriter::writeFile(HyperBasevector): from_, from_edge_obj_, to_edge_obj_, edges_"""
        def lists(ls):
            out = [struct.pack("<Q", len(ls))]
            for l in ls:
                out.append(struct.pack("<Q", len(l)) + np.asarray(l, "<i4").tobytes())
            return b"".join(out)
        out = [b"BINWRITE", struct.pack("<i", self.K), lists(self.frm), lists(self.frm_e), lists(self.to_e), struct.pack("<Q", len(self.edges))]
        for s in self.edges:
            c = patchref.codes(s).astype(np.uint8)
            pad = np.zeros((len(c) + 3) // 4 * 4, np.uint8)
            pad[:len(c)] = c
            q = pad.reshape(-1, 4)
            out.append(struct.pack("<I", len(c)) + (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8).tobytes())
        return b"".join(out)


def inv_bytes(inv) -> bytes:
    return b"BINWRITE" + struct.pack("<Q", len(inv)) + np.asarray(inv, "<i4").tobytes()


def split_paths(offset, n_edges, edges):
    at = np.concatenate([[0], np.cumsum(np.asarray(n_edges, np.int64))])
    return [(int(offset[r]), [int(x) for x in edges[at[r]:at[r + 1]]]) for r in range(len(n_edges))]


def join_paths(paths):
    return (np.asarray([o for o, _ in paths], np.int32), np.asarray([len(p) for _, p in paths], np.uint32),
            np.asarray([x for _, p in paths for x in p], np.int32))


# ---- DeleteEdgesParallel + Cleanup

def delete_edges(a_hbv: bytes, inv, offset, n_edges, edges, dels):
    """-> namespace(a_hbv, a_inv, inv, offset, n_edges, edges, edge_map, edge_koff, counters, new_order: (highest-vertex order != eleft
    order), hb)"""
    hb = HB.from_file(a_hbv)
    inv = [int(x) for x in inv]
    E_old = len(hb.edges)
    paths = split_paths(offset, n_edges, edges)
    cnt = dict.fromkeys(COUNTERS, 0)
    dead = [False] * E_old
    for e in dels:
        dead[int(e)] = True
    cnt["n_deleted"] = sum(dead)
    hb.delete_edges(dead)
    # Cleanup: the truncation (GapToyTools.cc:1290-1297)
    used = hb.used()
    for i, (o, p) in enumerate(paths):
        for j, e in enumerate(p):
            if e < 0 or e >= E_old or not used[e]:
                paths[i] = (o, p[:j])
                cnt["n_truncated"] += 1
                cnt["n_emptied"] += j == 0
                break
    # RemoveUnneededVertices2
    K = hb.K
    kill = [False] * hb.N
    queue = []
    to_left, to_right = hb.to_left_right()
    for v in range(hb.N):
        if len(hb.frm[v]) == 1 and len(hb.to[v]) == 1 and hb.frm[v][0] != hb.to[v][0] and len(hb.edges[hb.frm_e[v][0]]) > 0 and len(hb.edges[hb.to_e[v][0]]) > 0:
            kill[v] = True
            queue.append(v)
    bound = []
    while queue:
        v = queue.pop()
        if not kill[v]:
            continue
        vleft = v
        while True:
            kill[vleft] = False
            eleft = hb.to_e[vleft][0]
            vleft = hb.to[vleft][0]
            if not kill[vleft]:
                break
        vright = v
        while True:
            kill[vright] = False
            eright = hb.frm_e[vright][0]
            vright = hb.frm[vright][0]
            if not kill[vright]:
                break
        if eleft < inv[eright]:
            bound.append((eleft, eright))
            bound.append((inv[eright], inv[eleft]))
    lefts = [b[0] for b in bound[0::2]]
    renum = list(range(E_old))
    offsets = [0] * E_old
    new_nos, to_delete = [], []
    while bound:
        first, second = bound.pop()
        no = len(hb.edges)
        new_edge = hb.edges[first]
        off = hb.kmers(first)
        renum[first] = no
        to_delete.append(first)
        v, run = to_right[first], 1
        while v != to_right[second]:
            e = hb.frm_e[v][0]
            to_delete.append(e)
            new_edge = new_edge + hb.edges[e][K - 1:]            # TrimCat
            offsets[e] = off
            renum[e] = no
            off += hb.kmers(e)
            v = hb.frm[v][0]
            run += 1
        hb.add_edge(to_left[first], to_right[second], new_edge)
        new_nos.append(no)
        cnt["n_runs"] += 1
        cnt["n_absorbed"] += run
        cnt["max_run"] = max(cnt["max_run"], run)
    dead2 = [False] * len(hb.edges)
    for e in to_delete:
        dead2[e] = True
    hb.delete_edges(dead2)
    inv = inv + [-1] * (len(hb.edges) - E_old)
    for i in range(0, len(new_nos), 2):
        inv[new_nos[i]], inv[new_nos[i + 1]] = new_nos[i + 1], new_nos[i]
    for i, (o, p) in enumerate(paths):
        if p:
            q = [renum[p[0]]]
            for e in p[1:]:
                if renum[e] != q[-1]:
                    q.append(renum[e])
                else:
                    cnt["n_collapsed"] += 1
            paths[i] = (o + offsets[p[0]], q)
    # CleanupCore
    used = hb.used()
    to_new, count = [-1] * len(used), 0
    for i, u in enumerate(used):
        if u:
            to_new[i] = count
            count += 1
    inv2 = [(-1 if inv[i] < 0 else to_new[inv[i]]) for i in range(len(used)) if used[i]]
    paths = [(o, [to_new[e] for e in p]) for o, p in paths]
    assert all(e >= 0 for _, p in paths for e in p)
    hb.remove_dead_edge_objects()
    hb.remove_edgeless_vertices()
    off2, ne2, ed2 = join_paths(paths)
    edge_map = np.asarray([(-1 if dead[e] else to_new[renum[e]]) for e in range(E_old)], np.int32)
    return SimpleNamespace(a_hbv=hb.hbv_bytes(), a_inv=inv_bytes(inv2), inv=np.asarray(inv2, np.int32), offset=off2, n_edges=ne2, edges=ed2, edge_map=edge_map,
                           edge_koff=np.asarray(offsets, np.int32), counters=cnt, lefts=lefts, hb=hb)


# ---- the hanging-end selection (RunStages.cc:91-146)

def hanging_ends(a_hbv: bytes, inv, n_edges, edges, max_kmers=200):
    """-> (support i32[E], dels ascending distinct)"""
    g = a48xref.parse_hbv(a_hbv)
    inv = np.asarray(inv, np.int64)
    lens = np.asarray([len(s) for s in patchref.edge_strings(g)], np.int64)
    rs = np.zeros(g.E, np.int64)
    ed = np.asarray(edges, np.int64)
    np.add.at(rs, ed, 1)
    np.add.at(rs, inv[ed], 1)
    n_from, n_to = np.diff(g.from_off), np.diff(g.to_off)
    dels = set()
    for e in range(g.E):
        if rs[e] > 0 or lens[e] - g.K + 1 > max_kmers:
            continue
        v, w = g.v_left[e], g.v_right[e]
        if (n_to[v] == 0 and n_from[v] == 1) or (n_from[w] == 0 and n_to[w] == 1):
            dels.update((e, int(inv[e])))
    return rs.astype(np.int32), np.asarray(sorted(dels), np.int32)


# ---- the cases.  A maker builds unitigs with a tests/handunitigs.py generator and returns what the case does with them:
# dict(dels=[unitig strings whose two edges go], second=[...] (a second edit), bare=[strings whose edges and inverses carry no path],
# bare_fw=[strings whose OWN edge carries no path while its inverse does], hang=[strings the hanging-end rule must pick, hand-stated])

def _comb(g, n, tips_out=True):
    """a spine of n edges with a side branch at each of its n - 1 inner junctions -> (spine, tips)"""
    js = [g.junction() for _ in range(n + 1)]
    spine = [g.edge(js[i], 0, js[i + 1], 0) for i in range(n)]
    tips = [(g.edge(js[i], 0, g.junction(), 0) if tips_out or i % 2 else g.edge(g.junction(), 0, js[i], 0)) for i in range(1, n)]
    return spine, tips


def _run(n):
    def make(g):
        _, tips = _comb(g, n, tips_out=False)
        return dict(dels=tips)
    return make


def _c_fork(g):
    _, tips = _comb(g, 2)
    return dict(dels=tips)


def _c_hairpin(g):
    # x1 -> x2 -> J, the hairpin J -> rc(J) and its other strand, then rc(x2) -> rc(x1): a run next to its own reverse complement
    a, m, j = g.junction(), g.junction(), g.junction()
    g.edge(a, 0, m, 0)
    g.edge(m, 0, j, 0)
    tip = g.edge(m, 0, g.junction(), 0)
    g.edge(j, 0, j, 1, 9)
    return dict(dels=[tip])


def _c_selfinv(g):
    # a -> p -> rc(a) with p palindromic: eleft == inv[eright], never merged
    pal = g.pal(g.K)                             # (with K even only a single k-mer is a palindromic unitig)
    a, j = g.junction(), g.junction(pal[:g.K - 1])
    j.take(j.slot(0, 0, pal[g.K - 1]))
    g.add(pal)
    g.edge(a, 0, j, 0)
    tip = g.edge(j, 0, g.junction(), 0)
    return dict(dels=[tip])


def _circle(n):
    def make(g):
        js = [g.junction() for _ in range(n)]
        for i in range(n):
            g.edge(js[i], 0, js[(i + 1) % n], 0)
        return dict(dels=[g.edge(js[i], 0, g.junction(), 0) for i in range(n)])
    return make


def _c_two_cycle(g):
    a, b, c = g.junction(), g.junction(), g.junction()
    g.edge(a, 0, b, 0)
    g.edge(b, 0, a, 0)
    g.edge(c, 0, c, 0, 5)                        # a self-loop
    return dict(dels=[g.edge(a, 0, g.junction(), 0), g.edge(b, 0, g.junction(), 0), g.edge(c, 0, g.junction(), 0)])


def _c_parallel(g):
    a, b = g.junction(), g.junction()
    g.edge(a, 0, b, 0, 7)
    x = g.edge(a, 0, b, 0, 7)
    g.edge(g.junction(), 0, a, 0, 11)
    g.edge(b, 0, g.junction(), 0, 3)
    return dict(dels=[x])


def _c_loop(g):
    # two loops at b, one of them with a side branch inside: the merged loop is left and entered again through the other one
    b, m1, m2 = g.junction(), g.junction(), g.junction()
    g.edge(b, 0, m1, 0)
    g.edge(m1, 0, m2, 0)
    g.edge(m2, 0, b, 0)
    g.edge(b, 0, b, 0, 6)
    return dict(dels=[g.edge(m1, 0, g.junction(), 0), g.edge(g.junction(), 0, m2, 0)])


def _c_multi(g):
    dels = []
    for n in (3, 2, 5, 2, 4, 3, 2, 6):
        dels += _comb(g, n, tips_out=n % 2 == 0)[1]
    return dict(dels=dels)


def _c_none(g):
    _comb(g, 4)
    hu._bubble(g)
    return dict(dels=[])


def _c_all(g):
    _comb(g, 3)
    hu._bubble(g)
    return dict(dels="all")


def _c_chain(g):
    _, tips = _comb(g, 9)
    return dict(dels=tips[0::2], second=tips[1::2])


def _c_hang(g):
    K = g.K
    j, a = g.junction(), g.junction()
    g.edge(a, 0, j, 0, 30)
    g.edge(g.junction(), 0, a, 0, 25)
    g.edge(j, 0, g.junction(), 0, 40)
    t200 = g.edge(j, 0, g.junction(), 0, 200 + 1 - K)          # K - 1 + n + K - 1 bases: 200 k-mers
    t201 = g.edge(j, 0, g.junction(), 0, 201 + 1 - K)
    tinv = g.edge(g.junction(), 0, a, 0, 20)                     # no path on it, paths on its inverse
    lone = g.add(g.rand(K + 12))                                 # an isolated edge: both ends qualify
    pal = g.add(g.pal(K))                                        # self-inverse and isolated (one palindromic k-mer)
    return dict(dels="hang", bare=[t200, t201, lone, pal], bare_fw=[tinv], hang=[t200, lone, pal])


_MAKERS = {"fork": _c_fork, "run3": _run(3), "run65": _run(65), "run1025": _run(1025), "run5000": _run(5000), "hairpin": _c_hairpin, "selfinv": _c_selfinv,
           "circle3": _circle(3), "circle100": _circle(100), "two_cycle": _c_two_cycle, "parallel": _c_parallel, "loop": _c_loop, "multi": _c_multi, "none": _c_none,
           "all": _c_all, "chain": _c_chain, "hang": _c_hang}
BIG = ("run1025", "run5000")                     # one K each: the graphs with thousands of edges
HAND = tuple(_MAKERS)
GOLDEN = ("synth_2k_err", "synth_6k_clean", "synth_20k_err", "adversarial", "synth_4k_dups")      # the K = 48 golden cases: their a.hbv, their paths
G_SEQ = tuple(f"g_{n}_seq" for n in GOLDEN)      # the hanging-end selection, then a seeded tenth of what is left
G_TENTH = tuple(f"g_{n}_tenth" for n in GOLDEN)  # a seeded tenth of the edges
ALL = tuple(f"{n}_k{K}" for n in HAND for K in (48, 60) if n not in BIG or K == (48 if n == "run1025" else 60)) + G_SEQ + G_TENTH


def tenth(inv, seed: str):
    """a seeded, inv-closed tenth of the edges, ascending"""
    inv = np.asarray(inv, np.int64)
    low = np.flatnonzero(np.arange(len(inv)) <= inv)
    if not len(low):
        return np.zeros(0, np.int32)
    pick = np.random.default_rng(zlib.crc32(seed.encode())).choice(low, max(1, len(low) // 10), replace=False)
    return np.unique(np.concatenate([pick, inv[pick]])).astype(np.int32)


def _golden_case(key: str):
    import a48ref
    import goldens
    name, kind = key[2:].rsplit("_", 1)
    gc = goldens.load(name)
    g = a48xref.parse_hbv(gc.exp_ahbv)
    es = patchref.edge_strings(g)
    inv = np.frombuffer(gc.exp_ainv, "<i4", offset=16).astype(np.int32)
    offset, n_edges, edges = a48xref.parse_paths(a48ref.load(name)["tmp.paths"])
    us = hu.bvcomp_sorted(gc.exp_unitigs)        # (as the reference orients them: the graph's numbering follows from it)
    if kind == "seq":
        dels, second = hanging_ends(gc.exp_ahbv, inv, n_edges, edges)[1], (lambda first: tenth(first.inv, f"second/{key}"))
    else:
        dels, second = tenth(inv, f"dels/{key}"), None
    return SimpleNamespace(key=key, K=48, a_hbv=gc.exp_ahbv, a_inv=gc.exp_ainv, inv=inv, unitigs=us, offset=offset, n_edges=n_edges, edges=edges, dels=dels, second=second,
                           hang_want=None)

_made: dict = {}


def _ids(es_index, strings):
    out = set()
    for s in strings:
        out.update((es_index[s], es_index[hu.rc(s)]))
    return out


def case(key: str):
    """-> namespace(key, K, a_hbv, a_inv, inv, unitigs (BVComp order), offset, n_edges, edges, dels (i32, shuffled, with duplicates), second
    (strings or None), hang_want (ascending ids, or None where the case states none))"""
    if key in _made:
        return _made[key]
    if key.startswith("g_"):
        _made[key] = _golden_case(key)
        return _made[key]
    if key.startswith("fuzz_"):                  # a seed of tests/patchgen.py: the edit step on its patched graph
        import patchgen
        c = patchgen.make_case(int(key[5:]))
        assert c is not None, f"{key}: the seed is skipped"
        return patchgen.edit_input(c)
    name, K = key.rsplit("_k", 1)
    K = int(K)
    gen = hu._Gen(f"edit/{name}", K)
    spec = _MAKERS[name](gen)
    us = patchref.new_unitigs(gen.unitigs, K)
    assert sorted(len(s) for s in us) == sorted(len(s) for s in gen.unitigs), "the generator's strings are not the graph's unitigs"
    a_hbv, a_inv = patchref.graph_files(us, K)
    g = a48xref.parse_hbv(a_hbv)
    es = patchref.edge_strings(g)
    index = {s: e for e, s in enumerate(es)}
    inv = np.frombuffer(a_inv, "<i4", offset=16).astype(np.int32)
    view = g if name not in BIG else SimpleNamespace(K=K, E=700, v_right=g.v_right, from_e=g.from_e, from_off=g.from_off)      # (walks from the first 700 edges)
    offset, n_edges, edges = patchref.place_paths(f"edit/{name}", view, [len(s) for s in es])
    paths = split_paths(offset, n_edges, edges)
    bare = _ids(index, spec.get("bare", ())) | {index[s] for s in spec.get("bare_fw", ())}
    meets = lambda p: all(g.v_right[a] == g.v_left[b] for a, b in zip(p, p[1:]))     # ([e, e] of place_paths is a path on a loop only)
    paths = [(o, p) for o, p in paths if not bare & set(p) and meets(p)]
    if len(paths) > MAX_PATHS:
        paths = paths[::len(paths) // MAX_PATHS + 1]
    offset, n_edges, edges = join_paths(paths)
    hang_want = np.asarray(sorted(_ids(index, spec["hang"])), np.int32) if "hang" in spec else None
    if spec["dels"] == "all":
        dels = np.arange(g.E, dtype=np.int32)
    elif spec["dels"] == "hang":
        dels = hang_want
    else:
        dels = np.asarray(sorted(_ids(index, spec["dels"])), np.int32)
    rng = np.random.default_rng(zlib.crc32(f"dels/{key}".encode()))
    dels = rng.permutation(np.concatenate([dels, dels[:len(dels) // 3]])).astype(np.int32)
    _made[key] = SimpleNamespace(key=key, K=K, a_hbv=a_hbv, a_inv=a_inv, inv=inv, unitigs=us, offset=offset, n_edges=n_edges, edges=edges, dels=dels,
                                 second=spec.get("second"), hang_want=hang_want)
    return _made[key]


def second_dels(first, strings):
    """the second list of a chained case, in the ids of the first result: by edge sequence, or by the case's own rule"""
    if callable(strings):
        return strings(first)
    es = first.hb.edges
    index = {s: e for e, s in enumerate(es)}
    return np.asarray(sorted(_ids(index, strings)), np.int32)


_rest: dict = {}


def restated(key: str):
    """-> [result of every edit of the case in turn]; made once"""
    if key not in _rest:
        c = case(key)
        r = [delete_edges(c.a_hbv, c.inv, c.offset, c.n_edges, c.edges, c.dels)]
        if c.second:
            f = r[0]
            r.append(delete_edges(f.a_hbv, f.inv, f.offset, f.n_edges, f.edges, second_dels(f, c.second)))
        _rest[key] = r
    return _rest[key]


def digest(c) -> bytes:
    return str(zlib.crc32(c.a_hbv + c.a_inv + c.offset.tobytes() + c.n_edges.tobytes() + c.edges.tobytes() + c.dels.tobytes())).encode()


_gold: dict = {}


def golden(key: str):
    """the fixture -> namespace(pinned: made by the reference (else by the restatement alone), steps: [namespace(a_hbv, a_inv, offset, n_edges,
    edges, pathsx)], support, hang_dels, ref_summary); the case is made again from its seed and compared with the fixture's digest first"""
    if key not in _gold:
        z = np.load(EDIT / f"{key}.npz")
        c = case(key)
        assert bytes(z["in_digest"]) == digest(c), f"{key}: the generator no longer makes the input of the fixture"
        assert "dels" not in z or np.array_equal(z["dels"], c.dels)      # (a fuzz_<seed> fixture holds results only: the digest covers dels)
        steps = [SimpleNamespace(a_hbv=bytes(z[f"a_hbv{i}"]), a_inv=bytes(z[f"a_inv{i}"]), offset=z[f"offset{i}"], n_edges=z[f"n_edges{i}"], edges=z[f"edges{i}"],
                                 pathsx=bytes(z[f"pathsx{i}"])) for i in range(int(z["n_steps"]))]
        _gold[key] = SimpleNamespace(pinned=bool(z["pinned"]), steps=steps, support=z["support"], hang_dels=z["hang_dels"], ref_summary=bytes(z["ref_summary"]).decode())
    return _gold[key]
