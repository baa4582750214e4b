"""Seeded random graphs, closures and deletion lists for gap-patch insertion (Engine.insert_patch; StageInsertPatch,
10X/runstages/RunStages.cc:176-230) and the graph edit behind it (Engine.delete_edges / hanging_ends / trim_hanging_ends; DeleteEdgesParallel
+ Cleanup, paths/long/large/GapToyTools.cc:1287-1302, and the selection of StageTrim) -- test infrastructure
(tests/test_patch_fuzz_host.py, tests/test_gpu_patch_fuzz.py, tests/golden/make_patch_golden.py, tests/golden/make_edit_golden.py).  numpy and
Python only.

The old graph (a tests/handunitigs.py generator, K = 48 and 60 in turn): 3 to 8 junctions with 4 to 15 random edges between them on both
strands -- hairpins, self-loops, parallel edges and vertices with one edge in and one out come by themselves --, 1 to 4 free unitigs of K to
K + 150 bases, and each of these by a coin: a ring of 1 to 3 pieces, a unitig of K bases, a palindromic k-mer, a unitig of 500 to 900 bases
(three pieces and more), handunitigs._hairpin_flanks, and two free unitigs of exactly 200 and 201 k-mers (the bound of the hanging-end
rule).

The closures: 0 to 30 per case, each of a drawn kind (KINDS).  A flank is a K-base window of an old edge, by a coin the edge's end or any
position, so closures land inside edges and cut them, several times per edge.
  bridge    flank + 0 to 60 random bases + flank (gap 0: 2K bases)
  tandem    the gap is a unit of 1 to 70 bases repeated to 1 to 400 bases: periods below and above K, k-mers twice in one closure
  rc        the reverse complement of an earlier closure
  sub       a prefix, suffix or middle of an earlier closure, K - 1 bases or more
  third     the gap runs K to K + 40 bases along a third old edge, between random pieces of 0 to 6 bases
  same      from an edge back into the same edge
  strand    from an edge onto its own other strand
  short     K - 1, K or K + 1 random bases, a palindromic K-mer, K bases of an old edge (forward, or reverse-complemented)
  boundary  256, 257, 512 - K, 513 - K or 769 - 2K bases: the lengths at which a sequence gains a piece
  branch    two closures with one gap of K to 2K bases and different flanks: a branch inside new sequence
The paths on the old graph are patchref.place_paths as it is.

The edit step's inputs (edit_input) are drawn from the same seed on the PATCHED graph -- the restatement's (patchref.insert_patch), which the
device must reproduce before its edit is looked at: place_paths on it, only walks whose consecutive edges meet at a vertex, without the
walks that touch a drawn, inv-closed fifth of bare edges (and the edges of 200 and 201 k-mers, bare always), every third of what is left;
the deletion list is editref.tenth of the patched graph, on odd seeds joined with the hanging-end selection, shuffled and with duplicates
as editref.case does.

    make_case(seed)  -> namespace(key, seed, K, a_hbv, a_inv (the old graph's files), old_unitigs (BVComp order), closures, kinds (one per
                        closure), offset, n_edges, edges) or None: the seed is skipped.  A skip is decided from the old graph alone:
                        handunitigs.check_valid fails, or the generator's strings are not the graph's unitigs.
    patched(c)       -> patchref.insert_patch of the case, made once
    edit_input(c)    -> the namespace editref.case returns (key, K, a_hbv, a_inv, inv, unitigs, offset, n_edges, edges, dels, ...)
    edited(c)        -> (editref.delete_edges of edit_input(c), (support, hanging-end selection) on the patched graph), made once
    chain(c)         -> everything the device is compared with, as one dict; computed afresh (what the planted changes of
                        tests/test_patch_fuzz_host.py go through)

Nothing the reference's own functions refuse was found on this distribution (tests/golden/patch/fuzz_<seed>.npz and
tests/golden/edit/fuzz_<seed>.npz: the pinned seeds PINNED), so no class of input is left out.
"""
from __future__ import annotations

import zlib
from types import SimpleNamespace

import numpy as np

import handunitigs as hu

N_SEEDS = 120
KINDS = ("bridge", "tandem", "rc", "sub", "third", "same", "strand", "short", "boundary", "branch")
HANG_KMERS = 200                                 # StageTrim's bound (RunStages.cc:91-146): edit_input keeps the edges next to it bare
# the seeds whose reference results are kept (6 per K): together every closure kind and every condition of test_patch_fuzz_host.py
PINNED = (0, 5, 8, 13, 16, 21, 24, 29, 32, 37, 40, 45)
_made: dict = {}


def sample() -> list:
    """every fourth seed, K = 48 and 60 in turn: what the CPU tests run the restatements over"""
    return [4 * i + i % 2 for i in range(N_SEEDS // 4)]


def key_of(seed: int) -> str:
    return f"fuzz_{seed}"


def generate(seed: int):
    """-> (K, the old graph's strings, draw(edge strings, inv) -> (closures, kinds)); one random stream per seed"""
    K = (48, 60)[seed % 2]
    g = hu._Gen(f"patchfuzz/{seed}", K)
    rng = g.rng
    ri = lambda lo, hi: int(rng.integers(lo, hi + 1))
    coin = lambda p=0.5: bool(rng.random() < p)
    js = [g.junction() for _ in range(ri(3, 8))]
    for _ in range(ri(4, 15)):
        a, b = js[ri(0, len(js) - 1)], js[ri(0, len(js) - 1)]
        g.edge(a, ri(0, 1), b, ri(0, 1), ri(20, 260) if coin(0.3) else None, must=False)
    for _ in range(ri(1, 4)):
        g.add(g.rand(K + ri(0, 150)))
    if coin():
        g.ring(ri(1, 3))
    if coin():
        g.add(g.rand(K))
    if coin():
        g.add(g.pal(K))
    if coin():
        g.add(g.rand(ri(500, 900)))
    if coin():
        hu._hairpin_flanks(g)
    if coin():
        g.add(g.rand(K - 1 + HANG_KMERS))
        g.add(g.rand(K + HANG_KMERS))

    def draw(es, inv):
        E = len(es)

        def window(e, right):
            """K bases of edge e: by a coin its end (what a closure leaves from, or its start: what a closure arrives at) or anywhere"""
            s = es[e]
            if coin():
                return s[:K] if right else s[-K:]
            p = ri(0, len(s) - K)
            return s[p:p + K]

        any_edge = lambda: ri(0, E - 1)
        left, right = (lambda: window(any_edge(), False)), (lambda: window(any_edge(), True))
        closures, kinds = [], []
        n = ri(0, 30)
        while len(closures) < n:
            kind = KINDS[ri(0, len(KINDS) - 1)]
            if kind in ("rc", "sub") and not closures or kind == "branch" and n - len(closures) < 2:
                kind = "bridge"
            if kind == "bridge":
                new = [left() + g.rand(ri(0, 60)) + right()]
            elif kind == "tandem":
                unit, L = g.rand(ri(1, 70)), ri(1, 400)
                new = [left() + (unit * (L // len(unit) + 1))[:L] + right()]
            elif kind == "rc":
                new = [hu.rc(closures[ri(0, len(closures) - 1)])]
            elif kind == "sub":
                x = closures[ri(0, len(closures) - 1)]
                L = ri(min(K - 1, len(x)), len(x))
                p = (0, len(x) - L, ri(0, len(x) - L))[ri(0, 2)]
                new = [x[p:p + L]]
            elif kind == "third":
                c = es[any_edge()]
                L = min(len(c), ri(K, K + 40))
                p = ri(0, len(c) - L)
                new = [left() + g.rand(ri(0, 6)) + c[p:p + L] + g.rand(ri(0, 6)) + right()]
            elif kind in ("same", "strand"):
                e = any_edge()
                new = [window(e, False) + g.rand(ri(0, 30)) + window(e if kind == "same" else int(inv[e]), True)]
            elif kind == "short":
                sub, e = ri(0, 5), any_edge()
                p = ri(0, len(es[e]) - K)
                new = [(g.rand(K - 1), g.rand(K), g.rand(K + 1), g.pal(K), es[e][p:p + K], hu.rc(es[e][p:p + K]))[sub]]
            elif kind == "boundary":
                L = (256, 257, 512 - K, 513 - K, 769 - 2 * K)[ri(0, 4)]
                new = [left() + g.rand(L - 2 * K) + right()]
            else:
                gap = g.rand(ri(K, 2 * K))
                new = [left() + gap + right(), left() + gap + right()]
            closures += new
            kinds += [kind] * len(new)
        return closures, kinds

    return K, g.unitigs, draw


def make_case(seed: int):
    """Made once per process and left unchanged."""
    if seed in _made:
        return _made[seed]
    import a48xref
    import patchref
    K, strings, draw = generate(seed)
    c = None
    try:
        hu.check_valid(hu.bvcomp_sorted(strings), K)
        us = patchref.new_unitigs(strings, K)    # the strings as the graph stage leaves them: canonical, circles rotated
        ok = sorted(len(s) for s in us) == sorted(len(s) for s in strings)
    except AssertionError:
        ok = False
    if ok:
        a_hbv, a_inv = patchref.graph_files(us, K)
        g = a48xref.parse_hbv(a_hbv)
        es = patchref.edge_strings(g)
        inv = np.frombuffer(a_inv, "<i4", offset=16).astype(np.int32)
        closures, kinds = draw(es, inv)
        offset, n_edges, edges = patchref.place_paths(f"fuzz/{seed}", g, [len(s) for s in es])
        c = SimpleNamespace(key=key_of(seed), seed=seed, K=K, a_hbv=a_hbv, a_inv=a_inv, old_unitigs=us, closures=closures, kinds=kinds, offset=offset, n_edges=n_edges,
                            edges=edges, want={})
    _made[seed] = c
    return c


def edit_input(c, m=None):
    """the edit step's input on the patched graph m (default: patched(c), and then made once)"""
    if m is None and "edit_input" in c.want:
        return c.want["edit_input"]
    import editref
    import patchref
    keep, m = m is None, patched(c) if m is None else m
    K, g3 = c.K, m.g3
    es = patchref.edge_strings(g3)
    lens = np.asarray([len(s) for s in es], np.int64)
    inv = np.frombuffer(m.a_inv, "<i4", offset=16).astype(np.int32)
    rng = np.random.default_rng(zlib.crc32(f"patchfuzz/edit/{c.seed}".encode()))
    low = np.flatnonzero(np.arange(g3.E) <= inv)
    pick = rng.choice(low, max(1, len(low) // 5), replace=False)
    bare = set(pick.tolist()) | set(inv[pick].tolist()) | set(np.flatnonzero(np.isin(lens - K + 1, (HANG_KMERS, HANG_KMERS + 1))).tolist())
    paths = editref.split_paths(*patchref.place_paths(f"fuzz-edit/{c.seed}", g3, lens))
    meets = lambda p: all(g3.v_right[a] == g3.v_left[b] for a, b in zip(p, p[1:]))
    paths = [(o, p) for o, p in paths if not bare & set(p) and meets(p)][::3]
    offset, n_edges, edges = editref.join_paths(paths)
    dels = editref.tenth(inv, f"dels/{c.key}")
    if c.seed % 2:
        dels = np.union1d(dels, editref.hanging_ends(m.a_hbv, inv, n_edges, edges, HANG_KMERS)[1]).astype(np.int32)
    dels = rng.permutation(np.concatenate([dels, dels[:len(dels) // 3]])).astype(np.int32)
    ec = SimpleNamespace(key=c.key, K=K, a_hbv=m.a_hbv, a_inv=m.a_inv, inv=inv, unitigs=m.unitigs, offset=offset, n_edges=n_edges, edges=edges, dels=dels, second=None,
                         hang_want=None)
    if keep:
        c.want["edit_input"] = ec
    return ec


def patched(c):
    if "patched" not in c.want:
        import patchref
        c.want["patched"] = patchref.insert_patch(c.K, c.a_hbv, c.closures, c.offset, c.n_edges, c.edges)
    return c.want["patched"]


def edited(c):
    if "edited" not in c.want:
        import editref
        ec = edit_input(c)
        c.want["edited"] = (editref.delete_edges(ec.a_hbv, ec.inv, ec.offset, ec.n_edges, ec.edges, ec.dels),
                            editref.hanging_ends(ec.a_hbv, ec.inv, ec.n_edges, ec.edges, HANG_KMERS))
    return c.want["edited"]


def chain(c) -> dict:
    """Both restatements over the case, nothing cached -> everything the device is compared with"""
    import editref
    import patchref
    m = patchref.insert_patch(c.K, c.a_hbv, c.closures, c.offset, c.n_edges, c.edges)
    ec = edit_input(c, m)
    d = editref.delete_edges(ec.a_hbv, ec.inv, ec.offset, ec.n_edges, ec.edges, ec.dels)
    support, hang = editref.hanging_ends(ec.a_hbv, ec.inv, ec.n_edges, ec.edges, HANG_KMERS)
    off, ids = patchref.flat(m.to3)
    return dict(a_hbv=m.a_hbv, a_inv=m.a_inv, to3_off=off, to3=ids, left3=m.left3, edge=m.edge, offset=m.offset, pathsx=m.pathsx, counters=tuple(m.counters[k] for k in patchref.COUNTERS),
                e_hbv=d.a_hbv, e_inv=d.a_inv, e_offset=d.offset, e_n_edges=d.n_edges, e_edges=d.edges, e_map=d.edge_map, e_koff=d.edge_koff,
                e_counters=tuple(d.counters[k] for k in editref.COUNTERS), support=support, hang=hang)


def same(a: dict, b: dict) -> bool:
    return all((np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]) for k in a)
