"""Hand-made graphs and read paths for FindEdgePairs (snk_dev_edge_pairs; 10X/Closomatic.cc:17-354) -- test infrastructure
(tests/golden/make_hops_golden.py, tests/test_hops_host.py, tests/test_gpu_hops.py).  numpy and Python only; the unitig sets are checked
by tests/handunitigs.py's check_valid.

One graph per K (48 and 60), made of small trees that share no edge, one or two per item.  An item is a handful of read PAIRS -- each
(path of read 2q, path of read 2q + 1, barcode, bad flag), paths as strand strings -- with the edge pairs it is there for stated next
to it: `expect[(first, second)] = (in the result with flags 0, in the result with SNK_HOPS_ONE_GOOD)`.  The maker asserts every
statement against the reference's own function before it saves the fixture, and the host test asserts them against the restatement,
so a later edit cannot lose what an item is for.

Building blocks.  A junction is a (K-1)-mer; into(J, km) is an edge of km k-mers that ends in it and starts at a dead end, outof(J, km)
one that leaves it and ends in a dead end (or in the junction its last K-1 bases make: at(strand)).  gadget(stubs) = an edge `a` of
30 k-mers into a junction that the stubs leave: `a` is a sink iff every stub has at most 120 k-mers and ends dead; with 30 k-mers it
is no start of part 3 (fewer than K + 1) and no `right` (fewer than 40).  A read on [m] makes e2 = rc(m) for its mate, and
source(rc(m)) holds iff sink(m).

    case(K) -> namespace(K, unitigs (BVComp order), off, bases, items)
    arrays(c, edge_of) -> (offset, n_edges, edges), bc i32[n], bad u8[n / 2]      edge_of: strand string -> HBV edge id
    assert_items(c, edge_of, inv, {0: pairs, 1: pairs}, who)
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import handunitigs as hu

rc = hu.rc
_made: dict = {}


class _J:
    def __init__(self, seq, used_in=""):
        self.seq, self.outs, self.ins = seq, list("ACGT"), [b for b in "ACGT" if b not in used_in]


def _build(K):
    g = hu._Gen("hops", K)
    items = []
    junc = lambda: _J(g.rand(K - 1))
    into = lambda J, km: g.add(g.rand(km - 1) + J.ins.pop(0) + J.seq)
    outof = lambda J, km: g.add(J.seq + J.outs.pop(0) + g.rand(km - 1))
    at = lambda s: _J(s[-(K - 1):], used_in=s[-K])

    def gadget(stubs, a_km=30):
        J = junc()
        return SimpleNamespace(a=into(J, a_km), J=J, stubs=[outof(J, km) for km in stubs])

    def target(km):
        """an edge r for the mates of part 3: rc(r) is no sink (a 130 k-mer edge leaves where it ends)"""
        J = junc()
        into(J, 130)
        return outof(J, km)

    def start3(km_e, outs=()):
        """an edge e for part 3: no sink (a 130 k-mer edge leaves its end), followed by edges of `outs` k-mers"""
        J = junc()
        e = into(J, km_e)
        outof(J, 130)
        return SimpleNamespace(e=e, J=J, outs=[outof(J, km) for km in outs])

    def item(name, pairs, expect):
        items.append(SimpleNamespace(name=name, pairs=[(p0, p1, bc, bad) for p0, p1, bc, bad in pairs], expect=expect))

    two = lambda p0, p1: [(p0, p1, 1, 0), (p0, p1, 2, 0)]          # the same pair of paths under two barcodes
    # ---- parts 1 and 2: the sink test
    A, M = gadget((120, 30)), gadget((50, 50))
    item("sink_stub_120", two([A.a], [M.a]), {(A.a, rc(M.a)): (True, True), (M.a, rc(A.a)): (True, True)})
    A, M = gadget((121, 30)), gadget((50, 50))
    # (M.a, rc(A.a)): the source side fails -- sink(A.a) does not hold -- so only ONE_GOOD gives it; rc(A.a) has 30 k-mers: no landing for part 2
    item("sink_stub_121_and_one_good", two([A.a], [M.a]), {(A.a, rc(M.a)): (False, False), (M.a, rc(A.a)): (False, True)})
    A, M = gadget((50,)), gadget((50, 50))
    into(at(A.stubs[0]), 50)
    item("sink_end_has_second_in_edge", two([A.a], [M.a]), {(A.a, rc(M.a)): (False, False)})
    A, M = gadget((50,)), gadget((50, 50))
    outof(at(A.stubs[0]), 50)
    item("sink_end_has_out_edge", two([A.a], [M.a]), {(A.a, rc(M.a)): (False, False)})
    A, M = gadget((50, 50)), gadget((50, 50))
    item("one_class", [([A.a], [M.a], 3, 0), ([A.a], [M.a], 3, 0)], {(A.a, rc(M.a)): (False, False)})
    A, M = gadget((50, 50)), gadget((50, 50))
    item("all_bc_zero_is_one_class", [([A.a], [M.a], 0, 0), ([A.a], [M.a], 0, 0), ([A.a], [M.a], 0, 0)], {(A.a, rc(M.a)): (False, False)})
    A, M = gadget((50, 50)), gadget((50, 50))
    item("bc_zero_and_one_are_two_classes", [([A.a], [M.a], 0, 0), ([A.a], [M.a], 1, 0)], {(A.a, rc(M.a)): (True, True)})
    A = gadget((50, 50))
    item("e2_is_e1", two([A.a], [rc(A.a)]), {(A.a, A.a): (False, False), (rc(A.a), rc(A.a)): (False, False)})
    # ---- part 2: the landing (the source side fails: a 121 k-mer stub behind m)
    for km, hit in ((100, True), (99, False)):
        A, M = gadget((50, 50)), gadget((121,), a_km=km)
        item(f"part2_landing_{km}", two([A.a], [M.a]), {(A.a, rc(M.a)): (hit, True)})
    J = junc()
    a, long_in, s = into(J, 30), into(J, 121), outof(J, 110)
    item("part2_same_vertex", two([a], [rc(s)]), {(a, s): (False, True)})          # ToRight(a) == ToLeft(s); source(s) fails on the 121 k-mer in-edge
    A, M1, M2 = gadget((50, 50)), gadget((50, 50)), gadget((121,), a_km=100)
    item("part2_e1_seen_by_part1", two([A.a], [M1.a]) + [([A.a], [M2.a], 3, 0), ([A.a], [M2.a], 4, 0)], {(A.a, rc(M1.a)): (True, True), (A.a, rc(M2.a)): (False, True)})
    # ---- part 3: who starts
    for km, hit in ((K + 1, True), (K, False)):
        S, r = start3(km), target(45)
        item(f"part3_start_{'K_plus_1' if hit else 'K'}", two([S.e], [rc(r)]), {(S.e, r): (hit, hit)})
    S, r = start3(K + 1), target(45)
    item("part3_one_class", [([S.e], [rc(r)], 5, 0), ([S.e], [rc(r)], 5, 0)], {(S.e, r): (False, False)})
    # ---- part 3: round 0
    for km, hit in ((99, True), (100, False)):
        S, r = start3(K + 1, (km,)), target(45)
        item(f"part3_round0_{km}", two([S.e, S.outs[0]], [rc(r)]), {(S.e, r): (hit, hit)})
    # ---- part 3: the closure.  e -> t1 -> t2 -> t3 -> t4 of 26 k-mers each; the mates of reads on e bring [t1 t2], [t2 t3], [t3 t4]
    for n_links, hit in ((3, False), (2, True)):
        S, r = start3(K + 1, (26,)), target(45)
        t = [S.outs[0]]
        for _ in range(3):
            t.append(outof(at(t[-1]), 26))
        pairs = two([S.e], [rc(r)]) + [([S.e, t[0]], [rc(t[1]), rc(t[0])], 1, 0)]
        pairs += [([S.e], [rc(t[i + 1]), rc(t[i])], 2, 0) for i in range(1, n_links)]
        item(f"part3_closure_{n_links}_links", pairs, {(S.e, r): (hit, hit)})
    # ... through an edge of one k-mer that loops on its vertex (the junction is one base K - 1 times): e -> loop -> loop -> tl of 99 k-mers
    for base, with_tail, hit in (("A", True, False), ("C", False, True)):
        r = target(45)
        Jl = _J(base * (K - 1))
        Jl.outs.remove(base)
        Jl.ins.remove(base)
        loop = g.add(base * K)
        e = into(Jl, K + 1)
        outof(Jl, 130)
        tl = outof(Jl, 99)
        pairs = two([e], [rc(r)]) + [([e, loop], [rc(r)], 1, 0)] + ([([e], [rc(tl), rc(loop), rc(loop)], 2, 0)] if with_tail else [])
        item(f"part3_closure_loop_{'with' if with_tail else 'without'}_tail", pairs, {(e, r): (hit, hit)})
    # ... an overlap that disagrees blocks the step: y = [z t1 t2] against x = [e t1]
    for blocked, hit in ((True, True), (False, False)):
        S, r = start3(K + 1, (30,)), target(45)
        z = into(S.J, 50)
        t2 = outof(at(S.outs[0]), 100)
        y = [z, S.outs[0], t2] if blocked else [S.outs[0], t2]
        pairs = two([S.e], [rc(r)]) + [([S.e, S.outs[0]], [rc(f) for f in reversed(y)], 1, 0)]
        item(f"part3_overlap_{'mismatch' if blocked else 'match'}", pairs, {(S.e, r): (hit, hit)})
    # ---- part 3: the rights
    for km, hit in ((40, True), (39, False)):
        S, r = start3(K + 1), target(km)
        item(f"part3_right_{km}", two([S.e], [rc(r)]), {(S.e, r): (hit, hit)})
    S = start3(K + 1, (45,))
    t = S.outs[0]
    item("part3_too_easy", two([S.e], [rc(t)]) + [([S.e, t], [], 3, 0)], {(S.e, t): (False, False)})
    S = start3(K + 1, (45,))
    t = S.outs[0]
    item("part3_not_too_easy", two([S.e], [rc(t)]), {(S.e, t): (True, True)})
    S, r = start3(K + 1), target(45)
    item("part3_only_bad_pairs", [([S.e], [rc(r)], 1, 1), ([S.e], [rc(r)], 2, 1), ([S.e], [rc(r)], 3, 1)], {(S.e, r): (False, False)})
    S, r = start3(K + 1), target(45)
    item("part3_one_good_class_left", [([S.e], [rc(r)], 1, 1), ([S.e], [rc(r)], 2, 0), ([S.e], [rc(r)], 2, 0)], {(S.e, r): (False, False)})
    S = start3(K + 1)
    item("part3_f_is_inv_e", two([S.e], [S.e]), {(S.e, rc(S.e)): (False, False)})
    # ---- part 3: a self-inverse edge (its index entry is read twice), and an edge twice on one path (index duplicates)
    jp, r = g.junction(), target(45)
    pal = g.palindrome_on(jp, 2 * K + 6)
    item("part3_palindrome", two([pal], [rc(r)]), {(pal, r): (True, True)})
    for twice, hit in ((True, False), (False, True)):
        r = target(45)
        Jr = junc()
        e = into(Jr, K + 1)
        outof(Jr, 130)
        back = g.add(Jr.seq + Jr.outs.pop(0) + g.rand(1) + Jr.ins.pop(0) + Jr.seq)       # K + 2 k-mers, leaves Jr and comes back to it
        # twice on the path: from `back` the sequence [back back] grows by itself to 2 (K + 2) >= 100 k-mers; once: nothing follows it
        item(f"part3_edge_{'twice' if twice else 'once'}_on_a_path", two([e] + [back] * (2 if twice else 1), [rc(r)]), {(back, r): (hit, hit), (e, r): (hit, hit)})
    return g, items


def case(K):
    """Made once per process and left unchanged."""
    if K not in _made:
        g, items = _build(K)
        us = hu.bvcomp_sorted(sorted({min(s, rc(s)) for s in g.unitigs}))
        hu.check_valid(us, K)
        off, bases = hu.to_arrays(us)
        _made[K] = SimpleNamespace(name=f"hand_k{K}", K=K, unitigs=us, off=off, bases=bases, items=items)
    return _made[K]


def arrays(c, edge_of):
    """-> (offset i32[n], n_edges u32[n], edges i32[]), bc i32[n], bad u8[n / 2]: two reads per pair of every item, in order"""
    ne, edges, bc, bad = [], [], [], []
    for it in c.items:
        for p0, p1, b, flag in it.pairs:
            for p in (p0, p1):
                ne.append(len(p))
                edges.extend(edge_of[s] for s in p)
                bc.append(b)
            bad.append(flag)
    n = len(ne)
    return (np.zeros(n, np.int32), np.asarray(ne, np.uint32), np.asarray(edges, np.int32)), np.asarray(bc, np.int32), np.asarray(bad, np.uint8)


def edge_index(eb) -> dict:
    """strand string -> HBV edge id, from the edges' bases (extref.edge_bases)"""
    return {"".join("ACGT"[b] for b in e): i for i, e in enumerate(eb)}


def assert_items(c, edge_of, inv, pairs_by_flag: dict, who: str):
    """every item's statements against a result per flag setting (0, 1)"""
    have = {og: {(int(a), int(b)) for a, b in p} for og, p in pairs_by_flag.items()}
    wrong = []
    for it in c.items:
        for (s1, s2), want in it.expect.items():
            for og in (0, 1):
                if ((edge_of[s1], edge_of[s2]) in have[og]) != want[og]:
                    wrong.append((it.name, og, want[og]))
    assert not wrong, f"{c.name}: {who} disagrees with the stated outcome of (item, ONE_GOOD, stated): {wrong}"
