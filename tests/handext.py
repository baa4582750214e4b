"""Hand-made graphs and reads for the path extension (snk_dev_extend_paths; ExtendPathsNew, 10X/Extend.cc:14-177) -- test infrastructure
(tests/golden/make_ext_golden.py, tests/test_extend_host.py, tests/test_gpu_extend.py).  numpy and Python only; the unitig sets are made
with tests/handunitigs.py's generator and checked by its check_valid.

One graph per K (48 and 60: the K=60 reference has no pather, so this is K=60's only source of paths), several components, and reads
walked along known paths with chosen qualities.  An input path is ONE edge at a chosen offset (or none).  Every read says what it is
for: `hits[back]` = the counters of the restatement (tests/extref.py) it must raise without and with the backward leg, and `n_out[back]`
= the number of edges its path must end with.  The maker asserts them through the restatement before it saves the fixture, the host test
asserts them again, so a later edit cannot lose what a read is for.

    case(K) -> namespace(K, unitigs (BVComp order), off, bases, reads: list of namespace(name, seq, quals, first (the strand the path's
               one edge is a copy of, or None: no path), offset, hits, n_out))
    arrays(c, edge_of) -> codes, quals, lens, (offset, n_edges, edges)      edge_of: strand string -> HBV edge id
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import handunitigs as hu

L = 150                  # the longest read
Q = 30                   # the quality of a base nobody chose one for
_made: dict = {}


def walk(K, *strands):
    """the bases of a walk over strands that overlap by K - 1"""
    s = strands[0]
    for t in strands[1:]:
        assert s[-(K - 1):] == t[:K - 1], "not a walk"
        s += t[K - 1:]
    return s


def _other(b, *more):
    return next(c for c in "ACGT" if c != b and c not in more)


def _tree(g, root, depth):
    """the full 4-ary tree of one-k-mer edges below `root`: node = a (K-1)-mer, its four out-edges = node + b"""
    K = g.K
    nodes = [root[-(K - 1):]]
    for _ in range(depth):
        nxt = []
        for x in nodes:
            for b in "ACGT":
                g.add(x + b)
                nxt.append(x[1:] + b)
        nodes = nxt


def _build(K):
    g = hu._Gen("extend", K)
    reads = []

    def read(name, seq, first, offset, hits0=(), n0=1, hits1=None, n1=None, quals=None):
        q = np.full(len(seq), Q, np.uint8) if quals is None else np.asarray(quals, np.uint8)
        assert len(q) == len(seq) <= L
        hits1 = hits0 if hits1 is None else hits1
        n1 = n0 if n1 is None else n1
        reads.append(SimpleNamespace(name=name, seq=seq, quals=q, first=first, offset=offset, hits=(frozenset(hits0), frozenset(hits1)), n_out=(n0, n1)))

    def mutate(s, i):
        return s[:i] + _other(s[i]) + s[i + 1:]

    # ---- a full 4-ary tree of depth 4 below a long root: the list passes 101 entries as soon as the read reaches 4 bases beyond the root
    r4 = g.add(g.rand(K + 70))
    _tree(g, r4, 4)
    beyond = "ACGT"[K % 4] + "GATC"
    s = r4[30:] + beyond                                   # 5 bases beyond the root, along one branch
    read("tree4_too_many_mismatch", mutate(s, 20), r4, 30, {"n_too_many"}, 1)          # a mismatch on the root: leg 3 stays out, the path is unchanged
    read("tree4_too_many_exact", s, r4, 30, {"n_too_many", "n_exact_extended"}, 5)      # ... without it leg 3 walks down the branch, to its leaf
    read("tree4_three_beyond", r4[30:] + beyond[:3], r4, 30, {"n_quality_extended"}, 4)   # 341 entries, but entry 101 is never looked at: 85 are expanded
    # ---- the depth-3 tree: 85 entries, 64 of them cover a read that ends on a leaf
    r3 = g.add(g.rand(K + 70))
    _tree(g, r3, 3)
    read("tree3_extended", r3[25:] + "TCA", r3, 25, {"n_quality_extended"}, 4)
    read("tree3_two_beyond", r3[25:] + "TC", r3, 25, {"n_quality_extended"}, 3)
    q = np.full(len(r3) - 25 + 3, Q, np.uint8)
    q[-1] = 4                                              # the last base decides between four leaves and weighs 4: declined, and leg 3 takes it
    read("tree3_ambiguous_then_exact", r3[25:] + "TCA", r3, 25, {"n_ambiguous", "n_exact_extended"}, 4, quals=q)
    # ---- MIN_GAIN, both sides: three tails below a junction; the read follows the first, the second differs from it in the first base
    # beyond the junction only (as far as the read goes), the third in the first two
    j = g.junction()
    rt = g.add(g.rand(60) + j.seq)
    b0, c0 = g.rand(1), g.rand(1)
    b1, b2 = _other(b0), _other(b0, _other(b0))
    t0 = g.add(j.seq + b0 + c0 + g.rand(25))
    t1 = g.add(j.seq + b1 + c0 + g.rand(21))
    t2 = g.add(j.seq + b2 + _other(c0) + g.rand(17))
    for b in (b0, b1, b2):
        j.take(("out", b))
    s = rt[10:] + t0[K - 1:K + 1]                          # two bases into the tails
    for qa, qb, hit, n in ((4, 1, "n_ambiguous", 2), (5, 1, "n_quality_extended", 2), (4, 0, "n_ambiguous", 2), (5, 0, "n_quality_extended", 2)):
        q = np.full(len(s), Q, np.uint8)
        q[-2], q[-1] = qa, qb                              # runner-up = the second tail at qa, the third at qa + qb
        read(f"gain_{qa}_{qb}", s, rt, 10, {hit} | ({"n_exact_extended"} if hit == "n_ambiguous" else set()), n, quals=q)
    # ---- a read that ends exactly at an edge's last base, and one base beyond it
    read("ends_at_edge_end", rt[20:], rt, 20, (), 1)
    read("one_beyond", rt[20:] + t1[K - 1], rt, 20, {"n_quality_extended"}, 2)
    # the backward leg: the same walk, the path given on the tail at a negative offset
    s = walk(K, rt, t2)[30:30 + 100]
    read("back_onto_root", s, t2, 30 - (len(rt) - (K - 1)), (), 1, {"n_back_extended", "n_quality_extended"}, 2)
    s2 = mutate(s, 3)                                      # a mismatch in front of the tail: no in-edge agrees
    read("back_declined", s2, t2, 30 - (len(rt) - (K - 1)), (), 1)
    # ---- a ring with an entry: leg 3 goes round it until the read ends
    jr = g.junction()
    body = g.rand(5)
    ring = g.add(jr.seq + body + jr.seq)
    ent = g.add(g.rand(40) + _other(body[-1]) + jr.seq)
    lap = len(ring) - (K - 1)
    s = walk(K, ent, ring, ring, ring, ring)
    at = len(ent) - (K - 1) - 7                            # 7 bases in front of the ring
    n_round = 1 + (L - 7 - len(ring) + lap - 1) // lap      # edges of a path over the L - 7 bases on the ring
    read("ring_exact", s[at:at + L], ring, -7, {"n_exact_extended"}, n_round, {"n_back_extended", "n_quality_extended"}, n_round + 1)
    read("ring_enumerated", s[at + 7:at + 7 + L], ring, 0, {"n_quality_extended"}, 1 + (L - len(ring) + lap - 1) // lap)
    # ---- a hairpin with two flanks: the walk leaves through the reverse complement of the other flank
    v = g.junction()
    h = g.edge(v, 0, v, 1, 9)
    f1 = g.edge(g.junction(), 0, v, 0, 5)
    f2 = g.edge(g.junction(), 0, v, 0, 17)
    s = walk(K, f1, h, hu.rc(f2))
    at = len(f1) - (K - 1) - 2
    read("hairpin", s[at:at + L], f1, at, {"n_quality_extended"}, 3)
    read("hairpin_back", s[len(f1) - (K - 1) - 4:][:L], h, -4, {"n_exact_extended"}, 2, {"n_back_extended", "n_quality_extended"}, 3)
    # ---- a palindromic edge on a junction
    jp = g.junction()
    pal = g.palindrome_on(jp, 2 * K + 6)
    fp = g.edge(g.junction(), 0, jp, 0, 4)
    s = walk(K, fp, pal, hu.rc(fp))
    at = len(fp) - (K - 1) - 2
    read("palindrome", s[at:at + L], fp, at, {"n_quality_extended"}, 3)
    # ---- no path, and reads shorter than K with one
    read("empty_path", g.rand(L), None, 0, (), 0)
    read("empty_path_short", g.rand(20), None, 0, (), 0)
    read("shorter_than_K", r4[40:40 + K - 10], r4, 40, (), 1)
    read("shorter_than_K_mismatch", mutate(r4[40:40 + K - 10], 5), r4, 40, (), 1)
    read("one_base", r3[len(r3) - 1:], r3, len(r3) - 1, (), 1)
    read("last_base_and_three", r3[len(r3) - 1:] + "GAT", r3, len(r3) - 1, {"n_quality_extended"}, 4)
    return g, reads


def case(K):
    """Made once per process and left unchanged."""
    if K not in _made:
        g, reads = _build(K)
        us = hu.bvcomp_sorted(g.unitigs)
        hu.check_valid(us, K)
        off, bases = hu.to_arrays(us)
        _made[K] = SimpleNamespace(name=f"hand_k{K}", K=K, unitigs=us, off=off, bases=bases, reads=reads)
    return _made[K]


def arrays(c, edge_of):
    """-> codes u8[n, L], quals u8[n, L], lens u16[n], (offset i32[n], n_edges u32[n], edges i32[])"""
    n = len(c.reads)
    codes, quals, lens = np.zeros((n, L), np.uint8), np.zeros((n, L), np.uint8), np.zeros(n, np.uint16)
    off, ne, edges = np.zeros(n, np.int32), np.zeros(n, np.uint32), []
    for i, r in enumerate(c.reads):
        lens[i] = len(r.seq)
        codes[i, :len(r.seq)] = hu._CODE[np.frombuffer(r.seq.encode(), np.uint8)]
        quals[i, :len(r.seq)] = r.quals
        if r.first is not None:
            off[i], ne[i] = r.offset, 1
            edges.append(edge_of[r.first])
    return codes, quals, lens, (off, ne, np.asarray(edges, np.int32))


def edge_index(eb) -> dict:
    """strand string -> HBV edge id, from the edges' bases (extref.edge_bases)"""
    return {"".join("ACGT"[b] for b in e): i for i, e in enumerate(eb)}


def special(kind, K=48):
    """Unitig sets with one read each for the refusals that no pather's path and no de Bruijn graph reaches:
      long_in_edge  an in-edge of more than 32767 k-mers in front of a path at a negative offset: the backward leg would move the offset
                    beyond what a ReadPathVecX holds
      multi_match   two out-edges of one vertex with the same base at K-1 (no de Bruijn graph has them), met by leg 3
    -> namespace(K, unitigs (BVComp order), seq, first, offset)"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{K}".encode()))
    rnd = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    v = rnd(K - 1)
    if kind == "long_in_edge":
        long, first = rnd(33000) + v, v + "A" + rnd(60)
        us = [long, first, v + "C" + rnd(30)]
        seq, offset = walk(K, long, first)[len(long) - (K - 1) - 30:][:110], -30
    elif kind == "multi_match":
        first = rnd(50) + v
        us = [first, v + "AC" + rnd(30), v + "AG" + rnd(25), v + "C" + rnd(20)]
        seq, offset = rnd(3) + first + "ACG", -3                       # three bases in front of the path: ExtendPath returns, leg 3 walks
    else:
        raise KeyError(kind)
    return SimpleNamespace(K=K, unitigs=hu.bvcomp_sorted(us), seq=seq, first=first, offset=offset)


def special_arrays(s, edge_of, n_edges=1):
    """-> codes u8[1, L], quals u8[1, L], lens u16[1], (offset, n_edges, edges): the read of special() with its first edge n_edges times"""
    codes, quals = np.zeros((1, L), np.uint8), np.full((1, L), Q, np.uint8)
    codes[0, :len(s.seq)] = hu._CODE[np.frombuffer(s.seq.encode(), np.uint8)]
    return codes, quals, np.array([len(s.seq)], np.uint16), (np.array([s.offset], np.int32), np.array([n_edges], np.uint32), np.full(n_edges, edge_of[s.first], np.int32))
