"""Hand-made graphs, reads and paths for MarkBads (snk_dev_mark_bads; 10X/SecretOps.cc:22-59,70-107) -- test infrastructure
(tests/golden/make_bads_golden.py, tests/test_bads_host.py, tests/test_gpu_bads.py).  numpy and Python only; the unitig sets are made
with tests/handunitigs.py's generator and checked by its check_valid.

One graph per K (48 and 60).  Every item is a PAIR of reads with the flag it must get stated next to it: `plain` (the ReadPath overload)
and `x` (the ReadPathVecX overload: int16 offsets).  The maker asserts both against the reference's own functions before it saves the
fixture, and the host test asserts them against the restatement, so a later edit cannot lose what a pair is for.

The usual device: five mismatches at quality 30 somewhere harmless (badsum = 150: not bad) and ONE more at quality 1 at the position
the pair is about.  The pair is bad iff that position is counted.

    case(K, plain_only=False) -> namespace(K, unitigs (BVComp order), off, bases, pairs: list of namespace(name, reads: two of
                   namespace(seq, quals, path (strand strings) or None, offset), plain, x))
        plain_only: the pairs whose paths a ReadPathVecX cannot hold -- SNK_BADS_X refuses them, so they have no x flag
    arrays(c, edge_of, only=None) -> codes, quals, lens, (offset, n_edges, edges)      edge_of: strand string -> HBV edge id
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import handunitigs as hu

L = 256                  # the longest read: the row width
Q = 30                   # the quality of a base nobody chose one for
QMAX = 63                # the largest quality the reference's PQVec takes (feudal/PQVec.cc:30-35)
_made: dict = {}


def cat(K, path):
    """hb.Cat, a chain of TrimCat (feudal/BaseVec.h:550-558): what is there loses its last K-1 bases, the next strand goes behind it whole
    -- adjacent or not"""
    m = path[0]
    for p in path[1:]:
        m = m[:len(m) - (K - 1)] + p
    return m


def _other(b):
    return "CGTA"["ACGT".index(b)]


def _read(m, offset, n, mism=(), fill="A"):
    """n bases that lie on m at `offset` (positions off m: `fill`), with the read positions in mism = ((l, quality), ...) changed"""
    s = [m[offset + l] if 0 <= offset + l < len(m) else fill for l in range(n)]
    q = np.full(n, Q, np.uint8)
    for l, ql in mism:
        s[l] = _other(s[l])
        q[l] = ql
    return "".join(s), q


def _build(K, plain_only):
    g = hu._Gen("bads", K)
    pairs = []

    def rd(path, offset, n, mism=(), seq=None, quals=None):
        if seq is None:
            seq, quals = _read(cat(K, path), offset, n, mism)
        elif quals is None:
            quals = np.full(len(seq), Q, np.uint8)
        assert len(seq) == len(quals) <= L
        return SimpleNamespace(seq=seq, quals=np.asarray(quals, np.uint8), path=path, offset=offset)

    def pair(name, r0, r1, plain, x=None):
        pairs.append(SimpleNamespace(name=name, reads=(r0, r1), plain=bool(plain), x=bool(plain if x is None else x)))

    five = lambda ls: tuple((l, Q) for l in ls)                   # badsum 150
    # ---- the graph (the same for both sets, so that both run on one a.hbv)
    A = g.add(g.rand(K + 260))                                     # alone
    j1, j2 = g.junction(), g.junction()
    b1, d1 = g.rand(1), g.rand(1)
    c0 = g.add(g.rand(60) + j1.seq)
    c1 = g.add(j1.seq + b1 + g.rand(20) + j2.seq)
    s1 = g.add(j1.seq + _other(b1) + g.rand(15))
    c2 = g.add(j2.seq + d1 + g.rand(70))
    s2 = g.add(j2.seq + _other(d1) + g.rand(12))
    j1.take(("out", b1)); j1.take(("out", _other(b1))); j2.take(("out", d1)); j2.take(("out", _other(d1)))
    jp = g.junction()
    pal = g.palindrome_on(jp, 2 * K + 6)
    fp = g.edge(g.junction(), 0, jp, 0, 4)
    jr = g.junction()
    body = g.rand(5)
    ring = g.add(jr.seq + body + jr.seq)
    ent = g.add(g.rand(40) + _other(body[-1]) + jr.seq)
    long = g.add(g.rand(66000))
    clean = lambda: rd([A], 10, 150)
    nopath = lambda n=150: rd(None, 0, n, seq=g.rand(n))
    if not plain_only:
        # ---- the threshold: > 150, per read
        pair("sum_150", rd([A], 10, 150, five((20, 40, 60, 80, 100))), clean(), False)
        pair("sum_151", rd([A], 10, 150, five((20, 40, 60, 80, 100)) + ((120, 1),)), clean(), True)
        pair("split_150_150", rd([A], 10, 150, five((20, 40, 60, 80, 100))), rd([A], 30, 150, five((1, 2, 3, 4, 149))), False)
        # ---- the ends of m: epos = -1 and |m| are skipped, 0 and |m| - 1 counted
        base = five((10, 20, 30, 40, 45))
        pair("epos_minus_1", rd([A], -1, 100, base + ((0, 1),)), clean(), False)
        pair("epos_0", rd([A], -1, 100, base + ((1, 1),)), clean(), True)
        pair("epos_end", rd([A], len(A) - 50, 100, base + ((50, 1),)), clean(), False)
        pair("epos_last", rd([A], len(A) - 50, 100, base + ((49, 1),)), clean(), True)
        pair("negative_offset", rd([A], -60, 150, five((60, 61, 62, 63, 149)) + ((0, QMAX), (59, QMAX))), clean(), False)
        # ---- the second and third edge: the last base of the overlap (S_j + K-2) and the first base of the edge's own (S_j + K-1)
        for tag, path in (("fw", [c0, c1, c2]), ("rc", [hu.rc(c2), hu.rc(c1), hu.rc(c0)])):
            S = [0]
            for p in path[:-1]:
                S.append(S[-1] + len(p) - (K - 1))
            o = 30 if tag == "fw" else S[1] - 20
            harmless = (0, 1, 2, 3, 4)
            pair(f"{tag}_150", rd(path, o, 200, five(harmless)), clean(), False)
            for j in (1, 2):
                for what, at in (("last_overlap", S[j] + K - 2), ("first_own", S[j] + K - 1)):
                    assert 4 < at - o < 200 and at < len(cat(K, path))
                    pair(f"{tag}_edge{j}_{what}", rd(path, o, 200, five(harmless) + ((at - o, 1),)), clean(), True)
        # ---- a self-inverse edge between a flank and its reverse complement
        path = [fp, pal, hu.rc(fp)]
        S1 = len(fp) - (K - 1)
        pair("palindrome_150", rd(path, 2, 150, five((0, 1, 2, 3, 4))), clean(), False)
        pair("palindrome_first_own", rd(path, 2, 150, five((0, 1, 2, 3, 4)) + ((S1 + K - 1 - 2, 1),)), clean(), True)
        pair("palindrome_middle", rd([pal], 0, len(pal), five((0, 1, 2, 3, 4)) + ((len(pal) // 2, 1),)), clean(), True)
        # ---- who has a path
        pair("mate_without_path", rd([A], 10, 150, five((20, 40, 60, 80, 100)) + ((120, 1),)), nopath(), True)
        pair("mate_without_path_first", nopath(), rd([A], 10, 150, five((20, 40, 60, 80, 100)) + ((120, 1),)), True)
        pair("both_bad", rd([A], 10, 150, five((20, 40, 60, 80, 100)) + ((120, 1),)), rd([A], 50, 150, five((1, 2, 3, 4, 5)) + ((6, 1),)), True)
        pair("no_paths", nopath(), nopath(40), False)
        # ---- lengths: 0 with a path, 1, 256
        pair("length_0_with_path", rd([A], 10, 0), clean(), False)
        pair("length_1", rd([A], 10, 1, ((0, QMAX),)), rd([A], len(A) - 1, 1, ((0, QMAX),)), False)
        pair("length_256_at_150", rd([A], 5, 256, five((0, 100, 200, 254, 255))), clean(), False)
        pair("length_256_last_base", rd([A], 5, 256, five((0, 100, 200, 253, 254)) + ((255, 1),)), clean(), True)
        seq = "".join(_other(b) for b in A[10:10 + 256])
        pair("all_mismatch_top_quality", rd([A], 10, 256, seq=seq, quals=np.full(256, QMAX, np.uint8)), clean(), True)
        # ---- a long edge: offsets an int16 cannot hold.  65536 + 5 wraps to 5, 32768 to -32768 (all of the read in front of m), -32769 to 32767
        lg = lambda a, n=150: long[a:a + n]
        comp = lambda s: "".join(_other(b) for b in s)
        pair("far_where_it_lies", rd([long], 65541, 150, seq=lg(65541)), nopath(), False, True)          # X compares it at base 5
        pair("far_lies_at_wrapped", rd([long], 65541, 150, seq=lg(5)), nopath(), True, False)
        pair("offset_32768", rd([long], 32768, 150, seq=comp(lg(32768))), nopath(), True, False)          # X: every position skipped
        pair("offset_32767", rd([long], 32767, 150, seq=comp(lg(32767))), nopath(), True, True)           # the last offset that fits
        pair("offset_minus_32769", rd([long], -32769, 150, seq=comp(lg(32767))), nopath(), False, True)   # plain: every position skipped
        pair("offset_minus_32769_match", rd([long], -32769, 150, seq=lg(32767)), nopath(), False, False)
        pair("offset_minus_32768", rd([long], -32768, 150, seq=comp(lg(32767))), nopath(), False, False)   # fits: skipped in both
    else:
        # ---- a path whose edges are not adjacent: m shows the LATER edge's bases in the K-1 bases the two would share
        path = [c0, s2]
        assert c0[-(K - 1):] != s2[:K - 1]
        pair("nonadjacent_later_wins", rd(path, 30, 80, five((0, 1, 2, 3, 4))), clean(), False)
        m_earlier = c0 + s2[K - 1:]                                  # what m would be if the earlier edge supplied the overlap
        seq, q = _read(m_earlier, 30, 80, five((0, 1, 2, 3, 4)))
        pair("nonadjacent_read_follows_earlier", rd(path, 30, 80, seq=seq, quals=q), clean(), True)
        # ---- a path of 256 edges: one more than a ReadPathVecX record counts
        path = [ent] + [ring] * 255
        at = len(ent) - (K - 1) - 7
        pair("path_256_edges_150", rd(path, at, 150, five((0, 1, 2, 3, 4))), clean(), False)
        pair("path_256_edges_151", rd(path, at, 150, five((0, 1, 2, 3, 4)) + ((149, 1),)), clean(), True)
    return g, pairs


def case(K, plain_only=False):
    """Made once per process and left unchanged."""
    k = (K, bool(plain_only))
    if k not in _made:
        g, pairs = _build(K, plain_only)
        us = hu.bvcomp_sorted(g.unitigs)
        hu.check_valid(us, K)
        off, bases = hu.to_arrays(us)
        _made[k] = SimpleNamespace(name=f"hand{'plain' if plain_only else ''}_k{K}", K=K, unitigs=us, off=off, bases=bases, pairs=pairs)
    return _made[k]


def arrays(c, edge_of, only=None):
    """-> codes u8[n, L], quals u8[n, L], lens u16[n], (offset i32[n], n_edges u32[n], edges i32[]); only: the names of the pairs to take"""
    reads = [r for p in c.pairs if only is None or p.name in only for r in p.reads]
    n = len(reads)
    codes, quals, lens = np.zeros((n, L), np.uint8), np.zeros((n, L), np.uint8), np.zeros(n, np.uint16)
    off, ne, edges = np.zeros(n, np.int32), np.zeros(n, np.uint32), []
    for i, r in enumerate(reads):
        lens[i] = len(r.seq)
        if len(r.seq):
            codes[i, :len(r.seq)] = hu._CODE[np.frombuffer(r.seq.encode(), np.uint8)]
            quals[i, :len(r.seq)] = r.quals
        if r.path is not None:
            off[i], ne[i] = r.offset, len(r.path)
            edges.extend(edge_of[s] for s in r.path)
    return codes, quals, lens, (off, ne, np.asarray(edges, np.int32))


def edge_index(eb) -> dict:
    """strand string -> HBV edge id, from the edges' bases (extref.edge_bases)"""
    return {"".join("ACGT"[b] for b in e): i for i, e in enumerate(eb)}
