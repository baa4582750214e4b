"""Hand-made graphs, reads and paths for MowLawn (snk_dev_mow_lawn; 10X/Lawnmower.cc:301-554) -- test infrastructure
(tests/golden/make_mow_golden.py, tests/test_mow_host.py, tests/test_gpu_mow.py).  numpy and Python only; the unitig sets are made with
tests/handunitigs.py's generator and checked by its check_valid.

One graph per K, one motif per thing the rule or a kernel can get wrong.  A motif is a junction J with two in-edges e1 (n + del k-mers)
and e2 (n k-mers, a tip) and one out-edge f.  Unless a motif says otherwise e1 and e2 differ, inside the window, in the ONE base in front
of J, so a read over that base with quality q gives the record -q when it lies on e1 (it speaks for e1) and +q when it lies on e2.
Every motif states its outcome: "deleted", "kept" (scored, not deleted), "limit" (dropped by the read limit) or "none" (no candidate),
and where it matters (qss1, qss2).  The maker asserts the outcomes against the reference, the host test against the restatement.

    case(K)  -> namespace(name, K, unitigs (BVComp order), off, bases, motifs: [namespace(name, e1, e2, outcome, qss)], reads: [namespace(seq,
                quals, path (strand strings) or None, offset)], bc)
    wide(K)  -> the same shape: one e1 with about 3 000 entries of which about 100 reach the window, a group of more than 64 records,
                and a few hundred small motifs behind it
    arrays(c, edge_of) -> codes, quals, lens, (offset, n_edges, edges)
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import handbads
import handunitigs as hu
from handbads import L, Q, _other, cat

_made: dict = {}


class _Maker:
    def __init__(self, name, K):
        self.K, self.g, self.motifs, self.reads = K, hu._Gen(name, K), [], []
        self._head = 0

    # ---- reads.  Every read is the first of a pair whose mate has no path and its own first five bases, so no two pairs are duplicates
    # unless a read is given an earlier pair's head.
    def _mate(self, head=None):
        if head is None:
            self._head += 1
            head = self._head
        s = "".join("ACGT"[(head >> (2 * i)) & 3] for i in range(6)) + self.g.rand(34)
        return SimpleNamespace(seq=s, quals=np.full(len(s), Q, np.uint8), path=None, offset=0), head

    def read(self, path, offset, n, quals=(), mism=(), head=None, rc=False, qfill=Q):
        """n bases of Cat(path) from `offset` on (off its ends: A); quals = ((position, quality), ...), mism = ((position, quality), ...)
        changes the base as well.  rc: the pair's read is the reverse complement, pathed on the reverse-complement path."""
        K = self.K
        m = cat(K, path)
        s = [m[offset + i] if 0 <= offset + i < len(m) else "A" for i in range(n)]
        q = np.full(n, qfill, np.uint8)
        for i, v in quals:
            q[i] = v
        for i, v in mism:
            s[i], q[i] = _other(s[i]), v
        s = "".join(s)
        if rc:
            s, q = hu.rc(s), q[::-1].copy()
            path = [hu.rc(p) for p in reversed(path)]
            offset = len(m) - offset - n
        mate, head = self._mate(head)
        self.reads += [SimpleNamespace(seq=s, quals=q, path=path, offset=offset), mate]
        return head

    # ---- graph
    def motif(self, n, dl, tail=40, snp=True):
        """-> (e1, e2, f, J).  snp: e2 = the end of e1 with the base in front of J changed (n <= K)"""
        g, K = self.g, self.K
        J = g.junction()
        b1 = g.rand(1)
        body = g.rand(n + dl - 1)
        e1 = g.add(body + b1 + J.seq)
        assert not snp or n <= K
        e2 = g.add((body[dl:] if snp else g.rand(n - 1)) + _other(b1) + J.seq)
        c = g.rand(1)
        f = g.add(J.seq + c + g.rand(tail))
        J.take(("in", b1)); J.take(("in", _other(b1))); J.take(("out", c))
        return e1, e2, f, J

    def state(self, name, e1, e2, outcome, qss=None):
        self.motifs.append(SimpleNamespace(name=name, e1=e1, e2=e2, outcome=outcome, qss=qss))

    def support(self, e1, f, k, q=50, first=0, length=100, **kw):
        """k reads on e1.f at k different starts, the base in front of J at quality q"""
        at = len(e1) - (self.K - 1) - 1                        # the base in front of J
        for i in range(k):
            o = at - 20 - first - i
            self.read([e1, f], o, length, quals=((at - o, q[i] if isinstance(q, (list, tuple)) else q),), **kw)

    def on_e2(self, e2, f, q, o=None, length=90, **kw):
        at = len(e2) - (self.K - 1) - 1
        o = at - 30 if o is None else o
        return self.read([e2, f], o, length, quals=((at - o, q),), **kw)


def _build(K):
    M = _Maker("mow", K)
    g = M.g
    # ---- the thresholds
    e1, e2, f, _ = M.motif(1, 60); M.support(e1, f, 7); M.state("qss1_300", e1, e2, "deleted", (300, 0))
    e1, e2, f, _ = M.motif(1, 60); M.support(e1, f, 7, q=[50] * 6 + [49]); M.state("qss1_299", e1, e2, "kept", (299, 0))
    e1, e2, f, _ = M.motif(1, 60); M.support(e1, f, 7); M.on_e2(e2, f, 30); M.on_e2(e2, f, 40, o=-33); M.state("qss2_30", e1, e2, "deleted", (300, 30))
    e1, e2, f, _ = M.motif(1, 60); M.support(e1, f, 7); M.on_e2(e2, f, 31); M.on_e2(e2, f, 40, o=-33); M.state("qss2_31", e1, e2, "kept", (300, 31))
    # ---- the read limit: npe 2 passes (above), 3 does not; a dup is not counted
    e1, e2, f, _ = M.motif(1, 60); M.support(e1, f, 7)
    for o in (-30, -33, -36):
        M.on_e2(e2, f, 10, o=o)
    M.state("npe_3", e1, e2, "limit")
    e1, e2, f, _ = M.motif(1, 60); M.support(e1, f, 7)
    h = M.on_e2(e2, f, 20, o=-30); M.on_e2(e2, f, 25, o=-33); M.on_e2(e2, f, 19, o=-30, head=h)      # the third is a dup of the first (lower quality sum)
    M.state("npe_dup_not_counted", e1, e2, "deleted", (300, 20))
    # ---- the quality filter: 4 mismatches of quality 30 elsewhere are not enough, 5 are, quality 29 does not count
    for name, ms, outcome, qss in (("hq_4", ((0, 30), (1, 30), (2, 30), (3, 30)), "deleted", (300, 0)),
                                   ("hq_5", ((0, 30), (1, 30), (2, 30), (3, 30), (4, 30)), "kept", (250, 0)),
                                   ("hq_q29", ((0, 30), (1, 30), (2, 30), (3, 30), (4, 29)), "deleted", (300, 0))):
        e1, e2, f, _ = M.motif(1, 60); M.support(e1, f, 6); M.support(e1, f, 1, first=10, mism=ms); M.state(name, e1, e2, outcome, qss)
    # ---- groups: same (fw, offset) with opposite signs is void, with the same sign one value (the larger); the cap
    e1, e2, f, _ = M.motif(1, 60); M.support(e1, f, 7)
    at = len(e1) - K
    M.read([e1, f], at - 20, 100, mism=((20, 40),))                       # lies where the first supporter lies and shows e2's base
    M.state("group_void", e1, e2, "kept", (250, 0))
    e1, e2, f, _ = M.motif(1, 60); M.support(e1, f, 7); M.support(e1, f, 1, q=20); M.state("group_same_sign", e1, e2, "deleted", (300, 0))
    e1, e2, f, _ = M.motif(1, 60); M.support(e1, f, 7, q=63); M.on_e2(e2, f, 63); M.on_e2(e2, f, 63, o=-33); M.state("cap_50", e1, e2, "kept", (300, 50))
    # ---- windows: both in-edges tips of equal length (n = Kmers(e1), both orders are candidates; the other order fails the read limit)
    e1, e2, f, _ = M.motif(1, 0); M.support(e1, f, 7, first=-20, length=60); M.state("equal_tips", e1, e2, "deleted", (300, 0)); M.state("equal_tips_swapped", e2, e1, "limit")
    e1, e2, f, _ = M.motif(K, 0, snp=False); M.support(e1, f, 7, length=120); M.state("n_equals_kmers_e1", e1, e2, "deleted", (300, 0)); M.state("n_equals_kmers_e1_swapped", e2, e1, "limit")
    # ---- read shapes: both strands, a read that starts before the edge, one that ends inside the window, ragged lengths, reads on e1
    # outside the window (no record)
    e1, e2, f, _ = M.motif(70, 200, snp=False)
    w0 = 200                                                       # the window starts at base 200 of e1
    for i, (o, n) in enumerate(((w0 - 40, 100), (w0 + 10, 150), (w0 + 30, 256), (w0 - 90, 95), (w0 + 60, 31))):
        M.read([e1, f], o, n, rc=i % 2 == 1)
    M.read([e1, f], 0, 150); M.read([e1, f], 40, 160, rc=True)            # in front of the window
    M.read([e1, f], w0 - 99, 100)                                   # touches it by one base
    M.read([e1, f], w0 - 100, 100)                                  # ends at it
    M.read([e2, f], -30, 120); M.read([e2, f], 20, 256, rc=True)
    M.state("shapes", e1, e2, "kept")
    e1, e2, f, _ = M.motif(1, 60); M.support(e1, f, 4); M.support(e1, f, 3, first=4, rc=True); M.state("both_strands", e1, e2, "deleted", (300, 0))
    # ---- e1 twice in one path: f leads back to e1 (a tip t keeps the junction between them a vertex)
    J, J2 = g.junction(), g.junction()
    b1, c, d1 = g.rand(1), g.rand(1), g.rand(1)
    e1 = g.add(J2.seq + d1 + g.rand(30) + b1 + J.seq)
    e2 = g.add(_other(b1) + J.seq)
    x = g.rand(1)
    f = g.add(J.seq + c + g.rand(25) + x + J2.seq)
    t = g.add(g.rand(9) + _other(x) + J2.seq)
    J.take(("in", b1)); J.take(("in", _other(b1))); J.take(("out", c)); J2.take(("out", d1)); J2.take(("in", x)); J2.take(("in", _other(x)))
    at = len(e1) - K
    for i in range(7):
        M.read([e1, f, e1, f], at - 20 - i, 200, quals=((20 + i, 50),))
    M.state("e1_twice", e1, e2, "deleted"); M.state("e1_twice_tip_into_the_loop", f, t, None)
    # ---- near-candidates: each would be deleted if it were one
    e1, e2, f, J = M.motif(1, 60); g.add(g.rand(12) + "A" + e2[:K - 1]); g.add(g.rand(12) + "C" + e2[:K - 1]); M.support(e1, f, 7)
    M.state("e2_source_has_in_edges", e1, e2, "none")
    e1, e2, f, J = M.motif(1, 60)
    c2 = next(b for b in "ACGT" if J.free(("out", b)))
    g.add(J.seq + c2 + g.rand(20)); J.take(("out", c2)); M.support(e1, f, 7); M.state("v_two_out_edges", e1, e2, "none")
    e1, e2, f, J = M.motif(1, 60)
    b3 = next(b for b in "ACGT" if J.free(("in", b)))
    g.add(g.rand(7) + b3 + J.seq); J.take(("in", b3)); M.support(e1, f, 7); M.state("v_three_in_edges", e1, e2, "none")
    # a self-inverse f: J, then a palindrome
    J = g.junction()
    b1 = g.rand(1)
    e1 = g.add(g.rand(60) + b1 + J.seq)
    e2 = g.add(_other(b1) + J.seq)
    f = g.palindrome_on(J, 2 * K + 4)
    J.take(("in", b1)); J.take(("in", _other(b1)))
    M.support(e1, f, 7, length=80); M.state("self_inverse_f", e1, e2, "deleted", (300, 0))        # (the rule does not look at inv[f])
    return M


def _build_wide(K):
    M = _Maker("mowwide", K)
    rng = np.random.default_rng(2026)
    e1, e2, f, _ = M.motif(40, 6000, snp=False)
    w0 = 6000
    for i in range(2900):                                           # in front of the window
        M.read([e1, f], int(rng.integers(0, w0 - 160)), int(rng.integers(60, 151)), rc=bool(i & 1))
    for i in range(100):                                            # reaching it
        n = int(rng.integers(60, 151))
        M.read([e1, f], int(rng.integers(w0 - n + 1, w0 + 30)), n, rc=bool(i & 1))
    for i in range(70):                                             # one group of 70 records (70 mates with their own heads)
        M.read([e1, f], w0 - 10, 100, qfill=20 + i % 30)
    M.state("wide", e1, e2, "deleted")
    for i in range(300):
        e1, e2, f, _ = M.motif(int(rng.integers(1, K + 1)), int(rng.integers(0, 40)), tail=int(rng.integers(5, 30)))
        k = int(rng.integers(0, 9))
        if k:
            M.support(e1, f, k, q=int(rng.integers(20, 60)), length=int(rng.integers(70, 120)))
        for j in range(int(rng.integers(0, 3))):
            M.on_e2(e2, f, int(rng.integers(5, 60)), o=-30 - 3 * j)
        M.state(f"small_{i}", e1, e2, None)
    return M


def _finish(M, name):
    us = hu.bvcomp_sorted(M.g.unitigs)
    hu.check_valid(us, M.K)
    off, bases = hu.to_arrays(us)
    n = len(M.reads)
    bc = (1 + np.arange(n, dtype=np.int32) // 2 % 7).astype(np.int32)
    return SimpleNamespace(name=name, K=M.K, unitigs=us, off=off, bases=bases, motifs=M.motifs, reads=M.reads, bc=bc,
                           pairs=[SimpleNamespace(name=str(i), reads=(M.reads[2 * i], M.reads[2 * i + 1])) for i in range(n // 2)])


def case(K):
    """Made once per process and left unchanged."""
    if ("hand", K) not in _made:
        _made[("hand", K)] = _finish(_build(K), f"hand_k{K}")
    return _made[("hand", K)]


def wide(K=48):
    if ("wide", K) not in _made:
        _made[("wide", K)] = _finish(_build_wide(K), f"wide_k{K}")
    return _made[("wide", K)]


arrays = handbads.arrays
edge_index = handbads.edge_index
