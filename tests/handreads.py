"""Reads walked over hand-made unitig sets, for the stages in front of the graph (count, prune, unitig pull) -- test infrastructure
(tests/test_handreads_host.py, tests/test_gpu_handreads.py, tests/golden/make_handreads_golden.py).  numpy and Python only.

A unitig set (a tests/handunitigs.py case or one of the sets below) is turned into reads that contain nothing but its k-mers:

  nodes      the unitig strands (a palindrome has one); strand t follows strand s iff s[-(K-1):] == t[:K-1].  Every k-mer of a walk over
             this relation is a k-mer of some unitig.
  junction   for every node and every (predecessor, successor) pair round it, reads of up to L = 150 bases over predecessor-node-successor
  reads      (short neighbours are extended along further neighbours).  A node that fits a read with a base to spare on either side gets
             one read that holds it and both junctions; a longer node is tiled at a stride of (L - K) / 3.  The first pair of a node is
             emitted `copies` times in different barcodes, the other pairs once.
  walks      seeded random walks from random positions; a walk that runs into a dead end gives a shorter read
  then       about half the reads are reverse-complemented, and all are shuffled with a fixed seed.

The generator then ASSERTS (plain Python over strings; conditions, not measurements): no read k-mer lies outside the case; every k-mer of
the case that lies on a walk of at least K + 1 bases occurs in at least MIN_FREQ reads' worth of instances from at least two barcodes > 0;
every junction (K+1)-mer occurs.  The k-mers of an isolated unitig of exactly K bases cannot be covered by a read of K + 1 bases: they are
listed in facts["unreachable"], their K-base reads stay in the input and the pipeline has to skip them (good length < K + 1).

noise=True adds reads that touch only what must be dropped, so that the retained table, the pruned contexts and the unitigs are by
construction those of the clean reads (only counts and the unpruned contexts differ): copies of reads with one substituted base, once or
twice each (below MIN_FREQ) -- the base next to a junction, the last base of a read, a base inside a palindromic k-mer and a base of a circle among them; at
barcodes=True (K=48: the reference's K=60 build has no barcode rule) four reads of ONE barcode that fork off for 20 bases (enough
instances, one barcode); a few copies with barcode 0.  This too is asserted over strings.

noise="paths" is the variant for the stages behind the graph (read pathing, MarkDups: tests/test_handreads_paths_host.py,
tests/test_gpu_handreads_paths.py, tests/golden/make_handreads_paths_golden.py): the clean reads at random qualities of 8..40 and, among
them, a layer of reads with substituted bases and of chimeras whose new k-mers occur once each (_make_paths) -- again the graph of the
clean reads by construction, and asserted over strings.

    unitig_set(name, K) -> list of strings          reads(name, K, noise=False) -> namespace(codes, quals, lens, bc, rows, read_len, facts, digest)
    load(name, K, noise) -> the reads and the reference's results for them (tests/golden/handreads/); differs() compares a result with them
    load_paths(name, noise) -> the reads and the reference's paths and duplicate flags for them (K=48; tests/golden/handreads/paths/); paths_differ()
"""
from __future__ import annotations

import hashlib
import json
import zlib
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import handunitigs as hu
from handunitigs import is_palindrome, rc

L = 150
MIN_FREQ = 3
MIN_BC = 2
N_BC = 24
KS = (48, 60)
GOLD = Path(__file__).resolve().parent / "golden" / "handreads"

FROM_HANDUNITIGS = ("single_k", "single_k1", "single_pal_k", "single_pal_2k", "circle", "ring_2", "ring_3", "hairpin", "hairpin_flanks", "bubble",
                    "full_vertex", "palindromes", "chain_5", "chain_1025", "forest_257", "long", "mixed_seed1", "mixed_seed2", "mixed_seed3", "mixed_seed4")
TINY_PERIODS = ("A", "AC", "AT", "ACG")


def _rotations(c):
    return {c[i:] + c[:i] for i in range(len(c))}


def _circle_unitig(c, K):
    """the one unitig of the circular string c: its len(c) k-mers, the first and last (K-1)-mer equal"""
    return (c * (2 + (K + len(c)) // len(c)))[:len(c) + K - 1]


def _random_circle(g, n, taken):
    """a circular string of n bases that has n distinct k-mers, none of them the reverse complement of one of its own or of an earlier
    circle's (taken: every rotation handed out so far, both strands)"""
    for _ in range(1000):
        c = g.rand(n)
        rot = _rotations(c)
        if len(rot) == n and rc(c) not in rot and not (rot & taken):
            taken |= rot | _rotations(rc(c))
            return c
    raise AssertionError("no free circle")


def _tiny_circles(g):
    K = g.K
    for c in TINY_PERIODS:
        g.add(_circle_unitig(c, K))
    taken = set()
    for c in TINY_PERIODS:
        taken |= _rotations(c) | _rotations(rc(c))
    # round the k-mer length, the ranking's splitter spacing (split_log2 = 5) and the 256-k-mer chunk
    for n in (5, 7, K - 1, K, K + 1, 31, 32, 33, 255, 256, 257, 1000):
        g.add(_circle_unitig(_random_circle(g, n, taken), K))


def _circles_5000(g):
    taken = set()
    for n in g.rng.integers(12, 41, 5000):
        g.add(_circle_unitig(_random_circle(g, int(n), taken), g.K))


def _turns(g):
    """X + rc(X): a strand that turns round into its own reverse complement.  Isolated, it is one palindromic unitig.  Behind a flank the
    string holds every k-mer of X twice (once per strand), so it is cut where a de Bruijn graph cuts it: the palindromic k-mer c in the
    middle is a unitig of its own, the strand that ends with c[:-1] leads into it and its reverse complement leaves it; with a flank on
    either side the two flanks meet at the first (K-1)-mer of X."""
    K = g.K
    for n in (K - 1, K, K + 1, 2 * K):
        x = g.rand(n)
        g.add(x + rc(x))
    for n in (K - 1, K, K + 1, 2 * K):
        x = g.rand(n)
        p = x + rc(x)
        g.add(g.rand(23) + p[:n + K // 2 - 1])
        g.add(p[n - K // 2:n + K // 2])
    for n in (K - 1, K, K + 1, 2 * K):
        x = g.rand(n)
        p = x + rc(x)
        a, b = g.rand(19), g.rand(31)
        while a[-1] == b[-1]:
            b = g.rand(31)
        g.add(a + x[:K - 1])
        g.add(b + x[:K - 1])
        g.add(p[:n + K // 2 - 1])
        g.add(p[n - K // 2:n + K // 2])


_OWN = {"tiny_circles": _tiny_circles, "circles_5000": _circles_5000, "turns": _turns}
CASES = FROM_HANDUNITIGS + tuple(_OWN)
COPIES = {"circles_5000": 2}          # (a read of 150 bases goes round a circle of at most 40 k-mers more than twice)
HASHED = ("long", "circles_5000")     # their results are kept as SHA-256 digests (tests/golden/handreads/big_hashes.json)

_sets: dict = {}


def unitig_set(name, K):
    if (name, K) not in _sets:
        if name in _OWN:
            g = hu._Gen("handreads/" + name, K)
            _OWN[name](g)
            us = hu.bvcomp_sorted(g.unitigs)
            hu.check_valid(us, K)
        else:
            us = hu.case(name, K).unitigs
        _sets[(name, K)] = us
    return _sets[(name, K)]


# ---- the walk graph

class _Graph:
    def __init__(self, unitigs, K):
        self.K = K
        self.seq, self.unitig, self.rcid = [], [], []
        for u, s in enumerate(unitigs):
            self.seq.append(s); self.unitig.append(u)
            if is_palindrome(s):
                self.rcid.append(len(self.seq) - 1)
            else:
                self.seq.append(rc(s)); self.unitig.append(u)
                self.rcid += [len(self.seq) - 1, len(self.seq) - 2]
        starts: dict = {}
        for i, s in enumerate(self.seq):
            starts.setdefault(s[:K - 1], []).append(i)
        self.succ = [starts.get(s[-(K - 1):], []) for s in self.seq]
        self.pred = [[self.rcid[j] for j in self.succ[self.rcid[i]]] for i in range(len(self.seq))]
        self.forward = [i for i in range(len(self.seq)) if self.rcid[i] >= i]

    def right(self, first, need):
        """up to `need` bases that follow a node when the walk goes on with node `first` and then along first successors"""
        out, n, j = [], 0, first
        while j is not None and n < need:
            t = self.seq[j][self.K - 1:]
            out.append(t); n += len(t)
            j = self.succ[j][0] if self.succ[j] else None
        return "".join(out)[:max(need, 0)]

    def left(self, first, need):
        return rc(self.right(None if first is None else self.rcid[first], need))

    def on_circle(self, i):
        """node i lies on a cycle of nodes that have one predecessor and one successor each"""
        j = i
        for _ in range(len(self.seq) + 1):
            if len(self.succ[j]) != 1 or len(self.pred[j]) != 1:
                return False
            j = self.succ[j][0]
            if j == i:
                return True
        return False


def _canon_counts(reads, bcs, K, into=None):
    """canonical k-mer -> [instances, set of barcodes > 0] over the reads of at least K + 1 bases (shorter ones are skipped by the pipeline)"""
    tab = {} if into is None else into
    for s, b in zip(reads, bcs):
        n = len(s)
        if n < K + 1:
            continue
        r = rc(s)
        for p in range(n - K + 1):
            k, q = s[p:p + K], r[n - K - p:n - p]
            e = tab.get(k if k <= q else q)
            if e is None:
                e = tab[k if k <= q else q] = [0, set()]
            e[0] += 1
            if b > 0:
                e[1].add(b)
    return tab


def _canon_set(strings, K):
    out = set()
    for s in strings:
        n = len(s)
        r = rc(s)
        for p in range(n - K + 1):
            k, q = s[p:p + K], r[n - K - p:n - p]
            out.add(k if k <= q else q)
    return out


def _standing(e, barcodes):
    return e is not None and e[0] >= MIN_FREQ and (not barcodes or len(e[1]) >= MIN_BC)


def _make(name, K, noise, barcodes):
    us = unitig_set(name, K)
    G = _Graph(us, K)
    rng = np.random.default_rng(zlib.crc32(f"handreads/{name}/{K}".encode()))
    copies = COPIES.get(name, 3)
    stride = (L - K) // 3
    reads, bcs, origin = [], [], []
    serial = [0]

    def emit(s, node, n_copies):
        for c in range(n_copies):
            reads.append(s); origin.append(node)
            bcs.append(1 + (serial[0] * 5 + c) % N_BC)
        serial[0] += 1

    for i in G.forward:
        n = G.seq[i]
        for pi, p in enumerate(G.pred[i] or [None]):
            for qi, q in enumerate(G.succ[i] or [None]):
                first = pi == 0 and qi == 0
                if len(n) + 2 <= L:
                    room = L - len(n)
                    lf = G.left(p, room // 2)
                    rf = G.right(q, room - len(lf))
                    lf = G.left(p, room - len(rf))
                    emit(lf + n + rf, i, copies if first else 1)
                else:
                    lf, rf = G.left(p, stride), G.right(q, stride)
                    w = lf + n + rf
                    starts = sorted(set(range(0, len(w) - L + 1, stride)) | {len(w) - L})
                    for a in starts:
                        if first or a < len(lf) or a + L > len(lf) + len(n):
                            emit(w[a:a + L], i, copies if first else 1)
    n_junction_reads = len(reads)
    for _ in range(max(16, n_junction_reads // 8)):
        j = int(rng.integers(0, len(G.seq)))
        s = G.seq[j][int(rng.integers(0, len(G.seq[j]))):]
        while len(s) < L and G.succ[j]:
            j = G.succ[j][int(rng.integers(0, len(G.succ[j])))]
            s += G.seq[j][K - 1:]
        reads.append(s[:L]); origin.append(-1); bcs.append(int(rng.integers(1, N_BC + 1)))

    # ---- the conditions
    case_kmers = _canon_set(us, K)
    isolated_k = [s for i, s in enumerate(G.seq) if G.rcid[i] >= i and len(s) == K and not G.succ[i] and not G.pred[i]]
    unreachable = _canon_set(isolated_k, K)
    reachable = case_kmers - unreachable
    tab = _canon_counts(reads, bcs, K)
    assert set(tab) <= case_kmers, "a read holds a k-mer that is not the case's"
    assert set(tab) == reachable, "a k-mer that a walk of K + 1 bases reaches is in no read (or an unreachable one is)"
    for k in reachable:
        assert tab[k][0] >= MIN_FREQ and len(tab[k][1]) >= MIN_BC, f"{name} K={K}: {k} has {tab[k][0]} instances in barcodes {sorted(tab[k][1])}"
    junctions = {G.seq[i][-K:] + G.seq[q][K - 1] for i in range(len(G.seq)) for q in G.succ[i]}
    have = _canon_set([s for s in reads if len(s) >= K + 1], K + 1)
    for j in junctions:
        assert min(j, rc(j)) in have, f"{name} K={K}: the junction {j} is in no read"
    assert all(any(s == r or rc(s) == r for r in reads) for s in isolated_k)
    facts = dict(n_unitigs_in=len(us), n_nodes=len(G.seq), n_case_kmers=len(case_kmers), n_reachable=len(reachable), unreachable=sorted(unreachable),
                 n_junctions=len(junctions), n_clean_reads=len(reads), noise=None)

    # ---- strands and order.  A noise read lies on the strand of the read it was made from: a palindromic k-mer cannot be turned to a
    # canonical strand, so the reference records "c followed by x" and "comp(x) followed by c" in different context bits, and the noisy
    # run has the clean run's contexts only if it shows every k-mer of the case in the orientations the clean run shows
    flip = list(rng.random(len(reads)) < 0.5)
    if noise:
        facts["noise"], parents = _add_noise(name, K, G, rng, reads, bcs, origin, case_kmers, reachable, tab, barcodes)
        flip += [flip[p] for p in parents]
    order = rng.permutation(len(reads))
    n = len(reads)
    codes = np.zeros((n, L), np.uint8)
    quals = np.zeros((n, L), np.uint8)
    lens = np.zeros(n, np.uint16)
    bc = np.zeros(n, np.int32)
    for row, i in enumerate(order):
        s = rc(reads[i]) if flip[i] else reads[i]
        lens[row] = len(s)
        codes[row, :len(s)] = hu._CODE[np.frombuffer(s.encode(), np.uint8)]
        quals[row, :len(s)] = 30
        bc[row] = bcs[i]
    facts["n_reads"] = n
    return SimpleNamespace(name=name, K=K, noise=noise, codes=codes, quals=quals, lens=lens, bc=bc, read_len=L, facts=facts,
                           digest=digest(codes, quals, lens, bc))


def _add_noise(name, K, G, rng, reads, bcs, origin, case_kmers, reachable, clean_tab, barcodes):
    """appends the noise reads; -> (what was added, per noise read the clean read it was made from)"""
    n_clean = len(reads)
    usable = [i for i in range(n_clean) if len(reads[i]) >= K + 1]
    subs = {"junction": 0, "end": 0, "palindrome": 0, "circle": 0, "random": 0}
    noise_reads, noise_bcs, parents = [], [], []
    used = set()         # the noise k-mers so far: a later spot must not add instances to them

    def substitute(i, pos, kind):
        s = reads[i]
        for d in (1, 2, 3):
            m = s[:pos] + "ACGT"[("ACGT".index(s[pos]) + d) % 4] + s[pos + 1:]
            touched = _canon_set([m[max(0, pos - K + 1):pos + K]], K)
            if not (touched & case_kmers) and not (touched & used):
                used.update(touched)
                for c in range(1 + sum(subs.values()) % 2):
                    noise_reads.append(m); noise_bcs.append(1 + (bcs[i] + 3 * c) % N_BC); parents.append(i)
                subs[kind] += 1
                return True
        return False

    # the base next to a junction (the first base a successor adds); where every base that may follow the junction is taken, as at a
    # full vertex, a substitution there makes a k-mer of the case: the next junction is tried
    free_junction = False
    for i in usable:
        o = origin[i]
        if o >= 0 and G.succ[o] and len(G.seq[o]) + 2 <= L:
            at = reads[i].find(G.seq[o])
            if at >= 0 and at + len(G.seq[o]) < len(reads[i]):
                free_junction |= len(G.succ[o]) < 4 and len(G.pred[G.succ[o][0]]) < 2
                if substitute(i, at + len(G.seq[o]), "junction"):
                    break
    # the last base of a read: its last k-mer becomes a noise k-mer and the k-mer in front of it, untouched, gets a context bit that the
    # prune has to clear -- also where a read has no room for anything else (a unitig of K + 1 bases)
    for i in usable:
        if substitute(i, len(reads[i]) - 1, "end"):
            break
    # a base inside a palindromic k-mer
    pals = {k for k in reachable if k == rc(k)}
    for i in usable:
        s = reads[i]
        at = next((p for p in range(len(s) - K + 1) if s[p:p + K] in pals), -1)
        if at >= 0 and substitute(i, at + K // 2, "palindrome"):
            break
    # a base of a circle
    for i in usable:
        if origin[i] >= 0 and G.on_circle(origin[i]) and substitute(i, len(reads[i]) // 2, "circle"):
            break
    for i in rng.choice(usable, min(len(usable), max(8, min(60, len(usable) // 40))), replace=False) if usable else []:
        substitute(int(i), int(rng.integers(0, len(reads[int(i)]))), "random")
    branch = 0
    if barcodes:
        at = next((i for i in usable if len(reads[i]) >= K + 40), None)
        if at is not None:
            src = reads[at]
            for _ in range(64):
                tail = "".join("ACGT"[x] for x in rng.integers(0, 4, 20))
                m = src[:len(src) - 20] + tail
                forked = _canon_set([m[len(src) - 20 - K + 1:]], K)
                if tail[0] != src[len(src) - 20] and not (forked & case_kmers) and not (forked & used):
                    for _ in range(4):
                        noise_reads.append(m); noise_bcs.append(N_BC + 1); parents.append(at)          # a barcode that no other read has
                    branch = 1
                    break
    unbarcoded = 0
    for i in (rng.choice(n_clean, min(n_clean, 5), replace=False) if n_clean else []):
        noise_reads.append(reads[int(i)]); noise_bcs.append(0); parents.append(int(i))
        unbarcoded += 1
    # no noise k-mer reaches the thresholds, no case k-mer loses its standing, the unreachable stay unreachable
    tab = _canon_counts(noise_reads, noise_bcs, K)
    for k, e in tab.items():
        if k in case_kmers:
            assert k in reachable, "a noise read covers an unreachable k-mer"
        else:
            assert not _standing(e, barcodes), f"{name} K={K}: the noise k-mer {k} would be kept"
    for k in reachable:
        e = clean_tab[k]
        assert _standing(e, barcodes)
    assert subs["junction"] > 0 or not free_junction
    assert subs["palindrome"] > 0 or not pals
    assert subs["end"] > 0 or not usable
    assert subs["circle"] > 0 or not any(G.on_circle(i) for i in G.forward)
    reads += noise_reads
    bcs += noise_bcs
    origin += [-2] * len(noise_reads)
    return dict(substitutions=subs, one_barcode_branch=branch, unbarcoded=unbarcoded, n_noise_reads=len(noise_reads),
                n_noise_kmers=sum(k not in case_kmers for k in tab)), parents


def digest(codes, quals, lens, bc) -> str:
    h = hashlib.sha256()
    for a in (codes, quals, lens, bc):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---- the third variant, for the pather: the clean reads at random qualities and a layer of reads with errors

KINDS = ("sub1", "first", "last", "sub2near", "sub2far", "chimera")
LAYER_BC = N_BC + 2          # the layer's own barcode (N_BC + 1 is the noisy variant's one-barcode branch)
VARIANTS = (False, True, "paths")


def vname(noise):
    return "paths" if noise == "paths" else "noisy" if noise else "clean"


def _make_paths(name, K):
    """The reads of noise="paths".  The clean reads keep their order among themselves, their strands and barcodes, at qualities drawn from
    8..40 (never below min_qual = 7: the trim and the count see what they saw).  Among them, at drawn places, lie the reads of the error
    layer: made from the clean reads of at least K + 1 bases, in a barcode of their own, at qualities drawn from 0..40, a quarter with a Q2
    tail of 0..30 bases.  One layer read per such clean read (five at least), its kind taken in turn from sub1, first, last, sub2near, sub2far (one
    substituted base anywhere / the first base / the last base / two fewer than 10 apart / two more than K apart: a captured gap between
    two seeds, where the read has 2K + 10 bases, else sub1); then one chimera per four clean reads, at least 8 (single_k1, whose one read of
    K + 1 bases has six joints with itself, gets those that are free): a prefix of at least K
    bases of one clean read joined to a suffix of another, reverse-complemented half the time, cut to L bases.
    ASSERTED over strings: every k-mer that covers a changed base or a chimera's joint lies outside the case and in no other layer read
    (one instance: never retained), so the table, the pruned contexts and the unitigs stay those of the clean reads; every kind occurs
    (sub2far where a clean read has 2K + 10 bases); the number of reads is even, so that MarkDups runs.  A case without a read of K + 1
    bases (single_k, single_pal_k) has no layer.  rows added to the namespace: kind i8[n] (-1: a clean read, else the index into KINDS),
    parent i32[n] (the row of the clean read a layer read was made from; a chimera's: its prefix's), clean_rows (the rows of the clean reads)."""
    c = reads(name, K, False)
    rng = np.random.default_rng(zlib.crc32(f"handreads/{name}/{K}/paths".encode()))
    asc = np.frombuffer(b"ACGT", np.uint8)
    clean = [asc[c.codes[i, :int(c.lens[i])]].tobytes().decode() for i in range(len(c.lens))]
    case_kmers = _canon_set(unitig_set(name, K), K)
    usable = [i for i, s in enumerate(clean) if len(s) >= K + 1]
    long_enough = [i for i in usable if len(clean[i]) >= 2 * K + 10]
    used: set = set()
    layer, kinds, parents = [], [], []

    def accept(m, windows):
        """the k-mers of m inside the windows (those that cover a changed base, or a chimera's joint) are new: outside the case, in no layer read"""
        touched = _canon_set([m[max(0, a):b] for a, b in windows], K)
        once = _canon_counts([m], [LAYER_BC], K)          # (a chimera of a read and its own reverse complement, two substitutions a circle's period apart: twice)
        if not touched or (touched & case_kmers) or (touched & used) or any(once[k][0] != 1 for k in touched):
            return False
        used.update(touched)
        return True

    def substituted(s, spots):
        m = s
        for pos in spots:
            for d in (1, 2, 3):
                t = m[:pos] + "ACGT"[("ACGT".index(m[pos]) + d) % 4] + m[pos + 1:]
                w = _canon_set([t[max(0, pos - K + 1):pos + K]], K)
                if not (w & case_kmers) and not (w & used):
                    break
            m = t
        return m if accept(m, [(pos - K + 1, pos + K) for pos in spots]) else None

    def spots_of(kind, n):
        if kind == "first":
            return [0]
        if kind == "last":
            return [n - 1]
        if kind == "sub2near":
            p = int(rng.integers(0, n - 1))
            return [p, min(n - 1, p + int(rng.integers(1, 10)))]
        if kind == "sub2far":
            p = int(rng.integers(0, n - K - 1))
            return [p, int(rng.integers(p + K + 1, n))]
        return [int(rng.integers(0, n))]

    for t in range(max(len(usable), 5) if usable else 0):          # (at least one turn per kind)
        i, kind = usable[t % len(usable)], KINDS[t % 5]
        if kind == "sub2far" and len(clean[i]) < 2 * K + 10:
            if long_enough and not kinds.count(4):
                i = long_enough[0]          # (the case has few reads of that length: the kind's first turn takes one of them)
            else:
                kind = "sub1"
        for _ in range(4):
            m = substituted(clean[i], spots_of(kind, len(clean[i])))
            if m is not None:
                layer.append(m); kinds.append(KINDS.index(kind)); parents.append(i)
                break
            if kind in ("first", "last"):
                break
    n_chimeras = max(8, len(clean) // 4) if usable else 0
    if usable:
        n_chimeras += (len(clean) + len(layer) + n_chimeras) % 2          # (an even number of reads)
    for _ in range(n_chimeras):
        for _ in range(32):
            i, j = (int(x) for x in rng.choice(usable, 2))
            a, b = clean[i], rc(clean[j]) if rng.random() < 0.5 else clean[j]
            cut = int(rng.integers(K, len(a) + 1))
            m = (a[:cut] + b[len(b) - int(rng.integers(K, len(b) + 1)):])[:L]
            if len(m) > cut and accept(m, [(cut - K + 1, cut + K - 1)]):
                layer.append(m); kinds.append(5); parents.append(i)
                break
    if (len(clean) + len(layer)) % 2 and layer:          # (a chimera found no free joint)
        layer.pop(); kinds.pop(); parents.pop()
    # every k-mer of a layer read is a k-mer of the case or one of the layer's own, and those occur once
    own = _canon_counts(layer, [LAYER_BC] * len(layer), K)
    for k, e in own.items():
        assert k in case_kmers or (k in used and e[0] == 1), f"{name} K={K}: the layer k-mer {k} has {e[0]} instances"
    n_kind = {k: kinds.count(x) for x, k in enumerate(KINDS)}
    if usable:
        assert all(n_kind[k] > 0 for k in KINDS if k != "sub2far") and (n_kind["sub2far"] > 0 or not long_enough), (name, K, n_kind)
        one_read = len({min(clean[i], rc(clean[i])) for i in usable}) == 1          # (single_k1: one read of K + 1 bases has six joints with itself)
        assert n_kind["chimera"] >= (1 if one_read else 8), (name, K, n_kind)
    for m, x, p in zip(layer, kinds, parents):
        s = clean[p]
        diff = [q for q in range(min(len(m), len(s))) if m[q] != s[q]]
        if KINDS[x] == "chimera":
            assert len(m) <= L and m[:K] == s[:K]
        else:
            assert len(m) == len(s) and len(diff) == (2 if x in (3, 4) else 1)
            assert x != 1 or diff == [0]
            assert x != 2 or diff == [len(s) - 1]
            assert x != 3 or diff[1] - diff[0] < 10
            assert x != 4 or (diff[1] - diff[0] > K and len(s) >= 2 * K + 10)
    # ---- the rows: the clean reads in their order, the layer's reads at drawn places among them
    n = len(clean) + len(layer)
    is_layer = np.zeros(n, bool)
    is_layer[rng.choice(n, len(layer), replace=False)] = True
    clean_rows = np.nonzero(~is_layer)[0]
    codes = np.zeros((n, L), np.uint8)
    quals = np.zeros((n, L), np.uint8)
    lens = np.zeros(n, np.uint16)
    bc = np.zeros(n, np.int32)
    kind = np.full(n, -1, np.int8)
    parent = np.full(n, -1, np.int32)
    codes[clean_rows], lens[clean_rows], bc[clean_rows] = c.codes, c.lens, c.bc
    for row in clean_rows:
        quals[row, :lens[row]] = rng.integers(8, 41, int(lens[row]))
    for t, row in enumerate(np.nonzero(is_layer)[0]):
        m = layer[t]
        lens[row], bc[row], kind[row], parent[row] = len(m), LAYER_BC, kinds[t], clean_rows[parents[t]]
        codes[row, :len(m)] = hu._CODE[np.frombuffer(m.encode(), np.uint8)]
        quals[row, :len(m)] = rng.integers(0, 41, len(m))
        if rng.random() < 0.25:
            quals[row, len(m) - int(rng.integers(0, 31)):len(m)] = 2
    facts = dict(c.facts, noise=None, n_reads=n, layer=dict(n_layer_reads=len(layer), n_layer_kmers=sum(k not in case_kmers for k in own), kinds=n_kind))
    assert n % 2 == 0 or not layer
    return SimpleNamespace(name=name, K=K, noise="paths", codes=codes, quals=quals, lens=lens, bc=bc, read_len=L, facts=facts, kind=kind, parent=parent,
                           clean_rows=clean_rows, digest=digest(codes, quals, lens, bc))


_reads: dict = {}


def reads(name, K, noise=False):
    """Made once per process and left unchanged.  The noisy reads carry the one-barcode branch at K=48 only; noise="paths" is the
    pather's variant (_make_paths)."""
    noise = "paths" if noise == "paths" else bool(noise)
    key = (name, K, noise)
    if key not in _reads:
        r = _make_paths(name, K) if noise == "paths" else _make(name, K, noise, barcodes=K == 48)
        r.rows = None
        _reads[key] = r
    return _reads[key]


def rows(r):
    from supernova_amd import synth
    if r.rows is None:
        r.rows = synth.pack_rows(r.codes)
    return r.rows


# ---- the reference's results

FIELDS = ("goodlens", "keys", "counts", "ctx", "hist", "unitigs")


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def normalised(K, goodlens, keys, counts, ctx, spectrum, unitigs) -> dict:
    """One result (the reference's, the oracle's or the device's) in the fixture's layout: keys u32[n, 3 or 4] (the unused fourth word of a
    K=48 key must be zero), counts clamped to the reference's 24 bits, the spectrum cut behind its last non-zero bin, the unitigs as text."""
    keys = np.asarray(keys, np.uint32)
    w = 3 if K == 48 else 4
    assert keys.ndim == 2 and keys.shape[1] >= w and not keys[:, w:].any()
    spec = np.asarray(spectrum).astype(np.int64)
    nz = np.nonzero(spec)[0]
    return dict(goodlens=np.asarray(goodlens).astype(np.uint32), keys=np.ascontiguousarray(keys[:, :w]),
                counts=np.minimum(np.asarray(counts).astype(np.uint32), (1 << 24) - 1).astype(np.uint32), ctx=np.asarray(ctx, np.uint8),
                hist=spec[:(nz[-1] + 1 if len(nz) else 0)], unitigs=np.frombuffer("\n".join(unitigs).encode(), np.uint8))


def key_strings(keys, K):
    """table keys (16 bases per 32-bit word from the top) -> the k-mers as strings"""
    keys = np.asarray(keys, np.uint32)
    j = np.arange(K)
    b = (keys[:, j // 16] >> (2 * (15 - j % 16)).astype(np.uint32)) & 3
    asc = np.frombuffer(b"ACGT", np.uint8)[b]
    return [row.tobytes().decode() for row in asc]


_gold: dict = {}


def golden(name, K):
    """-> namespace(hashed, clean: dict, noisy: dict, digests: {False: .., True: ..}, unitig_lens, n_circles): per field an array, or its
    SHA-256 for the HASHED cases.  The K=60 reference writes no spectrum: there "hist" is the histogram of its own counts."""
    if (name, K) not in _gold:
        if name in HASHED:
            z = json.loads((GOLD / "big_hashes.json").read_text())[f"{name}_k{K}"]
            g = SimpleNamespace(hashed=True, clean=z["clean"], noisy=z["noisy"], digests={False: z["reads_digest"], True: z["reads_digest_noisy"]},
                                unitig_lens=np.asarray(z["unitig_lens"], np.int64), n_kmers=int(z["n_kmers"]))
        else:
            z = np.load(GOLD / f"{name}_k{K}.npz")
            clean = {f: z[f] for f in FIELDS}
            noisy = dict(clean, goodlens=z["goodlens_noisy"], counts=z["counts_noisy"], hist=z["hist_noisy"])
            g = SimpleNamespace(hashed=False, clean=clean, noisy=noisy, digests={False: bytes(z["reads_digest"]).decode(), True: bytes(z["reads_digest_noisy"]).decode()},
                                unitig_lens=z["unitig_lens"].astype(np.int64), n_kmers=int(len(z["counts"])))
        _gold[(name, K)] = g
    return _gold[(name, K)]


def load(name, K, noise=False):
    """the reads and the reference's results for them -> (reads, expectation); the reads are regenerated and checked against the digest"""
    r, g = reads(name, K, noise), golden(name, K)
    assert r.digest == g.digests[bool(noise)], f"{name} K={K}: the generator no longer makes the reads the fixture was made from"
    return r, SimpleNamespace(hashed=g.hashed, fields=g.noisy if noise else g.clean, unitig_lens=g.unitig_lens, n_kmers=g.n_kmers)


# ---- the reference's paths (K=48: it has no K=60 pather), tests/golden/handreads/paths/, written by tests/golden/make_handreads_paths_golden.py

PATHS_GOLD = GOLD / "paths"
PATH_FIELDS = ("path_off", "path_n", "path_edges")
DUP_FIELDS = ("dup", "interdup", "art_perc")          # (where the number of reads is even: MarkDups takes pairs)
_pgold: dict = {}


def load_paths(name, noise):
    """The reads of one variant, regenerated and checked against the digest, and what the reference's pathReads and MarkDups made of them
    -> (reads, namespace(hashed, fields: per PATH_FIELDS / DUP_FIELDS name an array (a float for the two rates), or its SHA-256 for the
    HASHED cases, has_dups))"""
    if name not in _pgold:
        _pgold[name] = (json.loads((PATHS_GOLD / "big_hashes.json").read_text())[f"{name}_k48"] if name in HASHED
                        else dict(np.load(PATHS_GOLD / f"{name}_k48.npz")))
    z, v, r = _pgold[name], vname(noise), reads(name, 48, noise)
    if name in HASHED:
        fields, dg = dict(z[v]), z[v]["reads_digest"]
    else:
        fields = {f: z[f"{v}_{f}"] for f in PATH_FIELDS + DUP_FIELDS if f"{v}_{f}" in z}
        dg = bytes(z[f"{v}_reads_digest"]).decode()
    assert r.digest == dg, f"{name} {v}: the generator no longer makes the reads the fixture was made from"
    for f in ("interdup", "art_perc"):
        if f in fields:
            fields[f] = float(fields[f])
    return r, SimpleNamespace(hashed=name in HASHED, fields=fields, has_dups="dup" in fields)


def paths_differ(exp, got: dict):
    """None, or the name of the first field of PATH_FIELDS / DUP_FIELDS (those the expectation has) in which a result differs from it;
    got: path_off, path_n, path_edges, and with duplicate flags dup, interdup and n_art (the number of artifactual pairs)"""
    for f in PATH_FIELDS + DUP_FIELDS:
        if f not in exp.fields or (f == "art_perc" and "n_art" not in got):
            continue
        if f == "interdup":
            same = float(got[f]) == exp.fields[f]
        elif f == "art_perc":          # the reference only logs it, at two significant digits: the count goes through the same rounding
            same = float(f"{100.0 * got['n_art'] / max(len(got['dup']), 1):.2g}") == float(f"{exp.fields[f]:.2g}")
        else:
            a = np.ascontiguousarray(got[f], np.uint8 if f == "dup" else np.int32)
            same = sha(a) == exp.fields[f] if exp.hashed else np.array_equal(a, exp.fields[f])
        if not same:
            return f
    return None


def differs(exp, got: dict, fields=FIELDS):
    """None, or the name of the first field in which a normalised result differs from the expectation"""
    for f in fields:
        if (sha(got[f]) != exp.fields[f]) if exp.hashed else not np.array_equal(got[f], exp.fields[f]):
            return f
    if "unitigs" in fields:
        lens = np.asarray([len(u) for u in bytes(got["unitigs"]).decode().split("\n")] if len(got["unitigs"]) else [], np.int64)
        if not np.array_equal(lens, exp.unitig_lens):
            return "unitig_lens"
    return None
