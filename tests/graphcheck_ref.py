"""Plain-Python restatement of the graph verifier's rules (include/snk.h, "the graph verifier"), for the tests.

Written from the reference: EdgeBuilder (lib/assembly/src/paths/long/BuildReadQGraph48.cc:327-541: buildEdge :335-345, simpleCircle
:348-372, canonicalizeCircle :375-397, up/downstreamExtensionPossible :408-428, extend :445-464, addEdge :478-506), the adjacency prune
(kmers/ReadPather.h:346-385), Kmerizer::map (:155-172) and the reassembly checks of lib/tada/src/sim_tests.rs:297-404.  K-mers are
ACGT strings here; nothing is shared with the device code.
"""
from __future__ import annotations

import numpy as np

COUNTERS = ("table_duplicate_keys", "table_not_sorted", "count_below_min_freq", "bad_unitig", "unitig_kmer_missing", "kmer_repeated",
            "kmer_uncovered", "ctx_dangling", "ctx_not_reciprocal", "interior_break", "end_extendable", "not_canonical", "not_ordered",
            "group_mismatch", "count_mismatch", "ctx_mismatch", "good_len_mismatch", "instances_mismatch", "key_padding")
SAT = (1 << 24) - 1
_COMP = str.maketrans("ACGT", "TGCA")


def rc(s: str) -> str:
    return s.translate(_COMP)[::-1]


def form(s: str) -> int:
    """getCanonicalForm (dna/CanonicalForm.h:35-48): 0 FWD, 1 REV, 2 PALINDROME."""
    n = len(s)
    if n & 1:
        return 1 if s[n // 2] in "GT" else 0
    r = rc(s)
    return 0 if s < r else (1 if r < s else 2)


def ctx_rc(c: int) -> int:
    return int(f"{c:08b}"[::-1], 2)


def side(nib: int) -> int:
    return bin(nib & 15).count("1")


def only(nib: int) -> str:
    return "ACGT"[(nib & 15).bit_length() - 1]


def keys_to_strings(keys: np.ndarray, K: int) -> list[str]:
    """[n, 3|4] u32 words MSB-first -> the K bases of every key."""
    w = np.asarray(keys, dtype=np.uint32)
    n = w.shape[0]
    if n == 0:
        return []
    sh = np.arange(30, -2, -2, dtype=np.uint32)
    codes = ((w[:, :, None] >> sh[None, None, :]) & 3).reshape(n, -1)[:, :K].astype(np.uint8)
    asc = np.frombuffer(b"ACGT", np.uint8)[codes]
    return [bytes(r).decode() for r in asc]


class Table:
    """Entries (canonical k-mer, group) -> row; contexts looked up in the orientation a k-mer is met in."""

    def __init__(self, keys: np.ndarray, counts, ctx, K: int, groups=None):
        self.K = K
        self.kmers = keys_to_strings(keys, K)
        self.groups = [0] * len(self.kmers) if groups is None else [int(g) for g in groups]
        self.counts = [int(c) for c in counts]
        self.ctx = [int(c) for c in ctx]
        self.index: dict[tuple[str, int], int] = {}
        self.kmer_set: set[str] = set(self.kmers)       # every group's k-mers
        self.dups: list[int] = []
        for i, (k, g) in enumerate(zip(self.kmers, self.groups)):
            if (k, g) in self.index:
                self.dups.append(i)
            else:
                self.index[(k, g)] = i

    def lookup(self, s: str, g: int):
        """(row or None, context in s's orientation, palindrome)"""
        r = rc(s)
        rev = r < s
        i = self.index.get((r if rev else s, g))
        c = 0 if i is None else (ctx_rc(self.ctx[i]) if rev else self.ctx[i])
        return i, c, r == s

    def down_possible(self, s: str, c: int, g: int) -> bool:
        if side(c) != 1:
            return False
        i, c2, pal = self.lookup(s[1:] + only(c), g)
        return not pal and i is not None and side(c2 >> 4) == 1

    def up_possible(self, s: str, c: int, g: int) -> bool:
        if side(c >> 4) != 1:
            return False
        i, c2, pal = self.lookup(only(c >> 4) + s[:-1], g)
        return not pal and i is not None and side(c2) == 1


def canonical_circle(s: str, K: int) -> str:
    """canonicalizeCircle (:375-397) then addEdge's orientation (:478-486) of a circle whose last K-1 bases repeat its first."""
    L = len(s)
    m = L - K + 1
    best, idx, rev = None, 0, False
    for i in range(m):
        k = s[i:i + K]
        r = rc(k)
        c = min(k, r)
        if best is None or c < best:
            best, idx, rev = c, i, r < k
    sp = rc(s) if rev else s
    idx = L - idx - K if rev else idx
    rot = sp[idx:] + sp[K - 1:K - 1 + idx]
    return rc(rot) if form(rot) == 1 else rot


def check(keys, counts, ctx, unitigs: list[str], K: int, min_freq: int, unitig_groups=None, key_groups=None, sorted_table=True,
          ordered=True) -> dict:
    """Graph level.  keys [n, 3|4] u32 words; unitigs as ACGT strings in the order given (ordered: ascending first K bases,
    group-major); key_groups / unitig_groups: per-group runs."""
    t = Table(keys, counts, ctx, K, key_groups)
    n = {c: 0 for c in COUNTERS}
    w = np.asarray(keys, dtype=np.uint64)
    if key_groups is None and w.shape[1] == 4:       # the bits below the K bases (the group's place at K=48)
        n["key_padding"] = int(np.count_nonzero(w[:, 3] & np.uint64((1 << (128 - 2 * K)) - 1)))
    n["table_duplicate_keys"] = len(t.dups)
    n["count_below_min_freq"] = sum(1 for c in t.counts if c < min_freq)
    if sorted_table:
        rows = list(zip(t.kmers, t.groups))
        n["table_not_sorted"] = sum(1 for i in range(1, len(rows)) if rows[i] < rows[i - 1])
    for i, (k, g) in enumerate(zip(t.kmers, t.groups)):
        c = t.ctx[i]
        for b in range(4):
            for bit, nb, back in ((1 << b, k[1:] + "ACGT"[b], 0x10 << "ACGT".index(k[0])),
                                  (0x10 << b, "ACGT"[b] + k[:-1], 1 << "ACGT".index(k[-1]))):
                if c & bit:
                    j, c2, _ = t.lookup(nb, g)
                    if j is None:
                        n["ctx_dangling"] += 1
                    elif not c2 & back:
                        n["ctx_not_reciprocal"] += 1
    hits = [0] * len(t.kmers)
    circles = pals = 0
    prev_key = None
    for u, s in enumerate(unitigs):
        g = 0 if unitig_groups is None else int(unitig_groups[u])
        L = len(s)
        if L < K or any(ch not in "ACGT" for ch in s):
            n["bad_unitig"] += 1
            continue
        if ordered:
            key = (g, s[:K])
            if prev_key is not None and not prev_key < key:
                n["not_ordered"] += 1
            prev_key = key
        km = [s[i:i + K] for i in range(L - K + 1)]
        look = [t.lookup(k, g) for k in km]
        for k, (i, c, pal) in zip(km, look):
            if i is None and min(k, rc(k)) in t.kmer_set:
                n["group_mismatch"] += 1         # the k-mer is in the table, under another group
            elif i is None:
                n["unitig_kmer_missing"] += 1
            else:
                hits[i] += 1
        for j in range(1, len(km)):
            (i0, c0, p0), (i1, c1, p1) = look[j - 1], look[j]
            if i0 is None or i1 is None:
                continue
            if not (side(c0) == 1 and only(c0) == km[j][-1] and side(c1 >> 4) == 1 and not p0 and not p1):
                n["interior_break"] += 1
        f, l = look[0], look[-1]
        if L == K and f[2]:
            pals += 1
            continue
        circle = l[0] is not None and s[L - K + 1:] == s[:K - 1] and t.down_possible(km[-1], l[1], g)
        if circle:
            circles += 1
            if canonical_circle(s, K) != s:
                n["not_canonical"] += 1
            continue
        if (f[0] is not None and t.up_possible(km[0], f[1], g)) or (l[0] is not None and t.down_possible(km[-1], l[1], g)):
            n["end_extendable"] += 1
        if form(s) != 0:
            n["not_canonical"] += 1
    n["kmer_repeated"] = sum(1 for h in hits if h > 1)
    n["kmer_uncovered"] = sum(1 for h in hits if h == 0)
    return dict(counters=n, n_circles=circles, n_palindromes=pals, n_kmers=len(t.kmers), n_unitigs=len(unitigs),
                n_bases=sum(len(s) for s in unitigs))


def recount(keys, counts, ctx, codes: np.ndarray, good_lens, K: int, min_freq: int, n_instances: int = 0) -> dict:
    """Reads level: the k-mers of every read with good length >= K+1 at positions 0 .. good_len-K (Kmerizer::map, :155-172)."""
    t = Table(keys, counts, ctx, K)
    cnt = [0] * len(t.kmers)
    shadow = [0] * len(t.kmers)
    inst = 0
    asc = np.frombuffer(b"ACGT", np.uint8)
    for r in range(codes.shape[0]):
        gl = int(good_lens[r])
        if gl < K + 1:
            continue
        inst += gl - K + 1
        s = bytes(asc[codes[r, :gl]]).decode()
        prev = None
        for p in range(gl - K + 1):
            k = s[p:p + K]
            i, _, _ = t.lookup(k, 0)
            if i is not None:
                cnt[i] += 1
                if p and prev is not None:
                    pi, prev_rev = prev
                    sb, pb = 1 << "ACGT".index(k[-1]), 0x10 << "ACGT".index(s[p - 1])
                    shadow[pi] |= ctx_rc(sb) if prev_rev else sb
                    shadow[i] |= ctx_rc(pb) if rc(k) < k else pb
                prev = (i, rc(k) < k)
            else:
                prev = None
    n = {c: 0 for c in COUNTERS}
    n["count_mismatch"] = sum(1 for a, b in zip(cnt, t.counts) if min(a, SAT) != min(b, SAT))
    if min_freq > 1:
        n["ctx_mismatch"] = sum(1 for a, b in zip(shadow, t.ctx) if a != b)
    n["instances_mismatch"] = int(bool(n_instances) and inst != n_instances)
    return dict(counters=n, n_instances=inst)


def digests(keys, counts, ctx, unitigs: list[str]) -> tuple[int, int]:
    """The two digests written out one row / one base at a time (Python integers mod 2^64)."""
    M = (1 << 64) - 1

    def mix(z):
        z &= M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    td = 0
    for w, c, x in zip(np.asarray(keys, dtype=np.uint64), counts, ctx):
        w = [int(v) for v in w] + [0] * (4 - len(w))
        hi, lo = (w[0] << 32) | w[1], (w[2] << 32) | w[3]
        td += mix(lo ^ mix(hi ^ mix((min(int(c), SAT) << 8) | int(x))))
    ud = 0
    for s in unitigs:
        h = sum(mix((i << 2) | "ACGT".index(ch)) for i, ch in enumerate(s)) & M
        ud += mix(h ^ mix(len(s)))
    return td & M, ud & M
