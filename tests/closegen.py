"""Seeded random gaps for CloseGap / CloseGap2 (snk_dev_close_gaps; 10X/Closomatic.cc:356-657) -- test infrastructure
(tests/test_closures_fuzz_host.py, tests/test_gpu_closures_fuzz.py, tests/golden/make_closures_golden.py).  numpy and Python only.

A case is a graph of isolated edges as in tests/handclose.py, K = 48 and 60 in turn, with 2 to 5 loci.  A locus is a sequence
S = A + gap + B, edge A its first NA bases, edge B its last NB; the reads are laid with stated paths and offsets (nothing is pathed), read
2q and 2q + 1 are mates.  Both sides are made by one routine in the coordinates of T = S (side 0, X = A) or T = rc(S') (side 1,
X = rc(B) = inv[B], the edge CloseGap builds its second stack on): a read at t0 is given on X (a forward row: path [X], offset t0) or on
rc(X) (a reverse row: path [rc(X)], offset NX - (t0 + n), negative when the read ends behind X).  The reads of a side end at most `reach`
bases behind X, so the two stacks share reach0 + reach1 - gap columns, drawn around the thresholds of GetOffsets1.

What is drawn (see generate): edge lengths K + 5 .. 450 and 1 100, read lengths 80 / 100 / 150 (256 once) with ragged reads, the gap random
or a tandem repeat -- filling the gap, with the reads ending inside it, or thin (a short repeat inside the shared columns between flanks
of 4 to 9) --, 0 .. 30 rows a side (300 and 70 once in 20 seeds each), substitutions, a burst of 20 or more mismatches between the two sides
inside 40 shared columns (a bad window), a comb of mismatches 8 columns apart (no seed of 9), columns where all reads have qualities 0 .. 2
and disagree, reads in front of the edge, paths [X, X], follower edges F with 3 .. 8 reads [X, F] (two of them sharing 40 bases now and
then), and the mates of forward rows: slices of the other side's followers (31 bases: no 32-mer), of both shared stretches, random
bases, mates on the same side, mates on the other side.  Pairs: (A, B) per locus, sometimes (A, rc(A)), a pair across two loci, one pair
twice.

    generate(seed) -> namespace(seed, K, unitigs (BVComp order), codes, quals, lens, read_len, paths [(offset, [strand strings])],
                                pairs [(e1, e2) strand strings], marks) or None (the unitigs are no valid set: the seed is skipped)
    make_case(seed) -> generate(seed) on the graph as this library's writer numbers it: the namespace closeref's fixtures have
                       (K, unitigs, g, eb, inv, paths, pairs i32[n, 2] in the drawn order, reads, I), or None
"""
from __future__ import annotations

import zlib
from types import SimpleNamespace

import numpy as np

import handunitigs as hu

N_SEEDS = 160
SHARED = (0, 7, 8, 19, 20, 24, 25, 26, 30, 39, 40, 41, 60, 79, 80)       # MIN_STRETCH, W, 25 bits, WX, 2 WX and their neighbours
SHARED_DRAW = SHARED + (25, 25, 25, 26)
UNITS = (1, 2, 3, 5, 8, 13, 21, 34, 55)
QUALS = np.array([0, 1, 2, 10, 20, 30, 40, 41], np.uint8)
QUAL_P = np.array([0.012, 0.012, 0.012, 0.1, 0.2, 0.3, 0.2, 0.164])
_CODE = np.frombuffer(b"ACGT", np.uint8)
_made: dict = {}


def sample() -> list:
    """every fourth seed, K = 48 and 60 in turn: what the CPU tests run the restatement over"""
    return [4 * i + i % 2 for i in range(N_SEEDS // 4)]


def generate(seed: int):
    K = (48, 60)[seed % 2]
    rng = np.random.default_rng(zlib.crc32(f"closefuzz/{seed}".encode()))
    rand = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n)) if n > 0 else ""
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]
    def runit(u):
        """a repeat unit of u bases that is no homopolymer"""
        while True:
            x = rand(u)
            if u == 1 or len(set(x)) > 1:
                return x

    other = lambda b: "ACGT"[("ACGT".index(b) + 1 + int(rng.integers(0, 3))) % 4]
    big_side, many_idx, wide, long_reads = seed % 40 in (0, 25), seed % 40 in (8, 33), seed % 40 in (16, 5), seed == 13
    unitigs, reads, quals, paths, pairs, loci = [], [], [], [], [], []
    marks = dict(bursts=0, combs=0, duels=0, visited_twice=0, self_inverse=0, followers=0, second_followers=0)

    def add(seq, path, offset=0, q=None):
        """-> the read's id"""
        reads.append(seq)
        quals.append(rng.choice(QUALS, len(seq), p=QUAL_P) if q is None else np.full(len(seq), q, np.uint8))
        paths.append((int(offset), list(path)))
        return len(reads) - 1

    for li in range(int(rng.integers(2, 6))):
        RL = 256 if long_reads and li == 0 else pick((80, 100, 150))
        NX = [pick((K + 5, 120, 200, 380, 450)) for _ in range(2)]
        if wide and li == 0:
            NX[0] = 1100
        shared = pick(SHARED_DRAW) if rng.random() < 0.7 else int(rng.integers(0, 2 * (RL - K) + 1))
        mode = "random" if rng.random() < 0.45 else pick(("fill", "inside", "inside", "inside", "thin", "thin"))
        r = rng.random()
        special = "burst" if r < 0.1 else "comb" if r < 0.2 else None          # what side 1 sees of S (below)
        unit = pick(UNITS + (21, 34, 55) if mode == "inside" else UNITS)
        tail, f = None, 0
        if special == "burst":
            mode = "random"
            if rng.random() < 0.6:
                # a clean columns, 40 with exactly 20 mismatches, b with every third a mismatch: as a whole the overlap has 25 bits, no
                # stretch that stops 39 columns behind the start of a bad window has
                tail = (int(rng.integers(14, 21)), int(rng.integers(40, 51)))
                RL, shared = max(RL, 150), tail[0] + 40 + tail[1]
            else:
                RL, shared = max(RL, 100), max(shared, 45)
        elif special == "comb":                          # (2 mismatches in 26 columns have 20 bits, 4 in 40 have 27)
            mode, RL, shared = "random", max(RL, 100), max(shared, 40)
        elif mode == "inside" and unit >= 13:             # long units: the register a unit further on has 25 clean columns, or has not
            RL, shared = max(RL, 150), unit + pick((15, 18, 20, 24, 24, 25, 30, 20))
        elif mode == "thin":
            # a short repeat of R columns inside the shared ones, between flanks of f that end in a mismatch of every shifted register.
            # f = 10 = FLANK: the true register invalidates the shifted ones from f = 11 on.  f = 4, R about 30: the true register has
            # MIN_ADD more bits than the shifted ones, or not quite
            f = pick((4, 4, 4, 4, 5, 6, 8, 9, 10, 10, 10, 11))
            unit = pick((2, 2, 2, 3)) if f == 4 else pick((1, 2, 3, 3, 5))
            R = int(rng.integers(27, 35)) if f == 4 else int(rng.integers(42 + unit, 62)) if f >= 10 else int(rng.integers(20, 62))
            RL, shared = max(RL, 150 if R + f > 40 else 100), R + 2 * f
        half = RL - K
        shared = min(shared, 2 * half)
        reach = [half, half]
        gap = 2 * half - shared
        if mode == "inside":
            m = pick((unit, 2 * unit, 5)) if unit < 13 else 5
            if shared + m <= half:
                NX = [max(x, 200) for x in NX]
                gap = shared + 2 * m
                reach = [gap - m, gap - m]
            else:
                mode = "fill"
        NX = [max(NX[s], reach[1 - s] - gap) for s in range(2)]                # (no read of the other side goes on behind the edge)
        lo_sh, hi_sh = NX[0] + gap - reach[1], NX[0] + reach[0]                  # the columns of S that both stacks hold
        assert hi_sh - lo_sh == shared
        S = list(rand(NX[0] + gap + NX[1]))
        if mode in ("fill", "inside") and gap:
            n0, n1 = (int(rng.integers(1, 21)), int(rng.integers(1, 21))) if mode == "fill" and rng.random() < 0.5 else (0, 0)       # the repeat goes on into both edges
            S[NX[0] - n0:NX[0] + gap + n1] = (runit(unit) * ((n0 + gap + n1) // unit + 2))[:n0 + gap + n1]
        elif mode == "thin" and shared == R + 2 * f:
            r0, r1 = lo_sh + f, hi_sh - f
            S[r0:r1] = (runit(unit) * (R // unit + 2))[:R]
            while S[r0 - 1] == S[r0 - 1 + unit]:
                S[r0 - 1] = rand(1)
            while S[r1] == S[r1 - unit]:
                S[r1] = rand(1)
        S = "".join(S)
        # ---- side 1 sees S2: S, a burst of mismatches (a bad window), or a comb of them (matches of 8 and no longer)
        S2, plain = list(S), special is None
        if special == "burst" and tail and shared == tail[0] + 40 + tail[1]:
            w0 = lo_sh + tail[0]
            at = [w0, w0 + 39] + [int(x) for x in w0 + 1 + rng.choice(38, 18, replace=False)] + list(range(w0 + 42, hi_sh, 3))
        elif special == "burst" and shared >= 45:
            w0 = int(rng.integers(lo_sh, hi_sh - 40 + 1))
            at = [int(x) for x in w0 + rng.choice(40, int(rng.integers(20, 31)), replace=False)]
        elif special == "comb" and shared >= 40:
            at = list(range(lo_sh + int(rng.integers(0, 9)), hi_sh, 9))
        else:
            at, plain = [], True
        for x in at:
            S2[x] = other(S[x])
        if at:
            marks["bursts" if special == "burst" else "combs"] += 1
        S2 = "".join(S2)
        A, B = S[:NX[0]], S[len(S) - NX[1]:]
        X = [A, hu.rc(B)]
        T = [S, hu.rc(S2)]
        unitigs += [A, B]
        rate = 0.0 if not plain or mode == "thin" else pick((0.0, 0.0, 0.0, 0.01)) if mode == "inside" or shared in SHARED else pick((0.0, 0.0, 0.01, 0.05))
        # ---- the follower edges of either side
        foll = [[], []]
        for s in range(2):
            if rng.random() < 0.6:
                F = rand(pick((K + 1, 100, 220, 400)))
                foll[s].append((F, pick((3, 4, 5, 6, 8))))
                marks["followers"] += 1
                if rng.random() < 0.3:
                    a = int(rng.integers(0, max(1, len(F) - 40)))
                    F2 = rand(int(rng.integers(10, 120))) + F[a:a + 40] + rand(int(rng.integers(K, 150)))
                    foll[s].append((F2, pick((5, 6, 8))))
                    marks["second_followers"] += 1
            unitigs += [F for F, _ in foll[s]]

        def mate_for(s):
            """the mate of a forward row of side s: CloseGap2 looks for it among the followers of side 1 - s"""
            fs, r = foll[1 - s], rng.random()
            if fs and r < 0.35:
                F = pick(fs)[0]
                n = min(pick((31, 32, 60, 100)), len(F))
                a = int(rng.integers(0, len(F) - n + 1))
                return add(F[a:a + n], [], 0, 41)
            if len(fs) == 2 and r < 0.5:                                         # both shared stretches: two positions
                F, F2 = fs[0][0], fs[1][0]
                i = next(i for i in range(len(F2) - 39) if F2[i:i + 40] in F)
                return add(rand(int(rng.integers(0, 30))) + F2[i:i + 40] + rand(int(rng.integers(0, 30))), [], 0, 41)
            if r < 0.6:
                return add(rand(int(rng.integers(10, RL + 1))), [])
            return None

        def lay(s, t0, n, strand=None, path=None, err=True):
            """a read of n bases at t0 of T[s] -> its id"""
            r = list(T[s][max(t0, 0):t0 + n])
            if t0 < 0:
                r = list(rand(-t0)) + r
            if err and rate:
                for x in np.nonzero(rng.random(len(r)) < rate)[0]:
                    r[x] = other(r[x])
            r = "".join(r)
            fw = (rng.random() < (0.65, 0.35)[s]) if strand is None else strand
            if path is not None or fw:
                return add(r, [X[s]] if path is None else path, t0), True
            return add(hu.rc(r), [hu.rc(X[s])], NX[s] - (t0 + len(r))), False

        rows = [pick((0, 1, 3, 10, 30)) for _ in range(2)]
        if (big_side or many_idx) and li == 0:
            s = int(rng.integers(0, 2))
            rows[s] = 300 if big_side else 70
        if not plain or mode != "random" or NX[0] == 1100:
            rows = [max(r, 3) for r in rows]
        elif shared in SHARED:
            rows = [max(r, 1) for r in rows]
        if mode == "thin":
            rows = [max(r, 10) for r in rows]
        for s in range(2):
            for i in range(rows[s]):
                if len(reads) % 2:
                    add(rand(20), [])                                            # keeps mates apart
                n = RL if i == 0 or rng.random() < 0.75 else int(rng.integers(max(20, RL - 60), RL))
                top = max(0, min(NX[s] - K, NX[s] + reach[s] - n))               # K bases on X, and no further than the side reaches
                lo = -int(rng.integers(1, 21)) if rng.random() < 0.08 else 0
                t0 = top if i == 0 or rng.random() < 0.15 else int(rng.integers(lo, top + 1))
                if many_idx and li == 0 and rows[s] == 70:
                    rid, fw = lay(s, t0, n, strand=True)                         # 70 index entries on X itself
                elif rng.random() < 0.04:
                    rid, fw = lay(s, t0, n, path=[X[s], X[s]])
                    marks["visited_twice"] += 1
                else:
                    rid, fw = lay(s, t0, n)
                if fw and rid % 2 == 0:
                    r = rng.random()
                    if r < 0.08:
                        lay(s, int(rng.integers(0, top + 1)), RL, strand=True)    # a mate on the same side
                    elif r < 0.16 and rows[1 - s]:
                        lay(1 - s, int(rng.integers(0, max(1, NX[1 - s] - K))), RL, strand=False)         # a mate that is a reverse row of the other side
                    elif r < 0.2 and rows[1 - s]:
                        lay(1 - s, int(rng.integers(0, max(1, NX[1 - s] - K))), RL, strand=True)          # a forward row of the other side: not tried
                    else:
                        mate_for(s)
            for F, supports in foll[s]:
                for _ in range(supports):
                    if len(reads) % 2:
                        add(rand(20), [])
                    lay(s, max(0, min(NX[s] - K, NX[s] + reach[s] - RL)), RL, path=[X[s], F])
                    if rng.random() < 0.5:
                        mate_for(s)
        # ---- columns where every read has a quality of 0 .. 2 and the reads disagree in turn
        if rng.random() < 0.5:
            for _ in range(4):
                col = int(rng.integers(max(0, NX[0] - 60), len(S) - max(0, NX[1] - 60)))
                alt, k = other(S[col]), 0
                for rid in range(len(reads)):
                    off, p = paths[rid]
                    if len(p) != 1 or p[0] not in (A, hu.rc(A), B, hu.rc(B)):
                        continue
                    n = len(reads[rid])
                    on_a, rev = p[0] in (A, hu.rc(A)), p[0] in (hu.rc(A), hu.rc(B))
                    start = (NX[0] - off - n if rev else off) if on_a else len(S) - NX[1] + (NX[1] - off - n if rev else off)
                    j = col - start
                    if not 0 <= j < n:
                        continue
                    j = n - 1 - j if rev else j
                    b = S[col] if k % 2 == 0 else alt
                    r = list(reads[rid])
                    r[j] = hu.comp(b) if rev else b
                    reads[rid] = "".join(r)
                    quals[rid][j] = pick((0, 0, 1, 2))
                    k += 1
                marks["duels"] += k >= 2
        pairs.append((A, B))
        if rng.random() < 0.15:
            pairs.append((A, hu.rc(A)))
            marks["self_inverse"] += 1
        loci.append((A, B))
    a, b = (int(x) for x in rng.choice(len(loci), 2, replace=False))
    pairs.append((loci[a][0], loci[b][1]))                                       # two loci: no read joins them
    pairs.insert(int(rng.integers(0, len(pairs))), pairs[int(rng.integers(0, len(pairs)))])          # one pair twice
    if len(reads) % 2:
        add(rand(20), [])
    n, L = len(reads), max(len(r) for r in reads)
    codes, qs = np.zeros((n, L), np.uint8), np.zeros((n, L), np.uint8)
    for i, r in enumerate(reads):
        codes[i, :len(r)] = np.searchsorted(_CODE, np.frombuffer(r.encode(), np.uint8))
        qs[i, :len(r)] = quals[i]
    us = hu.bvcomp_sorted(sorted({min(u, hu.rc(u)) for u in unitigs}))
    try:
        hu.check_valid(us, K)
    except AssertionError:
        return None
    return SimpleNamespace(seed=seed, K=K, unitigs=us, codes=codes, quals=qs, lens=np.array([len(r) for r in reads], np.uint16), read_len=L, paths=paths, pairs=pairs,
                           marks=marks)


def make_case(seed: int):
    """Made once per process and left unchanged."""
    if seed in _made:
        return _made[seed]
    import tempfile
    from pathlib import Path

    import a48xref
    import closeref
    import extref
    import hopsref
    from supernova_amd import graphio
    t = generate(seed)
    c = None
    if t is not None:
        with tempfile.TemporaryDirectory() as td:
            graphio.write_hbv(Path(td) / "g.hbv", Path(td) / "g.inv", t.K, *graphio.unitigs_to_arrays(t.unitigs))
            a_hbv, a_inv = (Path(td) / "g.hbv").read_bytes(), (Path(td) / "g.inv").read_bytes()
        c = SimpleNamespace(name=f"fuzz_{seed}", seed=seed, a_hbv=a_hbv, a_inv=a_inv, unitigs=t.unitigs, g=a48xref.parse_hbv(a_hbv), marks=t.marks)
        c.eb = extref.edge_bases(c.g)
        edge_of = {"".join("ACGT"[x] for x in b): e for e, b in enumerate(c.eb)}
        c.paths = (np.array([o for o, _ in t.paths], np.int32), np.array([len(p) for _, p in t.paths], np.uint32),
                   np.array([edge_of[e] for _, p in t.paths for e in p], np.int32))
        c.bc, c.bad = np.zeros(len(t.paths), np.int32), np.zeros(len(t.paths) // 2, np.uint8)
        hopsref._finish(c)
        c.pairs = np.array([(edge_of[a], edge_of[b]) for a, b in t.pairs], np.int32).reshape(-1, 2)
        c.hops = hopsref.hops_bytes(c.pairs)
        c.edge_of = edge_of
        c.reads = SimpleNamespace(ids=np.arange(len(t.lens), dtype=np.int64), codes=t.codes, quals=t.quals, lens=t.lens)
        c.read_len = t.read_len
        c.I = closeref.Input(c.K, c.eb, c.inv, *c.paths, t.codes, t.quals, t.lens)
        c.want = {}
    _made[seed] = c
    return c


def expected(c, cg2: bool, max_width: int = 400):
    """closeref.close_gaps over the pairs of c, pair by pair with a fresh `why` each -> (closure_off, bases, pair_first, counters, bod_max):
    bod_max[p] = the most 32-mers the follower edges of one side of pair p have, what the device holds against bod_budget"""
    import closeref
    if (cg2, max_width) in c.want:
        return c.want[(cg2, max_width)]
    cnt = dict.fromkeys(closeref.COUNTERS, 0)
    cl, first, bod_max = [], [0], []
    for e1, e2 in c.pairs:
        why = {}
        cl += closeref.close_gap(c.I, int(e1), int(e2), cg2, max_width, cnt, why)
        first.append(len(cl))
        bod_max.append(int(why.get("bod_max", 0)))
    off = np.concatenate([[0], np.cumsum([len(x) for x in cl])]).astype(np.uint64)
    bases = np.concatenate(cl).astype(np.uint8) if cl else np.zeros(0, np.uint8)
    c.want[(cg2, max_width)] = (off, bases, np.array(first, np.uint64), cnt, np.array(bod_max, np.int64))
    return c.want[(cg2, max_width)]


def drawn(c):
    """-> (max_width, bod_budget) drawn for the case: a width of 100, 150 or 1 200, and a budget between the smallest and the largest
    bod_max of its pairs (expected(c, True))"""
    rng = np.random.default_rng(zlib.crc32(f"closefuzz/drawn/{c.seed}".encode()))
    width = (100, 150, 1200)[int(rng.integers(0, 3))]
    bod = expected(c, True)[4]
    return width, max(1, int(rng.integers(int(bod.min()), int(bod.max()) + 1)))
