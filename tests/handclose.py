"""Hand-made gaps for CloseGap / CloseGap2 (snk_dev_close_gaps; 10X/Closomatic.cc:356-657) -- test infrastructure
(tests/golden/make_closures_golden.py, tests/test_closures_host.py, tests/test_gpu_closures.py).  numpy and Python only.

One graph per K (48 and 60) of isolated edges.  A locus is a sequence S = A + gap + B, edge A its first NA bases (200 unless said), edge B
its last 200, and 100-base reads are laid at stated places: a read with the path [A] has its start in S as the offset, a read with the path
[B] its start minus B's (negative when it starts in the gap).  half = 100 - K: the A reads reach M1 = NA + half, the B reads begin at
NA + gap - half, so the two stacks share 2 half - gap columns.  The pair of an item is (A, B) unless said: side 0 is the rows on A, side 1
the rows on inv[B] = rc(B), reversed back.  Every item states the closures it must give -- with CloseGap2 (`closures`), with CloseGap
(`closures_cg1`, the same unless said) and at max_width 1 200 (`closures_wide`, the same unless said) -- and the filters of GetOffsets1 that
must remove an offset of its pair (`fires`).  The maker asserts the closures against the reference's own functions before it saves the
fixture, the tests assert them against the restatement and the device, and `fires` against the restatement.

  bridge                      reads from both sides cover every column: ONE closure, S itself
  one_side_has_no_reads       only A has reads: none
  quality_columns             the bridge with three places of stack 1 prepared: at 20 two reads disagree with qualities 0 and 1 (0.1 against 0.2:
                              the second read's base); at 30 two reads disagree with equal qualities (a tie: the HIGHER base code); 100 .. 104 no
                              read covers (an empty column: T in the closure, where the seed consensus has A)
  bits_24_columns / _25_      the stacks share 24 columns (24.08 bits: under the threshold of 25, none) / 25 columns (25.09 bits: S)
  two_offsets                 the gap is a tandem repeat of three long units: the true register and the one a unit off both survive -- TWO
                              closures, S without a unit and S, in offset order
  three_offsets               a shorter unit: three registers survive -- none (more than two offsets)
  invalidation                a short repeat well inside the shared columns: the registers a unit off reach 25 bits, the true one invalidates them: S
  big_near_small              a 3-base unit x 10 between flanks of which the stacks share 6 columns each: the true register has 42 columns (42
                              bits), the registers a unit or two off keep the repeat (under 40 bits) with their mismatches inside the flank of 10 that
                              no offset validates: only big near small removes them -- ONE closure, S
  wide_stack                  NA = 1 100 with reads every 50 bases: rows wholly in front of the kept 400 columns; the closure begins at column
                              M1 - 400 of A.  At max_width 1 200 the consensus has 1000 columns or more: none
  self_inverse                the pair (A, rc(A)), e1 == inv[e2]: both stacks are A's, both reversed -- ONE closure, rc(S[:M1])
  visited_twice               a read with the path [A, A]: the index lists it twice and each listing gives two rows; the second row lies Kmers(A)
                              further left and is all that covers columns 0 .. 9 -- the closure has that read's bases there
  negative_pos_and_rc_rows    the A reads are given on rc(A) (reverse-complement rows, the last with a negative pos), one forward read begins 20 bases
                              in front of A (cells with p < 0 are dropped), the B reads are given on rc(B) (forward rows of side 1): S
CloseGap2 (the B reads lie twice each, 60 per column and read; X, a read on rc(B), is the mate of Y; F is an edge of 220 bases that 5 reads
with the path [A, F] make a follower of A at distance Kmers(A); Y = F[100:200] with quality 63 would lie behind column M1):
  partner_placed_once         Y is placed: where one B read (60) covers, the closure has F's bases; CloseGap gives S
  follower_with_4_supports    4 reads with [A, F]: no follower, Y is not placed: S
  partner_found_twice         two followers F1 and F2 share 40 bases at different places, Y holds them: two positions, not placed: S
  partner_on_the_other_side   Y has the path [A] itself (quality 45, at the column where it would be placed): it is skipped; placed again it
                              would outweigh one B read
  long_follower (K = 48)      F has BOD_BUDGET + 1 000 bases, more 32-mers than the default bod_budget: the pair goes to the host routine; Y is
                              placed 1 000 columns on, the kept window holds nothing else of stack 1: none; CloseGap gives S

    case(K) -> namespace(K, unitigs (BVComp order), codes, quals, lens, paths [(offset, [strand strings])], pairs [(e1, e2)], items)
    assert_items(c, edge_of, pairs, closure_off, bases, pair_first, who, which)      which: "closures", "closures_cg1" or "closures_wide"
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import handunitigs as hu

L, NB = 100, 200
BOD_BUDGET = 1 << 18          # the library's default bod_budget (include/snk.h)
_made: dict = {}
rc = hu.rc


def case(K: int):
    if K in _made:
        return _made[K]
    half = L - K
    unitigs, reads, quals, paths, pairs, items = [], [], [], [], [], []

    def add(seq, path, offset=0, q=30):
        assert len(seq) == L
        reads.append(seq)
        quals.append(list(q) if isinstance(q, (list, tuple)) else [q] * L)
        paths.append((offset, list(path)))

    def even():
        if len(reads) % 2:
            add("A" * L, [])                          # a read without a path: it only keeps mates apart

    class Locus:
        def __init__(self, name, gap=40, NA=200, mid=None, pair=True):
            self.g = hu._Gen(f"close/{name}", K)
            mid = self.g.rand(gap) if mid is None else mid
            self.S = self.g.rand(NA) + mid + self.g.rand(NB)
            self.NA, self.b0 = NA, NA + len(mid)
            self.A, self.B = self.S[:NA], self.S[self.b0:]
            self.M1, self.L2 = NA + half, self.b0 - half
            unitigs.extend([self.A, self.B])
            if pair:
                pairs.append((self.A, self.B))
            even()

        def left(self, s0, q=30, change=None, path=None):
            r, ql = list(self.S[s0:s0 + L]), [q] * L
            for at, (b, qq) in (change or {}).items():
                r[at - s0], ql[at - s0] = b, qq
            add("".join(r), [self.A] if path is None else path, s0, ql)

        def right(self, s0, q=30):
            add(self.S[s0:s0 + L], [self.B], s0 - self.b0, q)

        def lefts(self):
            return (0, 52, 104, self.NA - K)

        def rights(self):
            return (self.L2, self.b0 + 20, self.b0 + 60, self.b0 + NB - L)

        def bridge(self):
            for s0 in self.lefts():
                self.left(s0)
            for s0 in self.rights():
                self.right(s0)

    def item(name, lc, closures, pair=None, fires=(), **other):
        items.append(SimpleNamespace(name=name, pair=pair or (lc.A, lc.B), closures=closures, closures_cg1=other.get("cg1", closures), closures_wide=other.get("wide", closures),
                                     fires=tuple(fires)))

    other_base = lambda b, k: "ACGT"[("ACGT".index(b) + k) % 4]

    lc = Locus("bridge")
    lc.bridge()
    item("bridge", lc, [lc.S])

    lc = Locus("one_side_has_no_reads")
    for s0 in lc.lefts() + lc.lefts():
        lc.left(s0)
    item("one_side_has_no_reads", lc, [])

    lc = Locus("quality_columns")
    S = lc.S
    b20, b30 = other_base(S[20], 1), other_base(S[30], 2)
    lc.left(0, change={20: (S[20], 0), 30: (S[30], 20)})              # first in the index: the row in front
    lc.left(0, change={20: (b20, 1), 30: (b30, 20)})
    for s0 in (105, lc.NA - K):                                      # 100 .. 104: no read
        lc.left(s0)
    for s0 in lc.rights():
        lc.right(s0)
    want = list(S)
    want[20], want[30] = b20, max(S[30], b30, key="ACGT".index)
    want[100:105] = "TTTTT"
    item("quality_columns", lc, ["".join(want)])

    for shared in (24, 25):
        lc = Locus(f"bits_{shared}", gap=2 * half - shared)
        lc.bridge()
        item(f"bits_{shared}_columns", lc, [lc.S] if shared == 25 else [], fires=("below_bits",) if shared == 24 else ())

    # the gap is a tandem repeat, u x copies (found by trying: the maker asserts what they give): the registers that agree everywhere survive
    for name, (u, copies) in (("two_offsets", (20, 3) if K == 48 else (16, 3)), ("three_offsets", (16, 3) if K == 48 else (10, 4))):
        g = hu._Gen(f"close/{name}/unit", K)
        lc = Locus(name, mid=g.rand(u) * copies)
        lc.bridge()
        for s0 in lc.lefts():                                         # the A reads twice: where the two stacks disagree at the register a unit off, stack 1 decides
            lc.left(s0)
        S = lc.S
        item(name, lc, [S[:lc.M1] + S[lc.M1 + u:], S] if name == "two_offsets" else [])

    # a short repeat well inside the shared columns: the registers a unit off have 25 bits or more, and their mismatches at the repeat's ends
    # lie 10 columns or more inside the true register's run of agreement, which invalidates them
    pad, u, copies = (0, 5, 7) if K == 48 else (2, 3, 9)
    g = hu._Gen("close/invalidation/unit", K)
    lc = Locus("invalidation", mid=g.rand(pad) + g.rand(u) * copies + g.rand(pad))
    lc.bridge()
    item("invalidation", lc, [lc.S], fires=("invalidated",))

    g = hu._Gen("close/big_near_small/unit", K)
    pad = half - 36
    lc = Locus("big_near_small", mid=g.rand(pad) + g.rand(3) * 10 + g.rand(pad))
    lc.bridge()
    lc.left(lc.NA - K), lc.right(lc.L2)                              # the outermost reads twice: the six shared flank columns are sure
    item("big_near_small", lc, [lc.S], fires=("big_near_small",))

    lc = Locus("wide_stack", NA=1100)
    for s0 in tuple(range(0, lc.NA - K, 50)) + (lc.NA - K,):
        lc.left(s0)
    for s0 in lc.rights():
        lc.right(s0)
    item("wide_stack", lc, [lc.S[lc.M1 - 400:]], wide=[])

    lc = Locus("self_inverse", pair=False)
    for s0 in lc.lefts():
        lc.left(s0)
    pairs.append((lc.A, rc(lc.A)))
    item("self_inverse", lc, [rc(lc.S[:lc.M1])], pair=(lc.A, rc(lc.A)))

    lc = Locus("visited_twice")
    for s0 in (10, 10, 10, 52, 52, 52, 104, 104, 104, lc.NA - K):          # (the index lists the read twice and each listing gives both rows: 60 per column)
        lc.left(s0)
    lc.left(lc.NA - K, path=[lc.A, lc.A])                            # second row: pos = offset - Kmers(A) = -1
    for s0 in lc.rights():
        lc.right(s0)
    s0 = lc.NA - K
    item("visited_twice", lc, [lc.S[s0 + 1:s0 + 11] + lc.S[10:]])

    lc = Locus("negative_pos_and_rc_rows")
    for s0 in lc.lefts():
        add(rc(lc.S[s0:s0 + L]), [rc(lc.A)], lc.NA - (s0 + L))
    add(lc.g.rand(20) + lc.S[:L - 20], [lc.A], -20)
    for s0 in lc.rights():
        add(rc(lc.S[s0:s0 + L]), [rc(lc.B)], NB - (s0 - lc.b0 + L))
    item("negative_pos_and_rc_rows", lc, [lc.S])

    # ---- CloseGap2
    def cg2_locus(name, followers, supports=5):
        """the bridge with the B reads twice and `supports` reads [A, F] per follower edge F; X on rc(B) in front of an even place, so that
        the next read is its mate"""
        lc = Locus(name)
        for s0 in lc.lefts()[:-1]:
            lc.left(s0)
        for F in followers:
            unitigs.append(F)
            for _ in range(supports):
                lc.left(lc.NA - K, path=[lc.A, F])
        for s0 in lc.rights() + lc.rights():
            lc.right(s0)
        even()
        s0 = lc.b0 + 60
        add(rc(lc.S[s0:s0 + L]), [rc(lc.B)], NB - (s0 - lc.b0 + L))            # X
        return lc

    def with_y(lc, yseq, weight):
        """S with Y's bases where Y, a forward row of stack 1 at column pos = Kmers(A) + 100, outweighs the B reads (60 per read) that cover the column"""
        pos = lc.NA - K + 1 + 100
        assert pos > lc.M1
        want = list(lc.S)
        for c in range(pos, pos + L):
            n = sum(1 for r in lc.rights() if r <= c < r + L)
            if weight > 60 * n:
                want[c] = yseq[c - pos]
        return "".join(want)

    g = hu._Gen("close/cg2", K)
    F = g.rand(220)
    lc = cg2_locus("partner_placed_once", [F])
    add(F[100:200], [], 0, 63)                                       # Y
    placed = with_y(lc, F[100:200], 63)
    assert placed != lc.S
    item("partner_placed_once", lc, [placed], cg1=[lc.S])

    F = g.rand(220)
    lc = cg2_locus("follower_with_4_supports", [F], supports=4)
    add(F[100:200], [], 0, 63)
    item("follower_with_4_supports", lc, [lc.S])

    sh = g.rand(40)
    F1, F2 = g.rand(50) + sh + g.rand(130), g.rand(120) + sh + g.rand(60)
    lc = cg2_locus("partner_found_twice", [F1, F2])
    add(g.rand(30) + sh + g.rand(30), [], 0, 63)
    item("partner_found_twice", lc, [lc.S])

    F = g.rand(220)
    lc = cg2_locus("partner_on_the_other_side", [F])
    add(F[100:200], [lc.A], lc.NA - K + 1 + 100, 45)                   # Y is a forward row of side 0 already
    assert with_y(lc, F[100:200], 45) == lc.S and with_y(lc, F[100:200], 90) != lc.S
    item("partner_on_the_other_side", lc, [lc.S])

    if K == 48:
        F = g.rand(BOD_BUDGET + 1000)
        lc = cg2_locus("long_follower", [F])
        add(F[1000:1100], [], 0, 63)
        item("long_follower", lc, [], cg1=[lc.S])

    even()
    codes = np.stack([np.searchsorted(np.frombuffer(b"ACGT", np.uint8), np.frombuffer(r.encode(), np.uint8)) for r in reads]).astype(np.uint8)
    us = hu.bvcomp_sorted(sorted({min(x, rc(x)) for x in unitigs}))
    hu.check_valid([x for x in us if len(x) < 10000], K)             # (the long follower is random: 48-mers of 260 000 random bases do not repeat)
    _made[K] = SimpleNamespace(K=K, unitigs=us, codes=codes, quals=np.array(quals, np.uint8), lens=np.full(len(reads), L, np.uint16), paths=paths, pairs=pairs, items=items)
    return _made[K]


def assert_items(c, edge_of, pairs, closure_off, bases, pair_first, who: str, which: str = "closures"):
    """every item's stated closures, by name, in a result over `pairs` (i32[n, 2], the order of pair_first)"""
    where = {(int(a), int(b)): i for i, (a, b) in enumerate(pairs)}
    for it in c.items:
        p = where[(edge_of[it.pair[0]], edge_of[it.pair[1]])]
        want = getattr(it, which)
        got = ["".join("ACGT"[x] for x in bases[int(closure_off[q]):int(closure_off[q + 1])]) for q in range(int(pair_first[p]), int(pair_first[p + 1]))]
        assert got == want, f"{who}, K = {c.K}, {which} of item {it.name}: {len(got)} closures {[len(x) for x in got]}, stated {[len(x) for x in want]}" + \
            (f"; first difference at column {next((i for i, (x, y) in enumerate(zip(got[0], want[0])) if x != y), None)}" if got and want else "")
