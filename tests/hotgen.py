"""A read set whose k-mer multiplicities reach the reference's 24-bit count field (kmers/ReadPather.h:127-131) -- test infrastructure.

Nothing is stored: the reads are generated (numpy, fixed seed) and checked against the SHA-256 digest the fixture carries
(tests/golden/hot_kmers.npz, made by the reference binary from these very arrays).  L = 250, reads 2q and 2q+1 are mates.

  over     88 184 reads, poly-G with poly-C mates, quality 30, barcodes cycling over 1..40: both orientations are one canonical k-mer
           seen 88 184 x 203 = 17 901 352 times at K=48 and 88 184 x 191 = 16 843 144 times at K=60 -- above SAT = 2^24-1 by more than
           2^16 both times, so a count that is not clamped is wrong by a wide margin
  under    poly-A / poly-T pairs whose lengths make the true K=48 count SAT-1 exactly: 82 646 full reads, one read of 123 bases
           (76 k-mers) and its mate, which is shorter than K.  A clamp that is too low, a 23-bit field or an off-by-one at the boundary
           changes this count; at K=60 it is 15 785 450, unsaturated
  solo     2 000 (GA)n reads (mates (TC)n) in ONE barcode: dropped by the two-barcode rule whatever their count, kept without barcodes;
           their unitig is the two-k-mer circle
  back     200 pairs over a random 3 kb genome, a few substitutions at quality 12, barcodes 0..40
The families lie one after the other in that order (a slab cut or a rank boundary at a fixed share of the reads falls inside one)."""
from __future__ import annotations

import hashlib

import numpy as np

L = 250
SAT = (1 << 24) - 1
N_OVER = 88_184
N_UNDER_FULL = 82_646
UNDER_SHORT = 123            # 123 - 48 + 1 = 76 k-mers at K=48
UNDER_MATE = 30              # shorter than K: no k-mer
N_SOLO = 2_000
SOLO_BC = 41
N_BACK_PAIRS = 200
SEED = 0x407C0DE


def true_count(family: str, K: int) -> int:
    """Instances of the family's homopolymer k-mer in the reads (both strands), unsaturated."""
    if family == "over":
        return N_OVER * (L - K + 1)
    return N_UNDER_FULL * (L - K + 1) + (UNDER_SHORT - K + 1)


assert true_count("over", 48) == 17_901_352 and true_count("over", 60) == 16_843_144
assert min(true_count("over", 48), true_count("over", 60)) - SAT > 1 << 16
assert true_count("under", 48) == SAT - 1 and true_count("under", 60) == 15_785_450 < SAT


def spans() -> dict:
    """family -> (first read, one past its last read)"""
    out, at = {}, 0
    for name, n in (("over", N_OVER), ("under", N_UNDER_FULL + 2), ("solo", N_SOLO), ("back", 2 * N_BACK_PAIRS)):
        out[name] = (at, at + n)
        at += n
    return out


def digest(codes, quals, lens, bc) -> bytes:
    h = hashlib.sha256()
    for a in (codes, quals, lens, bc):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest().encode()


def reads(expect_digest: bytes | None = None):
    """-> (codes u8[n, L], quals u8[n, L], lens u16[n], bc i32[n]); expect_digest: what the fixture was made from."""
    import pathgen
    sp = spans()
    n = sp["back"][1]
    codes = np.zeros((n, L), np.uint8)
    quals = np.full((n, L), 30, np.uint8)
    lens = np.full(n, L, np.uint16)
    bc = np.zeros(n, np.int32)
    a, b = sp["over"]
    codes[a:b:2] = 2
    codes[a + 1:b:2] = 1
    bc[a:b] = np.repeat(1 + np.arange((b - a) // 2, dtype=np.int32) % 40, 2)
    a, b = sp["under"]
    codes[a:b:2] = 0
    codes[a + 1:b:2] = 3
    bc[a:b] = np.repeat(1 + np.arange((b - a) // 2, dtype=np.int32) % 40, 2)
    lens[b - 2], lens[b - 1] = UNDER_SHORT, UNDER_MATE
    codes[b - 2, UNDER_SHORT:] = 0
    codes[b - 1, UNDER_MATE:] = 0
    a, b = sp["solo"]
    ga = np.resize(np.array([2, 0], np.uint8), L)
    codes[a:b:2] = ga
    codes[a + 1:b:2] = pathgen.rc(ga)
    bc[a:b] = SOLO_BC
    a, b = sp["back"]
    rng = np.random.default_rng(SEED)
    g, _ = pathgen.genome(rng, 3000, plants=False)
    codes[a:b], quals[a:b], lens[a:b], bc[a:b] = pathgen.pairs(rng, g, N_BACK_PAIRS, L, 0.002, 40, ragged=0.1)
    quals[a:b][np.arange(L)[None, :] >= lens[a:b, None]] = 0          # (pathgen leaves garbage behind a read; the fixture's reads are plain)
    if expect_digest is not None:
        assert digest(codes, quals, lens, bc) == bytes(expect_digest), "the generator no longer makes the reads the fixture was made from"
    return codes, quals, lens, bc


def homopolymer_key(family: str, K: int) -> np.ndarray:
    """The canonical homopolymer k-mer of a family as a table key: u32[4], 16 bases per word from the top, zero-filled."""
    # the canonical form is the smaller of the two strands: poly-C (over), poly-A (under)
    base = {"over": 1, "under": 0}[family]
    out = np.zeros(4, np.uint32)
    for i in range(K):
        out[i // 16] |= np.uint32(base << (2 * (15 - i % 16)))
    return out
