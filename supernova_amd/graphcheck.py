"""Host restatement of the graph verifier's two digests (include/snk.h, "the graph verifier"), in numpy.

A .bv file from anywhere -- the reference's own, another run's -- can be compared with a device run (snk_dev_check_graph,
Engine.check_graph / Result.check) without downloading the device's unitigs: equal digests, equal unitig multiset.  This is not a
CPU path of the product: it computes nothing but the two sums.

    table_digest  = sum over rows     mix(key_lo ^ mix(key_hi ^ mix((min(count, 2^24-1) << 8) | ctx)))
    unitig_digest = sum over unitigs  mix(h_u ^ mix(len_u ^ (group_u << 40))),  h_u = sum over i mix((i << 2) | base_{u,i})

mod 2^64, mix = the splitmix64 finaliser.
"""
from __future__ import annotations

import numpy as np

from . import graphio

_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_SAT = (1 << 24) - 1


def mix(z: np.ndarray) -> np.ndarray:
    """splitmix64 finaliser over a u64 array (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def _sum(x: np.ndarray) -> int:
    return int(np.sum(x, dtype=np.uint64)) if x.size else 0


def key_lohi(keys: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(lo, hi) u64 of keys given as [n, 4] u32 words MSB-first (words 0..2 only at K=48 is fine: [n, 3]) or [n, 2] u64 {lo, hi}."""
    keys = np.asarray(keys)
    if keys.dtype == np.uint64 and keys.ndim == 2 and keys.shape[1] == 2:
        return keys[:, 0], keys[:, 1]
    w = keys.astype(np.uint64)
    hi = (w[:, 0] << np.uint64(32)) | w[:, 1]
    lo = (w[:, 2] << np.uint64(32)) | (w[:, 3] if w.shape[1] > 3 else np.uint64(0))
    return lo, hi


def digest_table(keys: np.ndarray, counts: np.ndarray, ctx: np.ndarray) -> int:
    lo, hi = key_lohi(keys)
    c = np.minimum(np.asarray(counts, dtype=np.uint64), np.uint64(_SAT))
    inner = mix((c << np.uint64(8)) | np.asarray(ctx, dtype=np.uint64))
    return _sum(mix(lo ^ mix(hi ^ inner)))


def digest_unitigs(off: np.ndarray, bases: np.ndarray, groups: np.ndarray | None = None) -> int:
    """off u64[U + 1], bases u8 codes (A=0 C=1 G=2 T=3), groups u32[U] or None."""
    off = np.asarray(off, dtype=np.int64)
    U = len(off) - 1
    if U <= 0:
        return 0
    lens = np.diff(off)
    pos = np.arange(int(off[-1] - off[0]), dtype=np.int64) - np.repeat(off[:-1] - off[0], lens)
    b = np.asarray(bases[int(off[0]):int(off[-1])], dtype=np.uint64)
    per = mix((pos.astype(np.uint64) << np.uint64(2)) | b)
    h = np.add.reduceat(per, (off[:-1] - off[0]).clip(max=max(len(per) - 1, 0))) if len(per) else np.zeros(U, np.uint64)
    h = np.where(lens > 0, h, np.uint64(0)).astype(np.uint64)
    g = np.zeros(U, np.uint64) if groups is None else np.asarray(groups, dtype=np.uint64)
    return _sum(mix(h ^ mix(lens.astype(np.uint64) ^ (g << np.uint64(40)))))


def digest_strings(unitigs: list[str]) -> int:
    """unitig_digest of unitigs given as ACGT strings (the golden cases' form)."""
    lut = np.zeros(256, np.uint8)
    lut[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)
    joined = "".join(unitigs).encode()
    bases = lut[np.frombuffer(joined, np.uint8)] if joined else np.zeros(0, np.uint8)
    off = np.concatenate([[0], np.cumsum([len(u) for u in unitigs])]).astype(np.uint64)
    return digest_unitigs(off, bases)


def digest_bv(path: str) -> int:
    """unitig_digest of a .bv hand-off file (lib/tada/src/debruijn.rs:895-929)."""
    off, bases = graphio.read_bv(path)
    return digest_unitigs(off, bases)
