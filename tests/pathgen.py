"""Random read pairs for the f1 / f4 parity checks (tests/tools/fuzz_paths.py, tests/test_gpu_paths.py) -- test infrastructure.

Genomes carry planted repeats, a tandem run, a palindrome, a long homopolymer and a short-period repeat; reads come in pairs (reads
2q and 2q+1 are the two ends of one fragment), with ragged lengths (some shorter than K), substitutions at quality 12, Q2 tails and
garbage qualities behind the read; barcodes include 0.  Duplicate groups of 2-6 pairs are planted: exact copies (artifacts), copies
with another quality sum, copies with the same sum and other bases, ragged mates, a changed mate head, mixed barcodes."""
from __future__ import annotations

import numpy as np


def rc(x: np.ndarray) -> np.ndarray:
    return (3 - x[::-1]).astype(np.uint8)


def genome(rng, G: int, plants: bool = True):
    """-> (codes u8[G], [(start, length)] of the long homopolymer, the short-period repeat and the tandem run)."""
    g = rng.integers(0, 4, G, dtype=np.uint8)
    spots = []
    if plants:
        rep = g[100:100 + int(rng.integers(60, 400))].copy()
        for _ in range(int(rng.integers(1, 5))):
            p = int(rng.integers(0, G - len(rep))); g[p:p + len(rep)] = rep
        unit = rng.integers(0, 4, int(rng.integers(1, 9)), dtype=np.uint8)
        p = int(rng.integers(0, G - 200)); g[p:p + 160] = np.resize(unit, 160); spots.append((p, 160))
        x = rng.integers(0, 4, 30, dtype=np.uint8); p = int(rng.integers(0, G - 60)); g[p:p + 60] = np.concatenate([x, rc(x)])
        n = int(rng.integers(160, 261)); p = int(rng.integers(0, G - n)); g[p:p + n] = int(rng.integers(0, 4)); spots.append((p, n))
        n = int(rng.integers(150, 251)); unit = rng.integers(0, 4, int(rng.integers(2, 5)), dtype=np.uint8)
        p = int(rng.integers(0, G - n)); g[p:p + n] = np.resize(unit, n); spots.append((p, n))
    return g, spots


def pairs(rng, g: np.ndarray, n_pairs: int, L: int, err: float, nbc: int, spots=(), spot_frac: float = 0.2, ragged: float = 0.15):
    """-> codes u8[n, L], quals u8[n, L], lens u16[n], bc i32[n] for n = 2 n_pairs reads.  Behind a read's length its codes are 0 and
    its qualities garbage; mates share their barcode."""
    G = len(g)
    n = 2 * n_pairs
    codes = np.zeros((n, L), dtype=np.uint8)
    quals = rng.integers(0, 42, (n, L), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint16)
    bc = np.zeros(n, dtype=np.int32)
    for q in range(n_pairs):
        F = min(G, int(rng.integers(L, 3 * L + 1)))
        if spots and rng.random() < spot_frac:
            p, ln = spots[int(rng.integers(0, len(spots)))]
            s = p + int(rng.integers(0, ln)) - int(rng.integers(0, F))
        else:
            s = int(rng.integers(0, G - F + 1))
        s = min(max(s, 0), G - F)
        frag = g[s:s + F]
        if rng.random() < 0.5:
            frag = rc(frag)
        for m, src in ((0, frag), (1, rc(frag))):
            i = 2 * q + m
            ln = L if rng.random() >= ragged else int(rng.integers(20, L + 1))
            ln = min(ln, F)
            r = src[:ln].copy()
            qq = rng.integers(15, 41, ln, dtype=np.uint8)
            e = rng.random(ln) < err
            r[e] = (r[e] + 1 + rng.integers(0, 3, int(e.sum()))) & 3
            qq[e] = 12
            if rng.random() < 0.1:
                qq[int(rng.integers(0, ln)):] = 2
            codes[i, :ln] = r; quals[i, :ln] = qq; lens[i] = ln
        bc[2 * q] = bc[2 * q + 1] = int(rng.integers(0, nbc + 1))
    return codes, quals, lens, bc


def plant_dups(rng, codes, quals, lens, bc, frac: float, nbc: int):
    """Copies of a share `frac` of the pairs, 1-5 per pair (groups of 2-6), appended; then the pairs are shuffled."""
    n_pairs = codes.shape[0] // 2
    L = codes.shape[1]
    extra = []
    for t in rng.choice(n_pairs, max(1, int(n_pairs * frac)), replace=False):
        for _ in range(int(rng.integers(1, 6))):
            a, q, ln = codes[2 * t:2 * t + 2].copy(), quals[2 * t:2 * t + 2].copy(), lens[2 * t:2 * t + 2].copy()
            b = int(bc[2 * t])
            m = int(rng.integers(0, 2))
            kind = int(rng.integers(0, 5))
            if kind == 1:                         # another quality sum
                j = int(rng.integers(0, ln[m])); q[m, j] = 30 if q[m, j] != 30 else 31
            elif kind == 2 and ln[m] > 6:         # the same sum, another base (behind the mate head)
                j = int(rng.integers(5, ln[m])); a[m, j] = (a[m, j] + 1 + int(rng.integers(0, 3))) & 3
            elif kind == 3 and ln[m] > 21:        # a ragged mate: shorter, garbage behind
                k = int(rng.integers(20, ln[m])); a[m, k:] = 0; q[m, k:] = rng.integers(0, 42, L - k, dtype=np.uint8); ln[m] = k
            elif kind == 4:                       # another mate head: another group
                j = int(rng.integers(0, 5)); a[m, j] = (a[m, j] + 1) & 3
            if rng.random() < 0.3:                # mixed barcodes within one group
                b = int(rng.integers(0, nbc + 1))
            extra.append((a, q, ln, b))
    if extra:
        codes = np.concatenate([codes] + [x[0] for x in extra])
        quals = np.concatenate([quals] + [x[1] for x in extra])
        lens = np.concatenate([lens] + [x[2] for x in extra])
        bc = np.concatenate([bc] + [np.array([x[3], x[3]], dtype=np.int32) for x in extra])
    perm = rng.permutation(codes.shape[0] // 2)
    idx = np.stack([2 * perm, 2 * perm + 1], axis=1).reshape(-1)
    return codes[idx].copy(), quals[idx].copy(), lens[idx].copy(), bc[idx].copy()


def to_device(codes, quals, lens, bc, pad_seed=None):
    """-> (rows i32, quals u8, lens i16, bc i32) on cuda:0.  pad_seed: quality rows padded to a multiple of four bytes (and four more
    every other time) with garbage behind the read length, the layout the readers produce."""
    import torch
    from supernova_amd import synth
    dev = torch.device("cuda", 0)
    L = codes.shape[1]
    q = quals
    if pad_seed is not None:
        prng = np.random.default_rng(pad_seed)
        q = prng.integers(0, 42, (quals.shape[0], (L + 3) // 4 * 4 + 4 * int(prng.integers(0, 2))), dtype=np.uint8)
        q[:, :L] = quals
    return (torch.from_numpy(synth.pack_rows(codes).view(np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(q)).to(dev),
            torch.from_numpy(lens.astype(np.uint16).view(np.int16)).to(dev), torch.from_numpy(bc.astype(np.int32)).to(dev))
