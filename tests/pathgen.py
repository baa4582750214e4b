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


def plant_big_groups(rng, codes, quals, lens, bc, sizes):
    """Duplicate groups of exactly sizes[i] pairs each (far beyond plant_dups' 2-6), every group built from one seed pair: an existing
    full-length pair without a low quality, so that every copy keeps the seed's (first edge, offset, mate head).  The pairs are then
    shuffled, so the runs of a group interleave by read id.  -> (codes, quals, lens, bc, groups), groups[i] = the final pair indices
    of group i, ascending.

    Copy c of a group is, by c mod 10: 0-4 one of five variants tied in their quality sum -- the seed itself, two neighbouring
    qualities swapped in read 0, in read 1, in both, at another place of read 0 (tied but not identical: several runs per read, three
    or more exact copies each from size 25 on); 5 a variant again, in another barcode where the group mixes barcodes; 6 a lower
    quality sum; 7 the same sum with another base behind the mate head (each at a place of its own: never a solid k-mer); 8 a ragged
    mate (shorter, garbage behind); 9 the seed again.  Kinds 6-8 also swap two qualities of the other read at a place of their own.  By the group's index g mod 7:
      0  the member with the smallest read id has barcode 0 (the barcode walk starts at 0 and adopts the next)
      1  the seed is replaced by a fragment that is its own reverse complement (both mates the same read, same qualities: both mates
         of every pair sit in ONE group of 2 sizes[i] records, and in one run where they are exact copies); two barcodes
      2  three barcodes
      3  the member with the largest read id has the one larger quality sum: the best copy is the last member, after ties
      4  the member with the smallest read id has the one larger sum: the tie never fires, no artifact in the whole group
      5  two identical copies with the larger sum (a tie among the best); copies of kind 5 in another barcode
      6  0 and 2 and 3 together"""
    L = codes.shape[1]
    n_pairs = codes.shape[0] // 2
    full = [t for t in range(n_pairs) if lens[2 * t] == L and lens[2 * t + 1] == L and quals[2 * t:2 * t + 2].min() >= 15 and bc[2 * t] > 0]
    seeds = rng.choice(full, len(sizes), replace=False)
    codes, quals, lens, bc = codes.copy(), quals.copy(), lens.copy(), bc.copy()
    extra, members = [], []
    at = n_pairs

    def swap(q, m, j):
        while q[m, j] == q[m, j + 1]:
            j += 1
        q[m, j], q[m, j + 1] = q[m, j + 1], q[m, j]

    for g, (t, size) in enumerate(zip(seeds, sizes)):
        kind_g = g % 7
        if kind_g == 1:
            x = rng.integers(0, 4, L // 2, dtype=np.uint8)
            codes[2 * t] = codes[2 * t + 1] = np.concatenate([x, rc(x)])
            quals[2 * t + 1] = quals[2 * t]
        a0, q0, b0 = codes[2 * t:2 * t + 2], quals[2 * t:2 * t + 2], int(bc[2 * t])
        variants = []
        for v in range(5):
            q = q0.copy()
            if v in (1, 3): swap(q, 0, 10)
            if v in (2, 3): swap(q, 1, 20)
            if v == 4: swap(q, 0, 80)
            variants.append(q)
        members.append([int(t)])
        for c in range(1, size):
            a, q, ln, b = a0.copy(), q0.copy(), np.array([L, L], dtype=lens.dtype), b0
            k, m = c % 10, (c // 10) & 1
            if k <= 5:
                q = variants[(k + c // 10) % 5].copy()
                if k == 5 and kind_g == 5: b = b0 + 1
            elif k == 6:
                q[m, 30 + c % 100] -= 1
            elif k == 7:
                a[m, 60 + (c // 10) % (L - 60)] ^= 1 + (c // 20) % 3
            elif k == 8:
                cut = 60 + (7 * c) % (L - 60); a[m, cut:] = 0; q[m, cut:] = rng.integers(0, 42, L - cut, dtype=np.uint8); ln[m] = cut
            if k in (6, 7, 8):                    # ... and a quality layout of its own in the other read: an artifact in neither of its two groups
                swap(q, 1 - m, 5 + (5 * (c // 10) + k) % (L - 8))
            if kind_g in (2, 6): b = b0 + c % 3
            if kind_g == 1: b = b0 + c % 2
            if kind_g == 5 and c in (size // 3, size // 2):
                q = q0.copy(); q[0, 40] += 2
            extra.append((a, q, ln, b))
            members[-1].append(at); at += 1
    codes = np.concatenate([codes] + [x[0] for x in extra])
    quals = np.concatenate([quals] + [x[1] for x in extra])
    lens = np.concatenate([lens] + [x[2] for x in extra])
    bc = np.concatenate([bc] + [np.array([x[3], x[3]], dtype=np.int32) for x in extra])
    perm = rng.permutation(codes.shape[0] // 2)
    idx = np.stack([2 * perm, 2 * perm + 1], axis=1).reshape(-1)
    codes, quals, lens, bc = codes[idx].copy(), quals[idx].copy(), lens[idx].copy(), bc[idx].copy()
    inv = np.argsort(perm)
    groups = [np.sort(inv[np.asarray(m)]) for m in members]

    def better(p, seed):          # pair p becomes the seed pair with a larger quality sum
        for a in (codes, quals, lens):
            a[2 * p:2 * p + 2] = a[2 * seed:2 * seed + 2]
        quals[2 * p + (p & 1), 40] += 2

    for g, mem in enumerate(groups):
        kind_g, seed = g % 7, int(inv[members[g][0]])
        if kind_g in (3, 6):
            better(mem[-1], seed)
        if kind_g == 4:
            better(mem[0], seed)
        if kind_g in (0, 6):
            bc[2 * mem[0]:2 * mem[0] + 2] = 0
    return codes, quals, lens, bc, groups


def big_group_reads(seed=0xB16D0B5, sizes=(7, 63, 64, 65, 255, 256, 257), n_pairs=400, L=150, G=3000):
    """The dup_groups read set (tests/golden/dup_groups.npz): about 400 ordinary pairs over a plain 3 kb genome with the planted groups
    mixed in.  -> (codes, quals, lens, bc, groups)"""
    rng = np.random.default_rng(seed)
    g, _ = genome(rng, G, plants=False)
    codes, quals, lens, bc = pairs(rng, g, n_pairs, L, 0.001, 12)
    return plant_big_groups(rng, codes, quals, lens, bc, sizes)


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
