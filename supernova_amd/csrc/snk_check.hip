// snk_check.hip -- snk_dev_check_graph: the reassembly invariants of a k-mer table and its unitigs, checked on the device.
//
// The rules are the reference's own (lib/tada/src/sim_tests.rs:297-404; EdgeBuilder, lib/assembly/src/paths/long/
// BuildReadQGraph48.cc:327-541), restated from scratch: this file shares the key layout and the
// context / error / arena plumbing with the rest of libsnk and nothing else.  It has its own canonical form, its own
// open-addressing index over entry ids (load <= 0.5, its own hash) and its own trim, so a bug of the producer cannot
// vouch for itself.
//
// Sizes: entry ids live in 32-bit slots (up to 2^32 - 2 entries); positions, offsets and counters are 64-bit, and every
// kernel is a grid-stride loop over a grid far below 2^31 work items.
//
// Launches, in order:
//   table   per row: digest, count >= min_freq, ascending keys, key padding, insertion into the index (duplicates found there)
//   ctx     per row: every context bit names a neighbour in the table that carries the reciprocal bit
//   unitig  a wave per unitig: digest, base codes, offsets, order; lane 0 classifies (palindrome / circle / linear) and checks
//           the ends and the canonical form
//   pos     per segment of 32 bases: every k-mer of every unitig is looked up (visit marks, 2 bits per entry) and every step
//           inside a unitig obeys the walk rule
//   reads   per read (reads level): the trim, the k-mer instances, the recount and the shadow context
//   final   per entry: visit marks, recount and shadow against the stored count and context
#include <algorithm>

#include "snk_call.h"

namespace {

constexpr uint32_t CK_EMPTY = 0xFFFFFFFFu;
constexpr uint64_t CK_NONE = ~0ull;
constexpr int CB = 256;          // threads per block
constexpr uint64_t CK_SEG = 32;  // base positions per work item of the pos launch
constexpr uint32_t CK_SAT = (1u << 24) - 1;   // KDef::setCount saturates here (kmers/ReadPather.h:127-131)

enum : int {
    C_DUP = 0, C_NOT_SORTED, C_BELOW_MIN, C_BAD_UNITIG, C_MISSING, C_REPEATED, C_UNCOVERED, C_DANGLING, C_NOT_RECIP,
    C_INTERIOR, C_END_EXT, C_NOT_CANON, C_NOT_ORDERED, C_GROUP, C_COUNT_MM, C_CTX_MM, C_GOODLEN_MM, C_INST_MM, C_KEY_PAD
};

// device-side tallies: counters, first offenders, digests and what was found
struct ck_acc {
    unsigned long long count[SNK_CHECK_N_COUNTERS];
    unsigned long long first[SNK_CHECK_N_COUNTERS];
    unsigned long long table_digest, unitig_digest;
    unsigned long long n_circles, n_palindromes, n_instances;
};

// splitmix64 finaliser (the digests' `mix`, include/snk.h)
__host__ __device__ inline uint64_t ck_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// index hash: a different finaliser chain over both key words
__device__ inline uint64_t ck_hash(uint64_t hi, uint64_t lo) {
    uint64_t x = hi * 0xD6E8FEB86659FD93ull ^ (lo + 0xA0761D6478BD642Full);
    x ^= x >> 32; x *= 0xE7037ED1A0B428DBull;
    x ^= x >> 29; x *= 0x8EBC6AF09C88C6E3ull;
    return x ^ (x >> 32);
}

// ---- k-mers: 128-bit (hi, lo), base i at bits 127-2i..126-2i, the 128-2K bits below the bases zero
struct ck_kmer { uint64_t hi, lo; };
// the 32 two-bit groups of a word in reverse order
__device__ inline uint64_t ck_rev_pairs(uint64_t x) {
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    return (x >> 32) | (x << 32);
}
// reverse complement (App. A.3): complement every base, reverse the 64 groups, drop the reversed padding (sh = 128 - 2K, 0 < sh < 64)
__device__ inline ck_kmer ck_rc(ck_kmer k, uint32_t sh) {
    const uint64_t a = ck_rev_pairs(~k.lo), b = ck_rev_pairs(~k.hi);
    return ck_kmer{(a << sh) | (b >> (64 - sh)), b << sh};
}
__device__ inline bool ck_lt(ck_kmer a, ck_kmer b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ inline bool ck_eq(ck_kmer a, ck_kmer b) { return a.hi == b.hi && a.lo == b.lo; }
__device__ inline uint32_t ck_base(ck_kmer k, uint32_t i) {
    return i < 32 ? (uint32_t)(k.hi >> (62 - 2 * i)) & 3u : (uint32_t)(k.lo >> (62 - 2 * (i - 32))) & 3u;
}
// append b on the right (KMer::toSuccessor) / prepend on the left (KMer::toPredecessor)
__device__ inline ck_kmer ck_succ(ck_kmer k, uint32_t b, uint32_t sh) {
    return ck_kmer{(k.hi << 2) | (k.lo >> 62), (k.lo << 2) | ((uint64_t)b << sh)};
}
__device__ inline ck_kmer ck_pred(ck_kmer k, uint32_t b, uint32_t sh) {
    return ck_kmer{(k.hi >> 2) | ((uint64_t)b << 62), ((k.lo >> 2) | (k.hi << 62)) & ~((1ull << sh) - 1)};
}
__device__ inline ck_kmer ck_from_bases(const uint8_t* b, uint32_t K) {
    ck_kmer k{0, 0};
    for (uint32_t i = 0; i < K; ++i) {
        const uint64_t v = b[i] & 3u;
        if (i < 32) k.hi |= v << (62 - 2 * i);
        else k.lo |= v << (62 - 2 * (i - 32));
    }
    return k;
}
// context byte of the other strand = the byte's bits in reverse order (KMerContext.cc:19)
__device__ inline uint32_t ck_ctx_rc(uint32_t c) { return __brev(c & 0xFFu) >> 24; }
__device__ inline uint32_t ck_side(uint32_t nib) { return (uint32_t)__popc(nib & 0xFu); }
__device__ inline uint32_t ck_only(uint32_t nib) { return (uint32_t)__ffs(nib & 0xFu) - 1u; }

struct ck_table {
    const uint64_t* keys;    // {lo, hi} per row
    const uint32_t* counts;
    const uint8_t* ctx;
    const uint32_t* slots;   // index
    uint64_t cap, n;
    uint64_t kmask;          // the key bits that are k-mer (not group): the index hashes these only, so every group's copy of a k-mer
                             // lies on one probe chain
    uint32_t K, sh;
};
// the entry of a key; *other: the chain holds the same k-mer under another group
__device__ inline uint64_t ck_find(const ck_table& t, uint64_t hi, uint64_t lo, bool* other) {
    uint64_t p = __umul64hi(ck_hash(hi, lo & t.kmask), t.cap);
    for (uint64_t probe = 0; probe < t.cap; ++probe) {
        const uint32_t s = t.slots[p];
        if (s == CK_EMPTY) return CK_NONE;
        if (t.keys[2 * (uint64_t)s + 1] == hi) {
            const uint64_t klo = t.keys[2 * (uint64_t)s];
            if (klo == lo) return s;
            if ((klo & t.kmask) == (lo & t.kmask)) *other = true;
        }
        if (++p == t.cap) p = 0;
    }
    return CK_NONE;
}
// a k-mer as met in a sequence: its entry, its context in the orientation it was met in, whether it is a palindrome
struct ck_hit { uint64_t id; uint32_t ctx; bool rev, pal, other; };   // other: missing here, present under another group
__device__ inline ck_hit ck_lookup(const ck_table& t, ck_kmer k, uint32_t group) {
    const ck_kmer r = ck_rc(k, t.sh);
    ck_hit h;
    h.rev = ck_lt(r, k);       // CanonicalForm::REV <=> rc < fwd (dna/CanonicalForm.h:58-67)
    h.pal = ck_eq(r, k);
    const ck_kmer c = h.rev ? r : k;
    h.other = false;
    h.id = ck_find(t, c.hi, c.lo | group, &h.other);
    h.ctx = 0;
    if (h.id != CK_NONE) {
        const uint32_t s = t.ctx[h.id];
        h.ctx = h.rev ? ck_ctx_rc(s) : s;
    }
    return h;
}
// upstream/downstreamExtensionPossible (BuildReadQGraph48.cc:408-428) of a k-mer with context c in the orientation given
__device__ inline bool ck_down_possible(const ck_table& t, ck_kmer k, uint32_t c, uint32_t group) {
    if (ck_side(c) != 1) return false;
    const ck_hit h = ck_lookup(t, ck_succ(k, ck_only(c), t.sh), group);
    return !h.pal && h.id != CK_NONE && ck_side(h.ctx >> 4) == 1;
}
__device__ inline bool ck_up_possible(const ck_table& t, ck_kmer k, uint32_t c, uint32_t group) {
    if (ck_side(c >> 4) != 1) return false;
    const ck_hit h = ck_lookup(t, ck_pred(k, ck_only(c >> 4), t.sh), group);
    return !h.pal && h.id != CK_NONE && ck_side(h.ctx) == 1;
}

__device__ inline uint64_t ck_wave_sum(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline void ck_note(ck_acc* acc, int c, uint64_t n, uint64_t first) {
    if (n) {
        atomicAdd(&acc->count[c], (unsigned long long)n);
        atomicMin(&acc->first[c], (unsigned long long)first);
    }
}
// one per lane -> one atomic per wave
__device__ inline void ck_wave_add(unsigned long long* dst, uint64_t v) {
    v = ck_wave_sum(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

struct ck_args {
    ck_table t;
    uint32_t flags, min_freq, grouped, pad_mask_lo;   // pad_mask_lo: low key bits that must be zero outside grouped runs
    uint64_t n_unitigs, total_bases;
    const uint64_t* off;
    const uint8_t* bases;
    const uint32_t* ugroup;
    uint32_t* vis;          // 2 bits per entry
    uint32_t* recount;      // reads level
    uint32_t* shadow;       // reads level: 4 context bytes per word
    ck_acc* acc;
};

// ---- table: digest, per-row rules, index insertion
__global__ void __launch_bounds__(CB) ck_table_kernel(ck_args a, int build_index) {
    const ck_table& t = a.t;
    uint64_t dig = 0, nbelow = 0, nsort = 0, npad = 0, ndup = 0;
    uint64_t fbelow = CK_NONE, fsort = CK_NONE, fpad = CK_NONE, fdup = CK_NONE;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.n; i += stride) {
        const uint64_t lo = t.keys[2 * i], hi = t.keys[2 * i + 1];
        const uint32_t cnt = t.counts[i], c = t.ctx[i];
        dig += ck_mix(lo ^ ck_mix(hi ^ ck_mix(((uint64_t)min(cnt, CK_SAT) << 8) | c)));
        if (!build_index) continue;
        if (cnt < a.min_freq) { ++nbelow; fbelow = min(fbelow, i); }
        if ((a.flags & SNK_CHECK_SORTED_TABLE) && i > 0) {
            const uint64_t plo = t.keys[2 * i - 2], phi = t.keys[2 * i - 1];
            if (phi > hi || (phi == hi && plo > lo)) { ++nsort; fsort = min(fsort, i); }
        }
        if (lo & a.pad_mask_lo) { ++npad; fpad = min(fpad, i); }
        uint64_t p = __umul64hi(ck_hash(hi, lo & t.kmask), t.cap);
        for (uint64_t probe = 0; probe < t.cap; ++probe) {
            uint32_t s = t.slots[p];
            if (s == CK_EMPTY) {
                s = atomicCAS(const_cast<uint32_t*>(&t.slots[p]), CK_EMPTY, (uint32_t)i);
                if (s == CK_EMPTY) break;
            }
            if (t.keys[2 * (uint64_t)s + 1] == hi && t.keys[2 * (uint64_t)s] == lo) { ++ndup; fdup = min(fdup, i); break; }
            if (++p == t.cap) p = 0;
        }
    }
    ck_wave_add(&a.acc->table_digest, dig);
    ck_note(a.acc, C_BELOW_MIN, nbelow, fbelow);
    ck_note(a.acc, C_NOT_SORTED, nsort, fsort);
    ck_note(a.acc, C_KEY_PAD, npad, fpad);
    ck_note(a.acc, C_DUP, ndup, fdup);
}

// ---- contexts: every bit names a neighbour in the table that carries the reciprocal bit (ReadPather.h:356-381)
__global__ void __launch_bounds__(CB) ck_ctx_kernel(ck_args a) {
    const ck_table& t = a.t;
    uint64_t ndang = 0, nrec = 0, fdang = CK_NONE, frec = CK_NONE;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.n; i += stride) {
        const uint32_t c = t.ctx[i];
        if (!c) continue;
        const uint64_t lo = t.keys[2 * i], hi = t.keys[2 * i + 1];
        const uint32_t group = a.grouped ? (uint32_t)lo : 0u;
        const ck_kmer k{hi, a.grouped ? lo & ~0xFFFFFFFFull : lo};
        const uint32_t first = ck_base(k, 0), last = ck_base(k, t.K - 1);
        for (uint32_t b = 0; b < 4; ++b) {
            if (c & (1u << b)) {          // successor k+b: it must have k's first base as its predecessor
                const ck_hit h = ck_lookup(t, ck_succ(k, b, t.sh), group);
                if (h.id == CK_NONE) { ++ndang; fdang = min(fdang, i); }
                else if (!(h.ctx & (0x10u << first))) { ++nrec; frec = min(frec, i); }
            }
            if (c & (0x10u << b)) {       // predecessor b+k: it must have k's last base as its successor
                const ck_hit h = ck_lookup(t, ck_pred(k, b, t.sh), group);
                if (h.id == CK_NONE) { ++ndang; fdang = min(fdang, i); }
                else if (!(h.ctx & (1u << last))) { ++nrec; frec = min(frec, i); }
            }
        }
    }
    ck_note(a.acc, C_DANGLING, ndang, fdang);
    ck_note(a.acc, C_NOT_RECIP, nrec, frec);
}

// ---- unitigs: a wave per unitig
// base j of a unitig's sequence as stored
struct ck_seq {
    const uint8_t* b;
    uint64_t L;
    __device__ uint32_t at(uint64_t j) const { return b[j] & 3u; }
};
// getCanonicalForm of a sequence (dna/CanonicalForm.h:35-48): 0 FWD, 1 REV, 2 PALINDROME; `get(j)` gives base j
template <typename F>
__device__ inline int ck_form(uint64_t L, F get) {
    if (L & 1) return (get(L / 2) & 2u) ? 1 : 0;
    for (uint64_t i = 0, j = L; i < j;) {
        const uint32_t f = get(i), r = get(--j) ^ 3u;
        if (f < r) return 0;
        if (r < f) return 1;
        ++i;
    }
    return 2;
}

__device__ bool ck_circle_canonical(const ck_table& t, const ck_seq& s) {
    // canonicalizeCircle (BuildReadQGraph48.cc:375-397): the minimum canonical k-mer first, in FWD form; then addEdge's own
    // orientation of the whole sequence (:478-486).  The circle's L-K+1 k-mers are positions 0..L-K; its last K-1 bases repeat the first.
    const uint32_t K = t.K;
    const uint64_t L = s.L, m = L - K + 1;
    ck_kmer f = ck_from_bases(s.b, K), best{~0ull, ~0ull};
    uint64_t idx = 0;
    bool best_rev = false;
    for (uint64_t i = 0; i < m; ++i) {
        if (i) f = ck_succ(f, s.at(i + K - 1), t.sh);
        const ck_kmer r = ck_rc(f, t.sh);
        const bool rev = ck_lt(r, f);
        const ck_kmer c = rev ? r : f;
        if (ck_lt(c, best)) { best = c; idx = i; best_rev = rev; }
    }
    const uint64_t idx2 = best_rev ? L - idx - K : idx;
    auto sp = [&](uint64_t j) -> uint32_t { return best_rev ? (s.at(L - 1 - j) ^ 3u) : s.at(j); };
    auto rot = [&](uint64_t j) -> uint32_t { return j < L - idx2 ? sp(idx2 + j) : sp(K - 1 + (j - (L - idx2))); };
    const bool flip = ck_form(L, rot) == 1;
    for (uint64_t j = 0; j < L; ++j) {
        const uint32_t e = flip ? (rot(L - 1 - j) ^ 3u) : rot(j);
        if (e != s.at(j)) return false;
    }
    return true;
}

__global__ void __launch_bounds__(CB) ck_unitig_kernel(ck_args a, int digest_only) {
    const ck_table& t = a.t;
    const uint32_t K = t.K, lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    uint64_t dig = 0;
    uint64_t nbad = 0, nend = 0, ncan = 0, nord = 0;
    uint64_t fbad = CK_NONE, fend = CK_NONE, fcan = CK_NONE, ford = CK_NONE;
    uint64_t ncirc = 0, npal = 0;
    for (uint64_t u = wave; u < a.n_unitigs; u += nwaves) {
        uint64_t beg = a.off[u], end = a.off[u + 1];
        bool bad = (u == 0 && beg != 0) || end < beg || end > a.total_bases;
        if (end > a.total_bases) end = a.total_bases;
        if (beg > end) beg = end;
        const uint64_t L = end - beg;
        const uint32_t group = a.ugroup ? a.ugroup[u] : 0u;
        uint64_t h = 0;
        bool badbase = false;
        for (uint64_t j = lane; j < L; j += 64) {
            const uint32_t b = a.bases[beg + j];
            badbase |= b > 3;
            h += ck_mix((j << 2) | b);
        }
        h = ck_wave_sum(h);
        badbase = __any(badbase);
        if (lane) continue;
        dig += ck_mix(h ^ ck_mix(L ^ ((uint64_t)group << 40)));
        if (digest_only) continue;
        bad = bad || badbase || L < K;
        if (bad) { ++nbad; fbad = min(fbad, u); continue; }
        const ck_seq s{a.bases + beg, L};
        const ck_kmer f = ck_from_bases(s.b, K);
        if ((a.flags & SNK_CHECK_ORDERED) && u > 0) {
            // ordered by their first K bases, group-major when grouped (snk_dev_result); the previous unitig is read as stored
            const uint64_t pb = a.off[u - 1], pe = a.off[u];
            bool ok = true;
            if (pe >= pb + K && pe <= a.total_bases) {
                const ck_kmer pf = ck_from_bases(a.bases + pb, K);
                const uint32_t pg = a.ugroup ? a.ugroup[u - 1] : 0u;
                ok = pg < group || (pg == group && ck_lt(pf, f));
            }
            if (!ok) { ++nord; ford = min(ford, u); }
        }
        const ck_hit hf = ck_lookup(t, f, group);
        if (L == K && hf.pal) { ++npal; continue; }   // a palindrome is its own unitig (buildEdge :336-340)
        const ck_kmer l = ck_from_bases(s.b + L - K, K);
        const ck_hit hl = ck_lookup(t, l, group);
        bool circle = false;
        if (hl.id != CK_NONE) {      // L == K: a k-mer that is its own successor (a homopolymer) closes a circle of one k-mer
            bool wrap = true;
            for (uint32_t j = 0; j + 1 < K && wrap; ++j) wrap = s.at(L - K + 1 + j) == s.at(j);
            circle = wrap && ck_down_possible(t, l, hl.ctx, group);
        }
        if (circle) {
            ++ncirc;
            if (!ck_circle_canonical(t, s)) { ++ncan; fcan = min(fcan, u); }
            continue;
        }
        if ((hf.id != CK_NONE && ck_up_possible(t, f, hf.ctx, group)) || (hl.id != CK_NONE && ck_down_possible(t, l, hl.ctx, group))) {
            ++nend; fend = min(fend, u);
        }
        if (ck_form(L, [&](uint64_t j) { return s.at(j); }) != 0) { ++ncan; fcan = min(fcan, u); }
    }
    ck_wave_add(&a.acc->unitig_digest, dig);
    if (digest_only) return;
    ck_note(a.acc, C_BAD_UNITIG, nbad, fbad);
    ck_note(a.acc, C_END_EXT, nend, fend);
    ck_note(a.acc, C_NOT_CANON, ncan, fcan);
    ck_note(a.acc, C_NOT_ORDERED, nord, ford);
    if (ncirc) atomicAdd(&a.acc->n_circles, (unsigned long long)ncirc);
    if (npal) atomicAdd(&a.acc->n_palindromes, (unsigned long long)npal);
}

// ---- every k-mer of every unitig, and every step inside one (EdgeBuilder::extend, :445-464)
__device__ inline void ck_visit(uint32_t* vis, uint64_t e) {
    const uint32_t bit = 1u << (2 * (e & 15));
    const uint32_t old = atomicOr(&vis[e >> 4], bit);
    if (old & bit) atomicOr(&vis[e >> 4], bit << 1);
}
__global__ void __launch_bounds__(CB) ck_pos_kernel(ck_args a) {
    const ck_table& t = a.t;
    const uint32_t K = t.K;
    const uint64_t T = a.total_bases, nseg = (T + CK_SEG - 1) / CK_SEG;
    uint64_t nmiss = 0, nbrk = 0, ngrp = 0, fmiss = CK_NONE, fbrk = CK_NONE, fgrp = CK_NONE;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t sg = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; sg < nseg; sg += stride) {
        const uint64_t p0 = sg * CK_SEG, p1 = min(p0 + CK_SEG, T);
        // the unitig holding p0: the last u with off[u] <= p0
        uint64_t lo = 0, hi = a.n_unitigs;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (a.off[mid] <= p0) lo = mid; else hi = mid;
        }
        uint64_t u = lo;
        ck_kmer cur{0, 0};
        ck_hit prev{CK_NONE, 0, false, false, false};
        bool have = false;           // cur / prev hold the k-mer at p - 1 of the same unitig
        for (uint64_t p = p0; p < p1; ++p) {
            while (u + 1 < a.n_unitigs && a.off[u + 1] <= p) ++u;
            const uint64_t beg = a.off[u], end = min(a.off[u + 1], T);
            if (p < beg || p + K > end) { have = false; continue; }
            const uint32_t group = a.ugroup ? a.ugroup[u] : 0u;
            if (p == beg) have = false;
            if (!have && p > beg) {      // the step into p needs the k-mer before it
                cur = ck_from_bases(a.bases + p - 1, K);
                prev = ck_lookup(t, cur, group);
                have = true;
            }
            cur = have ? ck_succ(cur, a.bases[p + K - 1] & 3u, t.sh) : ck_from_bases(a.bases + p, K);
            const ck_hit h = ck_lookup(t, cur, group);
            if (h.id == CK_NONE && h.other) { ++ngrp; fgrp = min(fgrp, u); }   // the k-mer is there, under another group
            else if (h.id == CK_NONE) { ++nmiss; fmiss = min(fmiss, u); }
            else ck_visit(a.vis, h.id);
            if (have && h.id != CK_NONE && prev.id != CK_NONE) {
                const bool ok = ck_side(prev.ctx) == 1 && ck_only(prev.ctx) == (a.bases[p + K - 1] & 3u) && ck_side(h.ctx >> 4) == 1 &&
                                !h.pal && !prev.pal;
                if (!ok) { ++nbrk; fbrk = min(fbrk, u); }
            }
            prev = h;
            have = true;
        }
    }
    ck_note(a.acc, C_MISSING, nmiss, fmiss);
    ck_note(a.acc, C_GROUP, ngrp, fgrp);
    ck_note(a.acc, C_INTERIOR, nbrk, fbrk);
}

// ---- reads level: the k-mer instances of Kmerizer::map (BuildReadQGraph48.cc:155-172) against the table
struct ck_reads {
    const uint32_t* rows;
    const uint16_t* lens;
    const uint8_t* quals;
    const uint16_t* good_len;
    const uint32_t* group;
    uint64_t n;
    uint32_t row_words, read_len, qstride, min_qual;
};
__device__ inline uint32_t ck_row_base(const uint32_t* row, uint32_t i) { return (row[i >> 4] >> (30 - 2 * (i & 15))) & 3u; }
// GoodLenTailFinder (BuildReadQGraph48.cc:72-82; App. A.4): from the 3' end, the first run of K quals >= min_qual
__device__ inline uint32_t ck_trim(const uint8_t* q, uint32_t len, uint32_t K, uint32_t min_qual) {
    uint32_t good = 0;
    for (uint32_t i = len; i-- > 0;) {
        if (q[i] < min_qual) good = 0;
        else if (++good == K) return i + K;
    }
    return 0;
}
__device__ inline void ck_shadow(uint32_t* shadow, uint64_t e, uint32_t bits) {
    atomicOr(&shadow[e >> 2], bits << (8 * (e & 3)));
}
__global__ void __launch_bounds__(CB) ck_reads_kernel(ck_args a, ck_reads r) {
    const ck_table& t = a.t;
    const uint32_t K = t.K;
    uint64_t inst = 0, ngl = 0, fgl = CK_NONE;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < r.n; i += stride) {
        const uint32_t len = r.lens ? min((uint32_t)r.lens[i], r.read_len) : r.read_len;
        uint32_t gl;
        if (r.quals) {
            gl = ck_trim(r.quals + i * (uint64_t)r.qstride, len, K, r.min_qual);
            if (r.good_len && r.good_len[i] != gl) { ++ngl; fgl = min(fgl, i); }
        } else {
            gl = min((uint32_t)r.good_len[i], r.read_len);
        }
        if (gl < K + 1) continue;     // :160
        inst += gl - K + 1;
        const uint32_t* row = r.rows + i * (uint64_t)r.row_words;
        const uint32_t group = r.group ? r.group[i] : 0u;
        ck_kmer f{0, 0};
        for (uint32_t j = 0; j < K; ++j) {
            const uint64_t v = ck_row_base(row, j);
            if (j < 32) f.hi |= v << (62 - 2 * j);
            else f.lo |= v << (62 - 2 * (j - 32));
        }
        ck_hit prev{CK_NONE, 0, false, false, false};
        for (uint32_t p = 0; p + K <= gl; ++p) {
            if (p) f = ck_succ(f, ck_row_base(row, p + K - 1), t.sh);
            const ck_hit h = ck_lookup(t, f, group);
            if (h.id != CK_NONE) {
                atomicAdd(&a.recount[h.id], 1u);
                if (p && prev.id != CK_NONE) {
                    // prev -> f: prev gains the successor f's last base, f gains the predecessor prev's first base (read orientation)
                    const uint32_t s = 1u << ck_row_base(row, p + K - 1), q = 0x10u << ck_row_base(row, p - 1);
                    ck_shadow(a.shadow, prev.id, prev.rev ? ck_ctx_rc(s) : s);
                    ck_shadow(a.shadow, h.id, h.rev ? ck_ctx_rc(q) : q);
                }
            }
            prev = h;
        }
    }
    ck_wave_add(&a.acc->n_instances, inst);
    ck_note(a.acc, C_GOODLEN_MM, ngl, fgl);
}

// ---- per entry: visit marks; recount and shadow context against the table
__global__ void __launch_bounds__(CB) ck_final_kernel(ck_args a, int reads, int check_ctx) {
    const ck_table& t = a.t;
    uint64_t nunc = 0, nrep = 0, ncnt = 0, nctx = 0;
    uint64_t func = CK_NONE, frep = CK_NONE, fcnt = CK_NONE, fctx = CK_NONE;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < t.n; e += stride) {
        const uint32_t v = (a.vis[e >> 4] >> (2 * (e & 15))) & 3u;
        if (!(v & 1u)) { ++nunc; func = min(func, e); }
        if (v & 2u) { ++nrep; frep = min(frep, e); }
        if (!reads) continue;
        if (min(a.recount[e], CK_SAT) != min(t.counts[e], CK_SAT)) { ++ncnt; fcnt = min(fcnt, e); }
        if (check_ctx && ((a.shadow[e >> 2] >> (8 * (e & 3))) & 0xFFu) != t.ctx[e]) { ++nctx; fctx = min(fctx, e); }
    }
    ck_note(a.acc, C_UNCOVERED, nunc, func);
    ck_note(a.acc, C_REPEATED, nrep, frep);
    ck_note(a.acc, C_COUNT_MM, ncnt, fcnt);
    ck_note(a.acc, C_CTX_MM, nctx, fctx);
}

constexpr uint64_t CK_GRID_CAP = 65536;     // every kernel of this file strides over what its grid does not cover

}  // namespace

extern "C" int snk_dev_check_graph(snk_ctx* ctx, const snk_check_input* in, const snk_dev_reads* reads, snk_check_report* out, void* stream,
                                   char* err, size_t errcap) {
    if (!ctx || !in || !out) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_check_graph: NULL argument");
    if (out->struct_size < sizeof(snk_check_report))
        return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_check_graph: report struct_size %u < %zu (caller built against an older snk.h?)",
                        out->struct_size, sizeof(snk_check_report));
    const uint32_t struct_size = out->struct_size;
    memset(out, 0, sizeof(snk_check_report));
    out->struct_size = struct_size;
    const uint32_t K = in->K, flags = in->flags;
    const bool digest_only = flags & SNK_CHECK_DIGEST_ONLY, grouped = flags & SNK_CHECK_GROUPED;
    if (K != 48 && K != 60) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_check_graph: K=%u (48 or 60)", K);
    if (grouped && K != 48) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_check_graph: grouped keys need K=48");
    if (in->n_kmers > 0xFFFFFFFEull) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_check_graph: %llu entries (at most 2^32 - 2)",
                                                    (unsigned long long)in->n_kmers);
    if ((in->n_kmers && (!in->keys || !in->counts || !in->ctx)) || (in->n_unitigs && (!in->unitig_off || !in->unitig_bases)))
        return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_check_graph: NULL device array");
    if (grouped && in->n_unitigs && !in->unitig_group) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_check_graph: grouped without unitig_group");
    if (reads && !digest_only) {
        if (!reads->rows || (!reads->quals && !reads->good_len) || reads->read_len > 16 * reads->row_words || (reads->quals && reads->qstride < reads->read_len))
            return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_check_graph: reads need rows, quals or good_len, read_len <= 16 * row_words");
        if (grouped && !reads->group) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_check_graph: grouped reads without group ids");
    }
    // scratch after the arrays under test, handed back on return: the result being checked stays valid
    const int rc = snk_call_run(ctx, stream, "snk_dev_check_graph", out, err, errcap, [&](snk_call& c) -> int {
        const hipStream_t st = c.st;
        int rc;
        ck_acc* acc = nullptr;
        if ((rc = c.alloc(1, &acc))) return rc;
        SNK_HIP_TRY(hipMemsetAsync(acc, 0, sizeof(ck_acc), st));
        SNK_HIP_TRY(hipMemsetAsync(acc->first, 0xFF, sizeof(acc->first), st));

        ck_args a{};
        a.t.keys = (const uint64_t*)in->keys;
        a.t.counts = (const uint32_t*)in->counts;
        a.t.ctx = (const uint8_t*)in->ctx;
        a.t.n = in->n_kmers;
        a.t.K = K;
        a.t.sh = 128 - 2 * K;
        a.flags = flags;
        a.min_freq = in->min_freq;
        a.grouped = grouped;
        a.pad_mask_lo = grouped ? 0u : (uint32_t)((1ull << a.t.sh) - 1);
        a.t.kmask = grouped ? ~0xFFFFFFFFull : ~0ull;
        a.n_unitigs = in->n_unitigs;
        a.off = (const uint64_t*)in->unitig_off;
        a.bases = (const uint8_t*)in->unitig_bases;
        a.ugroup = grouped ? (const uint32_t*)in->unitig_group : nullptr;
        a.acc = acc;
        uint64_t total = 0;
        if (in->n_unitigs) {
            SNK_HIP_TRY(hipMemcpyAsync(&total, a.off + in->n_unitigs, 8, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(snk_sync(st));
        }
        a.total_bases = total;
        const bool do_reads = reads && !digest_only && reads->n_reads;

        SNK_HIP_TRY(c.stamp());
        if (!digest_only) {
            a.t.cap = std::max<uint64_t>(2 * a.t.n + 1, 64);     // load <= 0.5
            uint32_t* slots = nullptr;
            if ((rc = c.alloc(a.t.cap, &slots)) || (rc = c.alloc((a.t.n + 15) / 16, &a.vis))) return rc;
            SNK_HIP_TRY(hipMemsetAsync(slots, 0xFF, a.t.cap * 4, st));
            SNK_HIP_TRY(hipMemsetAsync(a.vis, 0, (a.t.n + 15) / 16 * 4, st));
            a.t.slots = slots;
        }
        if (a.t.n) SNK_HIP_TRY(snk_launch(ck_table_kernel, snk_blocks_capped(a.t.n, CB, CK_GRID_CAP), CB, 0, st, a, digest_only ? 0 : 1));
        if (a.n_unitigs) SNK_HIP_TRY(snk_launch(ck_unitig_kernel, snk_blocks_capped(a.n_unitigs, CB / 64, CK_GRID_CAP), CB, 0, st, a, digest_only ? 1 : 0));
        if (!digest_only) {
            if (a.t.n) SNK_HIP_TRY(snk_launch(ck_ctx_kernel, snk_blocks_capped(a.t.n, CB, CK_GRID_CAP), CB, 0, st, a));
            if (a.n_unitigs && total) SNK_HIP_TRY(snk_launch(ck_pos_kernel, snk_blocks_capped(snk_blocks(total, CK_SEG), CB, CK_GRID_CAP), CB, 0, st, a));
        }
        SNK_HIP_TRY(c.stamp());
        if (do_reads) {
            if ((rc = c.alloc(a.t.n, &a.recount)) || (rc = c.alloc((a.t.n + 3) / 4, &a.shadow))) return rc;
            SNK_HIP_TRY(hipMemsetAsync(a.recount, 0, std::max<uint64_t>(a.t.n * 4, 4), st));
            SNK_HIP_TRY(hipMemsetAsync(a.shadow, 0, std::max<uint64_t>((a.t.n + 3) / 4 * 4, 4), st));
            ck_reads r{};
            r.rows = (const uint32_t*)reads->rows;
            r.lens = (const uint16_t*)reads->lens;
            r.quals = (const uint8_t*)reads->quals;
            r.good_len = (const uint16_t*)reads->good_len;
            r.group = grouped ? (const uint32_t*)reads->group : nullptr;
            r.n = reads->n_reads;
            r.row_words = reads->row_words;
            r.read_len = reads->read_len;
            r.qstride = reads->qstride;
            r.min_qual = in->min_qual ? in->min_qual : 7;
            SNK_HIP_TRY(snk_launch(ck_reads_kernel, snk_blocks_capped(r.n, CB, CK_GRID_CAP), CB, 0, st, a, r));
        }
        if (!digest_only && a.t.n) SNK_HIP_TRY(snk_launch(ck_final_kernel, snk_blocks_capped(a.t.n, CB, CK_GRID_CAP), CB, 0, st, a, do_reads ? 1 : 0, in->min_freq > 1 ? 1 : 0));
        SNK_HIP_TRY(c.stamp());
        ck_acc h;
        SNK_HIP_TRY(hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));

        for (int i = 0; i < SNK_CHECK_N_COUNTERS; ++i) {
            out->count[i] = h.count[i];
            out->first[i] = h.first[i];
        }
        if (do_reads && in->n_instances && h.n_instances != in->n_instances) { out->count[C_INST_MM] = 1; out->first[C_INST_MM] = 0; }
        out->levels = digest_only ? 0u : (1u | (do_reads ? 2u : 0u));
        out->n_kmers = in->n_kmers;
        out->n_unitigs = in->n_unitigs;
        out->n_bases = total;
        out->n_circles = h.n_circles;
        out->n_palindromes = h.n_palindromes;
        out->n_instances = h.n_instances;
        out->table_digest = h.table_digest;
        out->unitig_digest = h.unitig_digest;
        out->peak_bytes = c.bytes;
        out->graph_ms = c.ms(0, 1);
        out->reads_ms = c.ms(1, 2);
        return c.end(SNK_OK);
    });
    out->struct_size = struct_size;
    return rc;
}
