// snk_graph.hip -- K9..K11: adjacency prune, unitig ("edge") pull and packing, all on device.
//
// What it replaces:
//   KmerDict fill + recomputeAdjacencies  lib/assembly/src/kmers/ReadPather.h:346-385 (drop context bits whose
//                                          neighbour k-mer was not retained)
//   EdgeBuilder / buildEdges              lib/assembly/src/paths/long/BuildReadQGraph48.cc:327-541
//                                          (maximal unbranched walks, palindromes are 1-k-mer edges, canonical
//                                          orientation :457-464,481-485, smooth circles :348-397)
//   == tada build_sedges/build_edges       lib/tada/src/debruijn.rs:147-320,539-776.
//
// The reference walks each unitig sequentially under a spin-lock.  On the synthetic benchmark the
// whole genome is ONE unitig, so a walk has no parallelism at all; here the problem is recast as
// list ranking on the graph of reciprocal-unique links:
//   1. retained table sorted by key (rocPRIM radix sort on the 2K significant bits) -> index order ==
//      k-mer order, which also makes the run deterministic;
//   2. open-addressing index (fingerprint | position) in HBM for membership probes;
//   3. prune: every set context bit is probed once; sides left with exactly one bit remember the
//      neighbour's position and relative strand;
//   4. links: side s of node i is linked to the facing side of node j iff both sides have degree 1 and
//      neither k-mer is a palindrome (BuildReadQGraph48.cc:408-428,445-456);
//   5. list ranking (snk_rank.hip) over the 2n directed states (node, exit side): distance to and identity
//      of both path ends for every node; states that never reach an end are on smooth circles: the
//      circle is cut at the left side of its minimum k-mer (canonicalizeCircle :375-397) and re-ranked;
//   6. orientation per path by the reference's rule (odd length: middle base & 2; even: lexicographic,
//      dna/CanonicalForm.h:35-48), prefix sums for offsets, one base per node scattered into place.
// Below the global stage: the sharded stage's answers and the fragment join (snk_dist_join, snk_join_*), which ranks fragment
// ends with the same snk_rank_lists.
#include <string.h>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "snk_ctx.h"
#include "snk_common.h"
#include "snk_kernels.h"
#include "snk_graph.h"
#include "snk_rank.h"
#include "snk_stages.h"

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int TB = 256;

__device__ __forceinline__ snk_kmer load_key(const snk_u128* keys, uint64_t i) {
    const uint64_t* p = reinterpret_cast<const uint64_t*>(keys + i);
    snk_kmer k;
    k.lo = p[0];
    k.hi = p[1];
    return k;
}

// ------------------------------------------------------------------ index build / probe
__global__ void __launch_bounds__(TB) index_build_kernel(const snk_u128* __restrict__ keys, uint64_t n,
                                                         unsigned long long* __restrict__ tab, uint64_t mask) {
    uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    snk_kmer k = load_key(keys, i);
    uint32_t h1, h2;
    snk_kmer_hash2(k, &h1, &h2);
    uint64_t slot = (((uint64_t)h1 << 32) | h2) & mask;
    unsigned long long ent = ((unsigned long long)h1 << 32) | (unsigned long long)(i + 1);
    for (;;) {
        unsigned long long old = atomicCAS(&tab[slot], 0ull, ent);
        if (old == 0ull) break;
        slot = (slot + 1) & mask;
    }
}

__device__ __forceinline__ int64_t index_find(const snk_u128* __restrict__ keys, const unsigned long long* __restrict__ tab,
                                              uint64_t mask, snk_kmer k) {
    uint32_t h1, h2;
    snk_kmer_hash2(k, &h1, &h2);
    uint64_t slot = (((uint64_t)h1 << 32) | h2) & mask;
    for (;;) {
        unsigned long long e = tab[slot];
        if (e == 0ull) return -1;
        if ((uint32_t)(e >> 32) == h1) {
            uint64_t idx = (uint32_t)e - 1u;
            snk_kmer c = load_key(keys, idx);
            if (snk_kmer_eq(c, k)) return (int64_t)idx;
        }
        slot = (slot + 1) & mask;
    }
}

template <int K>
__device__ __forceinline__ int64_t find_any(const snk_u128* keys, const unsigned long long* tab, uint64_t mask, snk_kmer k,
                                            uint32_t* rev) {
    snk_kmer r = snk_kmer_rc<K>(k);
    bool isrev = snk_kmer_lt(r, k);   // KmerDict::findEntry canonicalises (ReadPather.h:241-245)
    *rev = isrev ? 1u : 0u;
    return index_find(keys, tab, mask, isrev ? r : k);
}

// ------------------------------------------------------------------ prune (ReadPather.h:346-385)
// side 0 = successors (low nibble), side 1 = predecessors (high nibble)
template <int K>
__global__ void __launch_bounds__(TB) prune_kernel(const snk_u128* __restrict__ keys, const uint64_t* __restrict__ vals,
                                                   uint64_t n, const unsigned long long* __restrict__ tab, uint64_t mask,
                                                   uint32_t do_prune, uint8_t* __restrict__ ctx_out,
                                                   uint32_t* __restrict__ count_out, uint32_t* __restrict__ nbr) {
    uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    snk_kmer k = load_key(keys, i);
    uint64_t v = vals[i];
    uint32_t c = (uint32_t)(v & 0xFFu);
    count_out[i] = (uint32_t)(v >> 8);
    uint32_t keep = 0;
    uint32_t nb0 = NONE, nb1 = NONE;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
        if (c & (1u << b)) {
            uint32_t rev;
            int64_t j = find_any<K>(keys, tab, mask, snk_kmer_succ<K>(k, b), &rev);
            if (j >= 0 || !do_prune) { keep |= 1u << b; nb0 = j >= 0 ? ((uint32_t)j << 1) | rev : NONE; }
        }
        if (c & (0x10u << b)) {
            uint32_t rev;
            int64_t j = find_any<K>(keys, tab, mask, snk_kmer_pred<K>(k, b), &rev);
            if (j >= 0 || !do_prune) { keep |= 0x10u << b; nb1 = j >= 0 ? ((uint32_t)j << 1) | rev : NONE; }
        }
    }
    ctx_out[i] = (uint8_t)keep;
    nbr[2 * i + 0] = __popc(keep & 0x0Fu) == 1 ? nb0 : NONE;
    nbr[2 * i + 1] = __popc(keep & 0xF0u) == 1 ? nb1 : NONE;
}

// ------------------------------------------------------------------ links (BuildReadQGraph48.cc:408-428,445-456)
template <int K>
__global__ void __launch_bounds__(TB) link_kernel(const snk_u128* __restrict__ keys, const uint8_t* __restrict__ ctx,
                                                  const uint32_t* __restrict__ nbr, uint64_t n, uint32_t* __restrict__ link) {
    uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (s >= 2 * n) return;
    uint32_t nb = nbr[s];
    uint32_t out = NONE;
    if (nb != NONE) {
        uint64_t i = s >> 1;
        uint32_t side = (uint32_t)(s & 1);
        uint32_t j = nb >> 1, rev = nb & 1u;
        snk_kmer ki = load_key(keys, i), kj = load_key(keys, j);
        bool pal = snk_kmer_eq(ki, snk_kmer_rc<K>(ki)) || snk_kmer_eq(kj, snk_kmer_rc<K>(kj));
        uint32_t fs = side ^ 1u ^ rev;                 // side of j that faces i
        uint32_t cj = ctx[j];
        uint32_t deg = fs ? __popc(cj & 0xF0u) : __popc(cj & 0x0Fu);
        if (!pal && deg == 1) out = (j << 1) | fs;
    }
    link[s] = out;
}

// ------------------------------------------------------------------ orientation, offsets, emission
template <int K>
__device__ __forceinline__ uint32_t oriented_base(snk_kmer k, bool rc, int idx) {
    // base idx of the k-mer read forward, or of its reverse complement
    return rc ? (snk_kmer_base<K>(k, K - 1 - idx) ^ 3u) : snk_kmer_base<K>(k, idx);
}

struct node_place {
    uint32_t pid;     // path id = smaller terminal state
    uint32_t other;   // the larger terminal state
    uint32_t n;       // nodes on the path
    uint32_t pos;     // position walking from terminal `pid`
    bool rc;          // traversed as reverse complement when walking from `pid`
};
// rk[state] = (distance to the end of the path, terminal state): one 8-byte record per state, so the ranking's
// second walk does one scattered store per state instead of two
__device__ __forceinline__ node_place place_of(const uint2* rk, uint64_t i) {
    const uint2 a = rk[2 * i], b = rk[2 * i + 1];
    uint32_t tR = a.y, tL = b.y;
    uint32_t dR = a.x, dL = b.x;
    node_place p;
    p.n = dR + dL + 1u;
    if (tL < tR) { p.pid = tL; p.other = tR; p.pos = dL; p.rc = false; }
    else { p.pid = tR; p.other = tL; p.pos = dR; p.rc = true; }
    return p;
}

// REV decision per path (getCanonicalForm, dna/CanonicalForm.h:35-48); written by exactly one node of the path
template <int K>
__global__ void __launch_bounds__(TB) orient_kernel(const snk_u128* __restrict__ keys, const uint2* __restrict__ rk, uint64_t n, uint8_t* __restrict__ prev) {
    uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    node_place p = place_of(rk, i);
    uint64_t L = (uint64_t)K + p.n - 1;
    snk_kmer k = load_key(keys, i);
    if (L & 1) {
        uint64_t mid = L / 2;
        if (mid <= (uint64_t)(K - 1)) {
            if (p.pos == 0) prev[p.pid] = (oriented_base<K>(k, p.rc, (int)mid) & 2u) ? 1 : 0;
        } else if ((uint64_t)p.pos == mid - (K - 1)) {
            prev[p.pid] = (oriented_base<K>(k, p.rc, K - 1) & 2u) ? 1 : 0;
        }
    } else if (p.pos == 0) {
        snk_kmer first = p.rc ? snk_kmer_rc<K>(k) : k;
        uint32_t eB = p.other >> 1, xB = p.other & 1u;
        snk_kmer kb = load_key(keys, eB);
        snk_kmer rc_last = (xB == 0) ? snk_kmer_rc<K>(kb) : kb;   // rc of the last oriented k-mer
        prev[p.pid] = snk_kmer_lt(rc_last, first) ? 1 : 0;
    }
}

// head flags and unitig lengths
__global__ void __launch_bounds__(TB) head_kernel(const uint2* __restrict__ rk,
                                                  const uint8_t* __restrict__ prev, uint64_t n, uint32_t K,
                                                  uint32_t* __restrict__ hflag, uint64_t* __restrict__ hlen) {
    uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    node_place p = place_of(rk, i);
    uint32_t pos = prev[p.pid] ? p.n - 1u - p.pos : p.pos;
    bool head = pos == 0;
    hflag[i] = head ? 1u : 0u;
    hlen[i] = head ? (uint64_t)K + p.n - 1 : 0ull;
}
__global__ void __launch_bounds__(TB) head_place_kernel(const uint2* __restrict__ rk, const uint32_t* __restrict__ hflag,
                                                        const uint32_t* __restrict__ hidx, const uint64_t* __restrict__ hoff,
                                                        uint64_t n, uint64_t* __restrict__ poff, uint64_t* __restrict__ unitig_off) {
    uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    if (hflag[i]) {
        uint32_t tR = rk[2 * i].y, tL = rk[2 * i + 1].y;
        uint32_t pid = tL < tR ? tL : tR;
        poff[pid] = hoff[i];
        unitig_off[hidx[i]] = hoff[i];
    }
}
template <int K>
__global__ void __launch_bounds__(TB) emit_kernel(const snk_u128* __restrict__ keys, const uint2* __restrict__ rk,
                                                  const uint8_t* __restrict__ prev,
                                                  const uint64_t* __restrict__ poff, uint64_t n, uint8_t* __restrict__ bases) {
    uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    node_place p = place_of(rk, i);
    bool flip = prev[p.pid] != 0;
    uint32_t pos = flip ? p.n - 1u - p.pos : p.pos;
    bool rc = flip ? !p.rc : p.rc;
    snk_kmer k = load_key(keys, i);
    uint64_t off = poff[p.pid];
    if (pos == 0) {
        for (int b = 0; b < K; ++b) bases[off + b] = (uint8_t)oriented_base<K>(k, rc, b);
    } else {
        bases[off + (K - 1) + pos] = (uint8_t)oriented_base<K>(k, rc, K - 1);
    }
}

// k-mer spectrum of the retained table (WriteKmerSpectrum, BuildReadQGraph48.cc:199-216); LDS-privatised bins
constexpr int SPEC_LDS = 2048;
__global__ void __launch_bounds__(TB) spectrum_kernel(const uint32_t* __restrict__ counts, uint64_t n,
                                                      unsigned long long* __restrict__ bins, uint32_t nbins) {
    __shared__ uint32_t h[SPEC_LDS];
    for (int j = threadIdx.x; j < SPEC_LDS; j += TB) h[j] = 0;
    __syncthreads();
    uint64_t stride = (uint64_t)gridDim.x * TB;
    for (uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x; i < n; i += stride) {
        uint32_t c = counts[i];
        if (c > 0xFFFFFFu) c = 0xFFFFFFu;            // the reference's KDef count saturates at 2^24-1 (kmers/ReadPather.h:128-129,145)
        if (c >= nbins) c = nbins - 1;
        if (c < (uint32_t)SPEC_LDS) atomicAdd(&h[c], 1u);
        else atomicAdd(&bins[c], 1ull);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < SPEC_LDS && j < (int)nbins; j += TB)
        if (h[j]) atomicAdd(&bins[j], (unsigned long long)h[j]);
}

}  // namespace

__global__ void __launch_bounds__(256) sorted_check_kernel(const snk_u128* __restrict__ keys, uint64_t n, uint32_t* __restrict__ bad) {
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i + 1 >= n) return;
    if (!(keys[i] < keys[i + 1])) *bad = 1u;   // retained k-mers are distinct: strictly ascending
}

// sort (keys, vals) by key.  Only the top 2K bits are significant; rocPRIM's bit-range path is used for
// large inputs (onesweep) and the full 128-bit sort for small ones (its single-block/merge path mis-sorts
// 128-bit keys when begin_bit != 0 -- ROCm 7.2, see tools/probe/sort128.hip).  The result is verified.
int snk_graph_sort(snk_ctx* ctx, hipStream_t st, uint32_t K, uint64_t n, snk_u128* keys_in, uint64_t* vals_in,
                   snk_u128* keys_out, uint64_t* vals_out, char* err, size_t errcap) {
    if (n == 0) return SNK_OK;
    uint32_t* bad = nullptr;
    {
        void* q;
        int rc = snk_ctx_alloc(ctx, 16, &q, err, errcap);
        if (rc) return rc;
        bad = (uint32_t*)q;
    }
    for (int attempt = 0; attempt < 2; ++attempt) {
        unsigned begin_bit = (attempt == 0 && n >= (8u << 20)) ? 128u - 2u * K : 0u;
        size_t tmp_bytes = 0;
        SNK_HIP_TRY(rocprim::radix_sort_pairs((void*)nullptr, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n,
                                              begin_bit, 128u, st));
        void* tmp = nullptr;
        int rc = snk_ctx_alloc(ctx, tmp_bytes, &tmp, err, errcap);
        if (rc) return rc;
        SNK_HIP_TRY(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, begin_bit,
                                              128u, st));
        SNK_HIP_TRY(hipMemsetAsync(bad, 0, 4, st));
        SNK_HIP_TRY(snk_launch(sorted_check_kernel, snk_blocks(n, 256), 256, 0, st, keys_out, n, bad));
        uint32_t h_bad = 0;
        SNK_HIP_TRY(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        if (!h_bad) return SNK_OK;
        if (begin_bit == 0) break;
    }
    return snk_fail(SNK_E_INTERNAL, err, errcap, "retained k-mer table is not strictly ascending after the sort");
}

template <int K>
static int graph_impl(snk_ctx* ctx, hipStream_t st, const snk_u128* keys, const uint64_t* vals, uint64_t n,
                      uint32_t do_prune, bool want_unitigs, snk_graph_out* out, char* err, size_t errcap) {
    memset(out, 0, sizeof *out);
    if (n == 0) {      // nothing retained: empty but well-formed outputs
        constexpr uint32_t NB0 = 65536;
        G_ALLOC(out->spectrum, unsigned long long, NB0);
        SNK_HIP_TRY(hipMemsetAsync(out->spectrum, 0, NB0 * 8, st));
        out->spectrum_bins = NB0;
        G_ALLOC(out->unitig_off, uint64_t, 2);
        SNK_HIP_TRY(hipMemsetAsync(out->unitig_off, 0, 16, st));
        G_ALLOC(out->unitig_bases, uint8_t, 16);
        G_ALLOC(out->ctx, uint8_t, 16);
        G_ALLOC(out->counts, uint32_t, 4);
        return SNK_OK;
    }
    if (n >= (1ull << 31)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "more than 2^31 retained k-mers on one GPU (%llu)", (unsigned long long)n);
    // index
    uint64_t tg = 1024;
    while (tg < 2 * n) tg <<= 1;
    unsigned long long* tab;
    G_ALLOC(tab, unsigned long long, tg);
    SNK_HIP_TRY(hipMemsetAsync(tab, 0, tg * 8, st));
    SNK_HIP_TRY(snk_launch(index_build_kernel, snk_blocks(n, TB), TB, 0, st, keys, n, tab, tg - 1));
    // prune
    uint8_t* ctx_out; uint32_t* count_out; uint32_t* nbr;
    G_ALLOC(ctx_out, uint8_t, n);
    G_ALLOC(count_out, uint32_t, n);
    G_ALLOC(nbr, uint32_t, 2 * n);
    SNK_HIP_TRY(snk_launch(prune_kernel<K>, snk_blocks(n, TB), TB, 0, st, keys, vals, n, tab, tg - 1, do_prune, ctx_out,
                           count_out, nbr));
    out->ctx = ctx_out;
    out->counts = count_out;
    // spectrum
    {
        int rc = snk_spectrum(ctx, st, count_out, n, &out->spectrum, &out->spectrum_bins, err, errcap);
        if (rc) return rc;
    }
    if (!want_unitigs) return SNK_OK;

    const uint64_t ns = 2 * n;
    uint32_t* link;
    G_ALLOC(link, uint32_t, ns);
    SNK_HIP_TRY(snk_launch(link_kernel<K>, snk_blocks(ns, TB), TB, 0, st, keys, ctx_out, nbr, n, link));

    const uint2* rk = nullptr;
    {
        int rc = snk_rank_lists(ctx, st, link, n, nullptr, nullptr, &rk, &out->n_circles, &out->rank_rounds, err, errcap);
        if (rc) return rc;
    }

    uint8_t* prev;
    G_ALLOC(prev, uint8_t, ns);
    SNK_HIP_TRY(hipMemsetAsync(prev, 0, ns, st));
    SNK_HIP_TRY(snk_launch(orient_kernel<K>, snk_blocks(n, TB), TB, 0, st, keys, rk, n, prev));
    uint32_t *hflag, *hidx;
    uint64_t *hlen, *hoff;
    G_ALLOC(hflag, uint32_t, n + 1);
    G_ALLOC(hidx, uint32_t, n + 1);
    G_ALLOC(hlen, uint64_t, n + 1);
    G_ALLOC(hoff, uint64_t, n + 1);
    SNK_HIP_TRY(hipMemsetAsync(hflag + n, 0, 4, st));
    SNK_HIP_TRY(hipMemsetAsync(hlen + n, 0, 8, st));
    SNK_HIP_TRY(snk_launch(head_kernel, snk_blocks(n, TB), TB, 0, st, rk, prev, n, (uint32_t)K, hflag, hlen));
    {
        size_t t1 = 0, t2 = 0;
        SNK_HIP_TRY(rocprim::exclusive_scan((void*)nullptr, t1, hflag, hidx, 0u, (size_t)(n + 1), rocprim::plus<uint32_t>(), st));
        SNK_HIP_TRY(rocprim::exclusive_scan((void*)nullptr, t2, hlen, hoff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
        void* tmp;
        int rc = snk_ctx_alloc(ctx, t1 > t2 ? t1 : t2, &tmp, err, errcap);
        if (rc) return rc;
        SNK_HIP_TRY(rocprim::exclusive_scan(tmp, t1, hflag, hidx, 0u, (size_t)(n + 1), rocprim::plus<uint32_t>(), st));
        SNK_HIP_TRY(rocprim::exclusive_scan(tmp, t2, hlen, hoff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
    }
    uint64_t h_tot = 0;
    uint32_t h_nu = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&h_nu, hidx + n, 4, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(hipMemcpyAsync(&h_tot, hoff + n, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    uint64_t n_unitigs = h_nu, total_bases = h_tot;
    uint64_t *poff, *uoff;
    uint8_t* bases;
    G_ALLOC(poff, uint64_t, ns);
    G_ALLOC(uoff, uint64_t, n_unitigs + 1);
    G_ALLOC(bases, uint8_t, total_bases);
    SNK_HIP_TRY(snk_launch(head_place_kernel, snk_blocks(n, TB), TB, 0, st, rk, hflag, hidx, hoff, n, poff, uoff));
    SNK_HIP_TRY(hipMemcpyAsync(uoff + n_unitigs, hoff + n, 8, hipMemcpyDeviceToDevice, st));
    SNK_HIP_TRY(snk_launch(emit_kernel<K>, snk_blocks(n, TB), TB, 0, st, keys, rk, prev, poff, n, bases));
    out->n_unitigs = n_unitigs;
    out->total_bases = total_bases;
    out->unitig_off = uoff;
    out->unitig_bases = bases;
    return SNK_OK;
}

int snk_graph_build(snk_ctx* ctx, hipStream_t st, uint32_t K, const snk_u128* keys, const uint64_t* vals, uint64_t n,
                    uint32_t do_prune, bool want_unitigs, snk_graph_out* out, char* err, size_t errcap) {
    if (K == 48) return graph_impl<48>(ctx, st, keys, vals, n, do_prune, want_unitigs, out, err, errcap);
    if (K == 60) return graph_impl<60>(ctx, st, keys, vals, n, do_prune, want_unitigs, out, err, errcap);
    return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "K=%u is not supported (48 or 60)", K);
}

// =====================================================================================================================
// Sharded graph stage and fragment join.  The per-rank work (prune, links, fragments) is the bucket-
// local stage of snk_local.hip; here live the pieces that answer membership queries of other ranks and the join:
//   * a side whose single neighbour lives in another chunk (same rank or not) ends its fragment and exports a "half
//     link" (my terminal state -> the neighbour's state).  Two half links that point at each other are a link (the
//     reciprocal-unique rule of BuildReadQGraph48.cc:408-428 checked half on each owner);
//   * the fragments (tada's per-shard sedges, lib/tada/src/debruijn.rs:296-320) are joined (tada's MAIN_ASM_SN
//     build_edges, debruijn.rs:733-776) by list ranking weighted by k-mers, then get the reference's orientation.
// =====================================================================================================================
namespace {

constexpr unsigned long long NONE64 = ~0ull;

__global__ void __launch_bounds__(TB) answer_kernel(const unsigned long long* __restrict__ q, uint64_t nq,
                                                    const snk_u128* __restrict__ keys, const unsigned long long* __restrict__ tab,
                                                    uint64_t mask, uint32_t* __restrict__ ans) {
    uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (t >= nq) return;
    snk_kmer k;
    k.lo = q[3 * t];
    k.hi = q[3 * t + 1];
    int64_t j = index_find(keys, tab, mask, k);
    ans[t] = j >= 0 ? (uint32_t)j : NONE;
}

// answers come back in the order the queries were sent; qoff[r]..qoff[r+1] went to rank r
__global__ void __launch_bounds__(TB) apply_answers_kernel(const unsigned long long* __restrict__ q, const uint32_t* __restrict__ ans,
                                                           uint64_t nq, const unsigned long long* __restrict__ qoff, uint32_t world,
                                                           uint32_t do_prune, uint32_t* __restrict__ ctx_words,
                                                           uint32_t* __restrict__ rq_idx, uint16_t* __restrict__ rq_meta) {
    uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (t >= nq) return;
    unsigned long long m = q[3 * t + 2];
    uint64_t i = (uint32_t)m;
    uint32_t bit = (uint32_t)(m >> 32) & 0xFFu, rev = (uint32_t)(m >> 40) & 1u;
    uint32_t a = ans[t];
    uint32_t rank = 0;
    while (rank + 1 < world && t >= qoff[rank + 1]) ++rank;
    uint32_t side = bit >> 2;
    if (a == NONE) {
        if (do_prune) atomicAnd(&ctx_words[i >> 2], ~((1u << bit) << (8 * (i & 3))));
    } else {
        rq_idx[2 * i + side] = a;
        rq_meta[2 * i + side] = (uint16_t)(rank | (rev << 15));
    }
}

// ---- join (rank 0)
__global__ void __launch_bounds__(TB) jhash_build_kernel(const unsigned long long* __restrict__ hl_self, uint64_t ne,
                                                         unsigned long long* __restrict__ hk, uint32_t* __restrict__ hv, uint64_t mask) {
    uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= ne) return;
    unsigned long long key = hl_self[e] + 1;
    uint64_t slot = snk_mix64(key) & mask;
    for (;;) {
        unsigned long long old = atomicCAS(&hk[slot], 0ull, key);
        if (old == 0ull) { hv[slot] = (uint32_t)e; break; }
        slot = (slot + 1) & mask;
    }
}
__global__ void __launch_bounds__(TB) jmatch_kernel(const unsigned long long* __restrict__ hl_self, const unsigned long long* __restrict__ hl_nb,
                                                    uint64_t ne, const unsigned long long* __restrict__ hk, const uint32_t* __restrict__ hv,
                                                    uint64_t mask, uint32_t* __restrict__ flink) {
    uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= ne) return;
    unsigned long long nb = hl_nb[e];
    uint32_t out = NONE;
    if (nb != NONE64) {
        unsigned long long key = nb + 1;
        uint64_t slot = snk_mix64(key) & mask;
        for (;;) {
            unsigned long long h = hk[slot];
            if (h == 0ull) break;
            if (h == key) {
                uint32_t e2 = __hip_atomic_load(&hv[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (hl_nb[e2] == hl_self[e]) out = e2;      // the other owner points back at me: a link
                break;
            }
            slot = (slot + 1) & mask;
        }
    }
    flink[e] = out;
}

// one-GPU runs: every fragment end registered itself under its terminal state (sfrag[state] = 2*fragment + end), so the
// partner of a half link is one load away -- no hash table over the 2F ends.  Entries of non-terminal states are never
// written; a half link only ever names a terminal state, and the back-check below rejects anything else.
__global__ void __launch_bounds__(TB) jmatch_direct_kernel(const unsigned long long* __restrict__ hl_self,
                                                           const unsigned long long* __restrict__ hl_nb, uint64_t ne,
                                                           const uint32_t* __restrict__ sfrag, uint64_t n_states,
                                                           uint32_t* __restrict__ flink) {
    uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= ne) return;
    const unsigned long long nb = hl_nb[e];
    uint32_t out = NONE;
    if (nb != NONE64 && nb < n_states) {
        const uint32_t e2 = sfrag[nb];
        if (e2 < ne && hl_self[e2] == nb && hl_nb[e2] == hl_self[e]) out = e2;
    }
    flink[e] = out;
}

// ---- sharded runs: fragment links decided on the owners.  An end whose half link names a state of rank q asks q (24 bytes:
// target state, my state, my global end id | my local end << 32); q looks the state up in its terminal-state table and
// answers with the global id of the end that sits there and points back, or NONE.
// A workgroup takes RT_TILES tiles of TB items and goes to the per-owner device counters ONCE (count the tiles, reserve, then fill them):
// these cursors are a handful of words on one 64-byte line, atomics on one line are served one at a time (~10 ns each), and with a
// reservation per 256 items the 136 k workgroups of a 17 M-fragment rank WERE these kernels' time (1.65-1.76 ms each on one rank;
// times the number of owners on eight).
constexpr int RT_TILES = 16;
template <bool FILL>
__global__ void __launch_bounds__(TB) jlink_query_kernel(const unsigned long long* __restrict__ hl_self, const unsigned long long* __restrict__ hl_nb,
                                                         uint64_t ne, const unsigned long long* __restrict__ node_off, uint32_t world,
                                                         unsigned long long my_end_base, unsigned long long* __restrict__ qcount_or_cursor,
                                                         unsigned long long* __restrict__ qbuf) {
    extern __shared__ unsigned long long dynl[];          // [world] counts -> reserved bases, then [world] u32 local cursors
    uint32_t* lcur = reinterpret_cast<uint32_t*>(dynl + world);
    for (uint32_t r = threadIdx.x; r < world; r += TB) { dynl[r] = 0; lcur[r] = 0; }
    __syncthreads();
    const uint64_t e0 = (uint64_t)blockIdx.x * TB * RT_TILES + threadIdx.x;
    auto owner_of = [&](unsigned long long nb) { uint32_t o = 0; const unsigned long long node = nb >> 1; while (o + 1 < world && node >= node_off[o + 1]) ++o; return o; };
    for (int t = 0; t < RT_TILES; ++t) {
        const uint64_t e = e0 + (uint64_t)t * TB;
        const unsigned long long nb = e < ne ? hl_nb[e] : NONE64;
        if (nb != NONE64) atomicAdd(&dynl[owner_of(nb)], 1ull);
    }
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < world; r += TB) {
        const unsigned long long c = dynl[r];
        if (c) dynl[r] = FILL ? atomicAdd(&qcount_or_cursor[r], c) : (atomicAdd(&qcount_or_cursor[r], c), 0ull);
    }
    if (!FILL) return;
    __syncthreads();
    for (int t = 0; t < RT_TILES; ++t) {
        const uint64_t e = e0 + (uint64_t)t * TB;
        const unsigned long long nb = e < ne ? hl_nb[e] : NONE64;
        if (nb != NONE64) {
            const uint32_t owner = owner_of(nb);
            const unsigned long long slot = dynl[owner] + atomicAdd(&lcur[owner], 1u);
            qbuf[3 * slot + 0] = nb;
            qbuf[3 * slot + 1] = hl_self[e];
            qbuf[3 * slot + 2] = (my_end_base + e) | ((unsigned long long)e << 32);
        }
    }
}
__global__ void __launch_bounds__(TB) jlink_answer_kernel(const unsigned long long* __restrict__ q, uint64_t nq,
                                                          const unsigned long long* __restrict__ hl_self, const unsigned long long* __restrict__ hl_nb,
                                                          uint64_t ne, const uint32_t* __restrict__ sfrag, unsigned long long my_state_base,
                                                          uint64_t n_local_states, unsigned long long my_end_base, uint32_t* __restrict__ ans) {
    const uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (t >= nq) return;
    const unsigned long long target = q[3 * t], asker = q[3 * t + 1];
    uint32_t out = NONE;
    if (target >= my_state_base && target - my_state_base < n_local_states) {
        const uint32_t e2 = sfrag[target - my_state_base];
        if (e2 < ne && hl_self[e2] == target && hl_nb[e2] == asker) out = (uint32_t)(my_end_base + e2);
    }
    ans[t] = out;
}
__global__ void __launch_bounds__(TB) jlink_apply_kernel(const unsigned long long* __restrict__ q, const uint32_t* __restrict__ ans, uint64_t nq,
                                                         uint32_t* __restrict__ flink) {
    const uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (t >= nq) return;
    flink[(uint32_t)(q[3 * t + 2] >> 32)] = ans[t];
}

struct frag_place { uint32_t pid, other; uint64_t N; uint64_t koff; bool rc; };
__device__ __forceinline__ frag_place frag_place_of(const uint2* rk, const uint32_t* nk, uint64_t f) {
    const uint2 a = rk[2 * f], b = rk[2 * f + 1];
    uint32_t tL = a.y, tR = b.y;
    uint32_t dL = a.x, dR = b.x;
    frag_place p;
    p.N = (uint64_t)dL + dR + nk[f];
    if (tL < tR) { p.pid = tL; p.other = tR; p.koff = dL; p.rc = false; }
    else { p.pid = tR; p.other = tL; p.koff = dR; p.rc = true; }
    return p;
}
// Placement of the fragments [f0, f0 + Fl) of a ranked fragment list: the unitig a fragment belongs to is named by the
// smaller of its two terminal states (pid), koff = k-mers in front of it when the unitig is read from that end, rc = it
// is read from its right end.  The fragment whose own left/right state IS pid (koff == 0) heads the unitig; N = k-mers of
// the whole unitig.  Everything the emission needs -- the ranking itself stays behind (sharded runs rank the job's whole
// fragment list and place only their own fragments).
constexpr unsigned long long PL_RC = 1ull << 63;
// rk covers the fragments from rk_f0 on (0: the whole list; sharded runs with the partitioned ranking: this rank's own);
// circ == NULL: no circle was cut
__global__ void __launch_bounds__(TB) jplace_kernel(const uint2* __restrict__ rk, uint64_t rk_f0, const uint32_t* __restrict__ nk, const uint8_t* __restrict__ circ,
                                                    uint64_t f0, uint64_t Fl, uint32_t* __restrict__ pl_pid, unsigned long long* __restrict__ pl_koff,
                                                    unsigned long long* __restrict__ pl_N, uint8_t* __restrict__ pl_circ) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= Fl) return;
    const uint2 a = rk[2 * (f0 + i - rk_f0)], b = rk[2 * (f0 + i - rk_f0) + 1];
    const uint32_t w = nk[f0 + i];
    frag_place p;
    p.N = (uint64_t)a.x + b.x + w;
    if (a.y < b.y) { p.pid = a.y; p.other = b.y; p.koff = a.x; p.rc = false; }
    else { p.pid = b.y; p.other = a.y; p.koff = b.x; p.rc = true; }
    pl_pid[i] = p.pid;
    pl_koff[i] = p.koff | (p.rc ? PL_RC : 0ull);
    pl_N[i] = p.N;
    pl_circ[i] = circ ? circ[p.pid] : 0;
}
// gfid: global id of every fragment (NULL: fragment f is f); a head is the fragment that owns its unitig's terminal state
__global__ void __launch_bounds__(TB) jhead_kernel(const uint32_t* __restrict__ pl_pid, const unsigned long long* __restrict__ pl_koff,
                                                   const unsigned long long* __restrict__ pl_N, const uint32_t* __restrict__ gfid, uint64_t F, uint32_t K,
                                                   uint32_t* __restrict__ hflag, uint64_t* __restrict__ hlen) {
    uint64_t f = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (f >= F) return;
    const uint32_t me = gfid ? gfid[f] : (uint32_t)f;
    bool head = (pl_koff[f] & ~PL_RC) == 0 && (pl_pid[f] >> 1) == me;
    hflag[f] = head ? 1u : 0u;
    hlen[f] = head ? pl_N[f] + K - 1 : 0ull;
}
// poff is indexed by (pid - pid_base): the terminal states of this rank's own fragments (every unitig is emitted by the
// rank that owns its head fragment)
__global__ void __launch_bounds__(TB) jhead_place_kernel(const uint32_t* __restrict__ pl_pid, const uint8_t* __restrict__ pl_circ,
                                                         const uint32_t* __restrict__ hflag,
                                                         const uint32_t* __restrict__ hidx, const uint64_t* __restrict__ hoff,
                                                         uint64_t F, uint32_t pid_base, uint64_t* __restrict__ poff,
                                                         uint64_t* __restrict__ uoff, uint8_t* __restrict__ ucirc,
                                                         const uint32_t* __restrict__ fgroup, uint32_t* __restrict__ ugroup) {
    uint64_t f = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (f >= F || !hflag[f]) return;
    poff[pl_pid[f] - pid_base] = hoff[f];
    uoff[hidx[f]] = hoff[f];
    ucirc[hidx[f]] = pl_circ[f];
    if (fgroup) ugroup[hidx[f]] = fgroup[f];
}
// Base arrays are bytes (one per base) at arbitrary byte offsets.  A lane that moves one byte per instruction makes the copy
// kernels instruction-bound (a wave instruction moves 64 bytes); these move 4 / 16 bytes per lane with dword accesses at byte
// alignment (the device runs in unaligned-access mode; the packed struct tells the compiler so).
struct __attribute__((packed)) u32_any { uint32_t v; };
__device__ __forceinline__ uint32_t ld_u32_any(const uint8_t* p) { return reinterpret_cast<const u32_any*>(p)->v; }
__device__ __forceinline__ void st_u32_any(uint8_t* p, uint32_t v) { reinterpret_cast<u32_any*>(p)->v = v; }
// 16 bytes dst[0..16) = src[0..16), or (rev) the reverse complement of the 16 bytes that END at src_end: dst[j] = src_end[-1-j] ^ 3
__device__ __forceinline__ void copy16(uint8_t* dst, const uint8_t* src, bool rev) {
    if (!rev) {
        const uint32_t a = ld_u32_any(src), b = ld_u32_any(src + 4), c = ld_u32_any(src + 8), d = ld_u32_any(src + 12);
        st_u32_any(dst, a); st_u32_any(dst + 4, b); st_u32_any(dst + 8, c); st_u32_any(dst + 12, d);
    } else {
        const uint32_t a = ld_u32_any(src - 4), b = ld_u32_any(src - 8), c = ld_u32_any(src - 12), d = ld_u32_any(src - 16);
        st_u32_any(dst, __builtin_bswap32(a) ^ 0x03030303u); st_u32_any(dst + 4, __builtin_bswap32(b) ^ 0x03030303u);
        st_u32_any(dst + 8, __builtin_bswap32(c) ^ 0x03030303u); st_u32_any(dst + 12, __builtin_bswap32(d) ^ 0x03030303u);
    }
}
constexpr uint32_t JCH = 4096;            // bases per work item of the unitig copy kernels: 256 lanes x 16
// number of JCH-base chunks of every unitig (work items of the copy kernels)
__global__ void __launch_bounds__(TB) jchunks_kernel(const uint64_t* __restrict__ boff, uint64_t F, uint32_t* __restrict__ nch) {
    uint64_t f = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (f >= F) return;
    nch[f] = (uint32_t)((boff[f + 1] - boff[f] + JCH - 1) / JCH);
}
__global__ void __launch_bounds__(TB) jchunk_owner_kernel(const uint32_t* __restrict__ choff, uint64_t F, uint32_t* __restrict__ owner) {
    uint64_t f = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (f >= F) return;
    if (choff[f + 1] > choff[f]) owner[choff[f]] = (uint32_t)f;
}
// provisional unitig sequences: every fragment copies the bases it alone stands for.
// Fragments are short (K-1 + ~17 bases): 8 lanes per fragment, 32 fragments per workgroup, no per-chunk owner tables.
__global__ void __launch_bounds__(256) jemit_kernel(uint64_t F, const uint64_t* __restrict__ boff, const uint8_t* __restrict__ fbases,
                                                    const uint32_t* __restrict__ pl_pid, const unsigned long long* __restrict__ pl_koff,
                                                    const uint32_t* __restrict__ nk, const uint64_t* __restrict__ poff, uint32_t pid_base,
                                                    uint32_t K, uint8_t* __restrict__ prov) {
    // (a grid-stride loop: eight lanes per fragment are more work items than one launch may have -- 2^32 -- from 2^29 fragments on, and such a
    // launch is cut short without an error: found at 750 M reads on one GPU, tools/r6_full_job.py)
    for (uint64_t f = (uint64_t)blockIdx.x * 32 + (threadIdx.x >> 3); f < F; f += (uint64_t)gridDim.x * 32) {
    const uint32_t sub = threadIdx.x & 7u;
    const unsigned long long ko = pl_koff[f];
    const bool rc = (ko & PL_RC) != 0;                  // dst[p] = src[len - 1 - p] ^ 3
    // A fragment's first K-1 bases are the last K-1 of the fragment before it in the unitig: only the unitig's first fragment writes
    // them (round 4: every fragment copied all K-1 + ~15 of its bases -- 1.1 GB for 0.27 GB of unitigs).  In destination order the bases
    // that are left are [K-1, len): read forward from src + K-1, or backward from src + len - K (the same first `len` bytes of the code below).
    const uint32_t skip = (ko & ~PL_RC) == 0 ? 0u : K - 1;
    const uint32_t len = nk[f] + K - 1 - skip;
    const uint8_t* src = fbases + boff[f] + (rc ? 0u : skip);
    uint8_t* dst = prov + poff[pl_pid[f] - pid_base] + (ko & ~PL_RC) + skip;
    // bytes up to the first 4-byte boundary of dst, dwords, the last bytes
    uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
    if (head > len) head = len;
    if (sub < head) dst[sub] = rc ? (uint8_t)(src[len - 1 - sub] ^ 3u) : src[sub];
    const uint32_t ndw = (len - head) >> 2;
    for (uint32_t j = sub; j < ndw; j += 8) {
        const uint32_t o = head + 4 * j;
        const uint32_t v = rc ? (__builtin_bswap32(ld_u32_any(src + len - 4 - o)) ^ 0x03030303u) : ld_u32_any(src + o);
        *reinterpret_cast<uint32_t*>(dst + o) = v;
    }
    const uint32_t t0 = head + 4 * ndw;
    if (sub < len - t0) { const uint32_t q = t0 + sub; dst[q] = rc ? (uint8_t)(src[len - 1 - q] ^ 3u) : src[q]; }
    }
}
// canonical form of every unitig (dna/CanonicalForm.h:35-48) decided on the provisional sequence
__global__ void __launch_bounds__(TB) jform_kernel(const uint64_t* __restrict__ uoff, uint64_t U, const uint8_t* __restrict__ prov,
                                                   uint8_t* __restrict__ urev) {
    uint64_t u = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (u >= U) return;
    const uint8_t* b = prov + uoff[u];
    uint64_t len = uoff[u + 1] - uoff[u];
    uint8_t rev = 0;
    if (len & 1) rev = (b[len / 2] & 2) ? 1 : 0;
    else {
        for (uint64_t i = 0, j = len; i < j; ++i) {
            uint8_t f = b[i], r = (uint8_t)(b[--j] ^ 3);
            if (f < r) break;
            if (r < f) { rev = 1; break; }
        }
    }
    urev[u] = rev;
}
__global__ void __launch_bounds__(TB) jfinal_kernel(const uint64_t* __restrict__ uoff, const uint32_t* __restrict__ uowner_of_chunk,
                                                    const uint32_t* __restrict__ uchoff, const uint8_t* __restrict__ urev,
                                                    const uint8_t* __restrict__ prov, uint8_t* __restrict__ out) {
    const uint32_t item = blockIdx.x;
    const uint32_t u = uowner_of_chunk[item];
    const uint64_t len = uoff[u + 1] - uoff[u];
    const uint64_t p0 = (uint64_t)(item - uchoff[u]) * JCH + 16u * threadIdx.x;
    if (p0 >= len) return;
    const uint64_t o = uoff[u];
    const bool rev = urev[u] != 0;
    if (p0 + 16 <= len) copy16(out + o + p0, rev ? prov + o + len - p0 : prov + o + p0, rev);
    else for (uint64_t p = p0; p < len; ++p) out[o + p] = rev ? (uint8_t)(prov[o + len - 1 - p] ^ 3u) : prov[o + p];
}

__global__ void __launch_bounds__(TB) jcirc_list_kernel(const uint8_t* __restrict__ ucirc, uint64_t U, uint32_t* __restrict__ clist,
                                                        uint32_t* __restrict__ cnt) {
    uint64_t u = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (u < U && ucirc[u]) clist[atomicAdd(cnt, 1u)] = (uint32_t)u;
}
// One workgroup per circular unitig.  prov holds the closed sequence (N k-mers, N+K-1 bases, the last K-1 repeat the
// first K-1) cut at an arbitrary k-mer.  Reference form (canonicalizeCircle, BuildReadQGraph48.cc:375-397): the circle
// starts at its minimum canonical k-mer read forward.  Candidates: the k-mer at ring position j on strand 0, and its
// reverse complement, which sits at position (N-K-j) mod N of the reverse-complemented ring.
template <int K>
__global__ void __launch_bounds__(256) jcircle_kernel(const uint32_t* __restrict__ clist, const uint32_t* __restrict__ ccnt,
                                                      const uint64_t* __restrict__ uoff, uint8_t* __restrict__ prov, uint8_t* __restrict__ tmp) {
    __shared__ uint64_t bhi[256], blo[256];
    __shared__ uint32_t bpos[256];      // rotation << 1 | strand
    __shared__ uint32_t win;
    const uint32_t n_circ = *ccnt;      // the list's length stays on the device: the workgroups stride over it (no read-back for the grid)
    for (uint32_t c = blockIdx.x; c < n_circ; c += gridDim.x) {
    const uint32_t u = clist[c];
    const uint64_t o = uoff[u];
    const uint64_t len = uoff[u + 1] - o;
    const uint64_t N = len - (K - 1);
    uint8_t* ring = prov + o;
    const int tid = threadIdx.x;
    const uint64_t seg = (N + 255) / 256;
    const uint64_t a = (uint64_t)tid * seg, b = a + seg < N ? a + seg : N;
    snk_kmer best;
    best.hi = ~0ull; best.lo = ~0ull;
    uint32_t bp = 0xFFFFFFFFu;
    if (a < N) {
        snk_kmer f;
        f.hi = 0; f.lo = 0;
        for (int q = 0; q < K; ++q) f = snk_kmer_succ<K>(f, ring[a + q]);
        for (uint64_t j = a; j < b; ++j) {
            if (j > a) f = snk_kmer_succ<K>(f, ring[j + K - 1]);
            const snk_kmer r = snk_kmer_rc<K>(f);
            const uint32_t p0 = (uint32_t)j << 1;
            const uint32_t p1 = (uint32_t)((N - (K + j) % N) % N) << 1 | 1u;
            if (snk_kmer_lt(f, best) || (snk_kmer_eq(f, best) && p0 < bp)) { best = f; bp = p0; }
            if (snk_kmer_lt(r, best) || (snk_kmer_eq(r, best) && p1 < bp)) { best = r; bp = p1; }
        }
    }
    bhi[tid] = best.hi; blo[tid] = best.lo; bpos[tid] = bp;
    __syncthreads();
    if (tid == 0) {
        uint32_t w = 0;
        for (int t = 1; t < 256; ++t) {
            const bool lt = bhi[t] < bhi[w] || (bhi[t] == bhi[w] && (blo[t] < blo[w] || (blo[t] == blo[w] && bpos[t] < bpos[w])));
            if (lt) w = t;
        }
        win = bpos[w];
    }
    __syncthreads();
    const uint64_t i = win >> 1;
    const bool strand = win & 1u;
    uint8_t* t = tmp + o;
    for (uint64_t p = tid; p < len; p += 256) {
        if (!strand) t[p] = ring[(i + p) % N];
        else t[p] = (uint8_t)(ring[(2 * N - 1 - (i + p) % N) % N] ^ 3u);
    }
    __threadfence_block();
    __syncthreads();
    for (uint64_t p = tid; p < len; p += 256) ring[p] = t[p];
    __syncthreads();
    }
}

// deterministic output order: unitigs sorted by their first K bases (every k-mer belongs to exactly one unitig)
template <int K>
__global__ void __launch_bounds__(TB) jorder_key_kernel(const uint64_t* __restrict__ uoff, const uint8_t* __restrict__ bases, uint64_t U,
                                                        const uint32_t* __restrict__ ugroup, snk_u128* __restrict__ key,
                                                        uint32_t* __restrict__ idx) {
    uint64_t u = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (u >= U) return;
    const uint8_t* b = bases + uoff[u];
    snk_kmer f;
    f.hi = 0; f.lo = 0;
    for (int q = 0; q < K; ++q) f = snk_kmer_succ<K>(f, b[q]);
    snk_u128 k = ((snk_u128)f.hi << 64) | (snk_u128)f.lo;
    if (ugroup) k = ((snk_u128)ugroup[u] << 96) | (k >> 32);      // grouped runs (K=48: 96 key bits): group-major order
    key[u] = k;
    idx[u] = (uint32_t)u;
}
__global__ void __launch_bounds__(TB) jorder_len_kernel(const uint64_t* __restrict__ uoff, const uint32_t* __restrict__ idx, uint64_t U,
                                                        uint64_t* __restrict__ len) {
    uint64_t r = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (r > U) return;
    len[r] = r < U ? uoff[idx[r] + 1] - uoff[idx[r]] : 0ull;
}
__global__ void __launch_bounds__(256) jorder_copy_kernel(const uint32_t* __restrict__ owner, const uint32_t* __restrict__ choff,
                                                          const uint64_t* __restrict__ noff, const uint64_t* __restrict__ uoff,
                                                          const uint32_t* __restrict__ idx, const uint8_t* __restrict__ in,
                                                          const uint8_t* __restrict__ circ_in, uint8_t* __restrict__ out,
                                                          uint8_t* __restrict__ circ_out, const uint32_t* __restrict__ grp_in,
                                                          uint32_t* __restrict__ grp_out) {
    const uint32_t item = blockIdx.x;
    const uint32_t r = owner[item];
    const uint64_t len = noff[r + 1] - noff[r];
    const uint64_t p0 = (uint64_t)(item - choff[r]) * JCH + 16u * threadIdx.x;
    if (p0 == 0) { circ_out[r] = circ_in[idx[r]]; if (grp_in) grp_out[r] = grp_in[idx[r]]; }
    if (p0 >= len) return;
    const uint8_t* src = in + uoff[idx[r]] + p0;
    uint8_t* dst = out + noff[r] + p0;
    if (p0 + 16 <= len) copy16(dst, src, false);
    else for (uint64_t p = 0; p0 + p < len; ++p) dst[p] = src[p];
}

}  // namespace

// owner of every chunk from per-owner chunk counts: scatter the owner id at its first chunk, then max-scan
// total_ub != 0: an upper bound of the chunk count the caller knows without asking the device (sum of ceil(len / JCH) <= sum(len) / JCH
// + count): the tables are sized and the copy kernels launched for it -- no read-back; the owner of an item past the true total is the
// last owner, whose item then lies past its length, so the copy kernels' bound check drops it.
static int chunk_owners(snk_ctx* ctx, hipStream_t st, uint32_t* nch /*[count+1], last = 0*/, uint64_t count, uint32_t** choff_out,
                        uint32_t** owner_out, uint32_t* total_out, char* err, size_t errcap, uint64_t total_ub = 0) {
    uint32_t* choff;
    G_ALLOC(choff, uint32_t, count + 1);
    int rc = excl_scan<uint32_t>(ctx, st, nch, choff, count + 1, err, errcap);
    if (rc) return rc;
    uint32_t total = 0;
    if (total_ub) {
        if (total_ub > 0xFFFFFFF0ull) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "join: %llu copy chunks", (unsigned long long)total_ub);
        total = (uint32_t)total_ub;
    } else {
        SNK_HIP_TRY(hipMemcpyAsync(&total, choff + count, 4, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
    }
    uint32_t* owner;
    G_ALLOC(owner, uint32_t, (uint64_t)total + 1);
    SNK_HIP_TRY(hipMemsetAsync(owner, 0, ((uint64_t)total + 1) * 4, st));
    SNK_HIP_TRY(snk_launch(jchunk_owner_kernel, snk_blocks(count, TB), TB, 0, st, choff, count, owner));
    if (total) {
        size_t tb = 0;
        SNK_HIP_TRY(rocprim::inclusive_scan((void*)nullptr, tb, owner, owner, (size_t)total, rocprim::maximum<uint32_t>(), st));
        void* tmp;
        if ((rc = snk_ctx_alloc(ctx, tb, &tmp, err, errcap))) return rc;
        SNK_HIP_TRY(rocprim::inclusive_scan(tmp, tb, owner, owner, (size_t)total, rocprim::maximum<uint32_t>(), st));
    }
    *choff_out = choff;
    *owner_out = owner;
    *total_out = total;
    return SNK_OK;
}

int snk_dist_answer(snk_ctx* ctx, hipStream_t st, snk_dist_graph* g, const void* d_queries, uint64_t nq, void* d_ans, char* err,
                    size_t errcap) {
    SNK_HIP_TRY(snk_launch(answer_kernel, snk_blocks(nq, TB), TB, 0, st, (const unsigned long long*)d_queries, nq, g->keys, g->index, g->index_mask, (uint32_t*)d_ans));
    return SNK_OK;
}
int snk_dist_apply(snk_ctx* ctx, hipStream_t st, snk_dist_graph* g, const void* d_qbuf, const void* d_ans, uint64_t nq,
                   const unsigned long long* d_qoff, char* err, size_t errcap) {
    SNK_HIP_TRY(snk_launch(apply_answers_kernel, snk_blocks(nq, TB), TB, 0, st, (const unsigned long long*)d_qbuf, (const uint32_t*)d_ans, nq, d_qoff, g->world, g->do_prune, reinterpret_cast<uint32_t*>(g->ctx), g->rq_idx, g->rq_meta));
    return SNK_OK;
}

// all fragments of a job on one device (the one-GPU bucket-local stage) -> canonical unitigs
int snk_dist_join(snk_ctx* ctx, hipStream_t st, uint32_t K, uint64_t F, const uint32_t* nk, const unsigned long long* hl_self,
                  const unsigned long long* hl_nb, const uint64_t* boff, const uint8_t* fbases, uint64_t total_fbases,
                  snk_join_out* out, char* err, size_t errcap, const uint32_t* fgroup, const uint32_t* sfrag, uint64_t n_states) {
    memset(out, 0, sizeof *out);
    if (F == 0) return snk_join_emit(ctx, st, K, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, out, err, errcap);
    if (F >= (1ull << 31)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "more than 2^31 fragments at the join (%llu)", (unsigned long long)F);
    const uint64_t ne = 2 * F;
    uint32_t* flink;
    G_ALLOC(flink, uint32_t, ne);
    if (sfrag) {
        SNK_HIP_TRY(snk_launch(jmatch_direct_kernel, snk_blocks(ne, TB), TB, 0, st, hl_self, hl_nb, ne, sfrag, n_states, flink));
    } else {
        uint64_t tg = 1024;
        while (tg < 2 * ne) tg <<= 1;
        unsigned long long* hk;
        uint32_t* hv;
        G_ALLOC(hk, unsigned long long, tg);
        G_ALLOC(hv, uint32_t, tg);
        SNK_HIP_TRY(hipMemsetAsync(hk, 0, tg * 8, st));
        SNK_HIP_TRY(snk_launch(jhash_build_kernel, snk_blocks(ne, TB), TB, 0, st, hl_self, ne, hk, hv, tg - 1));
        SNK_HIP_TRY(snk_launch(jmatch_kernel, snk_blocks(ne, TB), TB, 0, st, hl_self, hl_nb, ne, hk, hv, tg - 1, flink));
    }
    uint8_t* circ;     // per fragment-end state: terminal created by cutting a circle
    G_ALLOC(circ, uint8_t, ne + 1);
    SNK_HIP_TRY(hipMemsetAsync(circ, 0, ne + 1, st));
    const uint2* rk;
    int rc = snk_rank_lists(ctx, st, flink, F, nk, circ, &rk, &out->n_circles, &out->rank_rounds, err, errcap);
    if (rc) return rc;
    snk_placement pl;
    if ((rc = snk_join_place(ctx, st, rk, nk, circ, 0, F, &pl, err, errcap))) return rc;
    const uint32_t nc = out->n_circles, rr = out->rank_rounds;
    if ((rc = snk_join_emit(ctx, st, K, F, nk, nullptr, pl.pid, pl.koff, pl.N, pl.circ, 0, ne, boff, fbases, fgroup, out, err, errcap))) return rc;
    out->n_circles = nc;
    out->rank_rounds = rr;
    return SNK_OK;
}

// ranking of a whole fragment list (sharded runs: every rank holds the job's links and k-mer counts) -- rk[2F], circ[2F]
int snk_join_rank(snk_ctx* ctx, hipStream_t st, uint64_t F, const uint32_t* nk, uint32_t* flink, const uint2** rk_out, uint8_t** circ_out,
                  uint32_t* n_circles, uint32_t* rounds, char* err, size_t errcap, uint8_t* circ_given, snk_rank_trace* trace) {
    if (F >= (1ull << 31)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "more than 2^31 fragments at the join (%llu)", (unsigned long long)F);
    uint8_t* circ = circ_given;          // given: the marks of circles an earlier (partitioned) attempt already cut in these links
    if (!circ) {
        G_ALLOC(circ, uint8_t, 2 * F + 1);
        SNK_HIP_TRY(hipMemsetAsync(circ, 0, 2 * F + 1, st));
    }
    *circ_out = circ;
    *n_circles = 0;
    *rounds = 0;
    if (F == 0) { *rk_out = nullptr; return SNK_OK; }
    return snk_rank_lists(ctx, st, flink, F, nk, circ, rk_out, n_circles, rounds, err, errcap, trace);
}

int snk_join_place(snk_ctx* ctx, hipStream_t st, const uint2* rk, const uint32_t* nk, const uint8_t* circ, uint64_t f0, uint64_t Fl,
                   snk_placement* pl, char* err, size_t errcap, uint64_t rk_f0) {
    memset(pl, 0, sizeof *pl);
    G_ALLOC(pl->pid, uint32_t, Fl + 1);
    G_ALLOC(pl->koff, unsigned long long, Fl + 1);
    G_ALLOC(pl->N, unsigned long long, Fl + 1);
    G_ALLOC(pl->circ, uint8_t, Fl + 1);
    SNK_HIP_TRY(snk_launch(jplace_kernel, snk_blocks(Fl, TB), TB, 0, st, rk, rk_f0, nk, circ, f0, Fl, pl->pid, pl->koff, pl->N, pl->circ));
    return SNK_OK;
}

// debugging aid (option join_dbg): bases outside 0..3 in a unitig buffer = bytes no fragment / copy wrote (the buffer is pre-filled with 0xEE)
__global__ void __launch_bounds__(256) jdbg_count_kernel(const uint8_t* __restrict__ b, uint64_t n, unsigned long long* __restrict__ out) {
    unsigned long long c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) c += b[i] > 3 ? 1ull : 0ull;
    if (c) atomicAdd(out, c);
}
static int jdbg_count(snk_ctx* ctx, hipStream_t st, const char* what, const uint8_t* b, uint64_t n, char* err, size_t errcap) {
    unsigned long long* d;
    G_ALLOC(d, unsigned long long, 1);
    SNK_HIP_TRY(hipMemsetAsync(d, 0, 8, st));
    SNK_HIP_TRY(snk_launch(jdbg_count_kernel, 4096, 256, 0, st, b, n, d));
    unsigned long long h = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&h, d, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    fprintf(stderr, "[snk join dbg] %s: %llu of %llu bytes are not bases\n", what, h, (unsigned long long)n);
    return SNK_OK;
}

// Emission of the unitigs whose head fragment is among the F fragments given (one-GPU runs: all of them; sharded runs:
// the fragments routed to this rank, the owner of their unitig's head): heads -> offsets, every fragment copied into
// place, circles rotated to the reference's cut, canonical orientation, deterministic order.
int snk_join_emit(snk_ctx* ctx, hipStream_t st, uint32_t K, uint64_t F, const uint32_t* nk, const uint32_t* gfid, const uint32_t* pl_pid,
                  const unsigned long long* pl_koff, const unsigned long long* pl_N, const uint8_t* pl_circ, uint32_t pid_base, uint64_t n_pid,
                  const uint64_t* boff, const uint8_t* fbases, const uint32_t* fgroup, snk_join_out* out, char* err, size_t errcap) {
    memset(out, 0, sizeof *out);
    if (F == 0) {
        G_ALLOC(out->unitig_off, uint64_t, 1);
        SNK_HIP_TRY(hipMemsetAsync(out->unitig_off, 0, 8, st));
        return SNK_OK;
    }
    int rc;
    uint32_t *hflag, *hidx;
    uint64_t *hlen, *hoff;
    G_ALLOC(hflag, uint32_t, F + 1);
    G_ALLOC(hidx, uint32_t, F + 1);
    G_ALLOC(hlen, uint64_t, F + 1);
    G_ALLOC(hoff, uint64_t, F + 1);
    SNK_HIP_TRY(hipMemsetAsync(hflag + F, 0, 4, st));
    SNK_HIP_TRY(hipMemsetAsync(hlen + F, 0, 8, st));
    SNK_HIP_TRY(snk_launch(jhead_kernel, snk_blocks(F, TB), TB, 0, st, pl_pid, pl_koff, pl_N, gfid, F, K, hflag, hlen));
    if ((rc = excl_scan<uint32_t>(ctx, st, hflag, hidx, F + 1, err, errcap))) return rc;
    if ((rc = excl_scan<uint64_t>(ctx, st, hlen, hoff, F + 1, err, errcap))) return rc;
    uint32_t h_nu = 0;
    uint64_t h_tot = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&h_nu, hidx + F, 4, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(hipMemcpyAsync(&h_tot, hoff + F, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    const uint64_t U = h_nu;
    const uint64_t chunks_ub = U ? h_tot / JCH + U : 0;      // both copy passes: every unitig's ceil(len / JCH), in either order
    uint64_t *poff, *uoff;
    uint8_t *ucirc, *prov, *final_bases, *urev;
    G_ALLOC(poff, uint64_t, n_pid + 1);
    G_ALLOC(uoff, uint64_t, U + 1);
    G_ALLOC(ucirc, uint8_t, U + 1);
    G_ALLOC(urev, uint8_t, U + 1);
    uint32_t* ugroup = nullptr;
    if (fgroup) G_ALLOC(ugroup, uint32_t, U + 1);
    G_ALLOC(prov, uint8_t, h_tot + 1);
    G_ALLOC(final_bases, uint8_t, h_tot + 1);
    const bool jdbg = snk_opt_u32(ctx, SNK_OPT_join_dbg) != 0;
    if (jdbg) { SNK_HIP_TRY(hipMemsetAsync(prov, 0xEE, h_tot + 1, st)); SNK_HIP_TRY(hipMemsetAsync(final_bases, 0xEE, h_tot + 1, st)); fprintf(stderr, "[snk join dbg] F %llu unitigs %llu bases %llu\n", (unsigned long long)F, (unsigned long long)U, (unsigned long long)h_tot); }
    SNK_HIP_TRY(snk_launch(jhead_place_kernel, snk_blocks(F, TB), TB, 0, st, pl_pid, pl_circ, hflag, hidx, hoff, F, pid_base, poff, uoff, ucirc, fgroup, ugroup));
    SNK_HIP_TRY(hipMemcpyAsync(uoff + U, hoff + F, 8, hipMemcpyDeviceToDevice, st));
    // copy every fragment into place
    SNK_HIP_TRY(snk_launch(jemit_kernel, snk_blocks_capped(F, 32, 1ull << std::min(22u, snk_opt_u32(ctx, SNK_OPT_emit_grid_log2))), 256, 0, st, F, boff, fbases, pl_pid, pl_koff, nk, poff, pid_base, K, prov));
    if (jdbg && (rc = jdbg_count(ctx, st, "provisional bases after the fragments' copies", prov, h_tot, err, errcap))) return rc;
    // circles that were cut at an arbitrary fragment boundary: rotate to the reference's cut (minimum k-mer, forward)
    {
        uint32_t *clist, *ccnt;
        G_ALLOC(clist, uint32_t, U + 1);
        G_ALLOC(ccnt, uint32_t, 4);
        SNK_HIP_TRY(hipMemsetAsync(ccnt, 0, 4, st));
        SNK_HIP_TRY(snk_launch(jcirc_list_kernel, snk_blocks(U, TB), TB, 0, st, ucirc, U, clist, ccnt));
        const uint64_t cg = U < 1024 ? U : 1024;
        if (K == 48) SNK_HIP_TRY(snk_launch(jcircle_kernel<48>, cg, 256, 0, st, clist, ccnt, uoff, prov, final_bases));
        else SNK_HIP_TRY(snk_launch(jcircle_kernel<60>, cg, 256, 0, st, clist, ccnt, uoff, prov, final_bases));
    }
    SNK_HIP_TRY(snk_launch(jform_kernel, snk_blocks(U, TB), TB, 0, st, uoff, U, prov, urev));
    uint32_t *unch, *uchoff, *uowner, utotal = 0;
    G_ALLOC(unch, uint32_t, U + 1);
    SNK_HIP_TRY(hipMemsetAsync(unch + U, 0, 4, st));
    SNK_HIP_TRY(snk_launch(jchunks_kernel, snk_blocks(U, TB), TB, 0, st, uoff, U, unch));
    if ((rc = chunk_owners(ctx, st, unch, U, &uchoff, &uowner, &utotal, err, errcap, chunks_ub))) return rc;
    SNK_HIP_TRY(snk_launch(jfinal_kernel, utotal, 256, 0, st, uoff, uowner, uchoff, urev, prov, final_bases));
    if (jdbg && (rc = jdbg_count(ctx, st, "oriented bases", final_bases, h_tot, err, errcap))) return rc;
    // deterministic order (fragment ids depend on the order in which workgroups reserved their output)
    uint64_t* noff = uoff;
    uint8_t* obases = final_bases;
    uint8_t* ocirc = ucirc;
    uint32_t* ogroup = ugroup;
    if (U > 1) {
        snk_u128 *ok_in, *ok_out;
        uint32_t *oi_in, *oi_out;
        uint64_t* olen;
        G_ALLOC(ok_in, snk_u128, U + 1);
        G_ALLOC(ok_out, snk_u128, U + 1);
        G_ALLOC(oi_in, uint32_t, U + 1);
        G_ALLOC(oi_out, uint32_t, U + 1);
        G_ALLOC(olen, uint64_t, U + 1);
        G_ALLOC(noff, uint64_t, U + 1);
        G_ALLOC(ocirc, uint8_t, U + 1);
        if (ugroup) G_ALLOC(ogroup, uint32_t, U + 1);
        obases = prov;         // the provisional buffer is dead: reuse it for the ordered copy
        if (K == 48) SNK_HIP_TRY(snk_launch(jorder_key_kernel<48>, snk_blocks(U, TB), TB, 0, st, uoff, final_bases, U, (const uint32_t*)ugroup, ok_in, oi_in));
        else SNK_HIP_TRY(snk_launch(jorder_key_kernel<60>, snk_blocks(U, TB), TB, 0, st, uoff, final_bases, U, (const uint32_t*)ugroup, ok_in, oi_in));
        {
            size_t tb = 0;
            SNK_HIP_TRY(rocprim::radix_sort_pairs((void*)nullptr, tb, ok_in, ok_out, oi_in, oi_out, (size_t)U, 0u, 128u, st));
            void* tmp;
            if ((rc = snk_ctx_alloc(ctx, tb, &tmp, err, errcap))) return rc;
            SNK_HIP_TRY(rocprim::radix_sort_pairs(tmp, tb, ok_in, ok_out, oi_in, oi_out, (size_t)U, 0u, 128u, st));
        }
        SNK_HIP_TRY(snk_launch(jorder_len_kernel, snk_blocks(U + 1, TB), TB, 0, st, uoff, oi_out, U, olen));
        if ((rc = excl_scan<uint64_t>(ctx, st, olen, noff, U + 1, err, errcap))) return rc;
        uint32_t *onch, *ochoff, *oowner, ototal = 0;
        G_ALLOC(onch, uint32_t, U + 1);
        SNK_HIP_TRY(hipMemsetAsync(onch + U, 0, 4, st));
        SNK_HIP_TRY(snk_launch(jchunks_kernel, snk_blocks(U, TB), TB, 0, st, noff, U, onch));
        if ((rc = chunk_owners(ctx, st, onch, U, &ochoff, &oowner, &ototal, err, errcap, chunks_ub))) return rc;
        if (jdbg) SNK_HIP_TRY(hipMemsetAsync(obases, 0xEE, h_tot + 1, st));
        SNK_HIP_TRY(snk_launch(jorder_copy_kernel, ototal, 256, 0, st, oowner, ochoff, noff, uoff, oi_out, final_bases, ucirc, obases, ocirc, (const uint32_t*)ugroup, ogroup));
        if (jdbg && (rc = jdbg_count(ctx, st, "ordered bases", obases, h_tot, err, errcap))) return rc;
    }
    // nothing is waited for here: the unitigs are stream-ordered results, the step's closing wait is the caller's
    out->n_unitigs = U;
    out->total_bases = h_tot;
    out->unitig_off = noff;
    out->unitig_bases = obases;
    out->unitig_circular = ocirc;
    out->unitig_group = ogroup;
    return SNK_OK;
}

// k-mer spectrum with as many bins as the largest (saturated) count needs -- WriteKmerSpectrum grows its vector to
// count+1 (BuildReadQGraph48.cc:199-216); at least 65536 bins
int snk_spectrum(snk_ctx* ctx, hipStream_t st, const uint32_t* counts, uint64_t n, unsigned long long** bins_out, uint32_t* nbins_out,
                 char* err, size_t errcap) {
    uint32_t h_max = 0;
    if (n) {
        uint32_t* d_max;
        G_ALLOC(d_max, uint32_t, 4);
        size_t tb = 0;
        SNK_HIP_TRY(rocprim::reduce((void*)nullptr, tb, counts, d_max, 0u, (size_t)n, rocprim::maximum<uint32_t>(), st));
        void* tmp;
        int rc = snk_ctx_alloc(ctx, tb, &tmp, err, errcap);
        if (rc) return rc;
        SNK_HIP_TRY(rocprim::reduce(tmp, tb, counts, d_max, 0u, (size_t)n, rocprim::maximum<uint32_t>(), st));
        SNK_HIP_TRY(hipMemcpyAsync(&h_max, d_max, 4, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
    }
    if (h_max > 0xFFFFFFu) h_max = 0xFFFFFFu;
    const uint32_t nbins = h_max + 1 > 65536u ? h_max + 1 : 65536u;
    unsigned long long* bins;
    G_ALLOC(bins, unsigned long long, nbins);
    SNK_HIP_TRY(hipMemsetAsync(bins, 0, (size_t)nbins * 8, st));
    if (n) SNK_HIP_TRY(snk_launch(spectrum_kernel, snk_blocks_capped(n, TB, 2048), TB, 0, st, counts, n, bins, nbins));
    *bins_out = bins;
    *nbins_out = nbins;
    return SNK_OK;
}

// ---- sharded runs: link matching on the owners
int snk_dist_links_query(snk_ctx* ctx, hipStream_t st, const snk_frag_out* fr, const unsigned long long* d_node_off, uint32_t world,
                         unsigned long long my_end_base, unsigned long long* d_cursor, void* d_qbuf, char* err, size_t errcap) {
    const uint64_t ne = 2 * fr->n_frags;
    if (ne == 0) return SNK_OK;
    if (ne >= (1ull << 32)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "more than 2^31 fragments on one rank");
    const size_t lds = (size_t)world * 12 + 16;
    SNK_HIP_TRY(snk_launch(jlink_query_kernel<true>, snk_blocks(snk_blocks(ne, RT_TILES), TB), TB, lds, st, fr->hl_self, fr->hl_nb, ne, d_node_off, world, my_end_base, d_cursor, (unsigned long long*)d_qbuf));
    return SNK_OK;
}
int snk_dist_links_answer(snk_ctx* ctx, hipStream_t st, const snk_frag_out* fr, const void* d_queries, uint64_t nq, unsigned long long my_state_base,
                          uint64_t n_local_states, unsigned long long my_end_base, void* d_ans, char* err, size_t errcap) {
    SNK_HIP_TRY(snk_launch(jlink_answer_kernel, snk_blocks(nq, TB), TB, 0, st, (const unsigned long long*)d_queries, nq, fr->hl_self, fr->hl_nb,
                           2 * fr->n_frags, fr->sfrag, my_state_base, n_local_states, my_end_base, (uint32_t*)d_ans));
    return SNK_OK;
}
// the answers applied: queries / answers sit in per-destination regions of `cap` items (one-pass routing, snk_shard_step.hip)
int snk_dist_links_apply_regions(snk_ctx* ctx, hipStream_t st, const snk_frag_out* fr, const void* d_qbuf, const void* d_ans, uint32_t world, uint64_t cap,
                                 const unsigned long long* counts, uint32_t** flink_out, char* err, size_t errcap) {
    const uint64_t ne = 2 * fr->n_frags;
    uint32_t* flink;
    G_ALLOC(flink, uint32_t, ne + 2);
    SNK_HIP_TRY(hipMemsetAsync(flink, 0xFF, (ne + 2) * 4, st));
    for (uint32_t p = 0; p < world; ++p)
        SNK_HIP_TRY(snk_launch(jlink_apply_kernel, snk_blocks(counts[p], TB), TB, 0, st, (const unsigned long long*)d_qbuf + 3 * cap * p,
                               (const uint32_t*)d_ans + cap * p, (uint64_t)counts[p], flink));
    *flink_out = flink;
    return SNK_OK;
}

