// snk_mow.hip -- MowLawn on the device (10X/Lawnmower.cc:301-554, the ReadPathVecX overload that StageTrim calls,
// 10X/runstages/RunStages.cc:84): the weak-branch rule that picks the first and larger batch of StageTrim's deletions.  include/snk.h,
// "snk_dev_mow_lawn", states the semantics.
//
// The reference goes candidate by candidate and reads, through the paths index, every read on e1, e2 and their inverses.  Two facts let
// the device go read by read instead, with no index: a group of records keeps only its extremes, so a read that the index names k
// times counts once per path entry; and an entry whose read does not reach the window [0, n) gives q1 = q2 = 0 and no record, so the
// window test -- arithmetic on the offset, the read's length, del and n -- runs before a base or a quality is loaded.  Only npe counts
// with multiplicity, and "the entries equal to e2 or inv[e2]" is that count.
//
// Passes.
//   host             the candidates (v, e1, e2) from the From / To lists, ascending by e2, and per edge its four roles: e1, e2, inv[e1] and
//                    inv[e2] of which candidate (an edge has at most one of each: e1 names its right vertex, whose other in-edge is e2).
//                    Edge-sized work, as the rule of snk_dev_hanging_ends.
//   m_limit_kernel   one lane per read that is no dup: an entry on e2 or inv[e2] of candidate c adds one to npe[c] -- an integer sum, the
//                    only thing an atomic does here.  A read none of whose entries has a role (nearly all) loads one role record per entry.
//   m_items_kernel   the same walk twice (count, scan, write): every (entry, role) of a candidate with npe <= 2 at a position the rule takes,
//                    whose read reaches the window, becomes a work item (read, candidate | pass | fw, first epos, offset_l), in the order of
//                    the reads, then of the entries.  A long e1 with hundreds of thousands of entries is so many items, not one wave's work.
//   m_score_kernel   four lanes per item.  The quality filter is MarkBads's comparison (snk_bads.hip) with another tally: the same XOR of 16
//                    read bases against pg_edge16, the same masks, the same walk forward through the pieces of Cat(path); it counts the
//                    mismatches of quality >= 30 where MarkBads sums qualities.  The window is two more XORs, against x1 and x2, over the
//                    read as the record orients it.  The sums are shuffles.  A record is the key (candidate, fw, offset_l) and q1 - q2.
//   sort, reduce     the library's radix sort by key; one reduce-by-key leaves each group's smallest and largest difference, a kernel turns
//                    them into the group's value for z1 or z2, two more reduce-by-keys leave per candidate (sum, max) of either: qss = sum -
//                    max.  All integers, so the order of the reduction does not show.
//   host             the two thresholds over the candidates, `scored` and the deleted edges.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "snk_bads.h"
#include "snk_call.h"
#include "snk_common.h"
#include "snk_pathgraph.h"

namespace {

constexpr unsigned MB = 256;                     // lanes of a workgroup
constexpr unsigned LPI = 4, IPB = MB / LPI;      // lanes per work item (as MarkBads takes four per mate), items per workgroup and step
constexpr uint64_t M_GRID_CAP = 1u << 20;
constexpr int MAX_READS2 = 2, MAX_QS = 50, MIN_QS_RIGHT = 300, MAX_QS_WRONG = 30, MAX_HQ_DIFFS = 5, MIN_HQ = 30;      // Lawnmower.cc:309-314
constexpr uint32_t IT_FW = 1u << 31, IT_PASS2 = 1u << 30, IT_CAND = IT_PASS2 - 1;
constexpr unsigned long long NO_RECORD = ~0ull;
enum { N_ON_CAND, N_IN_WINDOW, N_HQ_EXCLUDED, N_RECORDS, N_MIXED, N_COUNTED, N_COUNTERS = 8 };

struct m_paths {
    uint64_t n;
    const unsigned long long* start;
    const uint32_t* n_edges;
    const int32_t* offset;
    const uint32_t* edges;
};
struct m_cands {                                 // per candidate, ascending by e2; per edge
    const int32_t *e1, *e2;
    const uint32_t *n, *del;                     // Kmers(e2); Kmers(e1) - Kmers(e2)
    const int4* role;                            // [E] the candidate this edge is e1 (x), e2 (y), inv[e1] (z), inv[e2] (w) of, or -1
    const uint32_t* kmers;                       // [E]
    const uint32_t* npe;                         // [C]
};

// the counters of a workgroup: one atomic each
__device__ __forceinline__ void m_flush(const uint32_t (&cnt)[N_COUNTED], uint32_t (*l_cnt)[N_COUNTED], unsigned long long* counters) {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N_COUNTED; ++k) {
        uint32_t v = cnt[k];
        for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
        if ((tid & 63) == 0) l_cnt[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < N_COUNTED) {
        uint32_t v = 0;
        for (unsigned w = 0; w < MB / 64; ++w) v += l_cnt[w][tid];
        if (v) atomicAdd(&counters[tid], (unsigned long long)v);
    }
}

__global__ void __launch_bounds__(MB) m_limit_kernel(m_paths P, const uint8_t* __restrict__ dup, const int4* __restrict__ role, uint32_t* __restrict__ npe) {
    for (uint64_t r = (uint64_t)blockIdx.x * MB + threadIdx.x; r < P.n; r += (uint64_t)gridDim.x * MB) {
        const uint32_t m = P.n_edges[r];
        if (!m || dup[r >> 1]) continue;
        const uint64_t s = P.start[r];
        for (uint32_t j = 0; j < m; ++j) {
            const int4 ro = role[P.edges[s + j]];
            if (ro.y >= 0) atomicAdd(npe + ro.y, 1u);
            if (ro.w >= 0) atomicAdd(npe + ro.w, 1u);
        }
    }
}

template <bool WRITE>
__global__ void __launch_bounds__(MB) m_items_kernel(m_paths P, snk_reads_view R, const uint8_t* __restrict__ dup, m_cands Q, int K, uint32_t* __restrict__ n_items,
                                                     const unsigned long long* __restrict__ pos, uint4* __restrict__ items, unsigned long long* __restrict__ counters) {
    __shared__ uint32_t l_cnt[MB / 64][N_COUNTED];
    uint32_t cnt[N_COUNTED] = {0, 0, 0, 0, 0};
    for (uint64_t r = (uint64_t)blockIdx.x * MB + threadIdx.x; r <= P.n; r += (uint64_t)gridDim.x * MB) {
        if (r == P.n) { if (!WRITE) n_items[r] = 0; continue; }
        const uint32_t m = P.n_edges[r];
        uint32_t mine = 0;
        if (m && !dup[r >> 1]) {
            const uint64_t s = P.start[r];
            bool any = false;
            for (uint32_t l = 0; l < m && !any; ++l) {
                const int4 ro = Q.role[P.edges[s + l]];
                any = (ro.x & ro.y & ro.z & ro.w) >= 0;
            }
            if (any) {
                const int len = (int)snk_read_len(R, r);
                int offl = (int)(int16_t)P.offset[r];                      // (ReadPathParser.cc:184-198: the record holds static_cast<int16_t>)
                uint4* out = WRITE ? items + pos[r] : nullptr;
                for (uint32_t l = 0; l < m; ++l) {
                    const uint32_t x = P.edges[s + l];
                    const int4 ro = Q.role[x];
                    const int cs[4] = {ro.x, ro.y, ro.z, ro.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int c = cs[k];
                        const bool fw = k < 2, pass2 = k & 1;
                        if (c < 0 || (fw ? l + 1 >= m : l == 0) || Q.npe[c] > (uint32_t)MAX_READS2) continue;
                        ++cnt[N_ON_CAND];
                        const long long n = Q.n[c], dl = pass2 ? 0 : Q.del[c];
                        const long long first = fw ? (long long)offl - dl : n + K - 1 - (long long)offl - len;      // epos of the oriented read's base 0
                        if (len <= 0 || first >= n || first + len <= 0) continue;
                        ++cnt[N_IN_WINDOW];
                        if (WRITE) out[mine] = make_uint4((uint32_t)r, (uint32_t)c | (fw ? IT_FW : 0u) | (pass2 ? IT_PASS2 : 0u), (uint32_t)(int32_t)first, (uint32_t)offl);
                        ++mine;
                    }
                    offl -= (int)Q.kmers[x];
                }
            }
        }
        if (!WRITE) n_items[r] = mine;
    }
    if (!WRITE) m_flush(cnt, l_cnt, counters);
}

__global__ void __launch_bounds__(MB) m_score_kernel(path_graph G, snk_reads_view R, m_paths P, m_cands Q, int K, const uint4* __restrict__ items, uint64_t n_items,
                                                     unsigned long long* __restrict__ key, int32_t* __restrict__ val, unsigned long long* __restrict__ counters) {
    __shared__ uint32_t l_cnt[MB / 64][N_COUNTED];
    const uint32_t tid = threadIdx.x, q = tid & (LPI - 1);
    uint32_t cnt[N_COUNTED] = {0, 0, 0, 0, 0};
    // every lane of a workgroup makes the same number of steps: the shuffles below are reached by whole waves
    for (uint64_t base = (uint64_t)blockIdx.x * IPB; base < n_items; base += (uint64_t)gridDim.x * IPB) {
        const uint64_t i = base + tid / LPI;
        const bool on = i < n_items;
        int q30 = 0, q1 = 0, q2 = 0;
        uint4 it = make_uint4(0, 0, 0, 0);
        if (on) {
            it = items[i];
            const uint64_t r = it.x;
            const uint32_t c = it.y & IT_CAND;
            const bool fw = it.y & IT_FW;
            const int len = (int)snk_read_len(R, r);
            const uint32_t* row = R.rows + r * R.row_words;
            const uint8_t* qual = R.quals + r * R.qstride;
            // ---- the filter: the read at its path's offset against Cat(path), piece by piece (snk_bads.hip)
            {
                const uint32_t m = P.n_edges[r];
                const int off = (int)(int16_t)P.offset[r];
                const uint64_t s = P.start[r];
                uint32_t j = 0;
                pg_edge x = pg_edge_load(G, P.edges[s]);
                long long S = 0, b = m > 1 ? (long long)x.len - (K - 1) : (long long)x.len;
                for (int w = (int)q; 16 * w < len && j < m; w += (int)LPI) {
                    long long lo = (long long)off + 16 * w;
                    const long long hi = lo + min(16, len - 16 * w);
                    if (hi <= 0) continue;
                    if (lo < 0) lo = 0;
                    const uint32_t word = row[w];
                    while (lo < hi) {
                        while (b <= lo && ++j < m) {
                            S = b;
                            x = pg_edge_load(G, P.edges[s + j]);
                            b = S + (j + 1 < m ? (long long)x.len - (K - 1) : (long long)x.len);
                        }
                        if (j >= m) break;
                        const long long top = hi < b ? hi : b;
                        const int rp = (int)(lo - off);
                        uint32_t d = (word << (2 * (rp - 16 * w))) ^ pg_edge16(G, x, (uint32_t)(lo - S));
                        d = (d | (d << 1)) & 0xAAAAAAAAu;
                        const uint32_t n16 = (uint32_t)(top - lo);
                        if (n16 < 16) d &= ~(0xFFFFFFFFu >> (2 * n16));
                        while (d) {
                            const int g = __clz((int)d) >> 1;
                            q30 += qual[rp + g] >= MIN_HQ ? 1 : 0;
                            d &= ~(0x80000000u >> (2 * g));
                        }
                        lo = top;
                    }
                }
            }
            // ---- the window: bases [16 w, 16 w + 16) of the read as the record orients it, at epos = first + position
            {
                const long long n = Q.n[c], del = Q.del[c], first = (int32_t)it.z;
                const pg_edge x1 = pg_edge_load(G, Q.e1[c]), x2 = pg_edge_load(G, Q.e2[c]);
                for (int w = (int)q; 16 * w < len; w += (int)LPI) {
                    const int cnt16 = min(16, len - 16 * w);
                    const long long e0 = first + 16 * w;
                    const long long a = e0 < 0 ? 0 : e0, bnd = e0 + cnt16 < n ? e0 + cnt16 : n;
                    if (a >= bnd) continue;
                    uint32_t rb;
                    if (fw) rb = row[w];
                    else {
                        // the reverse complement's bases 16 w .. are the read's bases len - 1 - 16 w downwards
                        const int p0 = len - 16 - 16 * w;
                        const uint32_t t = p0 >= 0 ? snk_row16(row, R.row_words, (uint32_t)p0) : snk_row16(row, R.row_words, 0u) >> (2 * -p0);
                        rb = ~snk_rev2_32(t);
                    }
                    const int sh = (int)(a - e0);                           // slots of the word in front of the window
                    rb <<= 2 * sh;
                    const uint32_t n16 = (uint32_t)(bnd - a);
                    const uint32_t keep = n16 < 16 ? ~(0xFFFFFFFFu >> (2 * n16)) : 0xFFFFFFFFu;
                    uint32_t d1 = rb ^ pg_edge16(G, x1, (uint32_t)(del + a)), d2 = rb ^ pg_edge16(G, x2, (uint32_t)a);
                    d1 = (d1 | (d1 << 1)) & 0xAAAAAAAAu & keep;
                    d2 = (d2 | (d2 << 1)) & 0xAAAAAAAAu & keep;
                    uint32_t d = d1 | d2;
                    while (d) {
                        const int g = __clz((int)d) >> 1;
                        const uint32_t bit = 0x80000000u >> (2 * g);
                        const int mpos = 16 * w + sh + g;                   // position in the oriented read
                        const int qv = qual[fw ? mpos : len - 1 - mpos];
                        if (d1 & bit) q1 += qv;
                        if (d2 & bit) q2 += qv;
                        d &= ~bit;
                    }
                }
            }
        }
        q30 += __shfl_xor(q30, 1); q30 += __shfl_xor(q30, 2);
        q1 += __shfl_xor(q1, 1); q1 += __shfl_xor(q1, 2);
        q2 += __shfl_xor(q2, 1); q2 += __shfl_xor(q2, 2);
        if (on && q == 0) {
            const bool excluded = q30 >= MAX_HQ_DIFFS, rec = !excluded && q1 != q2;
            key[i] = rec ? ((unsigned long long)(it.y & IT_CAND) << 33) | ((unsigned long long)(it.y >> 31) << 32) | it.w : NO_RECORD;
            val[i] = q1 - q2;
            cnt[N_HQ_EXCLUDED] += excluded ? 1u : 0u;
            cnt[N_RECORDS] += rec ? 1u : 0u;
        }
    }
    m_flush(cnt, l_cnt, counters);
}

// ---- the reductions.  A pair of 32-bit values rides in one 64-bit word, so the library's reduce-by-key takes them as integers.
struct m_minmax {                                // (smallest, largest) difference of a group, each biased by 2^31
    __host__ __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const {
        const uint32_t lo = min((uint32_t)(a >> 32), (uint32_t)(b >> 32)), hi = max((uint32_t)a, (uint32_t)b);
        return ((unsigned long long)lo << 32) | hi;
    }
};
struct m_summax {                                // (sum << 8 | largest) of the group values of a candidate, a value being at most MAX_QS
    __host__ __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const {
        return (((a >> 8) + (b >> 8)) << 8) | max(a & 0xFFull, b & 0xFFull);
    }
};
struct u32_to_u64 { __host__ __device__ unsigned long long operator()(uint32_t x) const { return x; } };
struct m_both { __host__ __device__ unsigned long long operator()(int32_t v) const { const unsigned long long b = (uint32_t)v ^ 0x80000000u; return (b << 32) | b; } };

// one lane per group: its value goes to z1 (negative) or z2 (positive), as (value << 8 | value); a group of both signs counts for nothing
__global__ void __launch_bounds__(MB) m_groups_kernel(const unsigned long long* __restrict__ gkey, const unsigned long long* __restrict__ gmm, uint64_t n_groups,
                                                      uint32_t* __restrict__ ckey, unsigned long long* __restrict__ z1, unsigned long long* __restrict__ z2,
                                                      unsigned long long* __restrict__ counters) {
    __shared__ uint32_t l_cnt[MB / 64][N_COUNTED];
    uint32_t cnt[N_COUNTED] = {0, 0, 0, 0, 0};
    for (uint64_t g = (uint64_t)blockIdx.x * MB + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * MB) {
        const unsigned long long mm = gmm[g];
        const int lo = (int)((uint32_t)(mm >> 32) ^ 0x80000000u), hi = (int)((uint32_t)mm ^ 0x80000000u);
        unsigned long long a = 0, b = 0;
        if (lo > 0) { const unsigned long long v = (unsigned long long)min(hi, MAX_QS); b = (v << 8) | v; }                     // (:523-526: no record is zero)
        else if (hi < 0) { const unsigned long long v = (unsigned long long)min(-(long long)lo, (long long)MAX_QS); a = (v << 8) | v; }
        else ++cnt[N_MIXED];
        ckey[g] = (uint32_t)(gkey[g] >> 33);
        z1[g] = a; z2[g] = b;
    }
    m_flush(cnt, l_cnt, counters);
}
__global__ void __launch_bounds__(MB) m_qss_kernel(const uint32_t* __restrict__ ukey, const unsigned long long* __restrict__ s1, const unsigned long long* __restrict__ s2,
                                                   uint64_t n, int32_t* __restrict__ qss) {
    for (uint64_t j = (uint64_t)blockIdx.x * MB + threadIdx.x; j < n; j += (uint64_t)gridDim.x * MB) {
        const uint64_t c = ukey[j];
        qss[2 * c] = (int32_t)((s1[j] >> 8) - (s1[j] & 0xFFull));
        qss[2 * c + 1] = (int32_t)((s2[j] >> 8) - (s2[j] & 0xFFull));
    }
}

template <typename T>
int m_up(snk_call& c, const std::vector<T>& h, const T** out, char* err, size_t errcap) {
    T* d;
    const int rc = c.alloc(h.size(), &d);
    if (rc) return rc;
    if (!h.empty()) SNK_HIP_TRY(hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, c.st));
    *out = d;
    return SNK_OK;
}

struct mow_host {
    path_host H;
    std::vector<uint64_t> uoff;
    std::vector<uint32_t> kmers, cn, cdel, npe;
    std::vector<int32_t> ce1, ce2, qss, scored, dels;
    std::vector<int4> role;
};

int mow_impl(snk_call& c, mow_host& M, uint32_t K, uint64_t U, const void* d_uoff, const void* d_ub, const snk_hbv* h, const int32_t* inv, const snk_dev_reads* in,
             const snk_dev_paths* paths, const uint8_t* d_dup, snk_dev_mow* out, char* err, size_t errcap) {
    static const char who[] = "snk_dev_mow_lawn";
    const hipStream_t st = c.st;
    int rc;
    SNK_HIP_TRY(c.stamp());
    const uint64_t n = in->n_reads, E = (uint64_t)h->n_edges, N = (uint64_t)h->n_vertices;
    // ---- the graph tables and the refusals of a ReadPathVecX (the path table, the edge ids, what zip would not give back)
    bads_job job;
    if ((rc = snk_bads_begin(c, M.H, who, K, n, U, d_uoff, d_ub, h, paths, SNK_BADS_X, &job, err, errcap))) return rc;
    SNK_HIP_TRY(c.stamp());
    // ---- the candidates (Lawnmower.cc:407-416)
    const auto t0 = std::chrono::steady_clock::now();
    M.uoff.assign(U + 1, 0);
    if (U) SNK_HIP_TRY(hipMemcpyAsync(M.uoff.data(), d_uoff, (U + 1) * 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    M.kmers.resize(E);
    for (uint64_t e = 0; e < E; ++e) {
        const uint64_t u = (uint64_t)M.H.eu[e], len = M.uoff[u + 1] - M.uoff[u];
        if (M.uoff[u + 1] < M.uoff[u] || len < K || len > 0x7FFFFFFFull) return snk_fail(SNK_E_ARG, err, errcap, "%s: edge %llu has fewer than K bases, or 2^31 or more", who, (unsigned long long)e);
        M.kmers[e] = (uint32_t)len - K + 1;
    }
    const std::vector<int32_t>&off_to = M.H.off_to, &e_to = M.H.e_to, &off_from = M.H.off_from;
    std::vector<std::pair<int32_t, int32_t>> cand;      // (e2, e1)
    for (uint64_t v = 0; v < N; ++v) {
        if (off_to[v + 1] - off_to[v] != 2 || off_from[v + 1] - off_from[v] != 1) continue;
        for (int jj = 0; jj < 2; ++jj) {
            const int32_t e1 = e_to[off_to[v] + jj], e2 = e_to[off_to[v] + 1 - jj];
            const int32_t w = h->v_left[e2];
            if (M.kmers[e2] > M.kmers[e1] || off_to[w + 1] - off_to[w] > 0 || off_from[w + 1] - off_from[w] > 1) continue;
            cand.emplace_back(e2, e1);
        }
    }
    std::sort(cand.begin(), cand.end());
    const uint64_t C = cand.size();
    if (C > IT_CAND) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: too many candidates", who);
    M.ce1.resize(C); M.ce2.resize(C); M.cn.resize(C); M.cdel.resize(C);
    M.role.assign(E, make_int4(-1, -1, -1, -1));
    for (uint64_t i = 0; i < C; ++i) {
        const int32_t e2 = cand[i].first, e1 = cand[i].second;
        M.ce1[i] = e1; M.ce2[i] = e2; M.cn[i] = M.kmers[e2]; M.cdel[i] = M.kmers[e1] - M.kmers[e2];
        M.role[e1].x = (int)i; M.role[e2].y = (int)i; M.role[inv[e1]].z = (int)i; M.role[inv[e2]].w = (int)i;
    }
    const float cand_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    m_cands Q;
    uint32_t* npe;
    unsigned long long* counters;
    int32_t* qss;
    if ((rc = m_up(c, M.ce1, &Q.e1, err, errcap)) || (rc = m_up(c, M.ce2, &Q.e2, err, errcap)) || (rc = m_up(c, M.cn, &Q.n, err, errcap)) ||
        (rc = m_up(c, M.cdel, &Q.del, err, errcap)) || (rc = m_up(c, M.role, &Q.role, err, errcap)) || (rc = m_up(c, M.kmers, &Q.kmers, err, errcap)) ||
        (rc = c.alloc(C, &npe)) || (rc = c.alloc(N_COUNTERS, &counters)) || (rc = c.alloc(2 * C, &qss)))
        return rc;
    Q.npe = npe;
    SNK_HIP_TRY(hipMemsetAsync(npe, 0, (C ? C : 1) * 4, st));
    SNK_HIP_TRY(hipMemsetAsync(counters, 0, N_COUNTERS * 8, st));
    SNK_HIP_TRY(hipMemsetAsync(qss, 0, (C ? 2 * C : 1) * 4, st));
    SNK_HIP_TRY(c.stamp());
    // ---- the read limit
    m_paths P;
    P.n = n; P.start = job.start; P.n_edges = job.n_edges; P.offset = job.offset; P.edges = job.edges;
    const snk_reads_view R = snk_reads_view_of(in, n);
    const uint64_t grid = snk_blocks_capped(n + 1, MB, std::min<uint64_t>((uint64_t)c.ctx->n_cu * 64, M_GRID_CAP));
    if (C && n) SNK_HIP_TRY(snk_launch(m_limit_kernel, grid, MB, 0, st, P, d_dup, Q.role, npe));
    SNK_HIP_TRY(c.stamp());
    // ---- the work items: count, scan, write
    uint32_t* n_items;
    unsigned long long* pos;
    if ((rc = c.alloc(n + 1, &n_items)) || (rc = c.alloc(n + 1, &pos))) return rc;
    SNK_HIP_TRY(snk_launch(m_items_kernel<false>, grid, MB, 0, st, P, R, d_dup, Q, (int)K, n_items, (const unsigned long long*)nullptr, (uint4*)nullptr, counters));
    {
        rocprim::transform_iterator<const uint32_t*, u32_to_u64, unsigned long long> it(n_items, u32_to_u64());
        if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::exclusive_scan(tmp, tb, it, pos, 0ull, (size_t)(n + 1), rocprim::plus<unsigned long long>(), st); }))) return rc;
    }
    unsigned long long I = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&I, pos + n, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    if (I > 4 * paths->n_edges_total || I >= (1ull << 32)) return snk_fail(I >= (1ull << 32) ? SNK_E_UNSUPPORTED : SNK_E_INTERNAL, err, errcap, "%s: %llu work items", who, I);
    uint4* items;
    unsigned long long *key, *key2;
    int32_t *val, *val2;
    if ((rc = c.alloc((size_t)I, &items)) || (rc = c.alloc((size_t)I, &key)) || (rc = c.alloc((size_t)I, &key2)) || (rc = c.alloc((size_t)I, &val)) || (rc = c.alloc((size_t)I, &val2)))
        return rc;
    if (I) SNK_HIP_TRY(snk_launch(m_items_kernel<true>, grid, MB, 0, st, P, R, d_dup, Q, (int)K, n_items, (const unsigned long long*)pos, items, counters));
    SNK_HIP_TRY(c.stamp());
    // ---- the scores
    if (I) SNK_HIP_TRY(snk_launch(m_score_kernel, snk_blocks_capped(I, IPB, M_GRID_CAP), MB, 0, st, job.G, R, P, Q, (int)K, (const uint4*)items, (uint64_t)I, key, val, counters));
    SNK_HIP_TRY(c.stamp());
    // ---- the records by (candidate, fw, offset); what is no record sorts behind them
    if (I && (rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::radix_sort_pairs(tmp, tb, key, key2, val, val2, (size_t)I, 0u, 64u, st); }))) return rc;
    unsigned long long h_cnt[N_COUNTERS];
    SNK_HIP_TRY(hipMemcpyAsync(h_cnt, counters, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(c.stamp());
    SNK_HIP_TRY(snk_sync(st));
    const uint64_t n_rec = h_cnt[N_RECORDS];
    if (n_rec > I) return snk_fail(SNK_E_INTERNAL, err, errcap, "%s: more records than work items", who);
    // ---- the groups, then the candidates
    unsigned long long n_groups = 0, n_scored_cands = 0;
    if (n_rec) {
        unsigned long long *gkey, *gmm, *z1, *z2, *s1, *s2, *d_count;
        uint32_t *ckey, *ukey;
        if ((rc = c.alloc((size_t)n_rec, &gkey)) || (rc = c.alloc((size_t)n_rec, &gmm)) || (rc = c.alloc((size_t)n_rec, &z1)) || (rc = c.alloc((size_t)n_rec, &z2)) ||
            (rc = c.alloc((size_t)n_rec, &s1)) || (rc = c.alloc((size_t)n_rec, &s2)) || (rc = c.alloc((size_t)n_rec, &ckey)) || (rc = c.alloc((size_t)n_rec, &ukey)) ||
            (rc = c.alloc(2, &d_count)))
            return rc;
        rocprim::transform_iterator<const int32_t*, m_both, unsigned long long> both((const int32_t*)val2, m_both());
        if ((rc = c.with_temp([&](void* tmp, size_t& tb) {
                return rocprim::reduce_by_key(tmp, tb, (const unsigned long long*)key2, both, (unsigned int)n_rec, gkey, gmm, d_count, m_minmax(), rocprim::equal_to<unsigned long long>(), st);
            })))
            return rc;
        SNK_HIP_TRY(hipMemcpyAsync(&n_groups, d_count, 8, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        if (!n_groups || n_groups > n_rec) return snk_fail(SNK_E_INTERNAL, err, errcap, "%s: the groups do not add up", who);
        SNK_HIP_TRY(snk_launch(m_groups_kernel, snk_blocks_capped(n_groups, MB, M_GRID_CAP), MB, 0, st, (const unsigned long long*)gkey, (const unsigned long long*)gmm,
                               (uint64_t)n_groups, ckey, z1, z2, counters));
        for (int side = 0; side < 2; ++side)
            if ((rc = c.with_temp([&](void* tmp, size_t& tb) {
                    return rocprim::reduce_by_key(tmp, tb, (const uint32_t*)ckey, (const unsigned long long*)(side ? z2 : z1), (unsigned int)n_groups, ukey, side ? s2 : s1,
                                                  d_count + 1, m_summax(), rocprim::equal_to<uint32_t>(), st);
                })))
                return rc;
        SNK_HIP_TRY(hipMemcpyAsync(&n_scored_cands, d_count + 1, 8, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        if (n_scored_cands > n_groups) return snk_fail(SNK_E_INTERNAL, err, errcap, "%s: the candidates do not add up", who);
        SNK_HIP_TRY(snk_launch(m_qss_kernel, snk_blocks_capped(n_scored_cands, MB, M_GRID_CAP), MB, 0, st, (const uint32_t*)ukey, (const unsigned long long*)s1,
                               (const unsigned long long*)s2, (uint64_t)n_scored_cands, qss));
    }
    // ---- the thresholds (:532-535)
    M.npe.assign(C, 0); M.qss.assign(2 * C, 0);
    if (C) {
        SNK_HIP_TRY(hipMemcpyAsync(M.npe.data(), npe, C * 4, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(hipMemcpyAsync(M.qss.data(), qss, 2 * C * 4, hipMemcpyDeviceToHost, st));
    }
    SNK_HIP_TRY(hipMemcpyAsync(h_cnt, counters, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    uint64_t too_many = 0, deleted = 0;
    for (uint64_t i = 0; i < C; ++i) {
        if (M.npe[i] > (uint32_t)MAX_READS2) { ++too_many; continue; }
        const int32_t qss1 = M.qss[2 * i], qss2 = M.qss[2 * i + 1];
        M.scored.insert(M.scored.end(), {M.ce1[i], M.ce2[i], qss1, qss2});
        if (qss1 >= MIN_QS_RIGHT && qss2 <= MAX_QS_WRONG) { ++deleted; M.dels.push_back(M.ce2[i]); M.dels.push_back(inv[M.ce2[i]]); }
    }
    std::sort(M.dels.begin(), M.dels.end());
    M.dels.erase(std::unique(M.dels.begin(), M.dels.end()), M.dels.end());
    const int32_t* d_scored;
    if ((rc = m_up(c, M.scored, &d_scored, err, errcap))) return rc;
    SNK_HIP_TRY(c.stamp());
    SNK_HIP_TRY(snk_sync(st));
    out->n_scored = M.scored.size() / 4; out->scored = d_scored;
    out->n_candidates = C; out->n_too_many_reads = too_many;
    out->n_entries_on_candidates = h_cnt[N_ON_CAND]; out->n_entries_in_window = h_cnt[N_IN_WINDOW]; out->n_reads_hq_excluded = h_cnt[N_HQ_EXCLUDED];
    out->n_records = n_rec; out->n_groups = n_groups; out->n_groups_mixed_sign = h_cnt[N_MIXED]; out->n_deleted_candidates = deleted;
    out->ms = c.ms(0, 7); out->tables_ms = c.ms(0, 1);
    out->phase_ms[0] = cand_ms;
    for (int k = 1; k < 6; ++k) out->phase_ms[k] = c.ms(k + 1, k + 2);
    out->n_dels = M.dels.size();
    out->dels = (int32_t*)malloc((M.dels.size() ? M.dels.size() : 1) * sizeof(int32_t));
    if (!out->dels) throw std::bad_alloc();
    if (!M.dels.empty()) memcpy(out->dels, M.dels.data(), M.dels.size() * sizeof(int32_t));
    return c.end(SNK_OK, {d_scored});
}

}  // namespace

extern "C" int snk_dev_mow_lawn(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, const snk_hbv* h, const int32_t* inv,
                                const snk_dev_reads* in, const snk_dev_paths* paths, const void* d_dup, uint32_t flags, snk_dev_mow* out, void* stream, char* err,
                                size_t errcap) {
    static const char who[] = "snk_dev_mow_lawn";
    if (!ctx || !h || !in || !paths || !out) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument", who);
    memset(out, 0, sizeof *out);
    if (flags) return snk_fail(SNK_E_ARG, err, errcap, "%s: flags = %u (no flag is defined)", who, flags);
    if (h->n_edges < 0 || h->n_vertices < 0) return snk_fail(SNK_E_ARG, err, errcap, "%s: a negative edge or vertex count", who);
    const uint64_t n = in->n_reads, E = (uint64_t)h->n_edges, N = (uint64_t)h->n_vertices;
    int rc = snk_bads_check_args(who, K, n, in->read_len, in->quals != nullptr, n_unitigs, d_unitig_off, d_unitig_bases, h, paths, SNK_BADS_X, err, errcap);
    if (rc) return rc;
    if (n && !d_dup) return snk_fail(SNK_E_ARG, err, errcap, "%s: d_dup == NULL (one flag per pair, as snk_dev_mark_dups returns it)", who);
    if (n && (!in->rows || in->read_len == 0 || in->row_words * 16 < in->read_len || in->row_words > 16))
        return snk_fail(SNK_E_ARG, err, errcap, "%s: need packed rows of at most 256 bases that hold read_len", who);
    if (n && in->qstride < in->read_len) return snk_fail(SNK_E_ARG, err, errcap, "%s: quality rows shorter than read_len", who);
    if (n >= (1ull << 32) - 1) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: too many reads", who);
    if (E && !inv) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument", who);
    for (uint64_t e = 0; e < E; ++e) {
        if (h->v_left[e] < 0 || (uint64_t)h->v_left[e] >= N || h->v_right[e] < 0 || (uint64_t)h->v_right[e] >= N)
            return snk_fail(SNK_E_ARG, err, errcap, "%s: edge %llu is out of range", who, (unsigned long long)e);
        if (inv[e] < 0 || (uint64_t)inv[e] >= E || inv[inv[e]] != (int32_t)e) return snk_fail(SNK_E_ARG, err, errcap, "%s: inv is not an involution at edge %llu", who, (unsigned long long)e);
    }
    mow_host M;            // (the uploads read it: declared in front of the frame)
    rc = snk_call_guarded(ctx, stream, who, err, errcap, [&](snk_call& c) -> int {
        return mow_impl(c, M, K, n_unitigs, d_unitig_off, d_unitig_bases, h, inv, in, paths, (const uint8_t*)d_dup, out, err, errcap);
    });
    if (rc) { free(out->dels); memset(out, 0, sizeof *out); }
    return rc;
}
