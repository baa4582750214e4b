// snk_edit.hip -- graph edits on the device: DeleteEdgesParallel + Cleanup (paths/long/large/GapToyTools.cc:1287-1302) and the
// hanging-end rule of StageTrim (10X/runstages/RunStages.cc:91-146).  include/snk.h, "graph edits", states the semantics.
//
//   snk_dev_delete_edges   The part that grows with the reads and the bases runs on the device: one lane per read cuts its path at the
//       first deleted edge, renumbers, drops an entry that repeats the new edge in front of it and moves the offset (count, scan, the
//       same walk writes); the bases of the new unitigs -- one per pair {e, inv[e]} of the new graph -- are copied from the old ones
//       segment by segment, four output bases per lane and one dword store.  The part that grows with the edges only runs on the host
//       in one pass over them, as snk_dev_hbv's small-graph flood does: vertex degrees, the unneeded vertices, the reference's own walk
//       from the highest unneeded vertex down (its list of runs IS the id order), the compaction of edges and vertices.  A device form
//       of that part (list ranking weighted by k-mers, as the join's snk_rank_lists) is not built.
//   snk_dev_hanging_ends   rs[e] = entries x with x == e or inv[x] == e.  Only (x == e) is counted; the inverse's count is added when the
//       tables are summed, which halves the increments.  No atomic touches global memory: up to SNK_HANG_LDS_MAX edges a workgroup
//       counts its share of the entries in LDS and writes its table out, and one lane per edge sums the tables; above that the entries
//       are sorted and one lane per edge finds the ends of its run.  The rule itself reads E counts and runs on the host.
// Nothing here looks at a tuning option and no atomic decides a result.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <utility>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "snk_call.h"
#include "snk_common.h"

namespace {

constexpr unsigned EB = 256;                     // lanes of a workgroup
constexpr unsigned HB = 512;                     // ... of the LDS histogram's
constexpr uint64_t E_GRID_CAP = 1u << 20;
constexpr uint32_t F_TABLE = 1, F_EDGE = 2, F_MEET = 4;
constexpr uint32_t SEG_RC = 1u << 31;
enum { N_TRUNCATED, N_EMPTIED, N_COLLAPSED, N_COUNTERS = 4 };

struct u32_to_u64 { __host__ __device__ unsigned long long operator()(uint32_t x) const { return x; } };

// ---- the path table against the graph
struct e_paths {
    uint64_t n, n_entries, E;
    const unsigned long long* start;
    const uint32_t* n_edges;
    const int32_t* offset;
    const uint32_t* edges;
};
// rows that add up, ids inside the graph and, with vl / vr, consecutive edges that meet at a vertex
__global__ void __launch_bounds__(EB) e_check_kernel(e_paths p, const int32_t* __restrict__ vl, const int32_t* __restrict__ vr, uint32_t* __restrict__ flags) {
    for (uint64_t r = (uint64_t)blockIdx.x * EB + threadIdx.x; r < p.n; r += (uint64_t)gridDim.x * EB) {
        if (!snk_paths_row_ok(p.start, p.n_edges, r, p.n, p.n_entries)) { atomicOr(flags, F_TABLE); continue; }
        const uint64_t s = p.start[r], m = p.n_edges[r];
        uint32_t prev = 0;
        for (uint64_t j = 0; j < m; ++j) {
            const uint32_t x = p.edges[s + j];
            if (x >= p.E) { atomicOr(flags, F_EDGE); break; }
            if (vl && j && vr[prev] != vl[x]) atomicOr(flags, F_MEET);
            prev = x;
        }
    }
}

// ---- the rewrite: cut, renumber, collapse, move the offset
struct r_args {
    e_paths in;
    const int32_t* map;            // [E] new id, -1 = deleted
    const int32_t* koff;           // [E]
    uint32_t* n_out;               // [n + 1]
    int32_t* off_out;              // [n]
    const unsigned long long* pos; // [n + 1]
    int32_t* edges_out;
    unsigned long long* counters;
};
template <bool WRITE>
__global__ void __launch_bounds__(EB) r_rewrite_kernel(r_args a) {
    __shared__ uint32_t cnt[N_COUNTERS];
    if (threadIdx.x < N_COUNTERS) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t r = (uint64_t)blockIdx.x * EB + threadIdx.x; r <= a.in.n; r += (uint64_t)gridDim.x * EB) {
        if (r == a.in.n) { if (!WRITE) a.n_out[r] = 0; continue; }
        const uint64_t s = a.in.start[r], m = a.in.n_edges[r];
        int32_t* out = WRITE ? a.edges_out + a.pos[r] : nullptr;
        uint32_t n = 0, collapsed = 0;
        int32_t prev = -1;
        bool cut = false;
        for (uint64_t j = 0; j < m; ++j) {
            const int32_t f = a.map[a.in.edges[s + j]];
            if (f < 0) { cut = true; break; }
            if (f == prev) { ++collapsed; continue; }
            if (WRITE) out[n] = f;
            ++n;
            prev = f;
        }
        if (WRITE) continue;
        a.n_out[r] = n;
        a.off_out[r] = a.in.offset[r] + (n ? a.koff[a.in.edges[s]] : 0);
        if (cut) { atomicAdd(cnt + N_TRUNCATED, 1u); if (!n) atomicAdd(cnt + N_EMPTIED, 1u); }
        if (collapsed) atomicAdd(cnt + N_COLLAPSED, collapsed);
    }
    __syncthreads();
    if (!WRITE && threadIdx.x < N_COUNTERS && cnt[threadIdx.x]) atomicAdd(a.counters + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

// ---- the bases of the new unitigs.  Segment s fills [dst[s], dst[s + 1]) with the bases from `skip` on of an old unitig (src, len),
// read forward or reverse-complemented.
struct seg_tab {
    const uint64_t* dst;           // [n + 1], ascending, dst[n] = total
    const uint64_t* src;           // [n] first base of the old unitig in the old array
    const uint32_t* len;           // [n] its bases
    const uint32_t* fl;            // [n] SEG_RC | skip
    uint64_t n;
};
__global__ void __launch_bounds__(EB) b_copy_kernel(seg_tab S, const uint8_t* __restrict__ ub, uint64_t total, uint32_t* __restrict__ nb) {
    const uint64_t words = (total + 3) / 4;
    for (uint64_t w = (uint64_t)blockIdx.x * EB + threadIdx.x; w < words; w += (uint64_t)gridDim.x * EB) {
        const uint64_t p0 = w * 4;
        uint64_t lo = 0, hi = S.n;               // the largest s with dst[s] <= p0
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (S.dst[mid] <= p0) lo = mid; else hi = mid; }
        uint64_t s = lo;
        uint32_t v = 0;
        for (uint32_t q = 0; q < 4 && p0 + q < total; ++q) {
            const uint64_t p = p0 + q;
            while (p >= S.dst[s + 1]) ++s;
            const uint32_t f = S.fl[s], len = S.len[s];
            const uint64_t i = p - S.dst[s] + (f & ~SEG_RC);
            const uint32_t b = f & SEG_RC ? 3u - (ub[S.src[s] + len - 1 - i] & 3u) : ub[S.src[s] + i] & 3u;
            v |= b << (8 * q);
        }
        nb[w] = v;                               // (the block has 16 bytes of slack behind `total`)
    }
}

// ---- read support
// LDS leg: table[g][e] = entries equal to e among workgroup g's share
__global__ void __launch_bounds__(HB) h_lds_kernel(const uint32_t* __restrict__ edges, uint64_t n_entries, uint32_t E, uint32_t* __restrict__ table, uint32_t* __restrict__ flags) {
    extern __shared__ uint32_t h_cnt[];
    for (uint32_t e = threadIdx.x; e < E; e += HB) h_cnt[e] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * HB + threadIdx.x; i < n_entries; i += (uint64_t)gridDim.x * HB) {
        const uint32_t x = edges[i];
        if (x >= E) { atomicOr(flags, F_EDGE); continue; }
        atomicAdd(h_cnt + x, 1u);
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < E; e += HB) table[(uint64_t)blockIdx.x * E + e] = h_cnt[e];
}
__global__ void __launch_bounds__(EB) h_sum_kernel(const uint32_t* __restrict__ table, uint32_t G, uint32_t E, const int32_t* __restrict__ inv, int32_t* __restrict__ support) {
    const uint32_t e = blockIdx.x * EB + threadIdx.x;
    if (e >= E) return;
    const uint32_t re = (uint32_t)inv[e];
    uint32_t sum = 0;
    for (uint32_t g = 0; g < G; ++g) sum += table[(uint64_t)g * E + e] + table[(uint64_t)g * E + re];
    support[e] = (int32_t)sum;
}
// sort leg: the run of x in the ascending entries
__device__ __forceinline__ uint64_t h_lower(const uint32_t* a, uint64_t n, uint32_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
__global__ void __launch_bounds__(EB) h_runs_kernel(const uint32_t* __restrict__ sorted, uint64_t n_entries, uint64_t E, const int32_t* __restrict__ inv, int32_t* __restrict__ support,
                                                   uint32_t* __restrict__ flags) {
    const uint64_t e = (uint64_t)blockIdx.x * EB + threadIdx.x;
    if (e == 0 && n_entries && sorted[n_entries - 1] >= E) atomicOr(flags, F_EDGE);      // compared as unsigned: a negative id is the largest
    if (e >= E) return;
    const uint32_t re = (uint32_t)inv[e];
    const uint64_t a = h_lower(sorted, n_entries, (uint32_t)e + 1) - h_lower(sorted, n_entries, (uint32_t)e);
    const uint64_t b = h_lower(sorted, n_entries, re + 1) - h_lower(sorted, n_entries, re);
    support[e] = (int32_t)(a + b);
}

template <typename T>
int e_up(snk_call& c, const std::vector<T>& h, const T** out, char* err, size_t errcap) {
    T* d;
    const int rc = c.alloc(h.size(), &d);
    if (rc) return rc;
    if (!h.empty()) SNK_HIP_TRY(hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, c.st));
    *out = d;
    return SNK_OK;
}
int e_scan32(snk_call& c, const uint32_t* in, unsigned long long* out, size_t count) {
    rocprim::transform_iterator<const uint32_t*, u32_to_u64, unsigned long long> it(in, u32_to_u64());
    return c.with_temp([&](void* tmp, size_t& tb) { return rocprim::exclusive_scan(tmp, tb, it, out, 0ull, count, rocprim::plus<unsigned long long>(), c.st); });
}
template <typename T>
T* e_malloc(size_t n) {
    T* p = (T*)malloc((n ? n : 1) * sizeof(T));
    if (!p) throw std::bad_alloc();
    return p;
}

// ---- what both entry points ask of their arguments before anything runs
int graph_args(const char* who, uint32_t K, uint64_t U, const void* d_uoff, const void* d_ub, bool need_bases, const snk_hbv* h, const int32_t* inv, const snk_dev_paths* paths,
               char* err, size_t errcap) {
    if (K != 48 && K != 60) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "K=%u is not supported (48 or 60)", K);
    if (U >= (1ull << 31)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: too many unitigs", who);
    if (h->n_edges < 0 || h->n_vertices < 0) return snk_fail(SNK_E_ARG, err, errcap, "%s: a negative edge or vertex count", who);
    const uint64_t E = (uint64_t)h->n_edges, N = (uint64_t)h->n_vertices;
    if (U && (!d_uoff || (need_bases && !d_ub))) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL unitig arrays", who);
    if (E && (!h->v_left || !h->v_right || !h->src_unitig || !h->is_rc || !inv)) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument", who);
    for (uint64_t e = 0; e < E; ++e) {
        if (h->v_left[e] < 0 || (uint64_t)h->v_left[e] >= N || h->v_right[e] < 0 || (uint64_t)h->v_right[e] >= N || h->src_unitig[e] < 0 || (uint64_t)h->src_unitig[e] >= U)
            return snk_fail(SNK_E_ARG, err, errcap, "%s: edge %llu is out of range", who, (unsigned long long)e);
        if (h->bvcomp_order && (h->bvcomp_order[h->src_unitig[e]] < 0 || (uint64_t)h->bvcomp_order[h->src_unitig[e]] >= U))
            return snk_fail(SNK_E_ARG, err, errcap, "%s: inconsistent translation tables", who);
    }
    for (uint64_t e = 0; e < E; ++e)
        if (inv[e] < 0 || (uint64_t)inv[e] >= E || inv[inv[e]] != (int32_t)e) return snk_fail(SNK_E_ARG, err, errcap, "%s: inv is not an involution at edge %llu", who, (unsigned long long)e);
    const uint64_t n = paths->n_reads, n_entries = paths->n_edges_total;
    if (n && (!paths->start || !paths->n_edges || !paths->offset)) return snk_fail(SNK_E_ARG, err, errcap, "%s: paths without their device arrays", who);
    if (n_entries && !paths->edges) return snk_fail(SNK_E_ARG, err, errcap, "%s: paths without their device arrays", who);
    if (!n && n_entries) return snk_fail(SNK_E_ARG, err, errcap, "%s: start / n_edges do not add up to n_edges_total = %llu", who, (unsigned long long)n_entries);
    if (n_entries && !E) return snk_fail(SNK_E_ARG, err, errcap, "%s: a path holds an edge id outside the graph's 0 edges", who);
    if (n >= (1ull << 32) - 1) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: too many reads", who);
    return SNK_OK;
}

// the unitig offsets on the host, checked; kmers[e] = k-mers of edge e, eu[e] = its unitig in the device arrays
int edge_lengths(snk_call& c, const char* who, uint32_t K, uint64_t U, const void* d_uoff, const snk_hbv* h, std::vector<uint64_t>& uoff, std::vector<int32_t>& eu,
                 std::vector<uint32_t>& kmers, char* err, size_t errcap) {
    uoff.assign(U + 1, 0);
    if (U) {
        SNK_HIP_TRY(hipMemcpyAsync(uoff.data(), d_uoff, (U + 1) * 8, hipMemcpyDeviceToHost, c.st));
        SNK_HIP_TRY(snk_sync(c.st));
    }
    for (uint64_t u = 0; u < U; ++u) {
        if (uoff[u + 1] < uoff[u] + K || (u == 0 && uoff[0] != 0)) return snk_fail(SNK_E_ARG, err, errcap, "%s: unitig %llu has fewer than K bases, or the offsets do not start at 0", who, (unsigned long long)u);
        if (uoff[u + 1] - uoff[u] > 0x7FFFFFFFull) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: a unitig of 2^31 bases or more", who);
    }
    const uint64_t E = (uint64_t)h->n_edges;
    eu.resize(E); kmers.resize(E);
    for (uint64_t e = 0; e < E; ++e) {
        const int32_t r = h->src_unitig[e];
        eu[e] = h->bvcomp_order ? h->bvcomp_order[r] : r;
        kmers[e] = (uint32_t)(uoff[(size_t)eu[e] + 1] - uoff[eu[e]]) - K + 1;
    }
    return SNK_OK;
}

int check_paths(snk_call& c, const char* who, const e_paths& p, const int32_t* d_vl, const int32_t* d_vr, uint32_t* flags, char* err, size_t errcap) {
    SNK_HIP_TRY(hipMemsetAsync(flags, 0, 4, c.st));
    SNK_HIP_TRY(snk_launch(e_check_kernel, p.n ? snk_blocks_capped(p.n, EB, E_GRID_CAP) : 0, EB, 0, c.st, p, d_vl, d_vr, flags));
    uint32_t f = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&f, flags, 4, hipMemcpyDeviceToHost, c.st));
    SNK_HIP_TRY(snk_sync(c.st));
    if (f & F_TABLE) return snk_fail(SNK_E_ARG, err, errcap, "%s: start / n_edges do not add up to n_edges_total = %llu", who, (unsigned long long)p.n_entries);
    if (f & F_EDGE) return snk_fail(SNK_E_ARG, err, errcap, "%s: a path holds an edge id outside the graph's %llu edges", who, (unsigned long long)p.E);
    if (f & F_MEET) return snk_fail(SNK_E_ARG, err, errcap, "%s: a path whose consecutive edges do not meet at a vertex", who);
    return SNK_OK;
}

// ---- the host's part of an edit
struct edit_plan {
    // per old edge
    std::vector<int32_t> map, koff;
    // the new graph
    std::vector<int32_t> vl, vr, inv, src, fwd, rev;
    std::vector<uint8_t> is_rc;
    int32_t N = 0;
    // the new unitigs as segments of old ones
    std::vector<uint64_t> uoff, seg_dst, seg_src;
    std::vector<uint32_t> seg_len, seg_fl;
    uint64_t n_deleted = 0, n_runs = 0, n_absorbed = 0, max_run = 0;
};
struct edit_host {
    std::vector<uint64_t> uoff;
    std::vector<int32_t> eu, vl, vr;
    std::vector<uint32_t> kmers;
    std::vector<uint8_t> dead;
    edit_plan P;
};

// RemoveUnneededVertices2 and CleanupCore over the graph h without the edges marked dead.  false: inv does not mirror the graph (the
// inverse of a run is no run, or an edge stays whose inverse goes)
bool plan_edit(uint32_t K, const snk_hbv* h, const int32_t* inv, const edit_host& H, edit_plan& P) {
    const int32_t E = h->n_edges, N = h->n_vertices;
    const int32_t *vl = h->v_left, *vr = h->v_right;
    const std::vector<uint8_t>& dead = H.dead;
    // degrees, and the one edge of a side that has one
    std::vector<uint32_t> n_in((size_t)N, 0), n_out((size_t)N, 0);
    std::vector<int32_t> e_in((size_t)N, -1), e_out((size_t)N, -1);
    for (int32_t e = 0; e < E; ++e) {
        if (dead[e]) { ++P.n_deleted; continue; }
        ++n_out[vl[e]]; e_out[vl[e]] = e;
        ++n_in[vr[e]]; e_in[vr[e]] = e;
    }
    // step 1 (GapToyTools3.cc:520-527)
    std::vector<uint8_t> kill((size_t)N, 0);
    for (int32_t v = 0; v < N; ++v) kill[v] = n_out[v] == 1 && n_in[v] == 1 && vr[e_out[v]] != vl[e_in[v]];
    // step 2 (:541-585): the queue holds the unneeded vertices ascending and is popped from the back
    std::vector<std::pair<int32_t, int32_t>> bound;
    for (int32_t v = N - 1; v >= 0; --v) {
        if (!kill[v]) continue;
        int32_t eleft, eright, x = v;
        do { kill[x] = 0; eleft = e_in[x]; x = vl[eleft]; } while (kill[x]);
        x = v;
        do { kill[x] = 0; eright = e_out[x]; x = vr[eright]; } while (kill[x]);
        if (eleft < inv[eright]) { bound.emplace_back(eleft, eright); bound.emplace_back(inv[eright], inv[eleft]); }
    }
    // steps 3 and 4 (:603-646): the list is taken from the back; a new edge is the list of its run
    std::vector<int32_t> renum((size_t)E);
    for (int32_t e = 0; e < E; ++e) renum[e] = e;
    P.koff.assign((size_t)E, 0);
    std::vector<uint8_t> gone(dead);                      // not in the graph any more: deleted or absorbed
    std::vector<int32_t> members, new_vl, new_vr;
    std::vector<uint64_t> first_member(1, 0);
    while (!bound.empty()) {
        const std::pair<int32_t, int32_t> b = bound.back();
        bound.pop_back();
        const int32_t id = E + (int32_t)new_vl.size();
        int32_t off = (int32_t)H.kmers[b.first];
        renum[b.first] = id; gone[b.first] = 1;
        members.push_back(b.first);
        for (int32_t v = vr[b.first]; v != vr[b.second]; v = vr[e_out[v]]) {
            if (n_out[v] != 1 || n_in[v] != 1 || members.size() > 2 * (size_t)E) return false;
            const int32_t e = e_out[v];
            members.push_back(e);
            P.koff[e] = off;
            renum[e] = id; gone[e] = 1;
            off += (int32_t)H.kmers[e];
        }
        new_vl.push_back(vl[b.first]); new_vr.push_back(vr[b.second]);
        first_member.push_back(members.size());
        const uint64_t run = first_member[first_member.size() - 1] - first_member[first_member.size() - 2];
        P.max_run = std::max(P.max_run, run);
    }
    const int32_t n_new = (int32_t)new_vl.size(), E_all = E + n_new;
    P.n_runs = (uint64_t)n_new; P.n_absorbed = members.size();
    // CleanupCore (GapToyTools.cc:1253-1285): the used edge objects in id order, the vertices that still have an edge in id order
    std::vector<int32_t> to_new((size_t)E_all, -1);
    int32_t E2 = 0;
    for (int32_t e = 0; e < E_all; ++e) if (e >= E || !gone[e]) to_new[e] = E2++;
    std::vector<int32_t> v_new((size_t)N, -1);
    auto left_of = [&](int32_t e) { return e < E ? vl[e] : new_vl[e - E]; };
    auto right_of = [&](int32_t e) { return e < E ? vr[e] : new_vr[e - E]; };
    for (int32_t e = 0; e < E_all; ++e) if (to_new[e] >= 0) { v_new[left_of(e)] = 0; v_new[right_of(e)] = 0; }
    for (int32_t v = 0; v < N; ++v) if (v_new[v] == 0) v_new[v] = P.N++;
    P.vl.resize((size_t)E2); P.vr.resize((size_t)E2); P.inv.resize((size_t)E2);
    for (int32_t e = 0; e < E_all; ++e) {
        const int32_t f = to_new[e];
        if (f < 0) continue;
        P.vl[f] = v_new[left_of(e)]; P.vr[f] = v_new[right_of(e)];
        P.inv[f] = to_new[e < E ? inv[e] : E + ((e - E) ^ 1)];       // (:640-646: the new edges pair up two by two)
    }
    for (int32_t f = 0; f < E2; ++f) if (P.inv[f] < 0 || P.inv[P.inv[f]] != f) return false;
    P.map.resize((size_t)E);
    for (int32_t e = 0; e < E; ++e) P.map[e] = dead[e] ? -1 : to_new[renum[e]];
    // the unitigs: one per pair, numbered by the smaller id, stored as that edge reads
    P.src.assign((size_t)E2, -1); P.is_rc.assign((size_t)E2, 0);
    P.uoff.assign(1, 0);
    P.seg_dst.clear();
    auto segment = [&](int32_t old_edge, uint32_t skip) {
        const int32_t u = H.eu[old_edge];
        const uint32_t len = (uint32_t)(H.uoff[(size_t)u + 1] - H.uoff[u]);
        P.seg_dst.push_back(P.uoff.back());
        P.seg_src.push_back(H.uoff[u]);
        P.seg_len.push_back(len);
        P.seg_fl.push_back((h->is_rc[old_edge] ? SEG_RC : 0u) | skip);
        P.uoff.back() += len - skip;
    };
    for (int32_t e = 0; e < E_all; ++e) {
        const int32_t f = to_new[e];
        if (f < 0 || P.inv[f] < f) continue;
        const int32_t u = (int32_t)P.fwd.size();
        P.fwd.push_back(f); P.rev.push_back(P.inv[f]);
        P.src[f] = u; P.src[P.inv[f]] = u;
        if (P.inv[f] != f) P.is_rc[P.inv[f]] = 1;
        P.uoff.push_back(P.uoff.back());
        if (e < E) segment(e, 0);
        else for (uint64_t i = first_member[e - E]; i < first_member[(size_t)(e - E) + 1]; ++i) segment(members[i], i == first_member[e - E] ? 0u : K - 1);
    }
    P.seg_dst.push_back(P.uoff.back());
    return true;
}

template <typename T>
T* e_copy_out(const std::vector<T>& v) {
    T* p = e_malloc<T>(v.size());
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

int delete_impl(snk_call& c, edit_host& H, uint32_t K, uint64_t U, const void* d_uoff, const uint8_t* d_ub, const snk_hbv* h, const int32_t* inv, const snk_dev_paths* paths,
                snk_dev_edit* out, char* err, size_t errcap) {
    const hipStream_t st = c.st;
    int rc;
    SNK_HIP_TRY(c.stamp());
    const uint64_t E = (uint64_t)h->n_edges, n = paths->n_reads;
    if ((rc = edge_lengths(c, "snk_dev_delete_edges", K, U, d_uoff, h, H.uoff, H.eu, H.kmers, err, errcap))) return rc;
    // ---- the paths against the graph
    H.vl.assign(h->v_left, h->v_left + E); H.vr.assign(h->v_right, h->v_right + E);
    const int32_t *d_vl, *d_vr;
    uint32_t* flags;
    unsigned long long* counters;
    if ((rc = e_up(c, H.vl, &d_vl, err, errcap)) || (rc = e_up(c, H.vr, &d_vr, err, errcap)) || (rc = c.alloc(1, &flags)) || (rc = c.alloc(N_COUNTERS, &counters))) return rc;
    e_paths p;
    p.n = n; p.n_entries = paths->n_edges_total; p.E = E;
    p.start = (const unsigned long long*)paths->start; p.n_edges = (const uint32_t*)paths->n_edges; p.offset = (const int32_t*)paths->offset; p.edges = (const uint32_t*)paths->edges;
    if ((rc = check_paths(c, "snk_dev_delete_edges", p, d_vl, d_vr, flags, err, errcap))) return rc;
    // ---- the host's part
    const auto t0 = std::chrono::steady_clock::now();
    edit_plan& P = H.P;
    if (!plan_edit(K, h, inv, H, P)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_delete_edges: inv does not mirror the graph (the inverse of a run of edges is no run)");
    const float graph_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const uint64_t E2 = P.vl.size(), U2 = P.fwd.size(), total = P.uoff.back();
    // ---- the bases
    seg_tab S;
    uint64_t* noff;
    uint32_t* nb;
    S.n = P.seg_src.size();
    if ((rc = e_up(c, P.seg_dst, &S.dst, err, errcap)) || (rc = e_up(c, P.seg_src, &S.src, err, errcap)) || (rc = e_up(c, P.seg_len, &S.len, err, errcap)) ||
        (rc = e_up(c, P.seg_fl, &S.fl, err, errcap)) || (rc = c.alloc(U2 + 1, &noff)) || (rc = c.alloc((total + 3) / 4, &nb)))
        return rc;
    SNK_HIP_TRY(hipMemcpyAsync(noff, P.uoff.data(), (U2 + 1) * 8, hipMemcpyHostToDevice, st));
    SNK_HIP_TRY(snk_launch(b_copy_kernel, total ? snk_blocks_capped((total + 3) / 4, EB, E_GRID_CAP) : 0, EB, 0, st, S, d_ub, total, nb));
    SNK_HIP_TRY(c.stamp());
    // ---- the paths: count, scan, write
    r_args a;
    memset(&a, 0, sizeof a);
    a.in = p; a.counters = counters;
    unsigned long long* pos;
    if ((rc = e_up(c, P.map, &a.map, err, errcap)) || (rc = e_up(c, P.koff, &a.koff, err, errcap)) || (rc = c.alloc(n + 1, &a.n_out)) || (rc = c.alloc(n, &a.off_out)) ||
        (rc = c.alloc(n + 1, &pos)))
        return rc;
    SNK_HIP_TRY(hipMemsetAsync(counters, 0, N_COUNTERS * 8, st));
    const uint64_t grid = snk_blocks_capped(n + 1, EB, std::min<uint64_t>((uint64_t)c.ctx->n_cu * 64, E_GRID_CAP));
    SNK_HIP_TRY(snk_launch(r_rewrite_kernel<false>, grid, EB, 0, st, a));
    if ((rc = e_scan32(c, a.n_out, pos, (size_t)(n + 1)))) return rc;
    unsigned long long n_total = 0, h_cnt[N_COUNTERS];
    SNK_HIP_TRY(hipMemcpyAsync(&n_total, pos + n, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(hipMemcpyAsync(h_cnt, counters, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    if (n_total > paths->n_edges_total) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_delete_edges: the scan's total is out of range");
    if ((rc = c.alloc((size_t)n_total, &a.edges_out))) return rc;
    a.pos = pos;
    SNK_HIP_TRY(snk_launch(r_rewrite_kernel<true>, grid, EB, 0, st, a));
    SNK_HIP_TRY(c.stamp());
    SNK_HIP_TRY(snk_sync(st));
    // ---- out (the host arrays last: nothing below fails except by bad_alloc, which snk_dev_delete_edges cleans up after)
    out->n_unitigs = U2; out->unitig_total_bases = total; out->unitig_off = noff; out->unitig_bases = nb;
    out->paths.n_reads = n; out->paths.n_edges_total = n_total; out->paths.offset = a.off_out; out->paths.n_edges = a.n_out; out->paths.start = pos; out->paths.edges = a.edges_out;
    out->paths.path_ms = c.ms(1, 2);
    out->n_old_edges = E; out->n_deleted = P.n_deleted; out->n_runs = P.n_runs; out->n_absorbed = P.n_absorbed; out->max_run = P.max_run;
    out->n_truncated = h_cnt[N_TRUNCATED]; out->n_emptied = h_cnt[N_EMPTIED]; out->n_collapsed = h_cnt[N_COLLAPSED];
    out->ms = c.ms(0, 2); out->graph_ms = graph_ms;
    out->h.n_vertices = P.N; out->h.n_edges = (int32_t)E2;
    out->h.v_left = e_copy_out(P.vl); out->h.v_right = e_copy_out(P.vr); out->h.src_unitig = e_copy_out(P.src); out->h.is_rc = e_copy_out(P.is_rc);
    out->h.fwd_xlat = e_copy_out(P.fwd); out->h.rev_xlat = e_copy_out(P.rev);
    out->inv = e_copy_out(P.inv); out->edge_map = e_copy_out(P.map); out->edge_koff = e_copy_out(P.koff);
    return c.end(SNK_OK, {noff, nb, a.off_out, a.n_out, pos, a.edges_out});
}

struct hang_host {
    std::vector<uint64_t> uoff;
    std::vector<int32_t> eu, inv, support;
    std::vector<uint32_t> kmers;
};

int hanging_impl(snk_call& c, hang_host& H, uint32_t K, uint64_t U, const void* d_uoff, const snk_hbv* h, const int32_t* inv, const snk_dev_paths* paths, uint32_t max_kmers,
                 uint32_t flags, snk_dev_hanging* out, char* err, size_t errcap) {
    const hipStream_t st = c.st;
    int rc;
    SNK_HIP_TRY(c.stamp());
    const uint64_t E = (uint64_t)h->n_edges, N = (uint64_t)h->n_vertices, n_entries = paths->n_edges_total;
    if ((rc = edge_lengths(c, "snk_dev_hanging_ends", K, U, d_uoff, h, H.uoff, H.eu, H.kmers, err, errcap))) return rc;
    uint32_t* fl;
    if ((rc = c.alloc(1, &fl))) return rc;
    e_paths p;
    p.n = paths->n_reads; p.n_entries = n_entries; p.E = E;
    p.start = (const unsigned long long*)paths->start; p.n_edges = (const uint32_t*)paths->n_edges; p.offset = (const int32_t*)paths->offset; p.edges = (const uint32_t*)paths->edges;
    if ((rc = check_paths(c, "snk_dev_hanging_ends", p, nullptr, nullptr, fl, err, errcap))) return rc;
    // ---- read support
    H.inv.assign(inv, inv + E);
    const int32_t* d_inv;
    int32_t* support;
    if ((rc = e_up(c, H.inv, &d_inv, err, errcap)) || (rc = c.alloc(E, &support))) return rc;
    const bool lds = flags & SNK_HANG_LDS ? true : flags & SNK_HANG_SORT ? false : E <= SNK_HANG_LDS_MAX;
    if (lds) {
        const uint64_t G = snk_blocks_capped(n_entries, (uint64_t)HB * 64, (uint64_t)c.ctx->n_cu * 2);
        uint32_t* table;
        if ((rc = c.alloc(G * E, &table))) return rc;
        SNK_HIP_TRY(snk_launch(h_lds_kernel, E ? G : 0, HB, E * 4, st, p.edges, n_entries, (uint32_t)E, table, fl));
        SNK_HIP_TRY(snk_launch(h_sum_kernel, snk_blocks(E, EB), EB, 0, st, table, (uint32_t)G, (uint32_t)E, d_inv, support));
    } else {
        uint32_t* sorted;
        if ((rc = c.alloc(n_entries, &sorted))) return rc;
        unsigned bits = 1;
        while (bits < 32 && (E >> bits)) ++bits;
        // (the ids were checked above; the bit range covers [0, E))
        if (n_entries && (rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::radix_sort_keys(tmp, tb, p.edges, sorted, (size_t)n_entries, 0u, bits, st); }))) return rc;
        SNK_HIP_TRY(snk_launch(h_runs_kernel, snk_blocks(E, EB), EB, 0, st, sorted, n_entries, E, d_inv, support, fl));
    }
    H.support.assign(E, 0);
    uint32_t f = 0;
    if (E) SNK_HIP_TRY(hipMemcpyAsync(H.support.data(), support, E * 4, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(hipMemcpyAsync(&f, fl, 4, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(c.stamp());
    SNK_HIP_TRY(snk_sync(st));
    if (f & F_EDGE) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_hanging_ends: an edge id outside the graph behind the check");
    // ---- the rule (RunStages.cc:128-143)
    std::vector<uint32_t> n_in(N, 0), n_out(N, 0);
    for (uint64_t e = 0; e < E; ++e) { ++n_out[h->v_left[e]]; ++n_in[h->v_right[e]]; }
    std::vector<int32_t> dels;
    uint64_t unsupported = 0;
    for (uint64_t e = 0; e < E; ++e) {
        if (H.support[e] > 0) continue;
        ++unsupported;
        if (H.kmers[e] > max_kmers) continue;
        const int32_t v = h->v_left[e], w = h->v_right[e];
        if ((n_in[v] == 0 && n_out[v] == 1) || (n_out[w] == 0 && n_in[w] == 1)) { dels.push_back((int32_t)e); dels.push_back(inv[e]); }
    }
    std::sort(dels.begin(), dels.end());
    dels.erase(std::unique(dels.begin(), dels.end()), dels.end());
    out->n_hbv_edges = E; out->n_entries = n_entries; out->support = support; out->n_dels = dels.size(); out->n_unsupported = unsupported;
    out->leg = lds ? SNK_HANG_LDS : SNK_HANG_SORT;
    out->ms = c.ms(0, 1);
    out->dels = e_copy_out(dels);
    return c.end(SNK_OK, {support});
}

}  // namespace

extern "C" void snk_dev_edit_free(snk_dev_edit* r) {
    if (!r) return;
    snk_hbv_free(&r->h);
    free(r->inv); free(r->edge_map); free(r->edge_koff);
    r->inv = r->edge_map = r->edge_koff = nullptr;
}

extern "C" int snk_dev_delete_edges(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, const snk_hbv* h, const int32_t* inv,
                                    const snk_dev_paths* paths, const int32_t* dels, uint64_t n_dels, uint32_t flags, snk_dev_edit* out, void* stream, char* err, size_t errcap) {
    if (!ctx || !h || !paths || !out || (n_dels && !dels)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_delete_edges: NULL argument");
    memset(out, 0, sizeof *out);
    if (flags) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_delete_edges: flags = %u (no flag is defined)", flags);
    const int rc0 = graph_args("snk_dev_delete_edges", K, n_unitigs, d_unitig_off, d_unitig_bases, true, h, inv, paths, err, errcap);
    if (rc0) return rc0;
    edit_host H;
    SNK_GUARD_AS("snk_dev_delete_edges",
        const uint64_t E = (uint64_t)h->n_edges;
        H.dead.assign(E, 0);
        for (uint64_t i = 0; i < n_dels; ++i) {
            if (dels[i] < 0 || (uint64_t)dels[i] >= E) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_delete_edges: dels holds the edge id %d outside the graph's %llu edges", dels[i], (unsigned long long)E);
            H.dead[dels[i]] = 1;
        }
        for (uint64_t e = 0; e < E; ++e)
            if (H.dead[e] && !H.dead[inv[e]]) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_delete_edges: dels holds edge %llu without its inverse %d", (unsigned long long)e, inv[e]);
    )
    const int rc = snk_call_guarded(ctx, stream, "snk_dev_delete_edges", err, errcap, [&](snk_call& c) -> int {
        return delete_impl(c, H, K, n_unitigs, d_unitig_off, (const uint8_t*)d_unitig_bases, h, inv, paths, out, err, errcap);
    });
    if (rc) { snk_dev_edit_free(out); memset(out, 0, sizeof *out); }
    return rc;
}

extern "C" int snk_dev_hanging_ends(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, const snk_hbv* h, const int32_t* inv,
                                    const snk_dev_paths* paths, uint32_t max_kmers, uint32_t flags, snk_dev_hanging* out, void* stream, char* err, size_t errcap) {
    if (!ctx || !h || !paths || !out) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_hanging_ends: NULL argument");
    memset(out, 0, sizeof *out);
    if ((flags & ~(SNK_HANG_LDS | SNK_HANG_SORT)) || flags == (SNK_HANG_LDS | SNK_HANG_SORT)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_hanging_ends: flags = %u", flags);
    const int rc0 = graph_args("snk_dev_hanging_ends", K, n_unitigs, d_unitig_off, d_unitig_bases, false, h, inv, paths, err, errcap);
    if (rc0) return rc0;
    if ((flags & SNK_HANG_LDS) && (uint64_t)h->n_edges > SNK_HANG_LDS_MAX)
        return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_hanging_ends: the LDS leg holds %u edges, the graph has %d", SNK_HANG_LDS_MAX, h->n_edges);
    hang_host H;
    const int rc = snk_call_guarded(ctx, stream, "snk_dev_hanging_ends", err, errcap, [&](snk_call& c) -> int {
        return hanging_impl(c, H, K, n_unitigs, d_unitig_off, h, inv, paths, max_kmers, flags, out, err, errcap);
    });
    if (rc) { free(out->dels); memset(out, 0, sizeof *out); }
    return rc;
}
