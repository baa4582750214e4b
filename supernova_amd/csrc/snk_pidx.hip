// snk_pidx.hip -- the paths index on the device: per HBV edge the ids of the reads whose path holds it, and the read support per edge.
//
// What it replaces: writePathsIndex, lib/assembly/src/10X/PathsIndex.cc:23-145 (called right after the pathing, 10X/DF.cc:588; results
// written as a.paths.inv and a.countsb).  The reference streams one (edge, read id) pair per path entry into 15 temporary chunk files by
// edge range, reads every chunk back, comparison-sorts it, cuts it into one ULongVec per edge (an empty one for an edge nobody visits,
// :101-102) and then adds the support of an edge and of its reverse complement (:122-133).
//
// Here: the path entries are already read-major with ascending read id (snk_dev_paths.edges), so the index is ONE stable reorder of the
// entries by edge id that carries the read id:
//   pidx_fill_kernel     read id of every entry (one thread per read writes its own n_edges ids: entries of neighbouring reads are
//                        neighbours, the stores coalesce)
//   max_edge_id_kernel   the largest edge id (an id outside [0, E) would index outside the offset table: refused before anything is written)
//   radix sort           stable LSD over the ceil(log2 E) key bits there are (14 on the bench graph's 7 605 unitigs, 24 at 12 M edges):
//                        digit histograms in LDS per workgroup, no atomic per entry anywhere -- a handful of edges hold most entries.
//                        rocPRIM's radix_sort_pairs, as in MarkDups (snk_dups.hip): the whole call runs at 2.9 TB/s of the data it has
//                        to move (100 M entries: 2.2 ms, DESIGN 4 "paths index"), which leaves a hand-written pass little to win
//   pidx_offsets_kernel  run boundaries of the sorted keys -> index_off[e] for every e (every offset is written exactly once, by the thread
//                        that sees the key change; the edges in a gap between two keys are the empty ones)
//   pidx_counts_kernel   counts[e] = own entries + entries of inv[e] (a self-inverse edge keeps its own), checked against 2^31 - 1
// Nothing here looks at a tuning option: the result is a pure function of the paths.
#include <string.h>
#include <algorithm>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "snk_call.h"
#include "snk_common.h"

namespace {

constexpr unsigned PB = 256;

// every launch of this file: a grid that covers its work items at PB a workgroup, cut at 2^20 workgroups -- the kernels stride over
// what is left, with 64-bit indices
constexpr uint64_t PIDX_GRID_CAP = 1u << 20;

__global__ void __launch_bounds__(PB) pidx_fill_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ n_edges, uint64_t n_reads,
                                                       uint64_t n_entries, unsigned long long* __restrict__ rid, uint32_t* __restrict__ bad) {
    for (uint64_t r = (uint64_t)blockIdx.x * PB + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * PB) {
        const uint64_t s = start[r], m = n_edges[r];
        if (s > n_entries || m > n_entries - s) { *bad = 1u; continue; }       // (a path table that does not add up: nothing is written outside rid[])
        for (uint64_t j = 0; j < m; ++j) rid[s + j] = r;
    }
}

// The largest edge id, compared as unsigned.  16 bytes per lane where the pointer allows: the (up to three) ids before the first 16-byte
// boundary and behind the last whole uint4 are peeled by workgroup 0.  slot = one of 256 words, looked at before it is touched (it
// stops moving early).
__global__ void __launch_bounds__(PB) max_edge_id_kernel(const uint32_t* __restrict__ edges, uint64_t n, uint32_t* __restrict__ range /* [256] */) {
    uint32_t m = 0;
    const uint64_t head = min(n, (uint64_t)((0u - (uint32_t)((uintptr_t)edges >> 2)) & 3u));
    const uint64_t n4 = (n - head) / 4, tail = head + n4 * 4;
    const uint4* e4 = reinterpret_cast<const uint4*>(edges + head);
    for (uint64_t i = (uint64_t)blockIdx.x * PB + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * PB) {
        const uint4 v = e4[i];
        m = max(max(m, v.x), max(max(v.y, v.z), v.w));
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) m = max(m, edges[threadIdx.x]);
        if (threadIdx.x < n - tail) m = max(m, edges[tail + threadIdx.x]);
    }
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
    __shared__ uint32_t wg_max;
    if (threadIdx.x == 0) wg_max = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&wg_max, m);
    __syncthreads();
    const uint32_t slot = blockIdx.x & 255u;
    if (threadIdx.x == 0 && wg_max > range[slot]) atomicMax(&range[slot], wg_max);
}

// sorted keys -> offsets.  Entry i opens a run when its key differs from the one before it: it then owns off[e] for every e in
// (key[i-1], key[i]] (the edges before key[i] in that range are empty: their run starts -- and ends -- here too).  The last entry owns
// the tail (key[n-1], E].  No entries at all: block 0 writes zeros.
__global__ void __launch_bounds__(PB) pidx_offsets_kernel(const uint32_t* __restrict__ skey, uint64_t n, uint64_t E, unsigned long long* __restrict__ off) {
    if (n == 0) {
        for (uint64_t e = (uint64_t)blockIdx.x * PB + threadIdx.x; e <= E; e += (uint64_t)gridDim.x * PB) off[e] = 0;
        return;
    }
    const uint64_t n4 = (n + 3) / 4;
    for (uint64_t q = (uint64_t)blockIdx.x * PB + threadIdx.x; q < n4; q += (uint64_t)gridDim.x * PB) {
        const uint64_t i0 = q * 4;
        uint32_t k[4];
        if (i0 + 4 <= n) {
            const uint4 v = reinterpret_cast<const uint4*>(skey)[q];
            k[0] = v.x; k[1] = v.y; k[2] = v.z; k[3] = v.w;
        } else {
            for (int j = 0; j < 4; ++j) k[j] = i0 + j < n ? skey[i0 + j] : 0u;
        }
        int64_t prev = i0 ? (int64_t)skey[i0 - 1] : -1;
        for (int j = 0; j < 4 && i0 + j < n; ++j) {
            for (int64_t e = prev + 1; e <= (int64_t)k[j]; ++e) off[e] = i0 + j;
            prev = k[j];
        }
        if (i0 + 4 >= n)
            for (uint64_t e = (uint64_t)prev + 1; e <= E; ++e) off[e] = n;
    }
}

__global__ void __launch_bounds__(PB) pidx_counts_kernel(const unsigned long long* __restrict__ off, const int32_t* __restrict__ inv, uint64_t E,
                                                         int32_t* __restrict__ counts, unsigned long long* __restrict__ stat /* [256] empty, [256] overflow */) {
    __shared__ uint32_t wg_empty, wg_over;
    if (threadIdx.x == 0) { wg_empty = 0; wg_over = 0; }
    __syncthreads();
    for (uint64_t base = (uint64_t)blockIdx.x * PB; base < E; base += (uint64_t)gridDim.x * PB) {
        const uint64_t e = base + threadIdx.x;
        bool empty = false, over = false;
        if (e < E) {
            const uint64_t own = off[e + 1] - off[e];
            const uint64_t r = (uint64_t)(uint32_t)inv[e];
            const uint64_t tot = r == e ? own : own + (off[r + 1] - off[r]);
            empty = own == 0;
            over = tot > 0x7FFFFFFFull;
            counts[e] = over ? 0x7FFFFFFF : (int32_t)tot;
        }
        const unsigned long long me = __ballot(empty), mo = __ballot(over);
        if ((threadIdx.x & 63) == 0) {
            if (me) atomicAdd(&wg_empty, (uint32_t)__popcll(me));
            if (mo) atomicAdd(&wg_over, (uint32_t)__popcll(mo));
        }
    }
    __syncthreads();
    const uint32_t slot = blockIdx.x & 255u;
    if (threadIdx.x == 0 && wg_empty) atomicAdd(&stat[slot], (unsigned long long)wg_empty);
    if (threadIdx.x == 0 && wg_over) atomicAdd(&stat[256 + slot], (unsigned long long)wg_over);
}

}  // namespace

hipError_t snk_max_edge_id(const uint32_t* edges, uint64_t n, uint32_t* range, hipStream_t st) {
    return snk_launch(max_edge_id_kernel, snk_blocks_capped(n / 4 + 1, PB, PIDX_GRID_CAP), PB, 0, st, edges, n, range);
}

int snk_pidx_lists(snk_call& c, const snk_dev_paths* paths, uint64_t E, const char* who, bool with_counts, unsigned long long** p_off, unsigned long long** p_ids,
                   int32_t** p_counts, uint32_t* p_key_bits, char* err, size_t errcap) {
    const hipStream_t st = c.st;
    const uint64_t n = paths->n_edges_total, n_reads = paths->n_reads;
    int rc;
    unsigned long long *off, *ids, *rid;
    uint32_t *skey, *range;
    *p_counts = nullptr;
    // (results first: what is handed back behind them coalesces)
    if ((rc = c.alloc(E + 1, &off)) || (rc = c.alloc(n, &ids)) || (with_counts && (rc = c.alloc(E, p_counts))) || (rc = c.alloc(n, &rid)) || (rc = c.alloc(n + 4, &skey)) ||
        (rc = c.alloc(256 + 1, &range)))
        return rc;
    SNK_HIP_TRY(hipMemsetAsync(range, 0, 257 * 4, st));
    uint32_t key_bits = 0;
    while (key_bits < 32 && (1ull << key_bits) < E) ++key_bits;
    if (n) {
        SNK_HIP_TRY(snk_launch(pidx_fill_kernel, snk_blocks_capped(n_reads, PB, PIDX_GRID_CAP), PB, 0, st, (const unsigned long long*)paths->start, (const uint32_t*)paths->n_edges, n_reads, n,
                               rid, range + 256));
        SNK_HIP_TRY(snk_max_edge_id((const uint32_t*)paths->edges, n, range, st));
        uint32_t h_range[257];
        SNK_HIP_TRY(hipMemcpyAsync(h_range, range, sizeof h_range, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        uint32_t emax = 0;
        for (int q = 0; q < 256; ++q) emax = std::max(emax, h_range[q]);
        if (h_range[256]) return snk_fail(SNK_E_ARG, err, errcap, "%s: start / n_edges do not add up to n_edges_total = %llu", who, (unsigned long long)n);
        if (emax >= E) return snk_fail(SNK_E_ARG, err, errcap, "%s: a path holds edge id %lld, the graph has %llu edges", who, (long long)(int32_t)emax, (unsigned long long)E);
        const uint32_t bits = std::max(1u, key_bits);
        if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::radix_sort_pairs(tmp, tb, (const uint32_t*)paths->edges, skey, rid, ids, (size_t)n, 0u, bits, st); })))
            return rc;
    }
    SNK_HIP_TRY(snk_launch(pidx_offsets_kernel, snk_blocks_capped(n ? (n + 3) / 4 : E + 1, PB, PIDX_GRID_CAP), PB, 0, st, skey, n, E, off));
    *p_off = off; *p_ids = ids; *p_key_bits = key_bits;
    return SNK_OK;
}

extern "C" int snk_dev_paths_index(snk_ctx* ctx, const snk_dev_paths* paths, uint64_t E, const int32_t* inv, snk_dev_pidx* out, void* stream, char* err,
                                   size_t errcap) {
    if (!ctx || !paths || !out || (E && !inv)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_index: NULL argument");
    memset(out, 0, sizeof *out);
    const uint64_t n = paths->n_edges_total;
    if (E > 0x7FFFFFFFull) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_index: %llu HBV edges (edge ids are int32)", (unsigned long long)E);
    if (n && (!paths->start || !paths->n_edges || !paths->edges)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_index: paths without their device arrays");
    if ((uintptr_t)paths->edges & 15u) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_index: paths->edges is not 16-byte aligned");
    if (n && !E) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_index: %llu path entries on a graph without edges", (unsigned long long)n);
    if (n >= (1ull << 32)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_paths_index: more than 2^32 path entries in one call");
    for (uint64_t e = 0; e < E; ++e) {
        const int64_t r = inv[e];
        if (r < 0 || (uint64_t)r >= E || (uint64_t)inv[r] != e)
            return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_index: inv is not an involution of [0, %llu) at edge %llu", (unsigned long long)E, (unsigned long long)e);
    }
    // the read ids in path order, the sorted keys, the involution and the sort's own scratch go back to the arena with the call; offsets,
    // ids and counts stay until the context's next top-level call
    return snk_call_run(ctx, stream, "snk_dev_paths_index", out, err, errcap, [&](snk_call& c) -> int {
        const hipStream_t st = c.st;
        SNK_HIP_TRY(c.stamp());
        int rc;
        unsigned long long *off, *ids, *stat;
        int32_t *counts, *d_inv;
        uint32_t key_bits;
        if ((rc = snk_pidx_lists(c, paths, E, "snk_dev_paths_index", true, &off, &ids, &counts, &key_bits, err, errcap))) return rc;
        if ((rc = c.alloc(E, &d_inv)) || (rc = c.alloc(512, &stat))) return rc;
        SNK_HIP_TRY(hipMemsetAsync(stat, 0, 512 * 8, st));
        if (E) SNK_HIP_TRY(hipMemcpyAsync(d_inv, inv, E * 4, hipMemcpyHostToDevice, st));
        if (E) SNK_HIP_TRY(snk_launch(pidx_counts_kernel, snk_blocks_capped(E, PB, PIDX_GRID_CAP), PB, 0, st, off, d_inv, E, counts, stat));
        unsigned long long h_stat[512];
        SNK_HIP_TRY(hipMemcpyAsync(h_stat, stat, sizeof h_stat, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(c.stamp());
        SNK_HIP_TRY(snk_sync(st));
        uint64_t n_empty = 0, n_over = 0;
        for (int q = 0; q < 256; ++q) { n_empty += h_stat[q]; n_over += h_stat[256 + q]; }
        if (n_over)
            return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_paths_index: the read support of %llu edge(s) and their reverse complements passes 2^31 - 1 (a.countsb holds int)",
                            (unsigned long long)n_over);
        out->n_hbv_edges = E;
        out->n_entries = n;
        out->index_off = off;
        out->index_ids = ids;
        out->counts = counts;
        out->n_empty_edges = n_empty;
        out->key_bits = key_bits;
        out->ms = c.ms(0, 1);
        return c.end(SNK_OK, {off, ids, counts});
    });
}
