// snk_pathsx.hip -- the compressed read paths on the device: ReadPathVecX (a.pathsX), made from snk_dev_paths and read back into them.
//
// What it replaces: InitializePathsXFromPaths, lib/assembly/src/10X/DfTools.cc:24-69 (10X/DF.cc:579, right after StageBuildGraph), which
// zips every ReadPath with RPParser::LLzip (10X/paths/ReadPathParser.cc:18-51,184-198), and ReadPathVecX::unzip / LLunzip (:106-132).
// Per read, in read order, the record is
//     u8 n  |  n > 0: i16 offset (static_cast: it wraps), u32 first edge, (n - 1 + 3) / 4 bytes of 2-bit branch ids, low bits first
// The branch id of a step e -> e' is the position of e' in From(ToRight(e)); a step whose e' is not there writes nothing and does not
// move the bit cursor (the loop at :40-50 simply finds no j), while the record's size still comes from n.  ZipIndex = the byte offset
// of every 10th read.
//
// Here: from the lists of snk_hbv_lists_build three arrays per edge -- v_left, v_right and from_pos (u8: the position of the edge in
// From(v_left)) -- so that a step is found iff v_left[e'] == v_right[e], and its id is from_pos[e'].
//   px_size_kernel     record size per read (u8), the empty reads, the offsets that wrap, a path table that does not add up (start must
//                      be the exclusive scan of n_edges and end at n_edges_total), n > 255
//   snk_max_edge_id    the largest edge id (one outside the graph would index outside the three arrays: refused before the encoder runs)
//   exclusive scan     64-bit byte offsets (rocPRIM)
//   px_index_kernel    ZipIndex: every 10th offset
//   px_encode_kernel   a workgroup takes 256 consecutive reads (at most 71 bytes each: a static LDS tile); one lane per read walks its
//                      path -- the bit cursor depends on the steps found before -- and builds the record in LDS at its scanned offset;
//                      the tile then goes to HBM coalesced: 16-byte stores for the aligned interior, byte stores for the head and
//                      tail bytes that share a 16-byte word with the neighbouring tiles.  No atomics: every output byte has one writer
//                      and the count of steps not found is one word per tile, summed afterwards.
//   px_walk_kernel     unzip: one lane per index group of 10 reads walks the records (sizes, offsets), checks the index and the end
//   px_decode_kernel   unzip: one lane per read turns branch ids back into edge ids through the From lists (CSR)
// Nothing here looks at a tuning option: the result is a pure function of the paths and the graph.
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "snk_call.h"
#include "snk_common.h"
#include "snk_hbvadj.h"

namespace {

constexpr unsigned XB = 256;                          // lanes of a workgroup = reads of a tile
constexpr unsigned X_SKIP = 10;                       // ReadPathVecX::skip
constexpr unsigned X_MAX_REC = 7 + (255 - 1 + 3) / 4; // 71
constexpr unsigned X_TILE = XB * X_MAX_REC + 16;      // + the tile's misalignment against a 16-byte word
constexpr uint64_t PX_GRID_CAP = 1u << 20;
// bits of the flag word
constexpr uint32_t F_TABLE = 1, F_LONG = 2, F_WALK = 4, F_BRANCH = 8, F_EDGE = 16;

__host__ __device__ __forceinline__ uint32_t rec_bytes(uint32_t n) { return n ? 7u + (n + 2u) / 4u : 1u; }

struct u8_to_u64 {
    __host__ __device__ unsigned long long operator()(uint8_t x) const { return x; }
};
struct u32_to_u64 {
    __host__ __device__ unsigned long long operator()(uint32_t x) const { return x; }
};

// stat: [0] empty reads, [1] wrapped offsets (256 slots each); flags: F_TABLE / F_LONG
__global__ void __launch_bounds__(XB) px_size_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ n_edges, const int32_t* __restrict__ offset,
                                                     uint64_t n_reads, uint64_t n_entries, uint8_t* __restrict__ sz, unsigned long long* __restrict__ stat,
                                                     uint32_t* __restrict__ flags) {
    __shared__ uint32_t wg_empty, wg_wrap;
    if (threadIdx.x == 0) { wg_empty = 0; wg_wrap = 0; }
    __syncthreads();
    for (uint64_t base = (uint64_t)blockIdx.x * XB; base <= n_reads; base += (uint64_t)gridDim.x * XB) {
        const uint64_t r = base + threadIdx.x;
        bool empty = false, wrap = false;
        if (r < n_reads) {
            const uint64_t m = n_edges[r];
            uint32_t n = (uint32_t)m;
            if (!snk_paths_row_ok(start, n_edges, r, n_reads, n_entries)) {
                atomicOr(flags, F_TABLE);
                n = 0;
            }
            else if (m > 255) { atomicOr(flags, F_LONG); n = 0; }
            sz[r] = (uint8_t)rec_bytes(n);
            empty = n == 0;
            const int32_t o = offset[r];
            wrap = n != 0 && o != (int32_t)(int16_t)o;
        } else if (r == n_reads) sz[r] = 0;          // (the scan runs over n_reads + 1 places: the last one is the total)
        const unsigned long long me = __ballot(empty), mw = __ballot(wrap);
        if ((threadIdx.x & 63) == 0) {
            if (me) atomicAdd(&wg_empty, (uint32_t)__popcll(me));
            if (mw) atomicAdd(&wg_wrap, (uint32_t)__popcll(mw));
        }
    }
    __syncthreads();
    const uint32_t slot = blockIdx.x & 255u;
    if (threadIdx.x == 0 && wg_empty) atomicAdd(&stat[slot], (unsigned long long)wg_empty);
    if (threadIdx.x == 0 && wg_wrap) atomicAdd(&stat[256 + slot], (unsigned long long)wg_wrap);
}

__global__ void __launch_bounds__(XB) px_index_kernel(const unsigned long long* __restrict__ off, uint64_t n_index, long long* __restrict__ index) {
    for (uint64_t i = (uint64_t)blockIdx.x * XB + threadIdx.x; i < n_index; i += (uint64_t)gridDim.x * XB) index[i] = (long long)off[i * X_SKIP];
}

// off[r] = byte offset of read r's record, off[n_reads] = n_bytes.  data is 16-byte aligned.  tile_nf[tile] = steps not found in it.
__global__ void __launch_bounds__(XB) px_encode_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ n_edges, const int32_t* __restrict__ offset,
                                                       const uint32_t* __restrict__ edges, const int32_t* __restrict__ v_left, const int32_t* __restrict__ v_right,
                                                       const uint8_t* __restrict__ from_pos, const unsigned long long* __restrict__ off, uint64_t n_reads, uint64_t n_tiles,
                                                       uint8_t* __restrict__ data, uint32_t* __restrict__ tile_nf) {
    __shared__ uint4 tile4[X_TILE / 16];
    __shared__ uint32_t wave_nf[XB / 64];
    uint8_t* tile = reinterpret_cast<uint8_t*>(tile4);
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t r0 = t * XB, r1 = min(r0 + XB, n_reads);
        const uint64_t g0 = off[r0], g1 = off[r1];          // the tile's bytes in data: [g0, g1), at most XB * X_MAX_REC of them
        const uint64_t a0 = g0 & ~15ull;                    // LDS place of byte g = g - a0: the same misalignment as in HBM
        const uint64_t r = r0 + threadIdx.x;
        uint32_t nf = 0;
        if (r < r1) {
            uint32_t p = (uint32_t)(off[r] - a0);
            const uint32_t n = min(n_edges[r], 255u);       // (a longer path was refused before this launch; the clamp keeps the tile's bound local)
            tile[p++] = (uint8_t)n;
            if (n) {
                const uint64_t s = start[r];
                const uint32_t o = (uint32_t)offset[r];
                uint32_t e = edges[s];
                tile[p] = (uint8_t)o; tile[p + 1] = (uint8_t)(o >> 8);
                tile[p + 2] = (uint8_t)e; tile[p + 3] = (uint8_t)(e >> 8); tile[p + 4] = (uint8_t)(e >> 16); tile[p + 5] = (uint8_t)(e >> 24);
                p += 6;
                const uint32_t end = p + (n + 2u) / 4u;
                uint32_t cur = 0, sub = 0;
                int32_t w = v_right[e];
                for (uint32_t j = 1; j < n; ++j) {
                    const uint32_t e2 = edges[s + j];
                    if (v_left[e2] == w) {
                        cur |= (uint32_t)from_pos[e2] << sub;
                        sub += 2;
                        if (sub > 7) { tile[p++] = (uint8_t)cur; cur = 0; sub = 0; }
                    } else ++nf;
                    w = v_right[e2];
                }
                if (sub) tile[p++] = (uint8_t)cur;
                while (p < end) tile[p++] = 0;              // what the steps not found left unused
            }
        }
        for (int o = 32; o > 0; o >>= 1) nf += (uint32_t)__shfl_xor((int)nf, o);
        if ((threadIdx.x & 63) == 0) wave_nf[threadIdx.x >> 6] = nf;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (unsigned q = 0; q < XB / 64; ++q) tot += wave_nf[q];
            tile_nf[t] = tot;
        }
        // head bytes up to the first 16-byte boundary, whole words, tail bytes
        const uint64_t head_end = min((g0 + 15) & ~15ull, g1);
        const uint64_t int_end = max(head_end, g1 & ~15ull);
        for (uint64_t g = g0 + threadIdx.x; g < head_end; g += XB) data[g] = tile[g - a0];
        for (uint64_t g = head_end + 16ull * threadIdx.x; g < int_end; g += 16ull * XB) *reinterpret_cast<uint4*>(data + g) = tile4[(g - a0) >> 4];
        for (uint64_t g = int_end + threadIdx.x; g < g1; g += XB) data[g] = tile[g - a0];
        __syncthreads();
    }
}

// unzip, first pass: group q = reads [10 q, 10 q + 10) starts at index[q]; its records must end at index[q + 1] (the last group's at n_bytes)
__global__ void __launch_bounds__(XB) px_walk_kernel(const uint8_t* __restrict__ data, uint64_t n_bytes, const long long* __restrict__ index, uint64_t n_index,
                                                     uint64_t n_reads, unsigned long long* __restrict__ rec_off, uint32_t* __restrict__ n_edges, uint32_t* __restrict__ flags) {
    for (uint64_t q = (uint64_t)blockIdx.x * XB + threadIdx.x; q <= n_index; q += (uint64_t)gridDim.x * XB) {
        if (q == n_index) { n_edges[n_reads] = 0; continue; }               // (the scan's last place)
        uint64_t at = (uint64_t)index[q];
        const uint64_t want = q + 1 < n_index ? (uint64_t)index[q + 1] : n_bytes;
        bool bad = at > n_bytes || want > n_bytes;
        const uint64_t r1 = min((q + 1) * X_SKIP, n_reads);
        for (uint64_t r = q * X_SKIP; r < r1; ++r) {
            uint32_t n = 0;
            if (!bad && at < n_bytes) {
                n = data[at];
                if (rec_bytes(n) > n_bytes - at) { bad = true; n = 0; }
            } else bad = true;
            rec_off[r] = bad ? 0 : at;
            n_edges[r] = bad ? 0 : n;
            if (!bad) at += rec_bytes(n);
        }
        if (bad || at != want) atomicOr(flags, F_WALK);
    }
}

__global__ void __launch_bounds__(XB) px_decode_kernel(const uint8_t* __restrict__ data, const unsigned long long* __restrict__ rec_off, const uint32_t* __restrict__ n_edges,
                                                       const unsigned long long* __restrict__ start, uint64_t n_reads, uint64_t E, const int32_t* __restrict__ v_right,
                                                       const unsigned long long* __restrict__ from_off, const int32_t* __restrict__ from_e, int32_t* __restrict__ offset,
                                                       int32_t* __restrict__ edges, uint32_t* __restrict__ flags) {
    for (uint64_t r = (uint64_t)blockIdx.x * XB + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * XB) {
        const uint32_t n = n_edges[r];
        if (!n) { offset[r] = 0; continue; }
        const uint8_t* b = data + rec_off[r];
        offset[r] = (int32_t)(int16_t)(uint16_t)(b[1] | (b[2] << 8));
        uint32_t e = (uint32_t)b[3] | ((uint32_t)b[4] << 8) | ((uint32_t)b[5] << 16) | ((uint32_t)b[6] << 24);
        int32_t* out = edges + start[r];
        bool bad = false;
        if (e >= E) { atomicOr(flags, F_EDGE); bad = true; e = 0; }
        out[0] = (int32_t)e;
        for (uint32_t j = 1; j < n; ++j) {
            if (!bad) {
                const uint32_t id = (b[7 + ((j - 1) >> 2)] >> (2 * ((j - 1) & 3))) & 3u;
                const int32_t w = v_right[e];
                const unsigned long long f0 = from_off[w];
                if (id >= from_off[w + 1] - f0) { atomicOr(flags, F_BRANCH); bad = true; }
                else e = (uint32_t)from_e[f0 + id];
            }
            out[j] = bad ? -1 : (int32_t)e;
        }
    }
}

}  // namespace

extern "C" int snk_dev_paths_zip(snk_ctx* ctx, const snk_dev_paths* paths, const snk_hbv* h, snk_dev_pathsx* out, void* stream, char* err, size_t errcap) {
    if (!ctx || !paths || !h || !out || (h->n_edges > 0 && (!h->v_left || !h->v_right))) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_zip: NULL argument");
    memset(out, 0, sizeof *out);
    const uint64_t n = paths->n_edges_total, n_reads = paths->n_reads;
    const uint64_t E = (uint64_t)(h->n_edges > 0 ? h->n_edges : 0);
    if (n_reads && (!paths->start || !paths->n_edges || !paths->offset)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_zip: paths without their device arrays");
    if (n && !paths->edges) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_zip: paths without their device arrays");
    if (n && !E) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_zip: %llu path entries on a graph without edges", (unsigned long long)n);
    if (!n_reads && n) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_zip: start / n_edges do not add up to n_edges_total = %llu", (unsigned long long)n);
    if (n_reads >= (1ull << 40)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_paths_zip: too many reads");
    // What the asynchronous uploads read on the host -- from_pos here, the lists in unzip -- is declared in front of the frame: it is
    // let go of after the frame's last wait, whichever way the call ends.
    std::vector<uint8_t> h_pos;
    // sizes, offsets, the per-edge arrays and the scan's scratch go back to the arena with the call; data and index stay until the
    // context's next top-level call
    return snk_call_run(ctx, stream, "snk_dev_paths_zip", out, err, errcap, [&](snk_call& c) -> int {
        // the three per-edge arrays from the shared lists
        snk_hbv_lists ls;
        int rc = snk_hbv_lists_build(h, &ls, "snk_dev_paths_zip", err, errcap);
        if (rc) return rc;
        h_pos.assign((size_t)E + 1, 0);
        for (int32_t v = 0; v < h->n_vertices; ++v)
            for (uint64_t i = ls.from_off[v]; i < ls.from_off[(size_t)v + 1]; ++i) {
                const uint64_t j = i - ls.from_off[v];
                if (j > 3)
                    return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_paths_zip: vertex %d has more than four out-edges (a branch id has two bits)", v);
                h_pos[ls.from_e[i]] = (uint8_t)j;
            }
        const hipStream_t st = c.st;
        SNK_HIP_TRY(c.stamp());
        const uint64_t n_index = (n_reads + X_SKIP - 1) / X_SKIP, n_tiles = snk_blocks(n_reads, XB);
        long long* index;
        unsigned long long *off, *stat;
        uint8_t *sz, *d_pos;
        int32_t *d_vl, *d_vr;
        uint32_t *range, *tile_nf;
        // (the result first: what is handed back behind it coalesces; data follows when its size is known)
        if ((rc = c.alloc(n_index, &index)) || (rc = c.alloc(n_reads + 1, &off)) || (rc = c.alloc(n_reads + 1, &sz)) || (rc = c.alloc(E, &d_vl)) || (rc = c.alloc(E, &d_vr)) ||
            (rc = c.alloc(E, &d_pos)) || (rc = c.alloc(512 + 1, &stat)) || (rc = c.alloc(256 + 1, &range)) || (rc = c.alloc(n_tiles, &tile_nf)))
            return rc;
        SNK_HIP_TRY(hipMemsetAsync(stat, 0, 513 * 8, st));
        SNK_HIP_TRY(hipMemsetAsync(range, 0, 257 * 4, st));
        if (E) {
            SNK_HIP_TRY(hipMemcpyAsync(d_vl, h->v_left, E * 4, hipMemcpyHostToDevice, st));
            SNK_HIP_TRY(hipMemcpyAsync(d_vr, h->v_right, E * 4, hipMemcpyHostToDevice, st));
            SNK_HIP_TRY(hipMemcpyAsync(d_pos, h_pos.data(), E, hipMemcpyHostToDevice, st));
        }
        uint32_t* flags = range + 256;
        SNK_HIP_TRY(snk_launch(px_size_kernel, snk_blocks_capped(n_reads + 1, XB, PX_GRID_CAP), XB, 0, st, (const unsigned long long*)paths->start, (const uint32_t*)paths->n_edges,
                               (const int32_t*)paths->offset, n_reads, n, sz, stat, flags));
        if (n) SNK_HIP_TRY(snk_max_edge_id((const uint32_t*)paths->edges, n, range, st));
        {
            rocprim::transform_iterator<const uint8_t*, u8_to_u64, unsigned long long> in(sz, u8_to_u64());
            if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::exclusive_scan(tmp, tb, in, off, 0ull, (size_t)(n_reads + 1), rocprim::plus<unsigned long long>(), st); })))
                return rc;
        }
        uint32_t h_range[257];
        unsigned long long n_bytes = 0;
        SNK_HIP_TRY(hipMemcpyAsync(h_range, range, sizeof h_range, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(hipMemcpyAsync(&n_bytes, off + n_reads, 8, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        uint32_t emax = 0;
        for (int q = 0; q < 256; ++q) emax = std::max(emax, h_range[q]);
        if (h_range[256] & F_TABLE) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_zip: start / n_edges do not add up to n_edges_total = %llu", (unsigned long long)n);
        if (n && emax >= E)
            return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_zip: a path holds edge id %lld, the graph has %llu edges", (long long)(int32_t)emax, (unsigned long long)E);
        if (h_range[256] & F_LONG)
            return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_paths_zip: a path of more than 255 edges (the record's edge count is one byte)");
        if (n_bytes > n_reads * (unsigned long long)X_MAX_REC) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_paths_zip: the scan's total is out of range");
        uint8_t* data;
        if ((rc = c.alloc((size_t)n_bytes, &data))) return rc;
        if ((uintptr_t)data & 15u) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_paths_zip: the arena handed out a block that is not 16-byte aligned");
        SNK_HIP_TRY(snk_launch(px_index_kernel, snk_blocks_capped(n_index, XB, PX_GRID_CAP), XB, 0, st, (const unsigned long long*)off, n_index, index));
        if (n_tiles) {
            SNK_HIP_TRY(snk_launch(px_encode_kernel, snk_blocks_capped(n_tiles, 1, PX_GRID_CAP), XB, 0, st, (const unsigned long long*)paths->start, (const uint32_t*)paths->n_edges,
                                   (const int32_t*)paths->offset, (const uint32_t*)paths->edges, (const int32_t*)d_vl, (const int32_t*)d_vr, (const uint8_t*)d_pos,
                                   (const unsigned long long*)off, n_reads, n_tiles, data, tile_nf));
            rocprim::transform_iterator<const uint32_t*, u32_to_u64, unsigned long long> in(tile_nf, u32_to_u64());
            if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::reduce(tmp, tb, in, stat + 512, 0ull, (size_t)n_tiles, rocprim::plus<unsigned long long>(), st); })))
                return rc;
        }
        unsigned long long h_stat[513];
        SNK_HIP_TRY(hipMemcpyAsync(h_stat, stat, sizeof h_stat, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(c.stamp());
        SNK_HIP_TRY(snk_sync(st));
        uint64_t n_empty = 0, n_wrap = 0;
        for (int q = 0; q < 256; ++q) { n_empty += h_stat[q]; n_wrap += h_stat[256 + q]; }
        out->n_reads = n_reads;
        out->n_bytes = n_bytes;
        out->n_index = n_index;
        out->data = data;
        out->index = index;
        out->n_empty = n_empty;
        out->n_steps_not_found = h_stat[512];
        out->n_offsets_wrapped = n_wrap;
        out->ms = c.ms(0, 1);
        return c.end(SNK_OK, {data, index});
    });
}

extern "C" int snk_dev_paths_unzip(snk_ctx* ctx, const snk_dev_pathsx* in, const snk_hbv* h, snk_dev_paths* out, void* stream, char* err, size_t errcap) {
    if (!ctx || !in || !h || !out || (h->n_edges > 0 && (!h->v_left || !h->v_right))) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_unzip: NULL argument");
    memset(out, 0, sizeof *out);
    const uint64_t n_reads = in->n_reads, n_bytes = in->n_bytes, n_index = in->n_index;
    const uint64_t E = (uint64_t)(h->n_edges > 0 ? h->n_edges : 0), N = (uint64_t)(h->n_vertices > 0 ? h->n_vertices : 0);
    if (n_index != (n_reads + X_SKIP - 1) / X_SKIP)
        return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_unzip: %llu index entries for %llu reads (one per %u)", (unsigned long long)n_index, (unsigned long long)n_reads, X_SKIP);
    if ((n_bytes && !in->data) || (n_index && !in->index)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_unzip: NULL data or index");
    if (n_bytes < n_reads || n_bytes > n_reads * (uint64_t)X_MAX_REC)
        return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_unzip: %llu bytes cannot hold %llu records", (unsigned long long)n_bytes, (unsigned long long)n_reads);
    snk_hbv_lists ls;
    return snk_call_run(ctx, stream, "snk_dev_paths_unzip", out, err, errcap, [&](snk_call& c) -> int {
        int rc = snk_hbv_lists_build(h, &ls, "snk_dev_paths_unzip", err, errcap);
        if (rc) return rc;
        const hipStream_t st = c.st;
        SNK_HIP_TRY(c.stamp());
        int32_t *offset, *edges, *d_vr, *d_fe;
        uint32_t *ne, *flags;
        unsigned long long *start, *rec_off, *d_fo;
        if ((rc = c.alloc(n_reads, &offset)) || (rc = c.alloc(n_reads + 1, &ne)) || (rc = c.alloc(n_reads + 1, &start)) || (rc = c.alloc(n_reads, &rec_off)) ||
            (rc = c.alloc(E, &d_vr)) || (rc = c.alloc(E, &d_fe)) || (rc = c.alloc(N + 1, &d_fo)) || (rc = c.alloc(4, &flags)))
            return rc;
        SNK_HIP_TRY(hipMemsetAsync(flags, 0, 16, st));
        SNK_HIP_TRY(hipMemcpyAsync(d_fo, ls.from_off.data(), (N + 1) * 8, hipMemcpyHostToDevice, st));
        if (E) {
            SNK_HIP_TRY(hipMemcpyAsync(d_vr, h->v_right, E * 4, hipMemcpyHostToDevice, st));
            SNK_HIP_TRY(hipMemcpyAsync(d_fe, ls.from_e.data(), E * 4, hipMemcpyHostToDevice, st));
        }
        SNK_HIP_TRY(snk_launch(px_walk_kernel, snk_blocks_capped(n_index + 1, XB, PX_GRID_CAP), XB, 0, st, (const uint8_t*)in->data, n_bytes, (const long long*)in->index, n_index, n_reads,
                               rec_off, ne, flags));
        {
            rocprim::transform_iterator<const uint32_t*, u32_to_u64, unsigned long long> it(ne, u32_to_u64());
            if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::exclusive_scan(tmp, tb, it, start, 0ull, (size_t)(n_reads + 1), rocprim::plus<unsigned long long>(), st); })))
                return rc;
        }
        uint32_t h_flags = 0;
        unsigned long long total = 0;
        SNK_HIP_TRY(hipMemcpyAsync(&h_flags, flags, 4, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(hipMemcpyAsync(&total, start + n_reads, 8, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        if (h_flags & F_WALK)
            return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_unzip: the records do not follow the index or do not end at n_bytes = %llu", (unsigned long long)n_bytes);
        if (total > n_reads * 255ull) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_paths_unzip: the scan's total is out of range");
        if (total && !E) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_unzip: %llu path entries on a graph without edges", total);
        if ((rc = c.alloc((size_t)total, &edges))) return rc;
        SNK_HIP_TRY(snk_launch(px_decode_kernel, snk_blocks_capped(n_reads, XB, PX_GRID_CAP), XB, 0, st, (const uint8_t*)in->data, (const unsigned long long*)rec_off, (const uint32_t*)ne,
                               (const unsigned long long*)start, n_reads, E, (const int32_t*)d_vr, (const unsigned long long*)d_fo, (const int32_t*)d_fe, offset, edges, flags));
        SNK_HIP_TRY(hipMemcpyAsync(&h_flags, flags, 4, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(c.stamp());
        SNK_HIP_TRY(snk_sync(st));
        if (h_flags & F_EDGE) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_unzip: a record's first edge id is outside the graph (%llu edges)", (unsigned long long)E);
        if (h_flags & F_BRANCH) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_paths_unzip: a branch id points past the out-edges of its vertex");
        out->n_reads = n_reads;
        out->n_edges_total = total;
        out->offset = offset;
        out->n_edges = ne;
        out->start = start;
        out->edges = edges;
        out->path_ms = c.ms(0, 1);
        return c.end(SNK_OK, {offset, ne, start, edges});
    });
}
