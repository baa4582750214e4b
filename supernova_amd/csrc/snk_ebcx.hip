// snk_ebcx.hip -- the edge -> barcode lists on the device: per HBV edge the ascending set of the barcodes whose reads visit the edge or
// its reverse complement.
//
// What it replaces: computeEdgeToBarcodeX, lib/assembly/src/10X/PathsIndex.cc:297-358 (StageEBC, 10X/runstages/RunStages.cc:31-38; the
// result is stored as a.ebcx and opened first by every scaffolding step).  The reference unzips the paths of one barcode's run of reads
// at a time, pushes e and inv[e] of every path entry into a vector per run, UniqueSorts it (:313-322), counts the runs per edge
// (:327-332) and fills the lists run by run, sequentially (:344-355).
//
// Here: one (edge, barcode) key for each strand of every path entry of a read with bc > 0, one stable radix sort, and the distinct keys
// in sorted order ARE the lists:
//   ebc_scan (rocPRIM)   per read, inclusive: path entries of the reads with bc > 0 so far (where its keys go) and the largest bc > 0 so
//                        far (bc is non-decreasing over those reads iff every one of them equals that maximum)
//   ebc_check_kernel     start / n_edges inside the entry table; the sortedness flag
//   max_edge_id_kernel   (snk_pidx.hip) the largest edge id: an id outside [0, E) would index outside inv[] and the offset table
//   -- sizing read-back: range, flags, number of keys --
//   ebc_emit_kernel      one thread per read writes the keys of its own entries: e and inv[e] next to each other (8 or 16 bytes a store;
//                        entries of neighbouring reads are neighbours).  A self-inverse edge writes its key twice: the twin is an equal
//                        key and falls to the distinct step like any other repeat
//   radix sort           rocPRIM, stable.  bc sorted: over the ceil(log2 E) bits of the edge id only, carrying bc -- the emission order is
//                        barcode-ascending already, so each edge's barcodes stay ascending and equal (edge, bc) keys stay neighbours.
//                        Otherwise (or SNK_EBC_GENERAL_SORT): the 64-bit key edge << 31 | bc over key_bits + 31 bits
//   ebc_heads_kernel     a key opens a run when (edge, bc) differs from the key before it: run heads per tile of 1024 keys
//   exclusive scan       of the tile counts (rocPRIM: one value per 1024 keys)
//   ebc_compact_kernel   rank of every run head = tile base + rank inside the tile (wave prefix by snk_wave_scan_excl, wave sums through LDS);
//                        ebc[rank] = bc; the head that sees the EDGE change writes ebc_off of its edge and of the empty edges in the gap
//                        before it, the last key those of the tail (as pidx_offsets_kernel does).  No atomic per key anywhere: a few
//                        edges hold most keys
//   ebc_stats_kernel     list lengths -> empty edges and the longest list, reduced per workgroup in LDS into 256 spread slots
//   -- final read-back: number of list entries, the two statistics --
// Nothing here looks at a tuning option: the result is a pure function of (paths, bc, inv), whichever sort ran.
#include <string.h>
#include <algorithm>
#include <rocprim/rocprim.hpp>

#include "snk_call.h"
#include "snk_common.h"

namespace {

constexpr unsigned EB = 256;                       // threads of a workgroup
constexpr unsigned KPT = 4;                        // keys of a thread: 16 bytes of sorted 32-bit keys, 32 of 64-bit ones
constexpr unsigned TILE = EB * KPT;                // keys of a tile
constexpr uint64_t EBC_GRID_CAP = 1u << 20;        // the kernels stride over what a capped grid leaves, with 64-bit indices

struct ebc_acc {                                   // the scan's element: 16 bytes, one load in the emit kernel
    unsigned long long n;                          // path entries of the reads with bc > 0, this one included
    int32_t mx, pad;                               // largest bc > 0 so far (0: none yet)
};
struct ebc_join {
    __host__ __device__ ebc_acc operator()(const ebc_acc& a, const ebc_acc& b) const { return ebc_acc{a.n + b.n, a.mx > b.mx ? a.mx : b.mx, 0}; }
};
struct ebc_read {                                  // read r -> its own contribution
    const int32_t* bc;
    const uint32_t* n_edges;
    __host__ __device__ ebc_acc operator()(unsigned long long r) const {
        const int32_t b = bc[r];
        return b > 0 ? ebc_acc{n_edges[r], b, 0} : ebc_acc{0ull, 0, 0};
    }
};

constexpr uint32_t F_TABLE = 1u, F_UNSORTED = 2u;

__global__ void __launch_bounds__(EB) ebc_check_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ n_edges, const int32_t* __restrict__ bc,
                                                       const ebc_acc* __restrict__ acc, uint64_t n_reads, uint64_t n_entries, uint32_t* __restrict__ flags) {
    uint32_t f = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * EB + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * EB) {
        const uint64_t s = start[r], m = n_edges[r];
        if (s > n_entries || m > n_entries - s) f |= F_TABLE;
        const int32_t b = bc[r];
        if (b > 0 && acc[r].mx != b) f |= F_UNSORTED;
    }
    if (f) atomicOr(flags, f);                     // (set by the few reads that have something to report)
}

// One thread per read with bc > 0: entry j of the read becomes the keys 2 * (first + j) and 2 * (first + j) + 1, first = entries of the
// contributing reads before it.  GENERAL: key64 = edge << 31 | bc; otherwise key32 = edge, val = bc.
template <bool GENERAL>
__global__ void __launch_bounds__(EB) ebc_emit_kernel(const unsigned long long* __restrict__ start, const uint32_t* __restrict__ n_edges, const int32_t* __restrict__ edges,
                                                      const int32_t* __restrict__ bc, const ebc_acc* __restrict__ acc, const int32_t* __restrict__ inv, uint64_t n_reads,
                                                      uint64_t n_pairs /* = n_keys / 2 */, uint32_t* __restrict__ key32, int32_t* __restrict__ val,
                                                      unsigned long long* __restrict__ key64) {
    for (uint64_t r = (uint64_t)blockIdx.x * EB + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * EB) {
        const int32_t b = bc[r];
        if (b <= 0) continue;
        const uint64_t s = start[r], m = n_edges[r];
        const uint64_t first = acc[r].n - m;
        if (first > n_pairs || m > n_pairs - first) continue;          // (cannot happen after the scan; nothing is written outside the keys)
        for (uint64_t j = 0; j < m; ++j) {
            const uint32_t e = (uint32_t)edges[s + j], t = (uint32_t)inv[e];
            if (GENERAL) {
                reinterpret_cast<ulonglong2*>(key64)[first + j] = make_ulonglong2((unsigned long long)e << 31 | (uint32_t)b, (unsigned long long)t << 31 | (uint32_t)b);
            } else {
                reinterpret_cast<uint2*>(key32)[first + j] = make_uint2(e, t);
                reinterpret_cast<int2*>(val)[first + j] = make_int2(b, b);
            }
        }
    }
}

// the KPT sorted keys of a thread from i0 on, as (edge << 31 | bc); 16-byte loads on whole groups (the arrays are the call's own, 256-byte
// aligned), single loads on the last, partial group.  Keys past n are not looked at by the callers.
template <bool GENERAL>
__device__ inline void ebc_load(const uint32_t* __restrict__ key32, const int32_t* __restrict__ val, const unsigned long long* __restrict__ key64, uint64_t i0, uint64_t n,
                                unsigned long long k[KPT]) {
    if (i0 + KPT <= n) {
        if (GENERAL) {
            const ulonglong2 a = reinterpret_cast<const ulonglong2*>(key64 + i0)[0], b = reinterpret_cast<const ulonglong2*>(key64 + i0)[1];
            k[0] = a.x; k[1] = a.y; k[2] = b.x; k[3] = b.y;
        } else {
            const uint4 e = *reinterpret_cast<const uint4*>(key32 + i0);
            const int4 b = *reinterpret_cast<const int4*>(val + i0);
            k[0] = (unsigned long long)e.x << 31 | (uint32_t)b.x; k[1] = (unsigned long long)e.y << 31 | (uint32_t)b.y;
            k[2] = (unsigned long long)e.z << 31 | (uint32_t)b.z; k[3] = (unsigned long long)e.w << 31 | (uint32_t)b.w;
        }
    } else {
        for (unsigned j = 0; j < KPT; ++j) {
            const uint64_t i = i0 + j;
            k[j] = i >= n ? 0ull : GENERAL ? key64[i] : (unsigned long long)key32[i] << 31 | (uint32_t)val[i];
        }
    }
}
template <bool GENERAL>
__device__ inline unsigned long long ebc_key_at(const uint32_t* __restrict__ key32, const int32_t* __restrict__ val, const unsigned long long* __restrict__ key64, uint64_t i) {
    return GENERAL ? key64[i] : (unsigned long long)key32[i] << 31 | (uint32_t)val[i];
}

// run heads per tile.  tile_heads has n_tiles + 1 entries; the last stays 0, so that its exclusive scan ends with the total.
template <bool GENERAL>
__global__ void __launch_bounds__(EB) ebc_heads_kernel(const uint32_t* __restrict__ key32, const int32_t* __restrict__ val, const unsigned long long* __restrict__ key64, uint64_t n,
                                                       uint64_t n_tiles, unsigned long long* __restrict__ tile_heads) {
    __shared__ uint32_t wg_heads;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (threadIdx.x == 0) wg_heads = 0;
        __syncthreads();
        const uint64_t i0 = tile * TILE + (uint64_t)threadIdx.x * KPT;
        uint32_t c = 0;
        if (i0 < n) {
            unsigned long long k[KPT];
            ebc_load<GENERAL>(key32, val, key64, i0, n, k);
            unsigned long long prev = i0 ? ebc_key_at<GENERAL>(key32, val, key64, i0 - 1) : ~0ull;
            for (unsigned j = 0; j < KPT && i0 + j < n; ++j) {
                c += k[j] != prev;
                prev = k[j];
            }
        }
        for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&wg_heads, c);
        __syncthreads();
        if (threadIdx.x == 0) tile_heads[tile] = wg_heads;
        __syncthreads();
    }
}

// tile_base = exclusive scan of the heads per tile (tile_base[n_tiles] = n_ebc).  Every head writes its barcode at its rank; a head whose
// edge differs from the key before it owns ebc_off[e] for every e in (that key's edge, its own edge]; the last key owns the tail.
template <bool GENERAL>
__global__ void __launch_bounds__(EB) ebc_compact_kernel(const uint32_t* __restrict__ key32, const int32_t* __restrict__ val, const unsigned long long* __restrict__ key64, uint64_t n,
                                                         uint64_t n_tiles, const unsigned long long* __restrict__ tile_base, uint64_t E, unsigned long long* __restrict__ off,
                                                         int32_t* __restrict__ ebc) {
    __shared__ uint32_t wave_heads[EB / 64];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i0 = tile * TILE + (uint64_t)threadIdx.x * KPT;
        unsigned long long k[KPT];
        unsigned long long before = ~0ull;
        uint32_t c = 0;
        if (i0 < n) {
            ebc_load<GENERAL>(key32, val, key64, i0, n, k);
            if (i0) before = ebc_key_at<GENERAL>(key32, val, key64, i0 - 1);
            unsigned long long prev = before;
            for (unsigned j = 0; j < KPT && i0 + j < n; ++j) {
                c += k[j] != prev;
                prev = k[j];
            }
        }
        // the heads in front of this lane inside the wave.  Every wave of the workgroup is here with all its lanes (the tile loop is
        // uniform, which the barriers below need as well): what snk_wave_scan_excl asks for
        uint32_t wave_total;
        const uint32_t excl = snk_wave_scan_excl(c, &wave_total);
        if (lane == 63) wave_heads[wave] = wave_total;
        __syncthreads();
        uint32_t base = 0;
        for (unsigned w = 0; w < wave; ++w) base += wave_heads[w];
        __syncthreads();                            // (wave_heads is written again in the next tile)
        if (i0 < n) {
            uint64_t rank = tile_base[tile] + base + excl;
            unsigned long long prev = before;
            for (unsigned j = 0; j < KPT && i0 + j < n; ++j) {
                if (k[j] != prev) {
                    ebc[rank] = (int32_t)(k[j] & 0x7FFFFFFFull);
                    const int64_t e_prev = i0 + j ? (int64_t)(prev >> 31) : -1, e = (int64_t)(k[j] >> 31);
                    for (int64_t x = e_prev + 1; x <= e; ++x) off[x] = rank;
                    ++rank;
                    prev = k[j];
                }
            }
            if (i0 + KPT >= n) {
                const unsigned long long total = tile_base[n_tiles];
                for (uint64_t x = (uint64_t)(prev >> 31) + 1; x <= E; ++x) off[x] = total;
            }
        }
    }
}

__global__ void __launch_bounds__(EB) ebc_zero_offsets_kernel(uint64_t E, unsigned long long* __restrict__ off) {
    for (uint64_t e = (uint64_t)blockIdx.x * EB + threadIdx.x; e <= E; e += (uint64_t)gridDim.x * EB) off[e] = 0;
}

__global__ void __launch_bounds__(EB) ebc_stats_kernel(const unsigned long long* __restrict__ off, uint64_t E, unsigned long long* __restrict__ stat /* [256] empty, [256] longest */) {
    __shared__ uint32_t wg_empty;
    __shared__ unsigned long long wg_max;
    if (threadIdx.x == 0) { wg_empty = 0; wg_max = 0; }
    __syncthreads();
    unsigned long long mx = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * EB; base < E; base += (uint64_t)gridDim.x * EB) {
        const uint64_t e = base + threadIdx.x;
        bool empty = false;
        if (e < E) {
            const unsigned long long len = off[e + 1] - off[e];
            empty = len == 0;
            mx = max(mx, len);
        }
        const unsigned long long me = __ballot(empty);
        if ((threadIdx.x & 63) == 0 && me) atomicAdd(&wg_empty, (uint32_t)__popcll(me));
    }
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned long long)__shfl_xor((long long)mx, o));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&wg_max, mx);
    __syncthreads();
    const uint32_t slot = blockIdx.x & 255u;
    if (threadIdx.x == 0 && wg_empty) atomicAdd(&stat[slot], (unsigned long long)wg_empty);
    if (threadIdx.x == 0 && wg_max > stat[256 + slot]) atomicMax(&stat[256 + slot], wg_max);
}

template <bool GENERAL>
int ebc_lists(snk_call& c, uint64_t n_keys, uint64_t E, uint32_t key_bits, uint32_t* key32a, uint32_t* key32b, int32_t* vala, int32_t* valb, unsigned long long* key64a,
              unsigned long long* key64b, unsigned long long* tile_heads, unsigned long long* tile_base, unsigned long long* off, int32_t* ebc, char* err, size_t errcap) {
    const hipStream_t st = c.st;
    const uint64_t n_tiles = snk_blocks(n_keys, TILE);
    int rc;
    if (GENERAL) {
        if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::radix_sort_keys(tmp, tb, key64a, key64b, (size_t)n_keys, 0u, key_bits + 31u, st); }))) return rc;
    } else {
        if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::radix_sort_pairs(tmp, tb, key32a, key32b, vala, valb, (size_t)n_keys, 0u, std::max(1u, key_bits), st); })))
            return rc;
    }
    SNK_HIP_TRY(snk_launch(ebc_heads_kernel<GENERAL>, snk_blocks_capped(n_tiles, 1, EBC_GRID_CAP), EB, 0, st, (const uint32_t*)key32b, (const int32_t*)valb,
                           (const unsigned long long*)key64b, n_keys, n_tiles, tile_heads));
    if ((rc = c.with_temp([&](void* tmp, size_t& tb) {
            return rocprim::exclusive_scan(tmp, tb, tile_heads, tile_base, 0ull, (size_t)(n_tiles + 1), rocprim::plus<unsigned long long>(), st);
        })))
        return rc;
    SNK_HIP_TRY(snk_launch(ebc_compact_kernel<GENERAL>, snk_blocks_capped(n_tiles, 1, EBC_GRID_CAP), EB, 0, st, (const uint32_t*)key32b, (const int32_t*)valb,
                           (const unsigned long long*)key64b, n_keys, n_tiles, (const unsigned long long*)tile_base, E, off, ebc));
    return SNK_OK;
}

}  // namespace

extern "C" int snk_dev_edge_barcodes(snk_ctx* ctx, const snk_dev_paths* paths, const void* d_bc, uint64_t E, const int32_t* inv, uint32_t flags, snk_dev_ebcx* out, void* stream,
                                     char* err, size_t errcap) {
    if (!ctx || !paths || !out || (E && !inv)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_edge_barcodes: NULL argument");
    memset(out, 0, sizeof *out);
    const uint64_t n = paths->n_edges_total, n_reads = paths->n_reads;
    if (n_reads && !d_bc) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_edge_barcodes: NULL argument (d_bc)");
    if (flags & ~SNK_EBC_GENERAL_SORT) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_edge_barcodes: unknown flag bits 0x%x", flags & ~SNK_EBC_GENERAL_SORT);
    if (E > 0x7FFFFFFFull) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_edge_barcodes: %llu HBV edges (edge ids are int32)", (unsigned long long)E);
    if (n_reads && (!paths->start || !paths->n_edges)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_edge_barcodes: paths without their device arrays");
    if (n && !paths->edges) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_edge_barcodes: paths without their device arrays");
    if ((uintptr_t)paths->edges & 3u) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_edge_barcodes: paths->edges is not 4-byte aligned");
    if (n && !E) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_edge_barcodes: %llu path entries on a graph without edges", (unsigned long long)n);
    if (n >= (1ull << 31))
        return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_edge_barcodes: 2^31 or more path entries in one call (two keys are sorted per entry)");
    if (n_reads >= (1ull << 32)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_edge_barcodes: 2^32 or more reads in one call");
    for (uint64_t e = 0; e < E; ++e) {
        const int64_t r = inv[e];
        if (r < 0 || (uint64_t)r >= E || (uint64_t)inv[r] != e)
            return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_edge_barcodes: inv is not an involution of [0, %llu) at edge %llu", (unsigned long long)E, (unsigned long long)e);
    }
    // the two lists stay until the context's next top-level call; the scan, the keys, the involution and the sort's own scratch go back to
    // the arena with the call.  ebc is sized for one entry per key before the number of distinct ones is known: no read-back in between
    return snk_call_run(ctx, stream, "snk_dev_edge_barcodes", out, err, errcap, [&](snk_call& c) -> int {
        const hipStream_t st = c.st;
        SNK_HIP_TRY(c.stamp());
        int rc;
        unsigned long long *off, *stat, *tile_heads = nullptr, *tile_base = nullptr, *key64a = nullptr, *key64b = nullptr;
        int32_t *ebc = nullptr, *d_inv, *vala = nullptr, *valb = nullptr;
        uint32_t *range, *key32a = nullptr, *key32b = nullptr;
        ebc_acc* acc;
        if ((rc = c.alloc(E + 1, &off)) || (rc = c.alloc(E, &d_inv)) || (rc = c.alloc(512, &stat)) || (rc = c.alloc(256 + 1, &range)) || (rc = c.alloc(n_reads, &acc))) return rc;
        SNK_HIP_TRY(hipMemsetAsync(stat, 0, 512 * 8, st));
        SNK_HIP_TRY(hipMemsetAsync(range, 0, 257 * 4, st));
        if (E) SNK_HIP_TRY(hipMemcpyAsync(d_inv, inv, E * 4, hipMemcpyHostToDevice, st));
        uint32_t key_bits = 0;
        while (key_bits < 32 && (1ull << key_bits) < E) ++key_bits;
        uint64_t n_keys = 0;
        uint32_t bc_sorted = 1, general = (flags & SNK_EBC_GENERAL_SORT) ? 1u : 0u;
        const unsigned long long* start = (const unsigned long long*)paths->start;
        const uint32_t* n_edges = (const uint32_t*)paths->n_edges;
        const int32_t *edges = (const int32_t*)paths->edges, *bc = (const int32_t*)d_bc;
        if (n_reads) {
            rocprim::transform_iterator<rocprim::counting_iterator<unsigned long long>, ebc_read, ebc_acc> in(rocprim::counting_iterator<unsigned long long>(0ull),
                                                                                                             ebc_read{bc, n_edges});
            if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::inclusive_scan(tmp, tb, in, acc, (size_t)n_reads, ebc_join(), st); }))) return rc;
            SNK_HIP_TRY(snk_launch(ebc_check_kernel, snk_blocks_capped(n_reads, EB, EBC_GRID_CAP), EB, 0, st, start, n_edges, bc, (const ebc_acc*)acc, n_reads, n, range + 256));
            if (n) SNK_HIP_TRY(snk_max_edge_id((const uint32_t*)edges, n, range, st));
            uint32_t h_range[257];
            ebc_acc h_last;
            SNK_HIP_TRY(hipMemcpyAsync(h_range, range, sizeof h_range, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(hipMemcpyAsync(&h_last, acc + (n_reads - 1), sizeof h_last, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(snk_sync(st));
            uint32_t emax = 0;
            for (int q = 0; q < 256; ++q) emax = std::max(emax, h_range[q]);
            if ((h_range[256] & F_TABLE) || h_last.n > n)
                return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_edge_barcodes: start / n_edges do not add up to n_edges_total = %llu", (unsigned long long)n);
            if (n && emax >= E)
                return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_edge_barcodes: a path holds edge id %lld, the graph has %llu edges", (long long)(int32_t)emax, (unsigned long long)E);
            n_keys = 2 * h_last.n;
            bc_sorted = (h_range[256] & F_UNSORTED) ? 0u : 1u;
            if (!bc_sorted) general = 1;
        }
        if ((rc = c.alloc(n_keys, &ebc))) return rc;
        if (n_keys) {
            const uint64_t n_tiles = snk_blocks(n_keys, TILE);
            if ((rc = c.alloc(n_tiles + 1, &tile_heads)) || (rc = c.alloc(n_tiles + 1, &tile_base))) return rc;
            SNK_HIP_TRY(hipMemsetAsync(tile_heads + n_tiles, 0, 8, st));
            if (general) {
                if ((rc = c.alloc(n_keys, &key64a)) || (rc = c.alloc(n_keys, &key64b))) return rc;
                SNK_HIP_TRY(snk_launch(ebc_emit_kernel<true>, snk_blocks_capped(n_reads, EB, EBC_GRID_CAP), EB, 0, st, start, n_edges, edges, bc, (const ebc_acc*)acc,
                                       (const int32_t*)d_inv, n_reads, n_keys / 2, key32a, vala, key64a));
                if ((rc = ebc_lists<true>(c, n_keys, E, key_bits, key32a, key32b, vala, valb, key64a, key64b, tile_heads, tile_base, off, ebc, err, errcap))) return rc;
            } else {
                if ((rc = c.alloc(n_keys, &key32a)) || (rc = c.alloc(n_keys, &key32b)) || (rc = c.alloc(n_keys, &vala)) || (rc = c.alloc(n_keys, &valb))) return rc;
                SNK_HIP_TRY(snk_launch(ebc_emit_kernel<false>, snk_blocks_capped(n_reads, EB, EBC_GRID_CAP), EB, 0, st, start, n_edges, edges, bc, (const ebc_acc*)acc,
                                       (const int32_t*)d_inv, n_reads, n_keys / 2, key32a, vala, key64a));
                if ((rc = ebc_lists<false>(c, n_keys, E, key_bits, key32a, key32b, vala, valb, key64a, key64b, tile_heads, tile_base, off, ebc, err, errcap))) return rc;
            }
        } else {
            SNK_HIP_TRY(snk_launch(ebc_zero_offsets_kernel, snk_blocks_capped(E + 1, EB, EBC_GRID_CAP), EB, 0, st, E, off));
        }
        if (E) SNK_HIP_TRY(snk_launch(ebc_stats_kernel, snk_blocks_capped(E, EB, EBC_GRID_CAP), EB, 0, st, (const unsigned long long*)off, E, stat));
        unsigned long long h_stat[512], h_n_ebc = 0;
        SNK_HIP_TRY(hipMemcpyAsync(h_stat, stat, sizeof h_stat, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(hipMemcpyAsync(&h_n_ebc, off + E, 8, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(c.stamp());
        SNK_HIP_TRY(snk_sync(st));
        uint64_t n_empty = 0, longest = 0;
        for (int q = 0; q < 256; ++q) { n_empty += h_stat[q]; longest = std::max<uint64_t>(longest, h_stat[256 + q]); }
        if (h_n_ebc > n_keys) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_edge_barcodes: %llu list entries from %llu keys", h_n_ebc, (unsigned long long)n_keys);
        out->n_hbv_edges = E;
        out->n_ebc = h_n_ebc;
        out->ebc_off = off;
        out->ebc = ebc;
        out->n_keys = n_keys;
        out->n_empty_edges = n_empty;
        out->max_list = longest;
        out->bc_sorted = bc_sorted;
        out->general_sort = general;
        out->key_bits = key_bits;
        out->ms = c.ms(0, 1);
        return c.end(SNK_OK, {off, ebc});
    });
}
