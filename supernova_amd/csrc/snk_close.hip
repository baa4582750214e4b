// snk_close.hip -- CloseGap and CloseGap2 on the device: the third step of StageFindPatch (10X/runstages/RunStages.cc:334-384) with
// STACKSTER=False, whose result DF keeps as closures.fastb (10X/DF.cc:645): for every pair of a.hops the closure sequences that
// StageInsertPatch puts into the graph.
//
// What it replaces: CloseGap / CloseGap2, lib/assembly/src/10X/Closomatic.cc:356-657, and what they call in paths/long/ReadStack.cc:
// GetOffsets1 (:1192-1512), readstack::Merge (:355-398), Consensus1 (:406-427), ColumnConsensus1 (:1841-1861), Trim (:714-725), Reverse
// (:346-353).  include/snk.h states the rules; here is how they run.
//
// A stack is never made.  A side of a pair is a list of rows (read id, pos, forward) in the reference's order; cell (row, column) is
// computed from the read's packed row, its quality row and pos (c_cell), through Trim's window [M - max_width, M) and Reverse.
//
// Passes.
//   c_pairs_kernel     the pair ids lie inside the graph (before anything indexes with them)
//   c_gather_kernel    one wave per (pair, side), lanes over the index entries of e, then of inv[e]: rows, forward rows and (CloseGap2) the
//                      follower entries (edge << 32 | distance) counted, then -- the host has made the offsets -- written in entry order
//                      (wave scans: no atomic, the order is the reference's)
//   segmented sort     rocPRIM, the follower entries of every (pair, side): a group of 5 or more is a run
//   c_bod_kernel       CloseGap2.  One wave per (pair, side): its follower groups and the 32-mers of their edges.  The host gives a pair with a
//                      side over bod_budget to the host routine, whole, and every other pair a hash table in device scratch (key + position,
//                      twice its larger side rounded up to a power of two); the tables of one launch share one block of at most C_TAB_CAP
//                      slots, so the pairs go in as many launches as that takes and the memory of a call is bounded
//   c_place_kernel     One workgroup per pair, twice (ei = 0, 1): the 32-mers of the follower edges of side 1 - ei into the pair's table,
//                      then one wave per distinct forward read of side ei
//                      whose partner is not a forward row of the other side: the partner's 32-mers are looked up, lanes over the places; exactly
//                      one distinct position - place puts it behind the rows of side 1 - ei.  The results land in the tail slots in row
//                      order and one wave compacts them (ballot + popcount), so the rows are in the reference's order
//   c_host_place       (host) the same placement for one pair with a std::unordered_multimap: no bound
//   c_close_kernel     one workgroup per pair: M of both sides, the column sums (one lane per column walks the rows in order: doubles
//                      added in the reference's order) and the two seed consensuses in LDS; the 8-mer seeds; per candidate offset the
//                      cumulative errors, the bad windows and per start the last admissible n, then lanes over `start` take minima over the
//                      table of log binomial sums (the hot loop: the table is read-only and stays in L2); bits >= 25; the invalidation,
//                      lanes over (offset, offset); big near small on one lane.  Result: at most two offsets and the closures' lengths
//   c_merge_kernel     after the host has summed the lengths: one workgroup per pair, lanes over the columns of the merged stack (stack 1's
//                      rows, then stack 2's), the HIGHEST base on a tie
// Nothing is placed by an atomic on a shared cursor, so the result is bit-identical from call to call.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <unordered_map>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "snk_bads.h"
#include "snk_call.h"
#include "snk_common.h"

namespace {

constexpr unsigned CB = 256;                       // lanes of a workgroup
constexpr uint64_t C_GRID_CAP = 1u << 16;
constexpr int MAX_OVERLAP = 1000;                  // ReadStack.cc:1213: a consensus of this many columns returns no offsets
constexpr int W_MIN = 20, WX = 40, MAX_EWX = 20, MIN_STRETCH = 8, FLANK = 10;          // :1205-1210, :1434
constexpr double MIN_BITS = 25.0, MIN_BITS_SAVE = 40.0, MIN_SLOPE = 2.0, MIN_ADD = 10.0;
constexpr int MIN_EDGE_COUNT = 5, L32 = 32;        // Closomatic.cc:494-495
constexpr int C_OFFS = 2 * MAX_OVERLAP;            // candidate offsets of two consensuses of fewer than 1000 columns
constexpr uint32_t C_BUDGET = 1u << 18;            // the most 32-mers the hash table of a pair takes (its slice is sized by what the pair needs: twice that, a power of two)
constexpr uint32_t C_MIN_SLOTS = 64;
constexpr unsigned long long C_TAB_CAP = 1ull << 26;   // slots (12 bytes each) the tables of one c_place_kernel launch share
constexpr int C_EMPTY = INT32_MIN;
constexpr unsigned long long C_NONE = ~0ull;
enum { PS_TRIED, PS_PLACED, N_PS };
enum { R_NOFF, R_O0, R_O1, R_C1, R_C2, R_M0, R_M1, R_KEPT, R_LONG, N_R = 10 };

// what the passes read: the paths, their index, per edge inv and Kmers, the reads.  The same struct serves the host routine.
struct c_view {
    const unsigned long long* start;
    const uint32_t* n_edges;
    const int32_t *edges, *offset;
    const unsigned long long *ioff, *iids;
    const int32_t *inv, *km;
    snk_reads_view R;
};
__host__ __device__ inline uint32_t c_hash(unsigned long long k, uint32_t mask) { return (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> 32) & mask; }

__global__ void __launch_bounds__(CB) c_pairs_kernel(const int32_t* __restrict__ pairs, uint64_t n2, uint64_t E, uint32_t* __restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * CB + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * CB)
        if (pairs[i] < 0 || (uint64_t)pairs[i] >= E) atomicOr(flag, 1u);
}
__global__ void __launch_bounds__(CB) c_km_kernel(path_graph G, int K, uint64_t E, int32_t* __restrict__ km) {
    for (uint64_t e = (uint64_t)blockIdx.x * CB + threadIdx.x; e < E; e += (uint64_t)gridDim.x * CB) km[e] = (int32_t)pg_edge_len(G, (int32_t)e) - K + 1;
}

// Closomatic.cc:381-392 and :505-531.  WRITE false: n_rows / n_fw / n_prec per (pair, side); true: the rows (id << 1 | forward, pos) at
// row_off and the follower entries at prec_off, both in entry order.
template <bool WRITE>
__global__ void __launch_bounds__(CB) c_gather_kernel(c_view V, uint64_t n_pairs, const int32_t* __restrict__ pairs, int cg2, uint32_t* __restrict__ n_rows,
                                                      uint32_t* __restrict__ n_fw, uint32_t* __restrict__ n_prec, const unsigned long long* __restrict__ row_off,
                                                      unsigned long long* __restrict__ row_idfw, int32_t* __restrict__ row_pos, const unsigned long long* __restrict__ prec_off,
                                                      unsigned long long* __restrict__ prec) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * CB + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * CB) >> 6;
    for (uint64_t item = wave; item < 2 * n_pairs; item += n_waves) {
        const int e = (item & 1) ? V.inv[pairs[item]] : pairs[item];          // es = { e1, inv[e2] }
        uint32_t rows_at = 0, prec_at = 0, fw = 0;
        for (int pass = 0; pass < 2; ++pass) {
            const int f = pass ? V.inv[e] : e;
            const unsigned long long a0 = V.ioff[f], n = V.ioff[f + 1] - a0;
            for (unsigned long long base = 0; base < n; base += 64) {
                const unsigned long long t = base + lane;
                uint32_t cr = 0, cp = 0;
                uint64_t r = 0;
                const int32_t* p = nullptr;
                int m = 0;
                if (t < n) {
                    r = V.iids[a0 + t];
                    p = V.edges + V.start[r];
                    m = (int)V.n_edges[r];
                    for (int j = 0; j < m; ++j)
                        if (p[j] == f) { ++cr; cp += (uint32_t)(pass ? j : m - 1 - j); }
                }
                if (!cg2) cp = 0;
                uint32_t tr, tp;                              // (reached by whole waves: item, pass and n are the wave's)
                const uint32_t er = snk_wave_scan_excl(cr, &tr), ep = snk_wave_scan_excl(cp, &tp);
                if (WRITE && cr) {
                    unsigned long long ra = row_off[item] + rows_at + er, pa = prec_off[item] + prec_at + ep;
                    int pos = V.offset[r];
                    for (int j = 0; j < m; ++j) {
                        if (p[j] == f) {
                            row_idfw[ra] = (unsigned long long)r << 1 | (pass ? 0ull : 1ull);
                            row_pos[ra++] = pos;
                            if (cg2) {
                                int add = 0;
                                if (!pass)
                                    for (int l = j + 1; l < m; ++l) { add += V.km[p[l - 1]]; prec[pa++] = (unsigned long long)(uint32_t)p[l] << 32 | (uint32_t)add; }
                                else
                                    for (int l = j - 1; l >= 0; --l) { add += V.km[p[l + 1]]; prec[pa++] = (unsigned long long)(uint32_t)V.inv[p[l]] << 32 | (uint32_t)add; }
                            }
                        }
                        pos -= V.km[p[j]];
                    }
                }
                rows_at += tr;
                prec_at += tp;
            }
            if (!pass) fw = rows_at;
        }
        if (!WRITE && lane == 0) { n_rows[item] = rows_at; n_fw[item] = fw; n_prec[item] = prec_at; }
    }
}

// is read id a forward row of the side whose rows begin at row_idfw (its first n_fw rows, ascending ids)
__host__ __device__ inline bool c_fw_member(const unsigned long long* row_idfw, uint32_t n_fw, uint64_t id) {
    uint32_t lo = 0, hi = n_fw;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if ((row_idfw[mid] >> 1) < id) lo = mid + 1; else hi = mid;
    }
    return lo < n_fw && (row_idfw[lo] >> 1) == id;
}

// entry i of the sorted follower entries [lo, hi) begins a group of MIN_EDGE_COUNT or more identical ones (Closomatic.cc:534-538).  Host and device.
__host__ __device__ inline bool c_is_head(const unsigned long long* prec, unsigned long long lo, unsigned long long hi, unsigned long long i) {
    return (i == lo || prec[i - 1] != prec[i]) && i + (MIN_EDGE_COUNT - 1) < hi && prec[i + (MIN_EDGE_COUNT - 1)] == prec[i];
}

// the follower groups of every (pair, side) and the 32-mers of their edges: what its hash table has to hold.  One wave per (pair, side)
// over its sorted entries.
__global__ void __launch_bounds__(CB) c_bod_kernel(path_graph G, uint64_t n2, const unsigned long long* __restrict__ prec_off, const unsigned long long* __restrict__ prec,
                                                   unsigned long long* __restrict__ bod_n, uint32_t* __restrict__ foll_n) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * CB + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * CB) >> 6;
    for (uint64_t item = wave; item < n2; item += n_waves) {
        const unsigned long long lo = prec_off[item], hi = prec_off[item + 1];
        unsigned long long sum = 0;
        uint32_t groups = 0;
        for (unsigned long long i = lo + lane; i < hi; i += 64)
            if (c_is_head(prec, lo, hi, i)) {
                const int nk = (int)pg_edge_len(G, (int32_t)(prec[i] >> 32)) - L32 + 1;
                sum += (unsigned long long)(nk > 0 ? nk : 0);
                ++groups;
            }
        for (int o = 32; o > 0; o >>= 1) {
            sum += (unsigned long long)__shfl_xor((long long)sum, o);
            groups += (uint32_t)__shfl_xor((int)groups, o);
        }
        if (lane == 0) { bod_n[item] = sum; foll_n[item] = groups; }
    }
}

// Closomatic.cc:532-581 for pairs [p_begin, p_end), one per workgroup; a pair with over[p] is the host's and is left alone.  The table of
// pair p is tab_off[p] - tab_off[p_begin] slots into tab_key / tab_pos.  pstat: [n_pairs][N_PS].
__global__ void __launch_bounds__(CB) c_place_kernel(c_view V, path_graph G, uint64_t p_begin, uint64_t p_end, const uint8_t* __restrict__ over,
                                                     const unsigned long long* __restrict__ row_off, const uint32_t* __restrict__ n_rows0, const uint32_t* __restrict__ n_fw,
                                                     unsigned long long* __restrict__ row_idfw, int32_t* __restrict__ row_pos, const unsigned long long* __restrict__ prec_off,
                                                     const unsigned long long* __restrict__ prec, const unsigned long long* __restrict__ bod_n,
                                                     const unsigned long long* __restrict__ tab_off, unsigned long long* __restrict__ tab_key, int* __restrict__ tab_pos,
                                                     uint32_t* __restrict__ n_rows_final, uint32_t* __restrict__ pstat) {
    __shared__ uint32_t s_head[CB];
    __shared__ uint32_t s_tried;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint64_t p = p_begin + blockIdx.x; p < p_end; p += gridDim.x) {
        if (over[p]) continue;                                             // (uniform)
        unsigned long long* h_key = tab_key + (tab_off[p] - tab_off[p_begin]);      // this pair's table: a power of two of slots, at most half full
        int* h_pos = tab_pos + (tab_off[p] - tab_off[p_begin]);
        const uint32_t slots = (uint32_t)(tab_off[p + 1] - tab_off[p]), mask = slots - 1;
        __syncthreads();
        if (tid == 0) s_tried = 0;
        uint32_t placed_total = 0;
        for (int ei = 0; ei < 2; ++ei) {
            const int t = 1 - ei;
            const unsigned long long lo = prec_off[2 * p + t], hi = prec_off[2 * p + t + 1];
            const bool empty = bod_n[2 * p + t] == 0;
            // ---- bod of side t: the 32-mers of its follower edges into the table
            if (!empty) {
                for (uint32_t i = tid; i < slots; i += CB) h_pos[i] = C_EMPTY;
                __syncthreads();
                for (unsigned long long base = lo; base < hi; base += CB) {
                    s_head[tid] = base + tid < hi && c_is_head(prec, lo, hi, base + tid) ? 1u : 0u;
                    __syncthreads();
                    for (unsigned q = 0; q < CB; ++q) {
                        if (!s_head[q]) continue;
                        const unsigned long long key = prec[base + q];
                        const int g = (int)(key >> 32), add = (int)(uint32_t)key, nk = (int)pg_edge_len(G, g) - L32 + 1;
                        for (int l = (int)tid; l < nk; l += (int)CB) {
                            unsigned long long x = 0;
                            for (int b = 0; b < L32; ++b) x = x << 2 | pg_edge_base(G, g, (uint32_t)(l + b));
                            uint32_t slot = c_hash(x, mask);
                            while (atomicCAS(&h_pos[slot], C_EMPTY, add + l) != C_EMPTY) slot = (slot + 1) & mask;      // (at most slots / 2 entries: ends)
                            h_key[slot] = x;
                        }
                    }
                    __syncthreads();
                }
            }
            __syncthreads();
            // ---- the partners of side ei's forward reads, one wave each; fw row k of side ei answers in tail slot k of side t
            const unsigned long long r_e = row_off[2 * p + ei], r_t = row_off[2 * p + t], tail = r_t + n_rows0[2 * p + t];
            const uint32_t F = n_fw[2 * p + ei], Ft = n_fw[2 * p + t];
            uint32_t tried = 0;
            for (uint32_t k = wave; k < F; k += CB / 64) {
                const uint64_t id1 = row_idfw[r_e + k] >> 1, id2 = id1 ^ 1ull;
                const bool cand = (k == 0 || (row_idfw[r_e + k - 1] >> 1) != id1) && !c_fw_member(row_idfw + r_t, Ft, id2);
                int state = 0, v0 = 0;                                   // 0: not found, 1: one distinct position, 2: more
                if (cand) {
                    ++tried;
                    if (!empty) {
                        const uint32_t* row = V.R.rows + id2 * V.R.row_words;
                        const int len = (int)snk_read_len(V.R, id2);
                        for (int l = (int)lane; l + L32 <= len; l += 64) {
                            unsigned long long x = 0;
                            for (int b = 0; b < L32; ++b) x = x << 2 | snk_row_base(row, (uint32_t)(l + b));
                            for (uint32_t slot = c_hash(x, mask); h_pos[slot] != C_EMPTY; slot = (slot + 1) & mask) {
                                if (h_key[slot] != x) continue;
                                const int v = h_pos[slot] - l;
                                if (state == 0) { state = 1; v0 = v; }
                                else if (v != v0) state = 2;
                            }
                        }
                    }
                }
                for (int o = 32; o > 0; o >>= 1) {
                    const int os = __shfl_xor(state, o), ov = __shfl_xor(v0, o);
                    if (os == 0) continue;
                    if (state == 0) { state = os; v0 = ov; }
                    else if (os == 2 || state == 2 || ov != v0) state = 2;
                }
                if (lane == 0) {
                    row_idfw[tail + k] = state == 1 ? (id2 << 1 | 1ull) : C_NONE;
                    row_pos[tail + k] = v0;
                }
            }
            if (lane == 0 && tried) atomicAdd(&s_tried, tried);
            __syncthreads();
            // ---- the placed ones, kept in row order
            if (wave == 0) {
                uint32_t w = 0;
                for (uint32_t base = 0; base < F; base += 64) {
                    const uint32_t k = base + lane;
                    unsigned long long idv = C_NONE;
                    int pv = 0;
                    if (k < F) { idv = row_idfw[tail + k]; pv = row_pos[tail + k]; }
                    const unsigned long long keep = __ballot(idv != C_NONE);
                    if (idv != C_NONE) {
                        const uint32_t at = w + (uint32_t)__popcll(keep & ((1ull << lane) - 1ull));
                        row_idfw[tail + at] = idv;
                        row_pos[tail + at] = pv;
                    }
                    w += (uint32_t)__popcll(keep);
                }
                if (lane == 0) n_rows_final[2 * p + t] = n_rows0[2 * p + t] + w;
                placed_total += w;
            }
            __syncthreads();
        }
        if (tid == 0) {
            pstat[p * N_PS + PS_TRIED] = s_tried;
            pstat[p * N_PS + PS_PLACED] = placed_total;
        }
    }
}

// a side of a pair as the later passes see it
struct c_side {
    unsigned long long r0;   // its rows
    uint32_t n;
    int ne, M, T, cols, rev;
};
// cell (row, column c) of the side's stack after Trim and Reverse: false = blank
__device__ __forceinline__ bool c_cell(const c_view& V, const c_side& S, unsigned long long idfw, int pos, int c, int* base, int* qual) {
    const int u = (S.rev ? S.cols - 1 - c : c) + S.T;          // column of the untrimmed stack
    const uint64_t id = idfw >> 1;
    const bool fw = idfw & 1ull;
    const int j = fw ? u - pos : S.ne - 1 - u - pos;
    if (j < 0 || j >= (int)snk_read_len(V.R, id)) return false;
    int b = (int)snk_row_base(V.R.rows + id * V.R.row_words, (uint32_t)j);
    if (!fw) b = 3 - b;
    if (S.rev) b = 3 - b;
    *base = b;
    *qual = (int)V.R.quals[id * V.R.qstride + j];
    return true;
}
__device__ __forceinline__ double c_weight(int q) { return q == 0 ? 0.1 : q <= 2 ? 0.2 : (double)q; }          // Q0 counts 0.1, Q1 and Q2 0.2

// does offset oa invalidate offset ob (ReadStack.cc:1422-1476): a mismatch (p1, p2) of ob both of whose positions oa validates -- they lie
// FLANK or more inside a run of agreement of oa
__device__ inline bool c_interior(const uint8_t* con1, int c1, const uint8_t* con2, int c2, int oa, int x) {
    const int lo = oa > 0 ? oa : 0, hi = c1 < c2 + oa ? c1 : c2 + oa;
    if (x - FLANK < lo || x + FLANK >= hi) return false;
    for (int d = -FLANK; d <= FLANK; ++d)
        if (con1[x + d] != con2[x + d - oa]) return false;
    return true;
}
__device__ inline bool c_invalidates(const uint8_t* con1, int c1, const uint8_t* con2, int c2, int oa, int ob) {
    const int lo = ob > 0 ? ob : 0, hi = c1 < c2 + ob ? c1 : c2 + ob;
    for (int p1 = lo; p1 < hi; ++p1) {
        const int p2 = p1 - ob;
        if (con1[p1] == con2[p2]) continue;
        if (c_interior(con1, c1, con2, c2, oa, p1) && c_interior(con1, c1, con2, c2, oa, p2 + oa)) return true;
    }
    return false;
}

__device__ inline void c_side_of(const c_view& V, const path_graph& G, const int32_t* pairs, const unsigned long long* row_off, const uint32_t* n_rows_final, uint64_t p, int s,
                                 int M, int max_width, c_side* S) {
    const int e2 = pairs[2 * p + 1], e = s ? V.inv[e2] : pairs[2 * p];
    S->r0 = row_off[2 * p + s];
    S->n = n_rows_final[2 * p + s];
    S->ne = (int)pg_edge_len(G, e);
    S->M = M;
    S->T = M > max_width ? M - max_width : 0;
    S->cols = M - S->T;
    S->rev = e == V.inv[e2];
}

// GetOffsets1 for one pair per workgroup.  res: [n_pairs][N_R].
__global__ void __launch_bounds__(CB) c_close_kernel(c_view V, path_graph G, uint64_t n_pairs, const int32_t* __restrict__ pairs, const unsigned long long* __restrict__ row_off,
                                                     const uint32_t* __restrict__ n_rows_final, const unsigned long long* __restrict__ row_idfw, const int32_t* __restrict__ row_pos,
                                                     int max_width, const double* __restrict__ tab, int32_t* __restrict__ res) {
    __shared__ uint8_t con[2][MAX_OVERLAP];
    __shared__ uint16_t kmer[2][MAX_OVERLAP];
    __shared__ uint8_t s_cand[C_OFFS], s_flag[C_OFFS];
    __shared__ uint16_t s_se[MAX_OVERLAP + 1], s_lim[MAX_OVERLAP];
    __shared__ uint8_t s_bw[MAX_OVERLAP + 1];
    __shared__ int s_off[C_OFFS];
    __shared__ double s_bits[C_OFFS];
    __shared__ double s_min[CB / 64];
    __shared__ int s_M[2], s_kept, s_ns;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint64_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        __syncthreads();
        if (tid == 0) { s_M[0] = s_M[1] = 0; s_kept = 0; s_ns = 0; }
        __syncthreads();
        c_side S[2];
        // ---- M over ALL rows of a side (Closomatic.cc:396-402)
        for (int s = 0; s < 2; ++s) {
            c_side_of(V, G, pairs, row_off, n_rows_final, p, s, 0, max_width, &S[s]);
            int m = 0;
            for (uint32_t r = tid; r < S[s].n; r += CB) {
                const unsigned long long idfw = row_idfw[S[s].r0 + r];
                const int pos = row_pos[S[s].r0 + r], v = (idfw & 1ull) ? pos + (int)snk_read_len(V.R, idfw >> 1) : S[s].ne - pos;
                m = v > m ? v : m;
            }
            if (m) atomicMax(&s_M[s], m);
        }
        __syncthreads();
        for (int s = 0; s < 2; ++s) {
            c_side_of(V, G, pairs, row_off, n_rows_final, p, s, s_M[s], max_width, &S[s]);
            // the rows Trim keeps: all of them without a trim, else those with a cell in the window
            int kept = 0;
            for (uint32_t r = tid; r < S[s].n; r += CB) {
                const unsigned long long idfw = row_idfw[S[s].r0 + r];
                const int pos = row_pos[S[s].r0 + r], len = (int)snk_read_len(V.R, idfw >> 1);
                kept += S[s].T == 0 || (len > 0 && ((idfw & 1ull) ? pos + len : S[s].ne - pos) > S[s].T);
            }
            if (kept) atomicAdd(&s_kept, kept);
        }
        const int c1 = S[0].cols, c2 = S[1].cols;
        const bool too_long = c1 >= MAX_OVERLAP || c2 >= MAX_OVERLAP;
        int n_off = 0, o_out[2] = {0, 0};
        if (!too_long) {
            // ---- the seed consensus of both sides: the LOWEST base on a tie (ColumnConsensus1)
            for (int s = 0; s < 2; ++s)
                for (int c = (int)tid; c < S[s].cols; c += (int)CB) {
                    double sum[4] = {0., 0., 0., 0.};
                    for (uint32_t r = 0; r < S[s].n; ++r) {
                        int b, q;
                        if (c_cell(V, S[s], row_idfw[S[s].r0 + r], row_pos[S[s].r0 + r], c, &b, &q)) sum[b] += c_weight(q);
                    }
                    int best = 0;
                    for (int b = 1; b < 4; ++b)
                        if (sum[b] > sum[best]) best = b;
                    con[s][c] = (uint8_t)best;
                }
            for (uint32_t i = tid; i < (uint32_t)C_OFFS; i += CB) s_cand[i] = 0;
            __syncthreads();
            // ---- 8-mer seeds -> candidate offsets
            const int n1 = c1 - MIN_STRETCH + 1, n2 = c2 - MIN_STRETCH + 1;
            for (int s = 0; s < 2; ++s)
                for (int i = (int)tid; i < (s ? n2 : n1); i += (int)CB) {
                    uint32_t x = 0;
                    for (int b = 0; b < MIN_STRETCH; ++b) x = x << 2 | con[s][i + b];
                    kmer[s][i] = (uint16_t)x;
                }
            __syncthreads();
            if (n1 > 0 && n2 > 0)
                for (int idx = (int)tid; idx < n1 * n2; idx += (int)CB) {
                    const int i = idx / n2, j = idx - i * n2;
                    if (kmer[0][i] == kmer[1][j]) s_cand[i - j + c2] = 1;
                }
            __syncthreads();
            // ---- per candidate offset, ascending: overlap, errors, bad windows, bits
            for (int idx = 0; idx < C_OFFS; ++idx) {
                if (!s_cand[idx]) continue;                               // (uniform)
                const int o = idx - c2, lo = o > 0 ? o : 0, hi = c1 < c2 + o ? c1 : c2 + o, overlap = hi - lo;
                if (wave == 0) {                                          // cumulative errors (sum_errors)
                    uint32_t carry = 0;
                    if (lane == 0) s_se[0] = 0;
                    for (int base = 0; base < overlap; base += 64) {
                        const int m = base + (int)lane;
                        const bool e = m < overlap && con[0][lo + m] != con[1][lo + m - o];
                        const unsigned long long mask = __ballot(e);
                        if (m < overlap) s_se[m + 1] = (uint16_t)(carry + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)) + (e ? 1u : 0u));
                        carry += (uint32_t)__popcll(mask);
                    }
                }
                __syncthreads();
                // bad_window[b] (:1292-1304): errs over (m - wx, m] >= max_ewx marks max(0, m - wx), m = 0 .. overlap - wx
                for (int b = (int)tid; b <= overlap; b += (int)CB) {
                    bool bad = false;
                    if (b == 0) {
                        for (int m = 0; m <= WX && m <= overlap - WX; ++m) bad |= (int)s_se[m + 1] - (int)s_se[m - WX + 1 > 0 ? m - WX + 1 : 0] >= MAX_EWX;
                    } else if (b + WX <= overlap - WX) {
                        bad = (int)s_se[b + WX + 1] - (int)s_se[b + 1] >= MAX_EWX;
                    }
                    s_bw[b] = bad ? 1 : 0;
                }
                __syncthreads();
                if (wave == 0) {                                          // per start the last n the loop reaches (:1307-1325)
                    int carry = 1 << 20;                                  // first bad window at or behind `start`
                    for (int top = overlap - 1; top >= 0; top -= 64) {
                        const int b = top - (int)lane;
                        int nb = (b >= 0 && s_bw[b]) ? b : 1 << 20;
                        for (int d = 1; d < 64; d <<= 1) {                // minimum over the lanes in front (= larger b)
                            const int up = __shfl_up(nb, d);
                            if (lane >= (unsigned)d) nb = up < nb ? up : nb;
                        }
                        nb = nb < carry ? nb : carry;
                        if (b >= 0) {
                            const int a = overlap - b, c = nb + (WX - 1) - b;
                            s_lim[b] = (uint16_t)(a < c ? a : c);
                        }
                        carry = __shfl(nb, 63);
                    }
                }
                __syncthreads();
                double minp = 0.;
                for (int start = (int)tid; start < overlap; start += (int)CB) {
                    const int L = (int)s_lim[start], s0 = (int)s_se[start];
                    for (int n = W_MIN; n <= L; ++n) {
                        const double v = tab[n * MAX_OVERLAP + ((int)s_se[start + n] - s0)];
                        minp = v < minp ? v : minp;
                    }
                }
                for (int d = 32; d > 0; d >>= 1) {
                    const double v = __shfl_xor(minp, d);
                    minp = v < minp ? v : minp;
                }
                if (lane == 0) s_min[wave] = minp;
                __syncthreads();
                if (tid == 0) {
                    for (unsigned w = 1; w < CB / 64; ++w) minp = s_min[w] < minp ? s_min[w] : minp;
                    const double bits = -minp * 10.0 / 6.0;
                    if (bits >= MIN_BITS) { s_off[s_ns] = o; s_bits[s_ns] = bits; ++s_ns; }
                }
                __syncthreads();
            }
            // ---- offsets that invalidate other offsets (:1422-1485)
            int ns = s_ns;
            for (int i = (int)tid; i < ns; i += (int)CB) s_cand[i] = 0, s_flag[i] = 0;          // invalidated[i], to_delete[i]
            __syncthreads();
            for (int idx = (int)tid; idx < ns * ns; idx += (int)CB) {
                const int j = idx / ns, i = idx - j * ns;
                if (j != i && !s_cand[i] && c_invalidates(con[0], c1, con[1], c2, s_off[j], s_off[i])) s_cand[i] = 1;
            }
            __syncthreads();
            for (int idx = (int)tid; idx < ns * ns; idx += (int)CB) {
                const int i = idx / ns, j = idx - i * ns;
                if (j != i && !s_cand[i] && !s_flag[j] && c_invalidates(con[0], c1, con[1], c2, s_off[i], s_off[j])) s_flag[j] = 1;
            }
            __syncthreads();
            if (tid == 0) {
                int m = 0;
                for (int i = 0; i < ns; ++i)
                    if (!s_flag[i]) { s_off[m] = s_off[i]; s_bits[m] = s_bits[i]; ++m; }
                ns = m;
                // big near small: delete small (:1487-1502)
                for (int i = 0; i < ns; ++i) s_flag[i] = 0;
                for (int i1 = 0; i1 < ns; ++i1)
                    for (int i2 = 0; i2 < ns; ++i2) {
                        if (s_flag[i1]) continue;
                        if (s_bits[i2] >= MIN_BITS_SAVE) continue;
                        const double delta = s_bits[i1] - s_bits[i2];
                        if (delta < MIN_ADD) continue;
                        const int d = s_off[i1] - s_off[i2];
                        if (delta / (double)(d < 0 ? -d : d) < MIN_SLOPE) continue;
                        s_flag[i2] = 1;
                    }
                m = 0;
                for (int i = 0; i < ns; ++i)
                    if (!s_flag[i]) { s_off[m] = s_off[i]; ++m; }
                s_ns = m;
            }
            __syncthreads();
            n_off = s_ns;
            if (n_off <= 2)
                for (int i = 0; i < n_off; ++i) o_out[i] = s_off[i];
        }
        __syncthreads();
        if (tid == 0) {
            int32_t* r = res + p * N_R;
            r[R_NOFF] = n_off > 2 ? 3 : n_off;
            r[R_O0] = o_out[0]; r[R_O1] = o_out[1];
            r[R_C1] = c1; r[R_C2] = c2;
            r[R_M0] = S[0].M; r[R_M1] = S[1].M;
            r[R_KEPT] = s_kept;
            r[R_LONG] = too_long ? 1 : 0;
        }
    }
}

// readstack::Merge + Consensus1(con, conq) for the one or two offsets of a pair: the closures' bases at closure_off[pair_first[p] ..]
__global__ void __launch_bounds__(CB) c_merge_kernel(c_view V, path_graph G, uint64_t n_pairs, const int32_t* __restrict__ pairs, const unsigned long long* __restrict__ row_off,
                                                     const uint32_t* __restrict__ n_rows_final, const unsigned long long* __restrict__ row_idfw, const int32_t* __restrict__ row_pos,
                                                     int max_width, const int32_t* __restrict__ res, const unsigned long long* __restrict__ pair_first,
                                                     const unsigned long long* __restrict__ closure_off, uint8_t* __restrict__ bases) {
    for (uint64_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const int32_t* r = res + p * N_R;
        const int n_off = r[R_NOFF];
        if (n_off < 1 || n_off > 2) continue;
        c_side S[2];
        for (int s = 0; s < 2; ++s) c_side_of(V, G, pairs, row_off, n_rows_final, p, s, r[R_M0 + s], max_width, &S[s]);
        for (int q = 0; q < n_off; ++q) {
            const int o = r[R_O0 + q], left1 = o < 0 ? -o : 0, left2 = o > 0 ? o : 0;
            const unsigned long long at = closure_off[pair_first[p] + q];
            const int len = (int)(closure_off[pair_first[p] + q + 1] - at);
            for (int x = (int)threadIdx.x; x < len; x += (int)CB) {
                double sum[4] = {0., 0., 0., 0.};
                for (int s = 0; s < 2; ++s) {
                    const int c = x - (s ? left2 : left1);
                    if (c < 0 || c >= S[s].cols) continue;
                    for (uint32_t i = 0; i < S[s].n; ++i) {
                        int b, ql;
                        if (c_cell(V, S[s], row_idfw[S[s].r0 + i], row_pos[S[s].r0 + i], c, &b, &ql)) sum[b] += c_weight(ql);
                    }
                }
                int best = 3;                                             // sorted descending as pair<double,int>: the HIGHEST base on a tie
                for (int b = 2; b >= 0; --b)
                    if (sum[b] > sum[best]) best = b;
                bases[at + (unsigned long long)x] = (uint8_t)best;
            }
        }
    }
}

// PrecomputedBinomialSums<1000>(20, 0.75) (ReadStack.cc:47-62) with BinomialSum's arithmetic (random/Bernoulli.cc:40-50): long double
// accumulation from pow(0.25, n), log10 of the sum as a double.  Entries never written are 0.0.  Made once per context.
int c_table(snk_ctx* ctx, const double** d_tab, char* err, size_t errcap) {
    if (!ctx->close_table) {
        std::vector<double> t((size_t)MAX_OVERLAP * MAX_OVERLAP, 0.0);
        const double p = 0.75;
        for (int n = W_MIN; n < MAX_OVERLAP; ++n) {
            long double sum = 0, choose = 1.0, product = pow(1.0 - p, double(n));
            for (int k = 0; k < n; ++k) {
                sum += choose * product;
                choose *= double(n - k);
                choose /= double(k + 1);
                product *= p / (1.0 - p);
                t[(size_t)n * MAX_OVERLAP + k] = log10((double)sum);
            }
        }
        void* d = nullptr;
        SNK_HIP_TRY(hipMalloc(&d, t.size() * 8));
        const hipError_t e = hipMemcpy(d, t.data(), t.size() * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d); SNK_HIP_TRY(e); }
        ctx->close_table = d;
        ctx->close_table_free = [](void* q) { (void)hipFree(q); };
    }
    *d_tab = (const double*)ctx->close_table;
    return SNK_OK;
}

// reads ids[0 .. n): their packed rows one behind the other, and their lengths (what the host placement looks up)
__global__ void __launch_bounds__(CB) c_fetch_kernel(c_view V, const unsigned long long* __restrict__ ids, uint64_t n, uint32_t* __restrict__ rows_out, uint16_t* __restrict__ lens_out) {
    for (uint64_t i = (uint64_t)blockIdx.x * CB + threadIdx.x; i < n * V.R.row_words; i += (uint64_t)gridDim.x * CB) {
        const uint64_t r = i / V.R.row_words, w = i - r * V.R.row_words;
        rows_out[i] = V.R.rows[ids[r] * V.R.row_words + w];
        if (w == 0) lens_out[r] = (uint16_t)snk_read_len(V.R, ids[r]);
    }
}

struct c_host_graph {          // what the host placement needs of the graph: per edge its unitig and strand, the unitig offsets
    const path_host* H;
    std::vector<unsigned long long> uoff;
    const uint8_t* d_ubases;
};

// Closomatic.cc:532-581 for one pair on the host: no bound.  rows / pos: the pair's rows of both sides (R rows each, room for the tail
// behind them); prec: its sorted follower entries per side.  -> rows placed per side; tried counted.
int c_host_place(snk_call& c, const c_view& DV, const c_host_graph& HG, const std::vector<unsigned long long> (&rows)[2], const uint32_t (&F)[2], const std::vector<unsigned long long> (&prec)[2],
                 std::vector<unsigned long long> (&add_id)[2], std::vector<int32_t> (&add_pos)[2], uint32_t* tried, char* err, size_t errcap) {
    std::vector<uint8_t> eb;
    for (int ei = 0; ei < 2; ++ei) {
        const int t = 1 - ei;
        std::unordered_multimap<unsigned long long, int> bod;
        const std::vector<unsigned long long>& P = prec[t];
        for (size_t i = 0; i < P.size(); ++i) {
            if (c_is_head(P.data(), 0, P.size(), i)) {
                const int g = (int)(P[i] >> 32), add = (int)(uint32_t)P[i];
                const uint32_t u = (uint32_t)HG.H->eu[g];
                const unsigned long long o = HG.uoff[u];
                const int len = (int)(HG.uoff[u + 1] - o);
                eb.resize((size_t)len);
                if (len) SNK_HIP_TRY(hipMemcpy(eb.data(), HG.d_ubases + o, (size_t)len, hipMemcpyDeviceToHost));
                const bool rc = HG.H->erc[g];
                for (int l = 0; l + L32 <= len; ++l) {
                    unsigned long long x = 0;
                    for (int b = 0; b < L32; ++b) x = x << 2 | (rc ? 3u - eb[(size_t)(len - 1 - (l + b))] : eb[(size_t)(l + b)]);
                    bod.emplace(x, add + l);
                }
            }
        }
        // the partners to look up, in row order; their rows and lengths come down in one copy
        std::vector<unsigned long long> ids;
        for (uint32_t k = 0; k < F[ei]; ++k) {
            const uint64_t id1 = rows[ei][k] >> 1, id2 = id1 ^ 1ull;
            if (k && (rows[ei][k - 1] >> 1) == id1) continue;
            if (c_fw_member(rows[t].data(), F[t], id2)) continue;
            ++*tried;
            ids.push_back(id2);
        }
        if (bod.empty() || ids.empty()) continue;
        const size_t m = ids.size(), rw = DV.R.row_words;
        unsigned long long* d_ids;
        uint32_t* d_rows;
        uint16_t* d_lens;
        int rc;
        if ((rc = c.alloc(m, &d_ids)) || (rc = c.alloc(m * rw, &d_rows)) || (rc = c.alloc(m, &d_lens))) return rc;
        std::vector<uint32_t> h_rows(m * rw);
        std::vector<uint16_t> h_lens(m);
        SNK_HIP_TRY(hipMemcpyAsync(d_ids, ids.data(), m * 8, hipMemcpyHostToDevice, c.st));
        SNK_HIP_TRY(snk_launch(c_fetch_kernel, snk_blocks_capped(m * rw, CB, C_GRID_CAP), CB, 0, c.st, DV, (const unsigned long long*)d_ids, (uint64_t)m, d_rows, d_lens));
        SNK_HIP_TRY(hipMemcpyAsync(h_rows.data(), d_rows, m * rw * 4, hipMemcpyDeviceToHost, c.st));
        SNK_HIP_TRY(hipMemcpyAsync(h_lens.data(), d_lens, m * 2, hipMemcpyDeviceToHost, c.st));
        SNK_HIP_TRY(snk_sync(c.st));
        snk_ctx_release_block(c.ctx, d_ids); snk_ctx_release_block(c.ctx, d_rows); snk_ctx_release_block(c.ctx, d_lens);      // (back to the arena: the next pair takes them again)
        for (size_t q = 0; q < m; ++q) {
            const uint32_t* row = h_rows.data() + q * rw;
            const int len = (int)h_lens[q];
            std::set<int> finds;
            for (int l = 0; l + L32 <= len; ++l) {
                unsigned long long x = 0;
                for (int b = 0; b < L32; ++b) x = x << 2 | snk_row_base(row, (uint32_t)(l + b));
                const auto range = bod.equal_range(x);
                for (auto it = range.first; it != range.second; ++it) finds.insert(it->second - l);
            }
            if (finds.size() == 1) { add_id[t].push_back(ids[q] << 1 | 1ull); add_pos[t].push_back(*finds.begin()); }
        }
    }
    return SNK_OK;
}

}  // namespace

extern "C" int snk_dev_close_gaps(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, const snk_hbv* h, const int32_t* inv,
                                  const snk_dev_reads* in, const snk_dev_paths* paths, const snk_dev_pidx* px, uint64_t n_pairs, const void* d_pairs, uint32_t max_width,
                                  uint32_t flags, uint32_t bod_budget, snk_dev_closures* out, void* stream, char* err, size_t errcap) {
    static const char who[] = "snk_dev_close_gaps";
    if (out) memset(out, 0, sizeof *out);
    if (!ctx || !h || !paths || !out) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument", who);
    if (flags & ~(SNK_CLOSE_CG1 | SNK_CLOSE_PLACE_HOST)) return snk_fail(SNK_E_ARG, err, errcap, "%s: unknown flag bits 0x%x", who, flags & ~(SNK_CLOSE_CG1 | SNK_CLOSE_PLACE_HOST));
    if (n_pairs && (!in || !in->rows || !in->quals)) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL reads (packed rows and quality rows) with %llu pairs", who, (unsigned long long)n_pairs);
    if (n_pairs && !d_pairs) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument (d_pairs)", who);
    if (in && in->n_reads != paths->n_reads) return snk_fail(SNK_E_ARG, err, errcap, "%s: %llu paths for %llu reads", who, (unsigned long long)paths->n_reads, (unsigned long long)in->n_reads);
    const uint64_t n = paths->n_reads, n_entries = paths->n_edges_total, E = (uint64_t)(h->n_edges > 0 ? h->n_edges : 0);
    int rc = snk_bads_check_args(who, K, n, in ? in->read_len : 0, true, n_unitigs, d_unitig_off, d_unitig_bases, h, paths, 0, err, errcap);
    if (rc) return rc;
    if (in && n && in->rows && (in->read_len == 0 || in->row_words * 16 < in->read_len || in->row_words > 16))
        return snk_fail(SNK_E_ARG, err, errcap, "%s: need packed rows of at most 256 bases that hold read_len", who);
    if (in && n && in->quals && in->qstride < in->read_len) return snk_fail(SNK_E_ARG, err, errcap, "%s: quality rows shorter than read_len", who);
    if (E && !inv) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument (inv)", who);
    if (n_pairs >= (1ull << 30)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: too many pairs", who);
    if (n_pairs && !E) return snk_fail(SNK_E_ARG, err, errcap, "%s: %llu pairs on a graph without edges", who, (unsigned long long)n_pairs);
    for (uint64_t e = 0; e < E; ++e) {
        const int64_t r = inv[e];
        if (r < 0 || (uint64_t)r >= E || (uint64_t)inv[r] != e)
            return snk_fail(SNK_E_ARG, err, errcap, "%s: inv is not an involution of [0, %llu) at edge %llu", who, (unsigned long long)E, (unsigned long long)e);
    }
    if (px && (px->n_hbv_edges != E || px->n_entries != n_entries))
        return snk_fail(SNK_E_ARG, err, errcap, "%s: a paths index of %llu edges and %llu entries for a graph of %llu edges and paths of %llu entries", who,
                        (unsigned long long)px->n_hbv_edges, (unsigned long long)px->n_entries, (unsigned long long)E, (unsigned long long)n_entries);
    if (px && (!px->index_off || (n_entries && !px->index_ids))) return snk_fail(SNK_E_ARG, err, errcap, "%s: a paths index without its device arrays", who);
    const int width = (int)(max_width ? max_width : 400u);
    if (width < 0 || width > (1 << 20)) return snk_fail(SNK_E_ARG, err, errcap, "%s: max_width = %u", who, max_width);
    const uint32_t budget = std::min(bod_budget ? bod_budget : C_BUDGET, C_BUDGET);
    const int cg2 = (flags & SNK_CLOSE_CG1) ? 0 : 1;
    path_host H;                // (the uploads read it: declared in front of the frame)
    std::vector<uint32_t> h_rows, h_fw, h_prec, h_final, h_pstat;
    std::vector<unsigned long long> h_row_off, h_prec_off, h_first, h_coff, h_bod, h_tab_off;
    std::vector<uint32_t> h_foll;
    std::vector<uint8_t> h_over;
    std::vector<int32_t> h_res;
    return snk_call_run(ctx, stream, who, out, err, errcap, [&](snk_call& c) -> int {
        const hipStream_t st = c.st;
        int rc2;
        SNK_HIP_TRY(c.stamp());
        // ---- the graph tables, the checks of the paths, the index, the pairs, the table of log binomial sums
        bads_job job;
        if ((rc2 = snk_bads_begin(c, H, who, K, n, n_unitigs, d_unitig_off, d_unitig_bases, h, paths, 0, &job, err, errcap))) return rc2;
        c_view V;
        memset(&V, 0, sizeof V);
        V.start = job.start; V.n_edges = job.n_edges; V.edges = (const int32_t*)job.edges; V.offset = job.offset;
        if (in) V.R = snk_reads_view_of(in, n);
        if (px) {
            V.ioff = (const unsigned long long*)px->index_off; V.iids = (const unsigned long long*)px->index_ids;
        } else {
            unsigned long long *off, *ids;
            int32_t* none;
            uint32_t key_bits;
            if ((rc2 = snk_pidx_lists(c, paths, E, who, false, &off, &ids, &none, &key_bits, err, errcap))) return rc2;
            V.ioff = off; V.iids = ids;
        }
        int32_t *d_inv, *km;
        uint32_t* d_flag;
        if ((rc2 = c.alloc(E, &d_inv)) || (rc2 = c.alloc(E, &km)) || (rc2 = c.alloc(1, &d_flag))) return rc2;
        V.inv = d_inv; V.km = km;
        const int32_t* pairs = (const int32_t*)d_pairs;
        SNK_HIP_TRY(hipMemsetAsync(d_flag, 0, 4, st));
        if (E) SNK_HIP_TRY(hipMemcpyAsync(d_inv, inv, E * 4, hipMemcpyHostToDevice, st));
        if (E) SNK_HIP_TRY(snk_launch(c_km_kernel, snk_blocks_capped(E, CB, C_GRID_CAP), CB, 0, st, job.G, (int)K, E, km));
        if (n_pairs) SNK_HIP_TRY(snk_launch(c_pairs_kernel, snk_blocks_capped(2 * n_pairs, CB, C_GRID_CAP), CB, 0, st, pairs, 2 * n_pairs, E, d_flag));
        uint32_t h_flag = 0;
        SNK_HIP_TRY(hipMemcpyAsync(&h_flag, d_flag, 4, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        if (h_flag) return snk_fail(SNK_E_ARG, err, errcap, "%s: a pair holds an edge id outside the graph's %llu edges", who, (unsigned long long)E);
        const double* tab = nullptr;
        if ((rc2 = c_table(ctx, &tab, err, errcap))) return rc2;
        SNK_HIP_TRY(c.stamp());
        // ---- the rows of every (pair, side): counted, placed by the host's sums, written
        const uint64_t n2 = 2 * n_pairs, wave_grid = snk_blocks_capped(n2, CB / 64, C_GRID_CAP), pair_grid = snk_blocks_capped(n_pairs, 1, C_GRID_CAP);
        uint32_t *n_rows0, *n_fw, *n_prec, *n_rows_final, *pstat;
        unsigned long long *row_off, *prec_off, *row_idfw, *prec = nullptr, *sprec = nullptr;
        int32_t *row_pos, *res;
        if ((rc2 = c.alloc(n2, &n_rows0)) || (rc2 = c.alloc(n2, &n_fw)) || (rc2 = c.alloc(n2, &n_prec)) || (rc2 = c.alloc(n2, &n_rows_final)) ||
            (rc2 = c.alloc(n_pairs * N_PS, &pstat)) || (rc2 = c.alloc(n2 + 1, &row_off)) || (rc2 = c.alloc(n2 + 1, &prec_off)) || (rc2 = c.alloc(n_pairs * N_R, &res)))
            return rc2;
        h_rows.assign(n2, 0); h_fw.assign(n2, 0); h_prec.assign(n2, 0); h_pstat.assign(n_pairs * N_PS, 0);
        h_row_off.assign(n2 + 1, 0); h_prec_off.assign(n2 + 1, 0);
        if (n_pairs) {
            SNK_HIP_TRY(snk_launch(c_gather_kernel<false>, wave_grid, CB, 0, st, V, n_pairs, pairs, cg2, n_rows0, n_fw, n_prec, (const unsigned long long*)nullptr,
                                   (unsigned long long*)nullptr, (int32_t*)nullptr, (const unsigned long long*)nullptr, (unsigned long long*)nullptr));
            SNK_HIP_TRY(hipMemcpyAsync(h_rows.data(), n_rows0, n2 * 4, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(hipMemcpyAsync(h_fw.data(), n_fw, n2 * 4, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(hipMemcpyAsync(h_prec.data(), n_prec, n2 * 4, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(snk_sync(st));
        }
        for (uint64_t i = 0; i < n2; ++i) {          // a side has room for its rows and one partner per forward row of the other side
            h_row_off[i + 1] = h_row_off[i] + h_rows[i] + (cg2 ? h_fw[i ^ 1] : 0u);
            h_prec_off[i + 1] = h_prec_off[i] + h_prec[i];
        }
        const uint64_t cap_rows = h_row_off[n2], total_prec = h_prec_off[n2];
        if (total_prec >= (1ull << 32) || cap_rows >= (1ull << 40)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: too many stack rows in one call", who);
        if ((rc2 = c.alloc(cap_rows, &row_idfw)) || (rc2 = c.alloc(cap_rows, &row_pos)) || (rc2 = c.alloc(total_prec, &prec)) || (rc2 = c.alloc(total_prec, &sprec))) return rc2;
        h_final = h_rows;
        if (n_pairs) {
            SNK_HIP_TRY(hipMemcpyAsync(row_off, h_row_off.data(), (n2 + 1) * 8, hipMemcpyHostToDevice, st));
            SNK_HIP_TRY(hipMemcpyAsync(prec_off, h_prec_off.data(), (n2 + 1) * 8, hipMemcpyHostToDevice, st));
            SNK_HIP_TRY(hipMemcpyAsync(n_rows_final, h_final.data(), n2 * 4, hipMemcpyHostToDevice, st));
            SNK_HIP_TRY(hipMemsetAsync(pstat, 0, n_pairs * N_PS * 4, st));
            SNK_HIP_TRY(snk_launch(c_gather_kernel<true>, wave_grid, CB, 0, st, V, n_pairs, pairs, cg2, n_rows0, n_fw, n_prec, (const unsigned long long*)row_off, row_idfw,
                                   row_pos, (const unsigned long long*)prec_off, prec));
        }
        // ---- CloseGap2: the followers sorted per (pair, side), the partners placed
        uint64_t n_place_host = 0;
        if (cg2 && n_pairs) {
            if (total_prec) {
                uint32_t e_bits = 1;
                while (e_bits < 32 && (1ull << e_bits) < E) ++e_bits;
                if ((rc2 = c.with_temp([&](void* tmp, size_t& tb) {
                        return rocprim::segmented_radix_sort_keys(tmp, tb, prec, sprec, (unsigned int)total_prec, (unsigned int)n2, prec_off, prec_off + 1, 0u, 32u + e_bits, st);
                    })))
                    return rc2;
            }
            // the follower groups and the 32-mers of every (pair, side); a pair with a side over the budget is the host's, whole
            unsigned long long *bod_n, *tab_off;
            uint32_t* foll_n;
            uint8_t* d_over;
            if ((rc2 = c.alloc(n2, &bod_n)) || (rc2 = c.alloc(n2, &foll_n)) || (rc2 = c.alloc(n_pairs, &d_over)) || (rc2 = c.alloc(n_pairs + 1, &tab_off))) return rc2;
            SNK_HIP_TRY(snk_launch(c_bod_kernel, wave_grid, CB, 0, st, job.G, n2, (const unsigned long long*)prec_off, (const unsigned long long*)sprec, bod_n, foll_n));
            h_bod.assign(n2, 0); h_foll.assign(n2, 0); h_over.assign(n_pairs, 0); h_tab_off.assign(n_pairs + 1, 0);
            SNK_HIP_TRY(hipMemcpyAsync(h_bod.data(), bod_n, n2 * 8, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(hipMemcpyAsync(h_foll.data(), foll_n, n2 * 4, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(snk_sync(st));
            // every device pair's table: twice the larger of its two sides' 32-mers, a power of two
            unsigned long long largest = 0;
            for (uint64_t p = 0; p < n_pairs; ++p) {
                const unsigned long long m = std::max(h_bod[2 * p], h_bod[2 * p + 1]);
                h_over[p] = (flags & SNK_CLOSE_PLACE_HOST) || m > budget;
                unsigned long long slots = 0;
                if (!h_over[p])
                    for (slots = C_MIN_SLOTS; slots < 2 * m;) slots <<= 1;
                h_tab_off[p + 1] = h_tab_off[p] + slots;
                largest = std::max(largest, slots);
            }
            if (h_tab_off[n_pairs]) {
                // the tables of a launch share one block of at most C_TAB_CAP slots: the pairs go in as many launches as that takes
                const unsigned long long cap = std::max<unsigned long long>(C_TAB_CAP, largest), block = std::min(cap, h_tab_off[n_pairs]);
                unsigned long long* tab_key;
                int* tab_pos;
                if ((rc2 = c.alloc(block, &tab_key)) || (rc2 = c.alloc(block, &tab_pos))) return rc2;
                SNK_HIP_TRY(hipMemcpyAsync(d_over, h_over.data(), n_pairs, hipMemcpyHostToDevice, st));
                SNK_HIP_TRY(hipMemcpyAsync(tab_off, h_tab_off.data(), (n_pairs + 1) * 8, hipMemcpyHostToDevice, st));
                for (uint64_t p0 = 0, p1; p0 < n_pairs; p0 = p1) {
                    for (p1 = p0 + 1; p1 < n_pairs && h_tab_off[p1 + 1] - h_tab_off[p0] <= cap;) ++p1;
                    SNK_HIP_TRY(snk_launch(c_place_kernel, snk_blocks_capped(p1 - p0, 1, C_GRID_CAP), CB, 0, st, V, job.G, p0, p1, (const uint8_t*)d_over,
                                           (const unsigned long long*)row_off, (const uint32_t*)n_rows0, (const uint32_t*)n_fw, row_idfw, row_pos,
                                           (const unsigned long long*)prec_off, (const unsigned long long*)sprec, (const unsigned long long*)bod_n,
                                           (const unsigned long long*)tab_off, tab_key, tab_pos, n_rows_final, pstat));
                }
                SNK_HIP_TRY(hipMemcpyAsync(h_final.data(), n_rows_final, n2 * 4, hipMemcpyDeviceToHost, st));
                SNK_HIP_TRY(hipMemcpyAsync(h_pstat.data(), pstat, n_pairs * N_PS * 4, hipMemcpyDeviceToHost, st));
            }
            SNK_HIP_TRY(snk_sync(st));
            c_host_graph HG;
            HG.H = &H; HG.d_ubases = (const uint8_t*)d_unitig_bases;
            for (uint64_t p = 0; p < n_pairs; ++p) {
                if (!h_over[p]) continue;
                if (HG.uoff.empty()) {
                    HG.uoff.resize(n_unitigs + 1);
                    SNK_HIP_TRY(hipMemcpy(HG.uoff.data(), d_unitig_off, (n_unitigs + 1) * 8, hipMemcpyDeviceToHost));
                }
                ++n_place_host;
                std::vector<unsigned long long> rows[2], pr[2], add_id[2];
                std::vector<int32_t> add_pos[2];
                uint32_t F[2], tried = 0;
                for (int s = 0; s < 2; ++s) {
                    const uint64_t i = 2 * p + s;
                    F[s] = h_fw[i];
                    rows[s].resize(h_fw[i]);
                    pr[s].resize(h_prec[i]);
                    if (h_fw[i]) SNK_HIP_TRY(hipMemcpy(rows[s].data(), row_idfw + h_row_off[i], (size_t)h_fw[i] * 8, hipMemcpyDeviceToHost));
                    if (h_prec[i]) SNK_HIP_TRY(hipMemcpy(pr[s].data(), sprec + h_prec_off[i], (size_t)h_prec[i] * 8, hipMemcpyDeviceToHost));
                }
                if ((rc2 = c_host_place(c, V, HG, rows, F, pr, add_id, add_pos, &tried, err, errcap))) return rc2;
                uint32_t placed = 0;
                for (int s = 0; s < 2; ++s) {
                    const uint64_t i = 2 * p + s, tail = h_row_off[i] + h_rows[i];
                    const size_t m = add_id[s].size();
                    if (m) SNK_HIP_TRY(hipMemcpy(row_idfw + tail, add_id[s].data(), m * 8, hipMemcpyHostToDevice));
                    if (m) SNK_HIP_TRY(hipMemcpy(row_pos + tail, add_pos[s].data(), m * 4, hipMemcpyHostToDevice));
                    h_final[i] = h_rows[i] + (uint32_t)m;
                    placed += (uint32_t)m;
                }
                h_pstat[p * N_PS + PS_TRIED] = tried; h_pstat[p * N_PS + PS_PLACED] = placed;
            }
            if (n_place_host) SNK_HIP_TRY(hipMemcpyAsync(n_rows_final, h_final.data(), n2 * 4, hipMemcpyHostToDevice, st));
        }
        SNK_HIP_TRY(c.stamp());
        // ---- the offsets of every pair; the closures' places; the closures
        h_res.assign(n_pairs * N_R, 0);
        if (n_pairs) {
            SNK_HIP_TRY(snk_launch(c_close_kernel, pair_grid, CB, 0, st, V, job.G, n_pairs, pairs, (const unsigned long long*)row_off, (const uint32_t*)n_rows_final,
                                   (const unsigned long long*)row_idfw, (const int32_t*)row_pos, width, tab, res));
            SNK_HIP_TRY(hipMemcpyAsync(h_res.data(), res, n_pairs * N_R * 4, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(snk_sync(st));
        }
        h_first.assign(n_pairs + 1, 0);
        h_coff.assign(1, 0);
        uint64_t by_off[4] = {0, 0, 0, 0}, kept = 0, too_long = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            const int32_t* r = h_res.data() + p * N_R;
            ++by_off[r[R_NOFF]];
            kept += (uint64_t)r[R_KEPT];
            too_long += (uint64_t)r[R_LONG];
            const int n_off = r[R_NOFF] <= 2 ? r[R_NOFF] : 0;
            for (int q = 0; q < n_off; ++q) {
                const int o = r[R_O0 + q], c1 = r[R_C1], c2 = r[R_C2];
                h_coff.push_back(h_coff.back() + (uint64_t)(std::max(c1, o + c2) - std::min(0, o)));
            }
            h_first[p + 1] = h_first[p] + (uint64_t)n_off;
        }
        const uint64_t n_cl = h_first[n_pairs], n_bases = h_coff.back();
        unsigned long long *d_first, *d_coff;
        uint8_t* bases;
        if ((rc2 = c.alloc(n_pairs + 1, &d_first)) || (rc2 = c.alloc(n_cl + 1, &d_coff)) || (rc2 = c.alloc(n_bases, &bases))) return rc2;
        SNK_HIP_TRY(hipMemcpyAsync(d_first, h_first.data(), (n_pairs + 1) * 8, hipMemcpyHostToDevice, st));
        SNK_HIP_TRY(hipMemcpyAsync(d_coff, h_coff.data(), (n_cl + 1) * 8, hipMemcpyHostToDevice, st));
        if (n_cl)
            SNK_HIP_TRY(snk_launch(c_merge_kernel, pair_grid, CB, 0, st, V, job.G, n_pairs, pairs, (const unsigned long long*)row_off, (const uint32_t*)n_rows_final,
                                   (const unsigned long long*)row_idfw, (const int32_t*)row_pos, width, (const int32_t*)res, (const unsigned long long*)d_first,
                                   (const unsigned long long*)d_coff, bases));
        SNK_HIP_TRY(c.stamp());
        SNK_HIP_TRY(snk_sync(st));
        out->n_closures = n_cl; out->n_bases = n_bases; out->n_pairs = n_pairs;
        out->closure_off = d_coff; out->bases = bases; out->pair_first = d_first;
        out->n_pairs_0 = by_off[0]; out->n_pairs_1 = by_off[1]; out->n_pairs_2 = by_off[2]; out->n_pairs_many = by_off[3];
        out->n_rows = kept;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            out->n_partners_tried += h_pstat[p * N_PS + PS_TRIED];
            out->n_partners_placed += h_pstat[p * N_PS + PS_PLACED];
        }
        for (uint32_t f : h_foll) out->n_followers += f;
        out->n_cons_too_long = too_long;
        out->n_place_host = n_place_host;
        out->ms = c.ms(0, 3);
        out->tables_ms = c.ms(0, 1);
        out->gather_ms = c.ms(1, 2);
        out->close_ms = c.ms(2, 3);
        out->max_width = (uint32_t)width;
        out->bod_budget = budget;
        return c.end(SNK_OK, {d_coff, bases, d_first});
    });
}
