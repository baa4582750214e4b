// snk_extend.hip -- path extension on the device: what StageExtension does to the read paths (10X/DF.cc:676,
// 10X/runstages/RunStages.cc:159-174).
//
// What it replaces: ExtendPathsNew, lib/assembly/src/10X/Extend.cc:14-177, and the HyperBasevectorX overload of ExtendPath,
// paths/long/large/GapToyTools4.cc:477-555 (min_gain 5, mode 1).  Three legs per read, each on the result of the one before:
//   1 backward (SNK_EXT_BACK; Extend.cc:25-61)  while offset < 0 and To(ToLeft(p[0])) is not empty: the first in-edge e, in To-list
//       order, whose bases agree with the read at every position l with l - offset - Kmers(e) >= 0 goes in front, offset += Kmers(e)
//   2 quality-aware (:63-95)                    the path is cut to its first edge; ExtendPath enumerates the continuations
//       breadth-first in From-list order, scores those that cover the read and takes the best iff it is alone or 5 ahead
//   3 exact (:97-177)                           a path that matches the read to its own end and ends inside the read goes on base by base
// Only the first edge of a path and its offset reach the result: leg 1 looks at p[0] alone and leg 2 drops everything behind the first
// edge.  So a read's state is (first edge, offset) and a list of edges that only grows at its end.
//
// Passes.
//   x_check_kernel     one lane per read: the path table, the first edge and the offset against the read and the edge (the refusals;
//                      two more can only be seen later: a path that grows beyond 255 edges, an offset leg 1 moves beyond 32767)
//   x_classify_kernel  one lane per read: leg 1, the early returns of ExtendPath (negative offset, the read ends on the first edge,
//                      no out-edge: almost every read of a real data set), leg 3 as a count.  A read that has to enumerate is listed
//   x_slow_kernel      one wave per listed read.  The breadth-first list lives in LDS as (parent, edge, len) triples: entries 0..100
//                      are expanded and a vertex has at most 4 out-edges, so it holds at most 1 + 101 * 4 = 405 entries (a graph with
//                      a vertex of more out-edges is refused, SNK_E_UNSUPPORTED -- a.pathsX could not hold its branch ids either).
//                      Lane 0 enumerates; the lanes score the candidates that cover the read, each walking its parent links and
//                      comparing 16 bases per step from the packed unitigs; lane 0 picks, then runs leg 3.  It runs twice: as a count
//                      and, once the places are known, to write
//   scan               64-bit places from the counts
//   x_write_kernel     one lane per read that was not listed: the first edge, and leg 3 again for the reads it extended
// The results need no fixed-capacity slots this way: a pass counts, the scan places, the same code writes.  Nothing here looks at a
// tuning option and no atomic decides a result: the output is a pure function of the arguments.
//
// Leg 3's inner loop has no break: where several out-edges carry the read's base at K-1 the reference pushes every one of them (a
// path that is none).  On a de Bruijn graph the out-edges of a vertex differ in that base, so this cannot happen; on other input it
// is REFUSED (SNK_E_UNSUPPORTED), not reproduced.  tests/extref.py keeps the behaviour.
#include <string.h>

#include <algorithm>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "snk_call.h"
#include "snk_common.h"
#include "snk_hbvadj.h"
#include "snk_pathgraph.h"

namespace {

constexpr unsigned EB = 256;                                   // lanes of a workgroup
constexpr int X_MAX_EXTS = 100;                                // ExtendPath's max_exts
constexpr int X_MIN_GAIN = 5;
constexpr int X_MAX_DEG = 4;
constexpr int X_LIST = 1 + (X_MAX_EXTS + 1) * X_MAX_DEG;       // 405
constexpr int X_MAX_PATH = 255;                                // edges of a path (the record's count is one byte)
constexpr int X_CHAIN = 256;
constexpr int X_WAVES = EB / 64;
constexpr uint64_t X_GRID_CAP = 1u << 20;
// bits of the flag word
constexpr uint32_t F_TABLE = 1, F_LONG_IN = 2, F_OFF16 = 4, F_OFF_RANGE = 8, F_LEN0 = 16, F_BACK_SHORT = 32, F_LONG_OUT = 64, F_MULTI = 128, F_EDGE0 = 256;
// bits of a read's class byte
constexpr uint8_t C_BACK = 1, C_MANY = 2, C_SLOW = 4;
// counters
enum { N_BACK, N_CUT, N_QUAL, N_AMBIG, N_TOO_MANY, N_EXACT, N_COUNTERS = 8 };

// the differing bases among the first c <= 16 of two words, as a mask of their top bits' groups
__device__ __forceinline__ uint32_t x_diff(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t x = a ^ b;
    x = (x | (x << 1)) & 0xAAAAAAAAu;
    return c < 16 ? x & ~(0xFFFFFFFFu >> (2 * c)) : x;
}
// how many of the `run` bases from rpos of the read and from epos of the edge agree before the first that does not
__device__ uint32_t x_match(const path_graph& G, const uint32_t* row, uint32_t rw, uint32_t rpos, const pg_edge& x, uint32_t epos, uint32_t run) {
    for (uint32_t done = 0; done < run; done += 16) {
        const uint32_t d = x_diff(snk_row16(row, rw, rpos + done), pg_edge16(G, x, epos + done), min(16u, run - done));
        if (d) return done + ((uint32_t)__clz((int)d) >> 1);
    }
    return run;
}

// leg 1: (e, off) -> the first edge and offset after it; returns the edges put in front
__device__ int x_leg1(const path_graph& G, int K, const uint32_t* row, uint32_t rw, int len, int32_t& e, int& off) {
    int nb = 0;
    while (off < 0 && nb <= X_MAX_PATH) {           // (every step adds one k-mer at least: |off| < len steps at most)
        const int32_t v = G.vleft[e];
        const int t0 = G.to_off[v], t1 = G.to_off[v + 1];
        bool ext = false;
        for (int j = t0; j < t1 && !ext; ++j) {
            const int32_t c = G.to_e[j];
            const pg_edge xc = pg_edge_load(G, c);
            const int km = (int)xc.len - (K - 1);
            if (km < 1) continue;
            const int l0 = max(0, off + km), run = (int)xc.len - l0, rp = l0 - off - km;
            if (rp + run > len) continue;           // (refused by x_check_kernel before this runs: the reference would read behind the read)
            if (x_match(G, row, rw, (uint32_t)rp, xc, (uint32_t)l0, (uint32_t)run) == (uint32_t)run) { e = c; off += km; ++nb; ext = true; }
        }
        if (!ext) break;
    }
    return nb;
}

// ExtendPath's early returns on the one-edge path [e] at off: 0, or how far the read reaches beyond the edge when it has to enumerate
__device__ __forceinline__ int x_reach(const path_graph& G, int32_t e, int off, int len) {
    if (off < 0) return 0;
    const int ext = len - ((int)pg_edge_len(G, e) - off);
    if (ext <= 0) return 0;
    const int32_t v = G.vright[e];
    return G.from_off[v + 1] == G.from_off[v] ? 0 : ext;
}

// leg 3 on the path e0, chain[0 .. nc): the edges it appends, counted, and with WRITE stored at out[0 .. cap)
template <bool WRITE>
__device__ int x_leg3(const path_graph& G, int K, const uint32_t* row, uint32_t rw, int len, int32_t e0, int off, const int32_t* chain, int nc, int32_t* out, int cap,
                      uint32_t* flag) {
    int32_t e = e0;
    pg_edge x = pg_edge_load(G, e);
    int rpos = off < 0 ? -off : 0, epos = off < 0 ? 0 : off, pp = 0;
    for (;;) {                                       // do the path's bases match the read's?
        const int run = min(len - rpos, (int)x.len - epos);
        if ((int)x_match(G, row, rw, (uint32_t)rpos, x, (uint32_t)epos, (uint32_t)run) < run) return 0;
        rpos += run; epos += run;
        if (rpos == len) return 0;
        if (++pp > nc) break;                        // off the path's last edge, inside the read
        e = chain[pp - 1];
        x = pg_edge_load(G, e);
        epos = K - 1;
    }
    int pushed = 0;
    for (;;) {
        if (epos < (int)x.len) {
            const int run = min(len - rpos, (int)x.len - epos);
            const int m = (int)x_match(G, row, rw, (uint32_t)rpos, x, (uint32_t)epos, (uint32_t)run);
            rpos += m; epos += m;
            if (m < run || rpos == len) break;
        } else {
            const int32_t v = G.vright[e];
            const uint32_t b = snk_row_base(row, (uint32_t)rpos);
            int found = 0;
            for (int j = G.from_off[v]; j < G.from_off[v + 1]; ++j) {
                const int32_t f = G.from_e[j];
                const pg_edge xf = pg_edge_load(G, f);
                if ((int)xf.len >= K && (pg_edge16(G, xf, (uint32_t)(K - 1)) >> 30) == b) {
                    e = f; x = xf; ++found;
                    if (WRITE && pushed < cap) out[pushed] = f;
                    ++pushed;
                }
            }
            if (!found) break;
            if (found > 1) atomicOr(flag, F_MULTI);
            epos = K;
            if (++rpos == len) break;
        }
    }
    return pushed;
}

// the refusals.  range[256] = flags
__global__ void __launch_bounds__(EB) x_check_kernel(path_graph G, snk_reads_view R, int K, uint32_t back, uint64_t E, const unsigned long long* __restrict__ start,
                                                     const uint32_t* __restrict__ n_edges, const int32_t* __restrict__ offset, const uint32_t* __restrict__ edges,
                                                     uint64_t n_entries, uint32_t* __restrict__ flags) {
    for (uint64_t r = (uint64_t)blockIdx.x * EB + threadIdx.x; r < R.n; r += (uint64_t)gridDim.x * EB) {
        if (!snk_paths_row_ok(start, n_edges, r, R.n, n_entries)) { atomicOr(flags, F_TABLE); continue; }
        const uint64_t s = start[r], m = n_edges[r];
        if (!m) continue;
        if (m > (uint64_t)X_MAX_PATH) { atomicOr(flags, F_LONG_IN); continue; }
        const int32_t o = offset[r];
        const uint32_t e = edges[s];
        const int len = (int)snk_read_len(R, r);
        if (e >= E) { atomicOr(flags, F_EDGE0); continue; }
        if (len == 0) { atomicOr(flags, F_LEN0); continue; }
        if (o < -32767 || o > 32767) { atomicOr(flags, F_OFF16); continue; }
        if (o <= -len || o >= (int)pg_edge_len(G, (int32_t)e)) { atomicOr(flags, F_OFF_RANGE); continue; }
        if (back && o < 0) {
            const int32_t v = G.vleft[e];
            if (G.to_off[v + 1] != G.to_off[v] && len < -o + K - 1) atomicOr(flags, F_BACK_SHORT);
        }
    }
}

struct x_args {
    path_graph G;
    snk_reads_view R;
    int K;
    uint32_t back;
    const unsigned long long* in_start;
    const uint32_t* in_n;
    const int32_t* in_off;
    const uint32_t* in_edges;
    int32_t* e0;                 // [n] first edge after leg 1
    int32_t* off;                // [n] result: offset
    uint32_t* n_out;             // [n + 1] result: edges
    uint8_t* cls;                // [n]
    uint32_t* slow;              // [n] the reads that enumerate, in no particular order (no result depends on it)
    unsigned long long* cursor;  // [0] reads listed
    unsigned long long* counters;
    uint32_t* flags;
    const unsigned long long* pos;   // [n + 1] places (the write passes)
    int32_t* edges;
    uint64_t n_slow;
};

__global__ void __launch_bounds__(EB) x_classify_kernel(x_args a) {
    const path_graph& G = a.G;
    uint32_t cnt[3] = {0, 0, 0};          // back, cut, exact
    for (uint64_t r = (uint64_t)blockIdx.x * EB + threadIdx.x; r <= a.R.n; r += (uint64_t)gridDim.x * EB) {
        if (r == a.R.n) { a.n_out[r] = 0; break; }          // (the scan's last place)
        const uint32_t m = a.in_n[r];
        if (!m) { a.n_out[r] = 0; a.off[r] = 0; a.e0[r] = -1; a.cls[r] = 0; continue; }
        const uint32_t* row = a.R.rows + r * a.R.row_words;
        const int len = (int)snk_read_len(a.R, r);
        int32_t e = (int32_t)a.in_edges[a.in_start[r]];
        int off = a.in_off[r];
        const int nb = a.back ? x_leg1(G, a.K, row, a.R.row_words, len, e, off) : 0;
        if ((int)m + nb > X_MAX_PATH) atomicOr(a.flags, F_LONG_OUT);
        if (off > 32767) atomicOr(a.flags, F_OFF16);          // (an in-edge of more than 32767 k-mers: the reference zips the path here, Extend.cc:57, and the offset wraps)
        uint8_t c = (nb ? C_BACK : 0) | ((int)m + nb >= 2 ? C_MANY : 0);
        cnt[0] += nb ? 1u : 0u;
        a.e0[r] = e;
        a.off[r] = off;
        if (x_reach(G, e, off, len)) {
            a.slow[atomicAdd(a.cursor, 1ull)] = (uint32_t)r;
            a.cls[r] = c | C_SLOW;
            a.n_out[r] = 0;
            continue;
        }
        const int pushed = x_leg3<false>(G, a.K, row, a.R.row_words, len, e, off, nullptr, 0, nullptr, 0, a.flags);
        if (1 + pushed > X_MAX_PATH) atomicOr(a.flags, F_LONG_OUT);
        cnt[1] += (c & C_MANY) ? 1u : 0u;
        cnt[2] += pushed ? 1u : 0u;
        a.cls[r] = c;
        a.n_out[r] = (uint32_t)min(1 + pushed, X_MAX_PATH);
    }
    const int which[3] = {N_BACK, N_CUT, N_EXACT};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        uint32_t v = cnt[q];
        for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&a.counters[which[q]], (unsigned long long)v);
    }
}

// one wave per listed read; WRITE: the second run, which stores the edges at their places
template <bool WRITE>
__global__ void __launch_bounds__(EB) x_slow_kernel(x_args a) {
    __shared__ int32_t l_edge[X_WAVES][X_LIST], l_len[X_WAVES][X_LIST], l_q[X_WAVES][X_LIST], l_chain[X_WAVES][X_CHAIN];
    __shared__ uint16_t l_par[X_WAVES][X_LIST];
    __shared__ int l_cnt[X_WAVES], l_fail[X_WAVES];
    const path_graph& G = a.G;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, K = a.K;
    int32_t *ed = l_edge[w], *ln = l_len[w], *qs = l_q[w], *chain = l_chain[w];
    uint16_t* par = l_par[w];
    for (uint64_t base = (uint64_t)blockIdx.x * X_WAVES; base < a.n_slow; base += (uint64_t)gridDim.x * X_WAVES) {
        const bool on = base + w < a.n_slow;
        const uint64_t r = on ? a.slow[base + w] : 0;
        const uint32_t* row = a.R.rows + r * a.R.row_words;
        const uint8_t* qual = a.R.quals + r * a.R.qstride;
        const int len = on ? (int)snk_read_len(a.R, r) : 0;
        const int32_t e0 = on ? a.e0[r] : 0;
        const int off = on ? a.off[r] : 0;
        const int ext = on ? x_reach(G, e0, off, len) : 0;        // > 0: that is why the read is here
        if (on && lane == 0) {
            // the enumeration: entry j = (its parent, its last edge, k-mers so far); entries of len >= ext are not expanded but count
            int cnt = 1, fail = 0;
            ed[0] = -1; ln[0] = 0; par[0] = 0;
            for (int j = 0; j < cnt; ++j) {
                if (j > X_MAX_EXTS) { fail = 1; break; }
                if (ln[j] >= ext) continue;
                const int32_t y = G.vright[j ? ed[j] : e0];
                for (int l = G.from_off[y]; l < G.from_off[y + 1] && cnt < X_LIST; ++l) {
                    const int32_t f = G.from_e[l];
                    ed[cnt] = f;
                    ln[cnt] = min(ln[j] + max((int)pg_edge_len(G, f) - (K - 1), 1), 1 << 20);
                    par[cnt] = (uint16_t)j;
                    ++cnt;
                }
            }
            l_cnt[w] = cnt; l_fail[w] = fail;
        }
        __syncthreads();
        if (on && !l_fail[w]) {
            // the candidates that cover the read, one per lane: summed quality of the mismatches of bases [len - ext, len) against the
            // edges' bases from K - 1 on -- entry i stands for the bases [ln[parent], ln[i]) of the continuation
            const int cnt = l_cnt[w];
            for (int j = lane; j < cnt; j += 64) {
                int q = -1;
                if (ln[j] >= ext) {
                    q = 0;
                    for (int i = j; i != 0; i = par[i]) {
                        const int m0 = ln[par[i]], m1 = min(ln[i], ext);
                        const pg_edge x = pg_edge_load(G, ed[i]);
                        for (int m = m0; m < m1; m += 16) {
                            uint32_t d = x_diff(snk_row16(row, a.R.row_words, (uint32_t)(len - ext + m)), pg_edge16(G, x, (uint32_t)(K - 1 + m - m0)), (uint32_t)min(16, m1 - m));
                            while (d) {
                                const int g = __clz((int)d) >> 1;
                                q += (int)qual[len - ext + m + g];
                                d &= ~(0x80000000u >> (2 * g));
                            }
                        }
                    }
                }
                qs[j] = q;
            }
        }
        __syncthreads();
        if (on && lane == 0) {
            const int cnt = l_cnt[w];
            int nc = 0, what = -1;
            if (l_fail[w]) what = N_TOO_MANY;
            else {
                int best = -1, q1 = 0x7FFFFFFF, q2 = 0x7FFFFFFF, kept = 0;
                for (int j = 1; j < cnt; ++j) {
                    const int q = qs[j];
                    if (q < 0) continue;
                    ++kept;
                    if (q < q1) { q2 = q1; q1 = q; best = j; }
                    else if (q < q2) q2 = q;
                }
                if (kept >= 2 && q2 - q1 < X_MIN_GAIN) what = N_AMBIG;
                else if (kept) {
                    what = N_QUAL;
                    for (int i = best; i != 0; i = par[i]) ++nc;
                    if (nc >= X_MAX_PATH) { atomicOr(a.flags, F_LONG_OUT); nc = 0; }
                    int d = nc;
                    for (int i = best; i != 0 && d > 0; i = par[i]) chain[--d] = ed[i];
                }
            }
            const int cap = WRITE ? (int)(a.pos[r + 1] - a.pos[r]) : 0;
            int32_t* out = WRITE ? a.edges + a.pos[r] : nullptr;
            const int pushed = x_leg3<WRITE>(G, K, row, a.R.row_words, len, e0, off, chain, nc, WRITE ? out + 1 + nc : nullptr, max(cap - 1 - nc, 0), a.flags);
            if (WRITE) {
                if (cap > 0) out[0] = e0;
                for (int i = 0; i < nc && 1 + i < cap; ++i) out[1 + i] = chain[i];
            } else {
                if (1 + nc + pushed > X_MAX_PATH) atomicOr(a.flags, F_LONG_OUT);
                a.n_out[r] = (uint32_t)min(1 + nc + pushed, X_MAX_PATH);
                if (what >= 0) atomicAdd(&a.counters[what], 1ull);
                if ((a.cls[r] & C_MANY) && nc == 0) atomicAdd(&a.counters[N_CUT], 1ull);
                if (pushed) atomicAdd(&a.counters[N_EXACT], 1ull);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(EB) x_write_kernel(x_args a) {
    for (uint64_t r = (uint64_t)blockIdx.x * EB + threadIdx.x; r < a.R.n; r += (uint64_t)gridDim.x * EB) {
        const uint32_t m = a.n_out[r];
        if (!m || (a.cls[r] & C_SLOW)) continue;
        int32_t* out = a.edges + a.pos[r];
        out[0] = a.e0[r];
        if (m > 1) x_leg3<true>(a.G, a.K, a.R.rows + r * a.R.row_words, a.R.row_words, (int)snk_read_len(a.R, r), a.e0[r], a.off[r], nullptr, 0, out + 1, (int)m - 1, a.flags);
    }
}

struct u32_to_u64 {
    __host__ __device__ unsigned long long operator()(uint32_t x) const { return x; }
};

}  // namespace

extern "C" int snk_dev_extend_paths(snk_ctx* ctx, uint32_t K, const snk_dev_reads* in, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases,
                                    const snk_hbv* h, const snk_dev_paths* paths, uint32_t flags, snk_dev_extend* out, void* stream, char* err, size_t errcap) {
    if (!ctx || !in || !h || !paths || !out) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: NULL argument");
    memset(out, 0, sizeof *out);
    if (K != 48 && K != 60) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "K=%u is not supported (48 or 60)", K);
    if (flags & ~SNK_EXT_BACK) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: unknown flag bits 0x%x", flags & ~SNK_EXT_BACK);
    const uint64_t n = in->n_reads, n_entries = paths->n_edges_total;
    const uint64_t E = (uint64_t)(h->n_edges > 0 ? h->n_edges : 0);
    if (paths->n_reads != n)
        return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: %llu paths for %llu reads", (unsigned long long)paths->n_reads, (unsigned long long)n);
    if (n && !in->quals) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: quals == NULL (leg 2 scores mismatches by the raw quality)");
    if (n && (!in->rows || in->read_len == 0 || in->read_len > 256 || in->row_words * 16 < in->read_len || in->row_words > 16))
        return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: need packed rows and quality rows, reads of at most 256 bases");
    if (n && in->qstride < in->read_len) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: quality rows shorter than read_len");
    if (n_unitigs && (!d_unitig_off || !d_unitig_bases)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: NULL unitig arrays");
    if (n_unitigs >= (1ull << 31)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_extend_paths: too many unitigs");
    if (E && (!h->v_left || !h->v_right || !h->src_unitig || !h->is_rc || !h->fwd_xlat || !h->rev_xlat)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: NULL argument");
    if (n && (!paths->start || !paths->n_edges || !paths->offset)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: paths without their device arrays");
    if (n_entries && !paths->edges) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: paths without their device arrays");
    if (n_entries && !E) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: %llu path entries on a graph without edges", (unsigned long long)n_entries);
    if (!n && n_entries) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: start / n_edges do not add up to n_edges_total = %llu", (unsigned long long)n_entries);
    if (n >= (1ull << 32) - 1) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_extend_paths: too many reads");
    for (uint64_t u = 0; u < n_unitigs; ++u)
        if (h->fwd_xlat[u] < 0 || h->rev_xlat[u] < 0 || (uint64_t)h->fwd_xlat[u] >= E || (uint64_t)h->rev_xlat[u] >= E ||
            (h->bvcomp_order && (h->bvcomp_order[u] < 0 || (uint64_t)h->bvcomp_order[u] >= n_unitigs)))
            return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: inconsistent translation tables");
    for (uint64_t e = 0; e < E; ++e)
        if (h->src_unitig[e] < 0 || (uint64_t)h->src_unitig[e] >= n_unitigs) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: edge %llu is out of range", (unsigned long long)e);
    // the graph tables on the host outlive the frame's last wait; everything but the four result arrays goes back to the arena with the call
    path_host H;
    return snk_call_run(ctx, stream, "snk_dev_extend_paths", out, err, errcap, [&](snk_call& c) -> int {
        const hipStream_t st = c.st;
        int rc;
        SNK_HIP_TRY(c.stamp());
        x_args a;
        memset(&a, 0, sizeof a);
        uint64_t total_bases = 0;
        if ((rc = snk_path_graph_tables(c, H, K, n_unitigs, (const uint64_t*)d_unitig_off, (const uint8_t*)d_unitig_bases, h, &a.G, &total_bases, "snk_dev_extend_paths", err, errcap)))
            return rc;
        for (int32_t v = 0; v < h->n_vertices; ++v)
            if (H.off_from[(size_t)v + 1] - H.off_from[v] > X_MAX_DEG)
                return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_extend_paths: vertex %d has more than four out-edges (the list of continuations holds %d entries)", v, X_LIST);
        a.R = snk_reads_view_of(in, n);
        a.K = (int)K; a.back = flags & SNK_EXT_BACK;
        a.in_start = (const unsigned long long*)paths->start; a.in_n = (const uint32_t*)paths->n_edges; a.in_off = (const int32_t*)paths->offset;
        a.in_edges = (const uint32_t*)paths->edges;
        // ---- the refusals, before any result is allocated
        uint32_t* range;
        unsigned long long* counters;
        if ((rc = c.alloc(256 + 1, &range)) || (rc = c.alloc(N_COUNTERS + 1, &counters))) return rc;
        SNK_HIP_TRY(hipMemsetAsync(range, 0, 257 * 4, st));
        SNK_HIP_TRY(hipMemsetAsync(counters, 0, (N_COUNTERS + 1) * 8, st));
        a.flags = range + 256; a.counters = counters; a.cursor = counters + N_COUNTERS;
        SNK_HIP_TRY(snk_launch(x_check_kernel, snk_blocks_capped(n, EB, X_GRID_CAP), EB, 0, st, a.G, a.R, a.K, a.back, E, a.in_start, a.in_n, a.in_off, a.in_edges, n_entries, a.flags));
        if (n_entries) SNK_HIP_TRY(snk_max_edge_id(a.in_edges, n_entries, range, st));
        uint32_t h_range[257];
        SNK_HIP_TRY(hipMemcpyAsync(h_range, range, sizeof h_range, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        uint32_t emax = 0;
        for (int q = 0; q < 256; ++q) emax = std::max(emax, h_range[q]);
        uint32_t f = h_range[256];
        if (f & F_TABLE) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: start / n_edges do not add up to n_edges_total = %llu", (unsigned long long)n_entries);
        if ((f & F_EDGE0) || (n_entries && emax >= E))
            return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: a path holds edge id %lld, the graph has %llu edges", (long long)(int32_t)emax, (unsigned long long)E);
        if (f & F_LONG_IN) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_extend_paths: a path of more than 255 edges (the record's edge count is one byte)");
        if (f & F_LEN0) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: a read of length 0 has a path");
        if (f & F_OFF16) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_extend_paths: an offset outside +-32767 (the reference's input is a ReadPathVecX: int16 offsets)");
        if (f & F_OFF_RANGE)
            return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: an offset at or beyond the end of its first edge, or at or below minus the read's length");
        if (f & F_BACK_SHORT)
            return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_extend_paths: a read ends inside the %u bases its first edge shares with its in-edges (SNK_EXT_BACK compares all of them)", K - 1);
        // ---- classify, list, count
        int32_t *offset, *e0, *edges;
        uint32_t *n_out, *slow;
        unsigned long long* pos;
        uint8_t* cls;
        if ((rc = c.alloc(n, &offset)) || (rc = c.alloc(n + 1, &n_out)) || (rc = c.alloc(n + 1, &pos)) || (rc = c.alloc(n, &e0)) || (rc = c.alloc(n, &cls)) || (rc = c.alloc(n, &slow)))
            return rc;
        a.e0 = e0; a.off = offset; a.n_out = n_out; a.cls = cls; a.slow = slow;
        const uint64_t gmax = std::min<uint64_t>((uint64_t)ctx->n_cu * 64, X_GRID_CAP);
        SNK_HIP_TRY(snk_launch(x_classify_kernel, snk_blocks_capped(n + 1, EB, gmax), EB, 0, st, a));
        unsigned long long n_slow = 0;
        SNK_HIP_TRY(hipMemcpyAsync(&n_slow, a.cursor, 8, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        if (n_slow > n) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_extend_paths: the list of reads that enumerate is out of range");
        a.n_slow = n_slow;
        const uint64_t g_slow = snk_blocks_capped(n_slow, X_WAVES, gmax);
        if (n_slow) SNK_HIP_TRY(snk_launch(x_slow_kernel<false>, g_slow, EB, 0, st, a));
        {
            rocprim::transform_iterator<const uint32_t*, u32_to_u64, unsigned long long> it(n_out, u32_to_u64());
            if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::exclusive_scan(tmp, tb, it, pos, 0ull, (size_t)(n + 1), rocprim::plus<unsigned long long>(), st); })))
                return rc;
        }
        unsigned long long total = 0;
        SNK_HIP_TRY(hipMemcpyAsync(&f, a.flags, 4, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(hipMemcpyAsync(&total, pos + n, 8, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        if (f & F_LONG_OUT) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_extend_paths: a path of more than 255 edges (the record's edge count is one byte)");
        if (f & F_OFF16)
            return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_extend_paths: the backward leg moves an offset beyond 32767 (the reference keeps the path in a ReadPathVecX between its legs: int16 offsets)");
        if (f & F_MULTI)
            return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_extend_paths: two out-edges of a vertex carry the same base at K-1 (the reference pushes both: not a path)");
        if (total > n * (unsigned long long)X_MAX_PATH) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_extend_paths: the scan's total is out of range");
        // ---- write
        if ((rc = c.alloc((size_t)total, &edges))) return rc;
        a.pos = pos; a.edges = edges;
        SNK_HIP_TRY(snk_launch(x_write_kernel, snk_blocks_capped(n, EB, gmax), EB, 0, st, a));
        if (n_slow) SNK_HIP_TRY(snk_launch(x_slow_kernel<true>, g_slow, EB, 0, st, a));
        unsigned long long h_cnt[N_COUNTERS];
        SNK_HIP_TRY(hipMemcpyAsync(h_cnt, counters, sizeof h_cnt, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(c.stamp());
        SNK_HIP_TRY(snk_sync(st));
        out->paths.n_reads = n;
        out->paths.n_edges_total = total;
        out->paths.offset = offset;
        out->paths.n_edges = n_out;
        out->paths.start = pos;
        out->paths.edges = edges;
        out->paths.path_ms = c.ms(0, 1);
        out->n_back_extended = h_cnt[N_BACK];
        out->n_cut_to_first = h_cnt[N_CUT];
        out->n_quality_extended = h_cnt[N_QUAL];
        out->n_ambiguous = h_cnt[N_AMBIG];
        out->n_too_many = h_cnt[N_TOO_MANY];
        out->n_exact_extended = h_cnt[N_EXACT];
        out->n_enumerated = n_slow;
        out->ms = c.ms(0, 1);
        return c.end(SNK_OK, {offset, n_out, pos, edges});
    });
}
