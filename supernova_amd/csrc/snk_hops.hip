// snk_hops.hip -- FindEdgePairs on the device: the second step of StageFindPatch (10X/runstages/RunStages.cc:263-266), whose result DF
// keeps as a.hops (10X/DF.cc:642-643): the edge pairs that gap closing tries.
//
// What it replaces: FindEdgePairs, lib/assembly/src/10X/Closomatic.cc:17-354, host code that unzips paths one by one out of a.paths.inv.
// Its result is UniqueSort of all pairs, so it does not depend on any order: the three parts below each make a list with repeats, every
// list is sorted and made unique, and so is their concatenation.  include/snk.h states the rules; here is how they run.
//
// "Two classes" never needs the classes sorted: (e1, e2) keys are sorted carrying the class as a value, and a run of equal keys holds
// two classes iff two NEIGHBOURS of the run differ (h_hits_kernel).  The same kernel serves the three parts.
//
// Passes.
//   h_edge_kernel      one lane per edge: Kmers(e), sink(e), source(e) from the From / To lists
//   h_keys_kernel      parts 1 and 2.  One lane per read: e2 = inv[last edge of the mate's path]; a key (e1 << 32 | e2, class) for every distinct
//                      sink edge e1 != e2 of its path.  Run twice: the first run only counts.  A wave adds up its lanes' keys with shuffles
//                      and takes its place in the list with ONE atomic
//   radix sort         rocPRIM, pairs, over the bits two edge ids have
//   h_hits_kernel<1>   part 1: a hit with source(e2) (or SNK_HOPS_ONE_GOOD) goes to the list and marks seen[e1]
//   h_hits_kernel<2>   part 2, after part 1 has ended: a hit with !seen[e1], Kmers(e2) >= 100, ToRight(e1) != ToLeft(e2)
//   h_classify_kernel  part 3.  One wave per edge of K + 1 k-mers or more, lanes over the index entries of e and inv[e]: are the classes
//                      all equal; does a member of X that begins with e carry 100 k-mers already (round 0).  X is never made: a member
//                      is (path, first position, direction, inverted or not) -- h_mem.  What is left -- two classes, not extended in
//                      round 0 -- is the residual list
//   h_useful_kernel    one wave per residual edge: the index entries that give a member of two edges or more, counted, then written in
//                      entry order (ballot + popcount); whether a member is [e] itself.  A read that lies on the edge alone brings nothing else
//   h_closure_kernel   one WAVE per residual edge, lanes over its useful entries: the closure as a worklist over the set of sequences reached
//                      so far, kept in LDS (at most ext_budget sequences, H_VINTS ints).  Reaching 100 k-mers ends it; so does a worklist
//                      that runs dry; a set that does not fit, or an edge of more than H_MAX_USEFUL useful entries, sends the edge to the host
//   h_host_closure     (host) the same closure over the downloaded paths and index, with a std::set: no bound
//   h_rights_kernel    one wave per not-extended edge, lanes over the entries of pairs with bad == 0: too_easy keys (e << 32 | f) and can
//                      keys with their class.  Run twice like h_keys_kernel
//   h_hits_kernel<3>   on the sorted can keys: a hit that a binary search does not find among the sorted too_easy keys
//   final              the three lists one behind the other, sorted, unique, unpacked to (first, second)
// The lists that atomics fill are in no fixed order; everything read from them is sorted first, so the result is bit-identical from
// call to call.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "snk_bads.h"
#include "snk_call.h"
#include "snk_common.h"

namespace {

constexpr unsigned HB = 256;                       // lanes of a workgroup
constexpr uint64_t H_GRID_CAP = 1u << 16;
constexpr int MAX_DIST_TO_END = 120;               // Closomatic.cc:31
constexpr int MIN_LANDING = 100;                   // :32
constexpr int GOOD_EXT = 100;                      // :185
constexpr int MIN_RIGHT = 40;                      // :186
constexpr uint32_t H_VCAP = 128;                   // sequences the set of an edge holds at most = the largest budget
constexpr uint32_t H_VINTS = 4096;                 // ints of that set (16 KB of LDS): per sequence its k-mers behind the first edge, then its edges
constexpr uint64_t H_MAX_USEFUL = 1u << 16;        // useful entries of an edge above which its closure is the host's: a lane walks at most
                                                   //     H_MAX_USEFUL / 64 entries, twice per sequence of the set
constexpr uint8_t FL_SINK = 1, FL_SOURCE = 2;
// state of an edge after part 3's steps
enum : uint8_t { ST_NONE = 0, ST_ROUND0 = 1, ST_NOT_EXT = 2, ST_EXT = 3, ST_HOST = 4, ST_RESIDUAL = 5 };
enum { C_SINK, C_LONG, C_TWO, C_R0, C_RES, C_KEYS, C_P1, C_P2, C_P3, C_EXT, C_NOT, C_HOST, C_NE, C_TE, C_CAN, N_CNT = 16 };

// what parts 1 to 3 read: the paths, their index, and per edge inv, Kmers and the flags.  The same struct serves the host routine with
// host arrays.
struct h_view {
    const unsigned long long* start;
    const uint32_t* n_edges;
    const int32_t* edges;
    const unsigned long long *ioff, *iids;
    const int32_t *inv, *km, *bc;
    const uint8_t* bad;
};
// a member of X: y[m] = p[pos0 + dir * m], through inv[] where inv != NULL
struct h_mem {
    const int32_t *p, *inv;
    int pos0, dir, len;
    __host__ __device__ int at(int m) const {
        const int v = p[pos0 + dir * m];
        return inv ? inv[v] : v;
    }
};
// The members that entry r of the index gives.  list 0: r is an entry of e -- the suffix from every occurrence of e, and the mate's path
// reversed and inverted (Closomatic.cc:203-223); list 1: r is an entry of re = inv[e] -- the reversed and inverted prefix up to every
// occurrence of re (:224-236).  f(member) -> true ends the enumeration (and is what h_members returns).
template <class F>
__host__ __device__ inline bool h_members(const h_view& V, int e, int re, int list, uint64_t r, F&& f) {
    const int32_t* p = V.edges + V.start[r];
    const int n = (int)V.n_edges[r];
    if (list == 0) {
        for (int j = 0; j < n; ++j)
            if (p[j] == e && f(h_mem{p, nullptr, j, 1, n - j})) return true;
        const uint64_t q = r ^ 1ull;
        const int nq = (int)V.n_edges[q];
        if (nq && f(h_mem{V.edges + V.start[q], V.inv, nq - 1, -1, nq})) return true;
    } else {
        for (int j = 0; j < n; ++j)
            if (p[j] == re && f(h_mem{p, V.inv, j, -1, j + 1})) return true;
    }
    return false;
}
// ... of every entry of e and of inv[e]
template <class F>
__host__ __device__ inline bool h_all_members(const h_view& V, int e, F&& f) {
    const int re = V.inv[e];
    for (int list = 0; list < 2; ++list) {
        const int x = list ? re : e;
        for (unsigned long long i = V.ioff[x]; i < V.ioff[x + 1]; ++i)
            if (h_members(V, e, re, list, V.iids[i], f)) return true;
    }
    return false;
}
// may x (n edges, the last one = y[l]) grow by y behind place l: they agree wherever they overlap (Closomatic.cc:269-276)
__host__ __device__ inline bool h_agrees(const int32_t* x, int n, const h_mem& y, int l) {
    for (int m = l - 1, i = n - 2; m >= 0 && i >= 0; --m, --i)
        if (x[i] != y.at(m)) return false;
    return true;
}

__global__ void __launch_bounds__(HB) h_edge_kernel(path_graph G, int K, uint64_t E, int32_t* __restrict__ km, uint8_t* __restrict__ fl, unsigned long long* __restrict__ cnt) {
    uint32_t n_sink = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * HB + threadIdx.x; e < E; e += (uint64_t)gridDim.x * HB) {
        km[e] = (int32_t)pg_edge_len(G, (int32_t)e) - K + 1;
        bool sink = true, source = true;
        const int32_t v = G.vright[e], u = G.vleft[e];
        for (int l = G.from_off[v]; l < G.from_off[v + 1]; ++l) {      // Closomatic.cc:43-53
            const int32_t w = G.from_v[l];
            if (G.from_off[w + 1] - G.from_off[w] > 0 || G.to_off[w + 1] - G.to_off[w] > 1 || (int)pg_edge_len(G, G.from_e[l]) - K + 1 > MAX_DIST_TO_END) sink = false;
        }
        for (int l = G.to_off[u]; l < G.to_off[u + 1]; ++l) {          // :84-94
            const int32_t w = G.to_v[l];
            if (G.to_off[w + 1] - G.to_off[w] > 0 || G.from_off[w + 1] - G.from_off[w] > 1 || (int)pg_edge_len(G, G.to_e[l]) - K + 1 > MAX_DIST_TO_END) source = false;
        }
        fl[e] = (uint8_t)((sink ? FL_SINK : 0) | (source ? FL_SOURCE : 0));
        n_sink += sink;
    }
    for (int o = 32; o > 0; o >>= 1) n_sink += (uint32_t)__shfl_xor((int)n_sink, o);
    if ((threadIdx.x & 63) == 0 && n_sink) atomicAdd(&cnt[C_SINK], (unsigned long long)n_sink);
}

// keys == NULL: count only.  cap: the keys the first run counted -- nothing is written behind them.
__global__ void __launch_bounds__(HB) h_keys_kernel(h_view V, const uint8_t* __restrict__ fl, uint64_t n_reads, unsigned long long* __restrict__ keys, int32_t* __restrict__ vals,
                                                    uint64_t cap, unsigned long long* __restrict__ cursor) {
    const uint64_t per_round = (uint64_t)gridDim.x * HB, rounds = n_reads / per_round + (n_reads % per_round != 0);
    for (uint64_t it = 0; it < rounds; ++it) {                        // every lane makes the same number of steps
        const uint64_t r = (it * gridDim.x + blockIdx.x) * HB + threadIdx.x;
        uint32_t c = 0;
        int e2 = -1;
        const int32_t* p = nullptr;
        int n = 0;
        if (r < n_reads) {
            n = (int)V.n_edges[r];
            const int nq = (int)V.n_edges[r ^ 1ull];
            if (n && nq) {
                p = V.edges + V.start[r];
                e2 = V.inv[V.edges[V.start[r ^ 1ull] + nq - 1]];
                for (int j = 0; j < n; ++j) {
                    const int e1 = p[j];
                    if (!(fl[e1] & FL_SINK) || e1 == e2) continue;
                    bool first = true;
                    for (int i = 0; i < j; ++i) first &= p[i] != e1;
                    c += first;
                }
            }
        }
        unsigned long long at = snk_wave_alloc(cursor, c);          // (every lane of the wave is here: see the loop)
        if (!keys || !c) continue;
        const int32_t cls = V.bc[r];
        for (int j = 0; j < n; ++j) {
            const int e1 = p[j];
            if (!(fl[e1] & FL_SINK) || e1 == e2) continue;
            bool first = true;
            for (int i = 0; i < j; ++i) first &= p[i] != e1;
            if (!first) continue;
            if (at < cap) { keys[at] = (unsigned long long)(uint32_t)e1 << 32 | (uint32_t)e2; vals[at] = cls; }
            ++at;
        }
    }
}

// Sorted (key, class): entry i is a hit when its key equals its neighbour's and the class does not -- a run of two classes or more has
// one at least.  PART 1 / 2 / 3 add their own conditions; a hit goes to out[] (at most one per entry: cap = n).
template <int PART>
__global__ void __launch_bounds__(HB) h_hits_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ val, uint64_t n, const uint8_t* __restrict__ fl,
                                                    const int32_t* __restrict__ km, path_graph G, uint32_t one_good, uint8_t* __restrict__ seen,
                                                    const unsigned long long* __restrict__ te, uint64_t n_te, unsigned long long* __restrict__ out,
                                                    unsigned long long* __restrict__ cursor) {
    for (uint64_t i = (uint64_t)blockIdx.x * HB + threadIdx.x + 1; i < n; i += (uint64_t)gridDim.x * HB) {
        const unsigned long long k = key[i];
        if (k != key[i - 1] || val[i] == val[i - 1]) continue;
        const uint32_t e1 = (uint32_t)(k >> 32), e2 = (uint32_t)k;
        if (PART == 1) {
            if (!one_good && !(fl[e2] & FL_SOURCE)) continue;
            seen[e1] = 1;
        } else if (PART == 2) {
            if (seen[e1] || km[e2] < MIN_LANDING || G.vright[e1] == G.vleft[e2]) continue;
        } else {
            uint64_t lo = 0, hi = n_te;                                // too_easy holds (e, f)?
            while (lo < hi) {
                const uint64_t mid = (lo + hi) / 2;
                if (te[mid] < k) lo = mid + 1; else hi = mid;
            }
            if (lo < n_te && te[lo] == k) continue;
        }
        out[atomicAdd(cursor, 1ull)] = k;                              // (hits are few: the pairs of the result, with repeats)
    }
}

__global__ void __launch_bounds__(HB) h_classify_kernel(h_view V, uint64_t E, int K, uint8_t* __restrict__ state, uint32_t* __restrict__ residual, unsigned long long* __restrict__ cnt) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * HB + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * HB) >> 6;
    uint32_t n_long = 0, n_two = 0, n_r0 = 0;
    for (uint64_t e = wave; e < E; e += n_waves) {
        uint8_t st = ST_NONE;
        if (V.km[e] >= K + 1) {                                        // Closomatic.cc:190
            ++n_long;
            const int re = V.inv[e];
            const unsigned long long a0 = V.ioff[e], nA = V.ioff[e + 1] - a0, b0 = V.ioff[re], nB = V.ioff[re + 1] - b0;
            if (nA + nB) {
                const int32_t c0 = V.bc[V.iids[nA ? a0 : b0]];
                bool two = false, r0 = false;
                for (unsigned long long t = lane; t < nA + nB; t += 64) {
                    const int list = t >= nA;
                    const uint64_t r = V.iids[list ? b0 + (t - nA) : a0 + t];
                    two |= V.bc[r] != c0;
                    if (!r0)
                        r0 = h_members(V, (int)e, re, list, r, [&](const h_mem& y) {
                            if (y.at(0) != (int)e) return false;
                            int k = 0;
                            for (int m = 1; m < y.len; ++m)
                                if ((k += V.km[y.at(m)]) >= GOOD_EXT) return true;
                            return false;
                        });
                }
                two = __any(two);
                r0 = __any(r0);
                if (two) {
                    ++n_two;
                    n_r0 += r0;
                    st = r0 ? ST_ROUND0 : ST_RESIDUAL;
                    if (!r0 && lane == 0) residual[atomicAdd(&cnt[C_RES], 1ull)] = (uint32_t)e;
                }
            }
        }
        if (lane == 0) state[e] = st;
    }
    if (lane == 0) {
        if (n_long) atomicAdd(&cnt[C_LONG], (unsigned long long)n_long);
        if (n_two) atomicAdd(&cnt[C_TWO], (unsigned long long)n_two);
        if (n_r0) atomicAdd(&cnt[C_R0], (unsigned long long)n_r0);
    }
}

// Which index entries of a residual edge matter to its closure: those that give a member of two edges or more.  A member of one edge can
// neither extend a sequence (no place behind its last) nor start one other than [e]; whether some member IS [e] is the edge's root1 flag.
// On the bench graph that leaves a handful of the ~6 600 entries of such an edge.  One wave per residual edge, 64 entries a step, the kept
// ones written in entry order (ballot and popcount: no atomic, so the closure meets them in the same order every time).  WRITE false:
// counts only (n_useful[i], root1[i]); true: the entries, list << 63 | read id, at useful_off[i].
template <bool WRITE>
__global__ void __launch_bounds__(HB) h_useful_kernel(h_view V, const uint32_t* __restrict__ residual, uint64_t n_res, unsigned long long* __restrict__ n_useful,
                                                      uint8_t* __restrict__ root1, const unsigned long long* __restrict__ useful_off, unsigned long long* __restrict__ useful) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * HB + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * HB) >> 6;
    for (uint64_t i = wave; i < n_res; i += n_waves) {
        const int e = (int)residual[i], re = V.inv[e];
        const unsigned long long a0 = V.ioff[e], nA = V.ioff[e + 1] - a0, b0 = V.ioff[re], nB = V.ioff[re + 1] - b0;
        unsigned long long at = WRITE ? useful_off[i] : 0ull;
        bool single = false;
        for (unsigned long long base = 0; base < nA + nB; base += 64) {
            const unsigned long long t = base + lane;
            bool keep = false;
            unsigned long long ent = 0;
            if (t < nA + nB) {
                const int list = t >= nA;
                const uint64_t r = V.iids[list ? b0 + (t - nA) : a0 + t];
                ent = (unsigned long long)list << 63 | r;
                h_members(V, e, re, list, r, [&](const h_mem& y) {
                    if (y.len >= 2) keep = true;
                    else if (y.at(0) == e) single = true;
                    return false;
                });
            }
            const unsigned long long mask = __ballot(keep);
            if (WRITE && keep) useful[at + __popcll(mask & ((1ull << lane) - 1ull))] = ent;
            at += __popcll(mask);
        }
        const bool any_single = __any(single);
        if (!WRITE && lane == 0) { n_useful[i] = at; root1[i] = any_single ? 1 : 0; }
    }
}

// The steps one entry offers a sequence x of n edges with kx k-mers behind its first (x == NULL: the sequences the entry STARTS, its
// members of two edges or more that begin with e): f(member, place l or -1, k-mers behind the first edge of the result, cut at 100)
// -> true ends the enumeration.  Closomatic.cc:249-250, :262-280.
template <class F>
__device__ inline bool h_steps(const h_view& V, int e, int re, unsigned long long ent, const int32_t* x, int n, int kx, F&& f) {
    return h_members(V, e, re, (int)(ent >> 63), ent & ~(1ull << 63), [&](const h_mem& y) {
        if (y.len < 2) return false;
        if (!x) {
            if (y.at(0) != e) return false;
            int k = 0;
            for (int m = 1; m < y.len && k < GOOD_EXT; ++m) k += V.km[y.at(m)];
            return f(y, -1, k);
        }
        for (int l = 0; l + 1 < y.len; ++l) {
            if (y.at(l) != x[n - 1] || !h_agrees(x, n, y, l)) continue;
            int k = kx;
            for (int z = l + 1; z < y.len && k < GOOD_EXT; ++z) k += V.km[y.at(z)];
            if (f(y, l, k)) return true;
        }
        return false;
    });
}

// The closure of a residual edge: one WAVE (a workgroup of 64) per edge, the lanes over its useful entries.  The set of sequences reached
// so far lives in LDS -- sequence q is data[off[q] .. off[q + 1]) = its k-mers behind the first edge, then its edges -- and is its own
// worklist.  Per sequence (q = -1: the starts) two phases: every lane walks its entries and says whether a step reaches 100 k-mers (the
// search ends: extended) and whether it has a step at all; then the lanes that have steps take turns, in lane order, to walk their
// entries again and put what is new behind the set.  A set that would pass `budget` sequences or H_VINTS ints, and an edge of more
// than H_MAX_USEFUL useful entries (whose walk would keep the kernel busy for long), go to the host: ST_HOST.  Nothing is written
// outside the set.
__global__ void __launch_bounds__(64) h_closure_kernel(h_view V, const uint32_t* __restrict__ residual, uint64_t n_res, uint32_t budget,
                                                       const unsigned long long* __restrict__ useful_off, const unsigned long long* __restrict__ useful,
                                                       const uint8_t* __restrict__ root1, uint8_t* __restrict__ state) {
    __shared__ int32_t data[H_VINTS];
    __shared__ uint16_t off[H_VCAP + 1];
    const unsigned lane = threadIdx.x;
    for (uint64_t i = blockIdx.x; i < n_res; i += gridDim.x) {
        const int e = (int)residual[i], re = V.inv[e];
        const unsigned long long u0 = useful_off[i], nu = useful_off[i + 1] - u0;
        if (nu > H_MAX_USEFUL) {
            if (lane == 0) state[e] = ST_HOST;
            continue;
        }
        __syncthreads();                                               // (the set of the edge before is done with)
        uint32_t cnt = root1[i] ? 1u : 0u;                             // the sequence [e]
        if (lane == 0) { off[0] = 0; data[0] = 0; data[1] = e; off[1] = 2; }
        __syncthreads();
        uint8_t result = ST_NOT_EXT;
        for (int q = -1; q < (int)cnt && result == ST_NOT_EXT; ++q) {
            const int32_t* x = q < 0 ? nullptr : data + off[q] + 1;
            const int n = q < 0 ? 0 : (int)(off[q + 1] - off[q]) - 1, kx = q < 0 ? 0 : data[off[q]];
            bool reaches = false, have = false;
            for (unsigned long long t = lane; t < nu && !reaches; t += 64)
                h_steps(V, e, re, useful[u0 + t], x, n, kx, [&](const h_mem&, int, int k) {
                    have = true;
                    return reaches = k >= GOOD_EXT;
                });
            if (__any(reaches)) { result = ST_EXT; break; }
            unsigned long long turns = __ballot(have);
            while (turns && result == ST_NOT_EXT) {
                const int turn = __ffsll((long long)turns) - 1;
                turns &= turns - 1;
                uint32_t now = cnt, full = 0;
                if ((int)lane == turn)
                    for (unsigned long long t = lane; t < nu && !full; t += 64)
                        h_steps(V, e, re, useful[u0 + t], x, n, kx, [&](const h_mem& y, int l, int k) {
                            const uint32_t at = off[now], len = 1u + (uint32_t)n + (uint32_t)(y.len - l - 1);
                            if (at + len > H_VINTS) return (full = 1) != 0;
                            data[at] = k;
                            for (int j = 0; j < n; ++j) data[at + 1 + j] = x[j];
                            for (int z = l + 1; z < y.len; ++z) data[at + 1 + n + (z - l - 1)] = y.at(z);
                            for (uint32_t p = 0; p < now; ++p) {       // new?
                                if ((uint32_t)(off[p + 1] - off[p]) != len) continue;
                                bool same = true;
                                for (uint32_t j = 1; j < len && same; ++j) same = data[off[p] + j] == data[at + j];
                                if (same) return false;
                            }
                            if (now == budget) return (full = 1) != 0;
                            off[++now] = (uint16_t)(at + len);
                            return false;
                        });
                __syncthreads();                                       // (the turn's sequences are in LDS before anyone reads them)
                cnt = (uint32_t)__shfl((int)now, turn);
                if (__shfl((int)full, turn)) result = ST_HOST;
            }
        }
        if (lane == 0) state[e] = result;
    }
}

// the residual edges by what became of them; those not extended into their list
__global__ void __launch_bounds__(HB) h_settle_kernel(const uint32_t* __restrict__ residual, uint64_t n_res, const uint8_t* __restrict__ state, uint32_t* __restrict__ not_ext,
                                                      unsigned long long* __restrict__ cnt) {
    for (uint64_t i = (uint64_t)blockIdx.x * HB + threadIdx.x; i < n_res; i += (uint64_t)gridDim.x * HB) {
        const uint32_t e = residual[i];
        if (state[e] == ST_EXT) atomicAdd(&cnt[C_EXT], 1ull);
        else if (state[e] == ST_NOT_EXT) not_ext[atomicAdd(&cnt[C_NE], 1ull)] = e;
    }
}

// What one index entry of a not-extended edge gives its rights (Closomatic.cc:288-326): te(f) for every edge behind e on the same path,
// can(f) for every edge of the mate's inverted path (list 0) or of the inverted prefix up to inv[e] (list 1); both only edges of 40
// k-mers or more other than e and inv[e].
template <class TE, class CAN>
__device__ inline void h_rights_of(const h_view& V, int e, int re, int list, uint64_t r, TE&& te, CAN&& can) {
    const auto right = [&](int f) { return V.km[f] >= MIN_RIGHT && f != e && f != re; };
    const int32_t* p = V.edges + V.start[r];
    const int n = (int)V.n_edges[r];
    if (!list) {
        for (int j = 0; j < n; ++j)
            if (p[j] == e)
                for (int l = j + 1; l < n; ++l)
                    if (right(p[l])) te(p[l]);
        const uint64_t q = r ^ 1ull;
        const int nq = (int)V.n_edges[q];
        const int32_t* pq = V.edges + V.start[q];
        for (int l = 0; l < nq; ++l)
            if (right(V.inv[pq[l]])) can(V.inv[pq[l]]);
    } else {
        for (int j = 0; j < n; ++j)
            if (p[j] == re)
                for (int l = 0; l <= j; ++l)
                    if (right(V.inv[p[l]])) can(V.inv[p[l]]);
    }
}

// too_easy and can of the not-extended edges, from the entries of pairs with bad == 0.  te == NULL: count only.  An entry's keys are
// counted, then written behind the place the count took.
__global__ void __launch_bounds__(HB) h_rights_kernel(h_view V, const uint32_t* __restrict__ not_ext, uint64_t n_ne, unsigned long long* __restrict__ te, uint64_t te_cap,
                                                      unsigned long long* __restrict__ can, int32_t* __restrict__ can_val, uint64_t can_cap, unsigned long long* __restrict__ cnt) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * HB + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * HB) >> 6;
    for (uint64_t i = wave; i < n_ne; i += n_waves) {
        const int e = (int)not_ext[i], re = V.inv[e];
        const unsigned long long a0 = V.ioff[e], nA = V.ioff[e + 1] - a0, b0 = V.ioff[re], nB = V.ioff[re + 1] - b0, hi = (unsigned long long)(uint32_t)e << 32;
        for (unsigned long long t = lane; t < nA + nB; t += 64) {
            const int list = t >= nA;
            const uint64_t r = V.iids[list ? b0 + (t - nA) : a0 + t];
            if (V.bad[r >> 1]) continue;
            uint32_t n_te = 0, n_can = 0;
            h_rights_of(V, e, re, list, r, [&](int) { ++n_te; }, [&](int) { ++n_can; });
            unsigned long long at_te = n_te ? atomicAdd(&cnt[C_TE], (unsigned long long)n_te) : 0, at_can = n_can ? atomicAdd(&cnt[C_CAN], (unsigned long long)n_can) : 0;
            if (!te) continue;
            const int32_t cls = V.bc[r];
            h_rights_of(V, e, re, list, r,
                        [&](int f) { if (at_te < te_cap) te[at_te] = hi | (uint32_t)f; ++at_te; },
                        [&](int f) { if (at_can < can_cap) { can[at_can] = hi | (uint32_t)f; can_val[at_can] = cls; } ++at_can; });
        }
    }
}

__global__ void __launch_bounds__(HB) h_unpack_kernel(const unsigned long long* __restrict__ key, uint64_t n, int32_t* __restrict__ pairs) {
    for (uint64_t i = (uint64_t)blockIdx.x * HB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * HB)
        reinterpret_cast<int2*>(pairs)[i] = make_int2((int32_t)(key[i] >> 32), (int32_t)(uint32_t)key[i]);
}

struct h_same { __host__ __device__ bool operator()(unsigned long long a, unsigned long long b) const { return a == b; } };

// (key, class) sorted by key over `bits` bits, into fresh arrays
int h_sort_pairs(snk_call& c, unsigned long long* key, int32_t* val, uint64_t n, uint32_t bits, unsigned long long** skey, int32_t** sval, char* err, size_t errcap) {
    int rc;
    if ((rc = c.alloc(n, skey)) || (rc = c.alloc(n, sval))) return rc;
    unsigned long long* ko = *skey;
    int32_t* vo = *sval;
    return c.with_temp([&](void* tmp, size_t& tb) { return rocprim::radix_sort_pairs(tmp, tb, key, ko, val, vo, (size_t)n, 0u, bits, c.st); });
}
// the distinct keys of list[0 .. n), ascending, into a fresh array
int h_sort_unique(snk_call& c, unsigned long long* list, uint64_t n, uint32_t bits, unsigned long long** out, uint64_t* n_out, char* err, size_t errcap) {
    int rc;
    unsigned long long *sorted, *uniq, *d_n;
    *n_out = 0;
    if ((rc = c.alloc(n, &sorted)) || (rc = c.alloc(n, &uniq)) || (rc = c.alloc(1, &d_n))) return rc;
    *out = uniq;
    if (!n) return SNK_OK;
    if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::radix_sort_keys(tmp, tb, list, sorted, (size_t)n, 0u, bits, c.st); }))) return rc;
    if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::unique(tmp, tb, sorted, uniq, d_n, (size_t)n, h_same(), c.st); }))) return rc;
    unsigned long long h_n = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&h_n, d_n, 8, hipMemcpyDeviceToHost, c.st));
    SNK_HIP_TRY(snk_sync(c.st));
    *n_out = h_n;
    return SNK_OK;
}

// The closure on the host, for the edges the device sent here: the same reachable set, kept in a std::set (Closomatic.cc:247-283).
bool h_host_closure(const h_view& V, int e) {
    std::set<std::vector<int>> seen;
    std::vector<std::vector<int>> work;
    const auto tail = [&](const std::vector<int>& x) {
        int k = 0;
        for (size_t j = 1; j < x.size(); ++j) k += V.km[x[j]];
        return k;
    };
    std::vector<int> x2;
    if (h_all_members(V, e, [&](const h_mem& y) {
            if (y.at(0) != e) return false;
            x2.clear();
            for (int m = 0; m < y.len; ++m) x2.push_back(y.at(m));
            if (tail(x2) >= GOOD_EXT) return true;
            if (seen.insert(x2).second) work.push_back(x2);
            return false;
        }))
        return true;
    while (!work.empty()) {
        const std::vector<int> x = std::move(work.back());
        work.pop_back();
        if (h_all_members(V, e, [&](const h_mem& y) {
                for (int l = 0; l + 1 < y.len; ++l) {
                    if (y.at(l) != x.back() || !h_agrees(x.data(), (int)x.size(), y, l)) continue;
                    x2 = x;
                    for (int z = l + 1; z < y.len; ++z) x2.push_back(y.at(z));
                    if (tail(x2) >= GOOD_EXT) return true;
                    if (seen.insert(x2).second) work.push_back(x2);
                }
                return false;
            }))
            return true;
    }
    return false;
}

struct h_host_copy {            // what the host routine reads (declared in front of the frame: asynchronous copies fill it)
    std::vector<unsigned long long> start, ioff, iids;
    std::vector<uint32_t> n_edges, residual;
    std::vector<int32_t> edges, km;
    std::vector<uint8_t> state;
};

}  // namespace

extern "C" int snk_dev_edge_pairs(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, const snk_hbv* h, const int32_t* inv,
                                  const snk_dev_paths* paths, const snk_dev_pidx* px, const void* d_bc, const void* d_bad, uint32_t flags, uint32_t ext_budget, snk_dev_hops* out,
                                  void* stream, char* err, size_t errcap) {
    static const char who[] = "snk_dev_edge_pairs";
    if (out) memset(out, 0, sizeof *out);
    if (!ctx || !h || !paths || !out) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument", who);
    if (flags & ~(SNK_HOPS_ONE_GOOD | SNK_HOPS_EXT_HOST)) return snk_fail(SNK_E_ARG, err, errcap, "%s: unknown flag bits 0x%x", who, flags & ~(SNK_HOPS_ONE_GOOD | SNK_HOPS_EXT_HOST));
    const uint64_t n = paths->n_reads, n_entries = paths->n_edges_total, E = (uint64_t)(h->n_edges > 0 ? h->n_edges : 0);
    int rc = snk_bads_check_args(who, K, n, 0, true, n_unitigs, d_unitig_off, d_unitig_bases, h, paths, SNK_BADS_X, err, errcap);
    if (rc) return rc;
    if (E && !inv) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument (inv)", who);
    if (n && (!d_bc || !d_bad)) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument (d_bc, d_bad)", who);
    if (n_entries >= (1ull << 32)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: more than 2^32 path entries in one call", who);
    for (uint64_t e = 0; e < E; ++e) {
        const int64_t r = inv[e];
        if (r < 0 || (uint64_t)r >= E || (uint64_t)inv[r] != e)
            return snk_fail(SNK_E_ARG, err, errcap, "%s: inv is not an involution of [0, %llu) at edge %llu", who, (unsigned long long)E, (unsigned long long)e);
    }
    if (px && (px->n_hbv_edges != E || px->n_entries != n_entries))
        return snk_fail(SNK_E_ARG, err, errcap, "%s: a paths index of %llu edges and %llu entries for a graph of %llu edges and paths of %llu entries", who,
                        (unsigned long long)px->n_hbv_edges, (unsigned long long)px->n_entries, (unsigned long long)E, (unsigned long long)n_entries);
    if (px && (!px->index_off || (n_entries && !px->index_ids))) return snk_fail(SNK_E_ARG, err, errcap, "%s: a paths index without its device arrays", who);
    const uint32_t budget = std::min(ext_budget ? ext_budget : H_VCAP, H_VCAP);
    uint32_t e_bits = 1;
    while (e_bits < 32 && (1ull << e_bits) < E) ++e_bits;
    path_host H;                // (the uploads read it: declared in front of the frame)
    h_host_copy hc;
    return snk_call_run(ctx, stream, who, out, err, errcap, [&](snk_call& c) -> int {
        const hipStream_t st = c.st;
        int rc2;
        SNK_HIP_TRY(c.stamp());
        // ---- the graph tables and the refusals of SNK_BADS_X (what a ReadPathVecX can hold), the index, the per-edge arrays
        bads_job job;
        if ((rc2 = snk_bads_begin(c, H, who, K, n, n_unitigs, d_unitig_off, d_unitig_bases, h, paths, SNK_BADS_X, &job, err, errcap))) return rc2;
        h_view V;
        V.start = job.start; V.n_edges = job.n_edges; V.edges = (const int32_t*)job.edges; V.bc = (const int32_t*)d_bc; V.bad = (const uint8_t*)d_bad;
        if (px) {
            V.ioff = (const unsigned long long*)px->index_off; V.iids = (const unsigned long long*)px->index_ids;
        } else {
            unsigned long long *off, *ids;
            int32_t* none;
            uint32_t key_bits;
            if ((rc2 = snk_pidx_lists(c, paths, E, who, false, &off, &ids, &none, &key_bits, err, errcap))) return rc2;
            V.ioff = off; V.iids = ids;
        }
        int32_t *d_inv, *km, *pairs;
        uint8_t *fl, *seen, *state;
        unsigned long long* cnt;
        uint32_t *residual, *not_ext;
        if ((rc2 = c.alloc(E, &d_inv)) || (rc2 = c.alloc(E, &km)) || (rc2 = c.alloc(E, &fl)) || (rc2 = c.alloc(E, &seen)) || (rc2 = c.alloc(E, &state)) ||
            (rc2 = c.alloc(N_CNT, &cnt)) || (rc2 = c.alloc(E, &residual)) || (rc2 = c.alloc(E, &not_ext)))
            return rc2;
        V.inv = d_inv; V.km = km;
        SNK_HIP_TRY(hipMemsetAsync(cnt, 0, N_CNT * 8, st));
        if (E) SNK_HIP_TRY(hipMemsetAsync(seen, 0, E, st));
        if (E) SNK_HIP_TRY(hipMemsetAsync(state, 0, E, st));
        if (E) SNK_HIP_TRY(hipMemcpyAsync(d_inv, inv, E * 4, hipMemcpyHostToDevice, st));
        if (E) SNK_HIP_TRY(snk_launch(h_edge_kernel, snk_blocks_capped(E, HB, H_GRID_CAP), HB, 0, st, job.G, (int)K, E, km, fl, cnt));
        SNK_HIP_TRY(c.stamp());
        unsigned long long h_cnt[N_CNT];
        const auto counters = [&]() -> int {
            SNK_HIP_TRY(hipMemcpyAsync(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(snk_sync(st));
            return SNK_OK;
        };
        unsigned long long *part[3] = {nullptr, nullptr, nullptr};
        uint64_t n_part[3] = {0, 0, 0};
        // ---- parts 1 and 2
        const uint64_t read_grid = snk_blocks_capped(n, HB, H_GRID_CAP);
        if (n && E) SNK_HIP_TRY(snk_launch(h_keys_kernel, read_grid, HB, 0, st, V, (const uint8_t*)fl, n, (unsigned long long*)nullptr, (int32_t*)nullptr, (uint64_t)0, cnt + C_KEYS));
        if ((rc2 = counters())) return rc2;
        const uint64_t n_keys = h_cnt[C_KEYS];
        if (n_keys) {
            unsigned long long *key, *skey, *hit1, *hit2;
            int32_t *val, *sval;
            if ((rc2 = c.alloc(n_keys, &key)) || (rc2 = c.alloc(n_keys, &val)) || (rc2 = c.alloc(n_keys, &hit1)) || (rc2 = c.alloc(n_keys, &hit2))) return rc2;
            SNK_HIP_TRY(hipMemsetAsync(cnt + C_KEYS, 0, 8, st));
            SNK_HIP_TRY(snk_launch(h_keys_kernel, read_grid, HB, 0, st, V, (const uint8_t*)fl, n, key, val, n_keys, cnt + C_KEYS));
            if ((rc2 = h_sort_pairs(c, key, val, n_keys, 32 + e_bits, &skey, &sval, err, errcap))) return rc2;
            const uint64_t grid = snk_blocks_capped(n_keys, HB, H_GRID_CAP);
            SNK_HIP_TRY(snk_launch(h_hits_kernel<1>, grid, HB, 0, st, (const unsigned long long*)skey, (const int32_t*)sval, n_keys, (const uint8_t*)fl, (const int32_t*)km, job.G,
                                   flags & SNK_HOPS_ONE_GOOD, seen, (const unsigned long long*)nullptr, (uint64_t)0, hit1, cnt + C_P1));
            SNK_HIP_TRY(snk_launch(h_hits_kernel<2>, grid, HB, 0, st, (const unsigned long long*)skey, (const int32_t*)sval, n_keys, (const uint8_t*)fl, (const int32_t*)km, job.G,
                                   0u, seen, (const unsigned long long*)nullptr, (uint64_t)0, hit2, cnt + C_P2));
            if ((rc2 = counters())) return rc2;
            if (h_cnt[C_KEYS] != n_keys) return snk_fail(SNK_E_INTERNAL, err, errcap, "%s: %llu keys counted, %llu written", who, (unsigned long long)n_keys, h_cnt[C_KEYS]);
            if ((rc2 = h_sort_unique(c, hit1, h_cnt[C_P1], 32 + e_bits, &part[0], &n_part[0], err, errcap))) return rc2;
            if ((rc2 = h_sort_unique(c, hit2, h_cnt[C_P2], 32 + e_bits, &part[1], &n_part[1], err, errcap))) return rc2;
        }
        SNK_HIP_TRY(c.stamp());
        // ---- part 3: classify, the closures of the residual edges, the rights of the not-extended ones
        uint64_t n_res = 0, n_host = 0, n_ext = 0, n_ne = 0;
        if (E) {
            SNK_HIP_TRY(snk_launch(h_classify_kernel, snk_blocks_capped(E, HB / 64, H_GRID_CAP), HB, 0, st, V, E, (int)K, state, residual, cnt));
            if ((rc2 = counters())) return rc2;
            n_res = h_cnt[C_RES];
        }
        if (n_res) {
            if (!(flags & SNK_HOPS_EXT_HOST)) {
                // the useful entries of every residual edge, sized by a counting run; then a wave per edge
                unsigned long long *n_useful, *useful_off, *useful;
                uint8_t* root1;
                if ((rc2 = c.alloc(n_res + 1, &n_useful)) || (rc2 = c.alloc(n_res + 1, &useful_off)) || (rc2 = c.alloc(n_res, &root1))) return rc2;
                SNK_HIP_TRY(hipMemsetAsync(n_useful + n_res, 0, 8, st));
                const uint64_t grid = snk_blocks_capped(n_res, HB / 64, H_GRID_CAP);
                SNK_HIP_TRY(snk_launch(h_useful_kernel<false>, grid, HB, 0, st, V, (const uint32_t*)residual, n_res, n_useful, root1, (const unsigned long long*)nullptr,
                                       (unsigned long long*)nullptr));
                if ((rc2 = c.with_temp([&](void* tmp, size_t& tb) {
                        return rocprim::exclusive_scan(tmp, tb, n_useful, useful_off, 0ull, (size_t)(n_res + 1), rocprim::plus<unsigned long long>(), st);
                    })))
                    return rc2;
                unsigned long long total_useful = 0;
                SNK_HIP_TRY(hipMemcpyAsync(&total_useful, useful_off + n_res, 8, hipMemcpyDeviceToHost, st));
                SNK_HIP_TRY(snk_sync(st));
                if ((rc2 = c.alloc(total_useful, &useful))) return rc2;
                SNK_HIP_TRY(snk_launch(h_useful_kernel<true>, grid, HB, 0, st, V, (const uint32_t*)residual, n_res, n_useful, root1, (const unsigned long long*)useful_off, useful));
                SNK_HIP_TRY(snk_launch(h_closure_kernel, snk_blocks_capped(n_res, 1, H_GRID_CAP), 64, 0, st, V, (const uint32_t*)residual, n_res, budget,
                                       (const unsigned long long*)useful_off, (const unsigned long long*)useful, (const uint8_t*)root1, state));
            }
            // the host leg: every residual edge with SNK_HOPS_EXT_HOST, else those whose set did not fit
            hc.residual.resize(n_res);
            hc.state.resize(E);
            SNK_HIP_TRY(hipMemcpyAsync(hc.residual.data(), residual, n_res * 4, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(hipMemcpyAsync(hc.state.data(), state, E, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(snk_sync(st));
            std::vector<uint32_t> todo;
            for (uint32_t e : hc.residual)
                if ((flags & SNK_HOPS_EXT_HOST) || hc.state[e] == ST_HOST) todo.push_back(e);
            n_host = todo.size();
            if (n_host) {
                hc.start.resize(n + 1); hc.n_edges.resize(n); hc.edges.resize(n_entries); hc.ioff.resize(E + 1); hc.iids.resize(n_entries); hc.km.resize(E);
                SNK_HIP_TRY(hipMemcpyAsync(hc.start.data(), V.start, (n + 1) * 8, hipMemcpyDeviceToHost, st));
                SNK_HIP_TRY(hipMemcpyAsync(hc.n_edges.data(), V.n_edges, n * 4, hipMemcpyDeviceToHost, st));
                if (n_entries) SNK_HIP_TRY(hipMemcpyAsync(hc.edges.data(), V.edges, n_entries * 4, hipMemcpyDeviceToHost, st));
                SNK_HIP_TRY(hipMemcpyAsync(hc.ioff.data(), V.ioff, (E + 1) * 8, hipMemcpyDeviceToHost, st));
                if (n_entries) SNK_HIP_TRY(hipMemcpyAsync(hc.iids.data(), V.iids, n_entries * 8, hipMemcpyDeviceToHost, st));
                SNK_HIP_TRY(hipMemcpyAsync(hc.km.data(), km, E * 4, hipMemcpyDeviceToHost, st));
                SNK_HIP_TRY(snk_sync(st));
                h_view HV;
                HV.start = hc.start.data(); HV.n_edges = hc.n_edges.data(); HV.edges = hc.edges.data(); HV.ioff = hc.ioff.data(); HV.iids = hc.iids.data();
                HV.inv = inv; HV.km = hc.km.data(); HV.bc = nullptr; HV.bad = nullptr;
                for (uint32_t e : todo) hc.state[e] = h_host_closure(HV, (int)e) ? ST_EXT : ST_NOT_EXT;
                SNK_HIP_TRY(hipMemcpyAsync(state, hc.state.data(), E, hipMemcpyHostToDevice, st));
            }
            SNK_HIP_TRY(snk_launch(h_settle_kernel, snk_blocks_capped(n_res, HB, H_GRID_CAP), HB, 0, st, (const uint32_t*)residual, n_res, (const uint8_t*)state, not_ext, cnt));
            if ((rc2 = counters())) return rc2;
            n_ext = h_cnt[C_EXT]; n_ne = h_cnt[C_NE];
            if (n_ext + n_ne != n_res) return snk_fail(SNK_E_INTERNAL, err, errcap, "%s: %llu residual edges, %llu settled", who, (unsigned long long)n_res, (unsigned long long)(n_ext + n_ne));
        }
        if (n_ne) {
            const uint64_t grid = snk_blocks_capped(n_ne, HB / 64, H_GRID_CAP);
            SNK_HIP_TRY(snk_launch(h_rights_kernel, grid, HB, 0, st, V, (const uint32_t*)not_ext, n_ne, (unsigned long long*)nullptr, (uint64_t)0, (unsigned long long*)nullptr,
                                   (int32_t*)nullptr, (uint64_t)0, cnt));
            if ((rc2 = counters())) return rc2;
            const uint64_t n_te = h_cnt[C_TE], n_can = h_cnt[C_CAN];
            if (n_can) {
                unsigned long long *te, *ste, *can, *scan, *hit3;
                int32_t *cval, *scval;
                uint64_t n_ste = 0;
                if ((rc2 = c.alloc(n_te, &te)) || (rc2 = c.alloc(n_can, &can)) || (rc2 = c.alloc(n_can, &cval)) || (rc2 = c.alloc(n_can, &hit3))) return rc2;
                SNK_HIP_TRY(hipMemsetAsync(cnt + C_TE, 0, 8, st));
                SNK_HIP_TRY(hipMemsetAsync(cnt + C_CAN, 0, 8, st));
                SNK_HIP_TRY(snk_launch(h_rights_kernel, grid, HB, 0, st, V, (const uint32_t*)not_ext, n_ne, te, n_te, can, cval, n_can, cnt));
                if ((rc2 = h_sort_unique(c, te, n_te, 32 + e_bits, &ste, &n_ste, err, errcap))) return rc2;
                if ((rc2 = h_sort_pairs(c, can, cval, n_can, 32 + e_bits, &scan, &scval, err, errcap))) return rc2;
                SNK_HIP_TRY(snk_launch(h_hits_kernel<3>, snk_blocks_capped(n_can, HB, H_GRID_CAP), HB, 0, st, (const unsigned long long*)scan, (const int32_t*)scval, n_can,
                                       (const uint8_t*)fl, (const int32_t*)km, job.G, 0u, seen, (const unsigned long long*)ste, n_ste, hit3, cnt + C_P3));
                if ((rc2 = counters())) return rc2;
                if (h_cnt[C_TE] != n_te || h_cnt[C_CAN] != n_can) return snk_fail(SNK_E_INTERNAL, err, errcap, "%s: the two runs over the rights disagree", who);
                if ((rc2 = h_sort_unique(c, hit3, h_cnt[C_P3], 32 + e_bits, &part[2], &n_part[2], err, errcap))) return rc2;
            }
        }
        SNK_HIP_TRY(c.stamp());
        // ---- the three lists as one
        const uint64_t n_all = n_part[0] + n_part[1] + n_part[2];
        unsigned long long *all, *uniq = nullptr;
        uint64_t n_pairs = 0;
        if ((rc2 = c.alloc(n_all, &all))) return rc2;
        for (uint64_t q = 0, at = 0; q < 3; at += n_part[q++])
            if (n_part[q]) SNK_HIP_TRY(hipMemcpyAsync(all + at, part[q], n_part[q] * 8, hipMemcpyDeviceToDevice, st));
        if ((rc2 = h_sort_unique(c, all, n_all, 32 + e_bits, &uniq, &n_pairs, err, errcap))) return rc2;
        if ((rc2 = c.alloc(2 * n_pairs, &pairs))) return rc2;
        if (n_pairs) SNK_HIP_TRY(snk_launch(h_unpack_kernel, snk_blocks_capped(n_pairs, HB, H_GRID_CAP), HB, 0, st, (const unsigned long long*)uniq, n_pairs, pairs));
        SNK_HIP_TRY(c.stamp());
        if ((rc2 = counters())) return rc2;
        out->n_pairs = n_pairs;
        out->pairs = pairs;
        out->n_part1 = n_part[0]; out->n_part2 = n_part[1]; out->n_part3 = n_part[2];
        out->n_sink_edges = h_cnt[C_SINK];
        out->n_long_edges = h_cnt[C_LONG];
        out->n_two_class = h_cnt[C_TWO];
        out->n_ext_round0 = h_cnt[C_R0];
        out->n_ext_closure = n_ext;
        out->n_ext_host = n_host;
        out->n_not_extended = n_ne;
        out->ms = c.ms(0, 4);
        out->tables_ms = c.ms(0, 1);
        out->part12_ms = c.ms(1, 2);
        out->part3_ms = c.ms(2, 3);
        out->ext_budget = budget;
        return c.end(SNK_OK, {pairs});
    });
}

extern "C" int snk_write_hops(const char* path, uint64_t n_pairs, const int32_t* pairs, char* err, size_t errcap) {
    if (!path || (n_pairs && !pairs)) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_hops: NULL argument");
    FILE* f = fopen(path, "wb");
    if (!f) return snk_fail(SNK_E_IO, err, errcap, "snk_write_hops: cannot create %s", path);
    bool ok = fwrite("BINWRITE", 1, 8, f) == 8 && fwrite(&n_pairs, 8, 1, f) == 1 && (!n_pairs || fwrite(pairs, 8, (size_t)n_pairs, f) == n_pairs);
    ok = fclose(f) == 0 && ok;
    if (!ok) return snk_fail(SNK_E_IO, err, errcap, "snk_write_hops: write error on %s", path);
    return SNK_OK;
}

extern "C" int snk_read_hops(const char* path, uint64_t* n_pairs, int32_t** pairs, char* err, size_t errcap) {
    if (!path || !n_pairs || !pairs) return snk_fail(SNK_E_ARG, err, errcap, "snk_read_hops: NULL argument");
    *n_pairs = 0;
    *pairs = nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) return snk_fail(SNK_E_IO, err, errcap, "snk_read_hops: cannot open %s", path);
    char magic[8];
    uint64_t n = 0;
    bool ok = fread(magic, 1, 8, f) == 8 && memcmp(magic, "BINWRITE", 8) == 0 && fread(&n, 8, 1, f) == 1;
    long at = ok ? ftell(f) : 0;
    ok = ok && fseek(f, 0, SEEK_END) == 0 && n <= (1ull << 40) && (uint64_t)ftell(f) == 16 + n * 8 && fseek(f, at, SEEK_SET) == 0;
    int32_t* p = nullptr;
    if (ok) {
        p = (int32_t*)malloc(n ? (size_t)n * 8 : 8);
        if (!p) { fclose(f); return snk_fail(SNK_E_NOMEM, err, errcap, "snk_read_hops: host allocation failed"); }
        ok = !n || fread(p, 8, (size_t)n, f) == n;
    }
    fclose(f);
    if (!ok) { free(p); return snk_fail(SNK_E_IO, err, errcap, "snk_read_hops: %s is not a BINWRITE file of int pairs", path); }
    *n_pairs = n;
    *pairs = p;
    return SNK_OK;
}
