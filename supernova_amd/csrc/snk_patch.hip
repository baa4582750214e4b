// snk_patch.hip -- gap patches into the graph on the device: what StageInsertPatch does (10X/DF.cc:656, 10X/runstages/RunStages.cc:176-230).
//
// The reference rebuilds the K-mer de Bruijn graph from the old edges, the junction (K+1)-mers and the closure sequences (BuildAll,
// paths/long/large/GapToyTools4.cc:187-214; readsToHBV_Sleek, kmers/BigKPather.cc:1528-1647), paths every old edge over the new graph
// (Pather_sleek, :594-630; to3 / left3, RunStages.cc:207-214) and moves every read path onto it (TranslatePaths, GapToyTools4.cc:220-266).
// That is the library's own hot path once more, so nothing here counts a k-mer: three calls stand around snk_dev_count_graph and
// snk_dev_hbv.
//
//   snk_dev_patch_pieces   allx as rows the count stage takes.  The graph needs every (K+1)-mer of every sequence once, on either
//       strand, so the old edges go in as their unitigs (an edge and its reverse complement are one unitig); a sequence of more than K
//       bases is cut into pieces of at most 256 bases, consecutive ones overlapping by K, so that each of its (K+1)-mers lies in one
//       piece and every piece has K+1 bases at least.  A junction (K+1)-mer is one piece.  One lane per (piece, row word).  The
//       sequences of exactly K bases have no (K+1)-mer: their k-mers are listed, canonical, sorted and distinct.
//   snk_dev_patch_merge    a listed k-mer that the new table does not hold is a one-k-mer unitig of its own (kmerize, :76-91, enters
//       it without a context): those are merged into the unitig arrays in the count stage's order (by first K bases).
//   snk_dev_patch_paths    to3 / left3 and the translated paths.  The first k-mer of every old edge is found by ONE pass over the new
//       unitigs' k-mers, each looked up in the sorted list of the k-mers asked for (16 bytes per old edge, instead of a dictionary of
//       24 bytes per new k-mer for as many look-ups as there are old edges); the walk then goes by From lists.  One lane per old edge
//       counts, a scan places, the same walk writes.  One lane per read translates; the reads that reach OverlapAppend (their start lies
//       behind the first new edge) get room for their list q by the same count / scan / write.
// Nothing here looks at a tuning option and no atomic decides a result.
#include <string.h>

#include <algorithm>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "snk_call.h"
#include "snk_common.h"
#include "snk_hbvadj.h"
#include "snk_pathgraph.h"

namespace {

constexpr unsigned PB = 256;                     // lanes of a workgroup
constexpr uint32_t PIECE = 256;                  // bases of a piece: the count stage's longest read
constexpr uint32_t ROW_WORDS = PIECE / 16;
constexpr uint64_t P_GRID_CAP = 1u << 20;
constexpr int KM_RUN = 16;                       // consecutive k-mer positions a lane of the landing pass rolls over
constexpr uint32_t F_TABLE = 1, F_EDGE = 2, F_WALK = 4, F_MISS = 8, F_BASE = 16, F_LONG = 32;
enum { N_FIRST, N_LATER, N_CLEARED, N_COUNTERS = 4 };

struct pk { uint64_t lo, hi; };                  // a canonical k-mer as the count stage's table holds it
struct pk_less { __host__ __device__ bool operator()(const pk& a, const pk& b) const { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); } };
struct pk_same { __host__ __device__ bool operator()(const pk& a, const pk& b) const { return a.hi == b.hi && a.lo == b.lo; } };
struct u32_to_u64 { __host__ __device__ unsigned long long operator()(uint32_t x) const { return x; } };

// the unitigs of a graph and which of them, read which way, an HBV edge is
struct p_graph {
    const uint64_t* uoff;
    const uint8_t* ub;
    const int32_t* e_unitig;
    const uint8_t* e_rc;
};
__device__ __forceinline__ uint32_t p_edge_len(const p_graph& S, int32_t e) { const int32_t u = S.e_unitig[e]; return (uint32_t)(S.uoff[u + 1] - S.uoff[u]); }
__device__ __forceinline__ uint32_t p_edge_base(const p_graph& S, int32_t e, uint32_t i) {
    const int32_t u = S.e_unitig[e];
    const uint64_t o = S.uoff[u], len = S.uoff[u + 1] - o;
    return S.e_rc[e] ? 3u - (S.ub[o + len - 1 - i] & 3u) : S.ub[o + i] & 3u;
}
// the largest s in [0, n) with first[s] <= p (first[0] = 0 <= p)
__device__ __forceinline__ uint64_t p_owner(const uint64_t* first, uint64_t n, uint64_t p) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (first[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}
template <int K>
__device__ __forceinline__ snk_kmer p_canon(snk_kmer f, bool* rev) {
    const snk_kmer r = snk_kmer_rc<K>(f);
    *rev = snk_kmer_lt(r, f);
    return *rev ? r : f;
}
__device__ __forceinline__ bool pk_lt(const pk& a, snk_kmer b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
// position of c in the ascending list q[0, n), or n
__device__ __forceinline__ uint64_t p_find(const pk* q, uint64_t n, snk_kmer c) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (pk_lt(q[mid], c)) lo = mid + 1; else hi = mid; }
    return lo < n && q[lo].hi == c.hi && q[lo].lo == c.lo ? lo : n;
}

// ---- pieces
__global__ void __launch_bounds__(PB) p_code_check_kernel(const uint8_t* __restrict__ b, uint64_t n, uint32_t* __restrict__ flags) {
    for (uint64_t i = (uint64_t)blockIdx.x * PB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * PB)
        if (b[i] > 3) atomicOr(flags, F_BASE);
}
// pieces of the sequences off[s] .. off[s + 1] of `bases` (unitigs, closures): piece first[s] + i starts at base i (256 - K) of sequence s
__global__ void __launch_bounds__(PB) p_seq_rows_kernel(const uint64_t* __restrict__ first, uint64_t n_seq, const uint64_t* __restrict__ off, const uint8_t* __restrict__ bases,
                                                       uint32_t K, uint64_t n_pieces, uint64_t row_base, uint32_t* __restrict__ rows, uint16_t* __restrict__ lens) {
    const uint64_t gid = (uint64_t)blockIdx.x * PB + threadIdx.x;
    const uint64_t p = gid / ROW_WORDS;
    const uint32_t w = (uint32_t)(gid % ROW_WORDS);
    if (p >= n_pieces) return;
    const uint64_t s = p_owner(first, n_seq, p);
    const uint64_t L = off[s + 1] - off[s], begin = (p - first[s]) * (uint64_t)(PIECE - K);
    const uint32_t len = (uint32_t)min((uint64_t)PIECE, L - begin);
    const uint8_t* src = bases + off[s] + begin;
    uint32_t v = 0;
    for (uint32_t j = 0; j < 16; ++j) { const uint32_t b = w * 16 + j; v = (v << 2) | (b < len ? (uint32_t)src[b] & 3u : 0u); }
    rows[(row_base + p) * ROW_WORDS + w] = v;
    if (w == 0) lens[row_base + p] = (uint16_t)len;
}
// the junction (K+1)-mers: the last K bases of e1 and base K - 1 of e2
__global__ void __launch_bounds__(PB) p_junction_rows_kernel(p_graph S, const int32_t* __restrict__ pairs, uint32_t K, uint64_t n_pieces, uint64_t row_base,
                                                            uint32_t* __restrict__ rows, uint16_t* __restrict__ lens) {
    const uint64_t gid = (uint64_t)blockIdx.x * PB + threadIdx.x;
    const uint64_t p = gid / ROW_WORDS;
    const uint32_t w = (uint32_t)(gid % ROW_WORDS);
    if (p >= n_pieces) return;
    const int32_t e1 = pairs[2 * p], e2 = pairs[2 * p + 1];
    const uint32_t L1 = p_edge_len(S, e1);
    uint32_t v = 0;
    for (uint32_t j = 0; j < 16; ++j) {
        const uint32_t b = w * 16 + j;
        v = (v << 2) | (b < K ? p_edge_base(S, e1, L1 - K + b) : b == K ? p_edge_base(S, e2, K - 1) : 0u);
    }
    rows[(row_base + p) * ROW_WORDS + w] = v;
    if (w == 0) lens[row_base + p] = (uint16_t)(K + 1);
}
// canonical k-mer of the K bases at where[i] (bit 63: of the closures, else of the unitigs)
template <int K>
__global__ void __launch_bounds__(PB) p_lonely_kernel(const uint64_t* __restrict__ where, uint64_t n, const uint8_t* __restrict__ ub, const uint8_t* __restrict__ cb, pk* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = where[i];
    const uint8_t* src = (a >> 63 ? cb : ub) + (a & ~(1ull << 63));
    snk_kmer f;
    f.hi = 0; f.lo = 0;
    for (int q = 0; q < K; ++q) f = snk_kmer_succ<K>(f, src[q] & 3u);
    bool rev;
    const snk_kmer c = p_canon<K>(f, &rev);
    out[i].lo = c.lo; out[i].hi = c.hi;
}

// ---- merge
template <int K>
__device__ __forceinline__ snk_kmer p_kmer_bytes(const uint8_t* src) {
    snk_kmer f;
    f.hi = 0; f.lo = 0;
    for (int q = 0; q < K; ++q) f = snk_kmer_succ<K>(f, src[q] & 3u);
    return f;
}
// per listed k-mer: is it missing from the table (keep), and how many unitigs come before it in the order by first K bases (rank)
template <int K>
__global__ void __launch_bounds__(PB) m_probe_kernel(const pk* __restrict__ lonely, uint64_t n, const pk* __restrict__ keys, uint64_t n_keys, const uint64_t* __restrict__ uoff,
                                                    const uint8_t* __restrict__ ub, uint64_t U, uint32_t* __restrict__ keep, uint64_t* __restrict__ rank) {
    const uint64_t i = (uint64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    snk_kmer c;
    c.hi = lonely[i].hi; c.lo = lonely[i].lo;
    keep[i] = p_find(keys, n_keys, c) == n_keys ? 1u : 0u;
    uint64_t lo = 0, hi = U;                      // unitigs [0, lo) start with a smaller k-mer
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (snk_kmer_lt(p_kmer_bytes<K>(ub + uoff[mid]), c)) lo = mid + 1; else hi = mid; }
    rank[i] = lo;
}
__global__ void __launch_bounds__(PB) m_compact_kernel(const pk* __restrict__ lonely, uint64_t n, const uint32_t* __restrict__ keep, const unsigned long long* __restrict__ pos,
                                                      const uint64_t* __restrict__ rank, pk* __restrict__ kept, uint64_t* __restrict__ kept_rank) {
    const uint64_t i = (uint64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= n || !keep[i]) return;
    kept[pos[i]] = lonely[i];
    kept_rank[pos[i]] = rank[i];
}
// kept k-mers whose rank is <= u: they come in front of unitig u
__device__ __forceinline__ uint64_t m_before(const uint64_t* kept_rank, uint64_t m, uint64_t u) {
    uint64_t lo = 0, hi = m;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (kept_rank[mid] <= u) lo = mid + 1; else hi = mid; }
    return lo;
}
// new offsets: unitig u moves behind the kept k-mers in front of it; kept k-mer j goes in front of unitig kept_rank[j]
__global__ void __launch_bounds__(PB) m_off_kernel(const uint64_t* __restrict__ uoff, uint64_t U, const uint64_t* __restrict__ kept_rank, uint64_t m, uint32_t K,
                                                  uint64_t* __restrict__ noff) {
    const uint64_t i = (uint64_t)blockIdx.x * PB + threadIdx.x;
    if (i <= U) {                                 // (i == U: the end of the last unitig; every kept k-mer lies in front of it)
        const uint64_t b = m_before(kept_rank, m, i);
        noff[i + b] = uoff[i] + (uint64_t)K * b;
    }
    if (i < m) noff[kept_rank[i] + i] = uoff[kept_rank[i]] + (uint64_t)K * i;
}
__global__ void __launch_bounds__(PB) m_bases_kernel(const uint64_t* __restrict__ uoff, const uint8_t* __restrict__ ub, uint64_t U, uint64_t total,
                                                    const uint64_t* __restrict__ kept_rank, uint64_t m, uint32_t K, uint8_t* __restrict__ nb) {
    for (uint64_t b = (uint64_t)blockIdx.x * PB + threadIdx.x; b < total; b += (uint64_t)gridDim.x * PB) {
        const uint64_t u = p_owner(uoff, U, b);
        nb[b + (uint64_t)K * m_before(kept_rank, m, u)] = ub[b];
    }
}
template <int K>
__global__ void __launch_bounds__(PB) m_kept_bases_kernel(const pk* __restrict__ kept, const uint64_t* __restrict__ kept_rank, uint64_t m, const uint64_t* __restrict__ uoff,
                                                         uint8_t* __restrict__ nb) {
    const uint64_t j = (uint64_t)blockIdx.x * PB + threadIdx.x;
    if (j >= m) return;
    snk_kmer c;
    c.hi = kept[j].hi; c.lo = kept[j].lo;
    uint8_t* dst = nb + uoff[kept_rank[j]] + (uint64_t)K * j;
    for (int q = 0; q < K; ++q) dst[q] = (uint8_t)snk_kmer_base<K>(c, q);
}

// ---- to3 / left3
template <int K>
__global__ void __launch_bounds__(PB) w_query_kernel(p_graph S, uint64_t E, pk* __restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * PB + threadIdx.x;
    if (e >= E) return;
    snk_kmer f;
    f.hi = 0; f.lo = 0;
    for (uint32_t q = 0; q < (uint32_t)K; ++q) f = snk_kmer_succ<K>(f, p_edge_base(S, (int32_t)e, q));
    bool rev;
    const snk_kmer c = p_canon<K>(f, &rev);
    out[e].lo = c.lo; out[e].hi = c.hi;
}
// every k-mer of the new unitigs against the list asked for: land[i] = position << 1 | the unitig holds the reverse complement of the
// canonical form.  A k-mer lies on a de Bruijn graph's unitigs once, so every entry has one writer.
template <int K>
__global__ void __launch_bounds__(PB) w_land_kernel(const uint64_t* __restrict__ uoff, const uint8_t* __restrict__ ub, uint64_t U, uint64_t total, const pk* __restrict__ asked,
                                                   uint64_t n_asked, unsigned long long* __restrict__ land) {
    const uint64_t p0 = ((uint64_t)blockIdx.x * PB + threadIdx.x) * KM_RUN;
    if (p0 >= total) return;
    uint64_t u = p_owner(uoff, U, p0);
    uint64_t ue = uoff[u + 1];
    snk_kmer f;
    f.hi = 0; f.lo = 0;
    bool have = false;
    for (uint64_t p = p0; p < p0 + KM_RUN && p < total; ++p) {
        while (p >= ue) { ++u; ue = uoff[u + 1]; have = false; }
        if (p + K > ue) { have = false; continue; }
        if (have) f = snk_kmer_succ<K>(f, ub[p + K - 1] & 3u);
        else { f = p_kmer_bytes<K>(ub + p); have = true; }
        bool rev;
        const snk_kmer c = p_canon<K>(f, &rev);
        const uint64_t i = p_find(asked, n_asked, c);
        if (i < n_asked) land[i] = (p << 1) | (rev ? 1ull : 0ull);
    }
}
struct w_args {
    p_graph old;
    uint64_t E_old;
    path_graph G;                  // the new graph
    uint64_t U_new;
    const pk* asked;
    uint64_t n_asked;
    const unsigned long long* land;
    uint32_t* n3;                  // [E_old + 1] edges of the walk
    int32_t* left3;
    const unsigned long long* pos; // [E_old + 1]
    int32_t* to3;
    uint32_t* flags;
};
// Pather_sleek::operator() (kmers/BigKPather.cc:594-630) for old edge e; WRITE: the edges go to out[0 .. n3[e])
template <int K, bool WRITE>
__global__ void __launch_bounds__(PB) w_walk_kernel(w_args a) {
    const uint64_t e = (uint64_t)blockIdx.x * PB + threadIdx.x;
    if (e > a.E_old) return;
    if (e == a.E_old) { if (!WRITE) a.n3[e] = 0; return; }
    int32_t* out = WRITE ? a.to3 + a.pos[e] : nullptr;
    // the first k-mer as (edge, offset)
    snk_kmer f;
    f.hi = 0; f.lo = 0;
    for (uint32_t q = 0; q < (uint32_t)K; ++q) f = snk_kmer_succ<K>(f, p_edge_base(a.old, (int32_t)e, q));
    bool qrev;
    const snk_kmer c = p_canon<K>(f, &qrev);
    const uint64_t i = p_find(a.asked, a.n_asked, c);
    const unsigned long long hit = i < a.n_asked ? a.land[i] : ~0ull;
    if (hit == ~0ull) { atomicOr(a.flags, F_MISS); if (!WRITE) { a.n3[e] = 0; a.left3[e] = 0; } return; }
    const uint64_t p = hit >> 1;
    const uint64_t u = p_owner(a.G.uoff, a.U_new, p);
    const uint32_t ulen = (uint32_t)(a.G.uoff[u + 1] - a.G.uoff[u]), o = (uint32_t)(p - a.G.uoff[u]);
    const bool against = qrev != (bool)(hit & 1);           // the unitig reads the k-mer the other way round
    int32_t cur = against ? a.G.rev[u] : a.G.fwd[u];
    const uint32_t offset = against ? ulen - K - o : o;
    uint32_t n = 0;
    if (WRITE) out[0] = cur;
    ++n;
    const uint64_t L = p_edge_len(a.old, (int32_t)e);
    uint64_t read_rem = L, edge_rem = (uint64_t)ulen - offset;
    while (read_rem > edge_rem) {
        read_rem = read_rem - edge_rem + K - 1;
        const uint32_t ro = (uint32_t)(L - read_rem);
        const int32_t v = a.G.vright[cur];
        int32_t next = -1;
        for (int32_t b = a.G.from_off[v]; b < a.G.from_off[v + 1] && next < 0; ++b) {
            const int32_t c2 = a.G.from_e[b];
            bool same = true;
            for (uint32_t q = 0; q < (uint32_t)K && same; ++q) same = pg_edge_base(a.G, c2, q) == p_edge_base(a.old, (int32_t)e, ro + q);
            if (same) next = c2;
        }
        if (next < 0) { atomicOr(a.flags, F_WALK); break; }
        cur = next;
        if (WRITE) out[n] = cur;
        ++n;
        edge_rem = pg_edge_len(a.G, cur);
    }
    if (!WRITE) { a.n3[e] = n; a.left3[e] = (int32_t)offset; }
}

// ---- translate
struct t_args {
    uint64_t n, n_entries, E_old;
    const unsigned long long* in_start;
    const uint32_t* in_n;
    const int32_t* in_off;
    const uint32_t* in_edges;
    const unsigned long long* to3_off;
    const int32_t* to3;
    const int32_t* left3;
    path_graph G;
    int K;
    uint32_t* need;                // [n + 1] entries of q a read may build (0: it never reaches OverlapAppend)
    const unsigned long long* qpos;
    int32_t* q;
    int32_t* e_out;                // [n] the edge, or -1
    int32_t* off_out;
    uint32_t* n_out;               // [n + 1]
    const unsigned long long* out_pos;
    int32_t* edges_out;
    unsigned long long* counters;
    uint32_t* flags;
};
__global__ void __launch_bounds__(PB) t_check_kernel(t_args a) {
    for (uint64_t r = (uint64_t)blockIdx.x * PB + threadIdx.x; r < a.n; r += (uint64_t)gridDim.x * PB) {
        if (!snk_paths_row_ok(a.in_start, a.in_n, r, a.n, a.n_entries)) atomicOr(a.flags, F_TABLE);
    }
    for (uint64_t i = (uint64_t)blockIdx.x * PB + threadIdx.x; i < a.n_entries; i += (uint64_t)gridDim.x * PB)
        if (a.in_edges[i] >= a.E_old) atomicOr(a.flags, F_EDGE);
}
// TranslatePaths (GapToyTools4.cc:228-262) up to the loop over the path; a read that reaches the loop only says how long q may get
// the three counters of a workgroup, in LDS; one global add each when the workgroup is through
struct t_counts {
    uint32_t* c;
    __device__ t_counts(uint32_t* lds) : c(lds) {
        if (threadIdx.x < N_COUNTERS) c[threadIdx.x] = 0;
        __syncthreads();
    }
    __device__ void add(int which) { atomicAdd(c + which, 1u); }
    __device__ void flush(unsigned long long* global) {
        __syncthreads();
        if (threadIdx.x < N_COUNTERS && c[threadIdx.x]) atomicAdd(global + threadIdx.x, (unsigned long long)c[threadIdx.x]);
    }
};
__global__ void __launch_bounds__(PB) t_first_kernel(t_args a) {
    __shared__ uint32_t lds[N_COUNTERS];
    t_counts cnt(lds);
    for (uint64_t r = (uint64_t)blockIdx.x * PB + threadIdx.x; r <= a.n; r += (uint64_t)gridDim.x * PB) {
        if (r == a.n) { a.need[r] = 0; a.n_out[r] = 0; continue; }
        const uint64_t s = a.in_start[r], m = a.in_n[r];
        uint32_t need = 0, n_out = 0;
        int32_t e_out = -1, off_out = 0;
        if (m) {
            const uint32_t e = a.in_edges[s];
            const long long start = (long long)a.in_off[r] + a.left3[e];
            const uint64_t t0 = a.to3_off[e], t1 = a.to3_off[e + 1];
            if (t0 == t1) cnt.add(N_CLEARED);
            else if (start < (long long)pg_edge_len(a.G, a.to3[t0])) {
                e_out = a.to3[t0]; off_out = (int32_t)start; n_out = 1;
                cnt.add(N_FIRST);
            } else {
                uint64_t sum = 0;
                for (uint64_t j = 0; j < m; ++j) {
                    const uint32_t x = a.in_edges[s + j];
                    const uint64_t c = a.to3_off[x + 1] - a.to3_off[x];
                    if (!c) break;
                    sum += c;
                }
                if (sum > 0xFFFFFFFFull) { atomicOr(a.flags, F_LONG); sum = 0; }
                need = (uint32_t)sum;
            }
        }
        a.need[r] = need; a.n_out[r] = n_out; a.e_out[r] = e_out; a.off_out[r] = off_out;
    }
    cnt.flush(a.counters);
}
// ... and the loop: q by OverlapAppend (Vec.h:604-619: the LONGEST overlap), then the trim
__global__ void __launch_bounds__(PB) t_later_kernel(t_args a) {
    __shared__ uint32_t lds[N_COUNTERS];
    t_counts cnt(lds);
    for (uint64_t r = (uint64_t)blockIdx.x * PB + threadIdx.x; r < a.n; r += (uint64_t)gridDim.x * PB) {
        if (!a.need[r]) continue;
        int32_t* q = a.q + a.qpos[r];
        const uint64_t s = a.in_start[r], m = a.in_n[r];
        long long start = (long long)a.in_off[r] + a.left3[a.in_edges[s]];
        uint64_t nq = 0;
        for (uint64_t j = 0; j < m; ++j) {
            const uint32_t x = a.in_edges[s + j];
            const int32_t* v = a.to3 + a.to3_off[x];
            const uint64_t nv = a.to3_off[x + 1] - a.to3_off[x];
            if (!nv) break;
            uint64_t best = 0;
            for (uint64_t o = min(nq, nv); o; --o) {
                bool same = true;
                for (uint64_t t = 0; t < o && same; ++t) same = q[nq - o + t] == v[t];
                if (same) { best = o; break; }
            }
            for (uint64_t t = best; t < nv; ++t) q[nq++] = v[t];
        }
        uint64_t trim = 0;
        while (start >= (long long)pg_edge_len(a.G, q[trim])) {
            start -= (long long)pg_edge_len(a.G, q[trim]) - (a.K - 1);
            if (++trim == nq) break;
        }
        if (trim == nq) { cnt.add(N_CLEARED); continue; }
        a.e_out[r] = q[trim]; a.off_out[r] = (int32_t)start; a.n_out[r] = 1;
        cnt.add(N_LATER);
    }
    cnt.flush(a.counters);
}
__global__ void __launch_bounds__(PB) t_gather_kernel(t_args a) {
    for (uint64_t r = (uint64_t)blockIdx.x * PB + threadIdx.x; r < a.n; r += (uint64_t)gridDim.x * PB)
        if (a.n_out[r]) a.edges_out[a.out_pos[r]] = a.e_out[r];
}

template <typename T>
int p_up(snk_call& c, const std::vector<T>& h, const T** out, char* err, size_t errcap) {
    T* d;
    const int rc = c.alloc(h.size(), &d);
    if (rc) return rc;
    if (!h.empty()) SNK_HIP_TRY(hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, c.st));
    *out = d;
    return SNK_OK;
}
int p_scan32(snk_call& c, const uint32_t* in, unsigned long long* out, size_t count) {
    rocprim::transform_iterator<const uint32_t*, u32_to_u64, unsigned long long> it(in, u32_to_u64());
    return c.with_temp([&](void* tmp, size_t& tb) { return rocprim::exclusive_scan(tmp, tb, it, out, 0ull, count, rocprim::plus<unsigned long long>(), c.st); });
}

// pieces of a sequence of L bases
inline uint64_t pieces_of(uint64_t L, uint32_t K) { return L <= K ? 0 : (L - K + (PIECE - K) - 1) / (PIECE - K); }

// what the host derives from the old graph and the closures: checked offsets, piece counts, the junction pairs' number
int plan_sizes(const char* who, uint32_t K, uint64_t U, const uint64_t* uoff, const snk_hbv* h, uint64_t C, const uint64_t* coff, snk_patch_plan* out, char* err, size_t errcap) {
    memset(out, 0, sizeof *out);
    if (K != 48 && K != 60) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "K=%u is not supported (48 or 60)", K);
    if (!h || (U && !uoff) || (C && !coff)) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument", who);
    if (U >= (1ull << 31)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: too many unitigs", who);
    const uint64_t E = (uint64_t)(h->n_edges > 0 ? h->n_edges : 0), N = (uint64_t)(h->n_vertices > 0 ? h->n_vertices : 0);
    if (E && (!h->v_left || !h->v_right || !h->src_unitig || !h->is_rc)) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument", who);
    for (uint64_t u = 0; u < U; ++u) {
        if (uoff[u + 1] < uoff[u] + K || (u == 0 && uoff[0] != 0)) return snk_fail(SNK_E_ARG, err, errcap, "%s: unitig %llu has fewer than K bases, or the offsets do not start at 0", who, (unsigned long long)u);
        if (uoff[u + 1] - uoff[u] > 0xFFFFFFFFull) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: a unitig of more than 2^32 - 1 bases", who);
        if (h->bvcomp_order && (h->bvcomp_order[u] < 0 || (uint64_t)h->bvcomp_order[u] >= U)) return snk_fail(SNK_E_ARG, err, errcap, "%s: inconsistent translation tables", who);
        out->n_unitig_pieces += pieces_of(uoff[u + 1] - uoff[u], K);
        out->n_lonely_max += uoff[u + 1] - uoff[u] == K;
    }
    for (uint64_t c = 0; c < C; ++c) {
        if (coff[c + 1] < coff[c] || (c == 0 && coff[0] != 0)) return snk_fail(SNK_E_ARG, err, errcap, "%s: the closure offsets do not ascend from 0", who);
        out->n_closure_pieces += pieces_of(coff[c + 1] - coff[c], K);
        out->n_lonely_max += coff[c + 1] - coff[c] == K;
    }
    std::vector<uint32_t> n_in(N, 0), n_out(N, 0);
    for (uint64_t e = 0; e < E; ++e) {
        if (h->v_left[e] < 0 || (uint64_t)h->v_left[e] >= N || h->v_right[e] < 0 || (uint64_t)h->v_right[e] >= N || h->src_unitig[e] < 0 || (uint64_t)h->src_unitig[e] >= U)
            return snk_fail(SNK_E_ARG, err, errcap, "%s: edge %llu is out of range", who, (unsigned long long)e);
        ++n_out[h->v_left[e]];
        ++n_in[h->v_right[e]];
    }
    for (uint64_t v = 0; v < N; ++v) out->n_junctions += (uint64_t)n_in[v] * n_out[v];
    out->n_pieces = out->n_unitig_pieces + out->n_junctions + out->n_closure_pieces;
    return SNK_OK;
}

struct pieces_host {
    std::vector<uint64_t> uoff, ufirst, coff, cfirst, where;
    std::vector<int32_t> pairs, eu;
    std::vector<uint8_t> erc;
};
// the old graph's edges as (unitig in the device arrays' numbering, strand)
void edge_tables(const snk_hbv* h, std::vector<int32_t>& eu, std::vector<uint8_t>& erc) {
    const int32_t E = h->n_edges > 0 ? h->n_edges : 0;
    eu.resize((size_t)E); erc.resize((size_t)E);
    for (int32_t e = 0; e < E; ++e) {
        const int32_t r = h->src_unitig[e];
        eu[e] = h->bvcomp_order ? h->bvcomp_order[r] : r;
        erc[e] = h->is_rc[e];
    }
}

template <int K>
int pieces_impl(snk_call& c, pieces_host& H, uint64_t U, const uint8_t* d_ub, const snk_hbv* h, uint64_t C, const uint8_t* d_cb, const snk_patch_plan& plan, uint32_t* rows,
                uint16_t* lens, pk* lonely, snk_dev_pieces* out, char* err, size_t errcap) {
    const hipStream_t st = c.st;
    int rc;
    SNK_HIP_TRY(c.stamp());
    uint32_t* flags;
    if ((rc = c.alloc(1, &flags))) return rc;
    SNK_HIP_TRY(hipMemsetAsync(flags, 0, 4, st));
    const uint64_t cbases = C ? H.coff[C] : 0;
    SNK_HIP_TRY(snk_launch(p_code_check_kernel, cbases ? snk_blocks_capped(cbases, PB, P_GRID_CAP) : 0, PB, 0, st, d_cb, cbases, flags));
    uint32_t f = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&f, flags, 4, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    if (f & F_BASE) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_pieces: a closure holds a base code above 3");
    // the host's part: first piece of every sequence, the junction pairs in BuildAll's order, where the K-base sequences lie
    H.ufirst.assign(U + 1, 0);
    for (uint64_t u = 0; u < U; ++u) {
        H.ufirst[u + 1] = H.ufirst[u] + pieces_of(H.uoff[u + 1] - H.uoff[u], K);
        if (H.uoff[u + 1] - H.uoff[u] == K) H.where.push_back(H.uoff[u]);
    }
    H.cfirst.assign(C + 1, 0);
    for (uint64_t i = 0; i < C; ++i) {
        H.cfirst[i + 1] = H.cfirst[i] + pieces_of(H.coff[i + 1] - H.coff[i], K);
        if (H.coff[i + 1] - H.coff[i] == K) H.where.push_back(H.coff[i] | (1ull << 63));
    }
    edge_tables(h, H.eu, H.erc);
    {
        snk_hbv_lists ls;
        if ((rc = snk_hbv_lists_build(h, &ls, "snk_dev_patch_pieces", err, errcap))) return rc;
        H.pairs.reserve(2 * plan.n_junctions);
        for (int32_t v = 0; v < h->n_vertices; ++v)
            for (uint64_t i1 = ls.to_off[v]; i1 < ls.to_off[(size_t)v + 1]; ++i1)
                for (uint64_t i2 = ls.from_off[v]; i2 < ls.from_off[(size_t)v + 1]; ++i2) { H.pairs.push_back(ls.to_e[i1]); H.pairs.push_back(ls.from_e[i2]); }
    }
    if (H.pairs.size() != 2 * plan.n_junctions || H.ufirst[U] != plan.n_unitig_pieces || H.cfirst[C] != plan.n_closure_pieces || H.where.size() != plan.n_lonely_max)
        return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_patch_pieces: the plan and the pieces differ");
    p_graph S;
    const uint64_t *d_ufirst, *d_cfirst, *d_coff, *d_where;
    const int32_t* d_pairs;
    if ((rc = p_up(c, H.uoff, &S.uoff, err, errcap)) || (rc = p_up(c, H.eu, &S.e_unitig, err, errcap)) || (rc = p_up(c, H.erc, &S.e_rc, err, errcap)) ||
        (rc = p_up(c, H.ufirst, &d_ufirst, err, errcap)) || (rc = p_up(c, H.cfirst, &d_cfirst, err, errcap)) || (rc = p_up(c, H.coff, &d_coff, err, errcap)) ||
        (rc = p_up(c, H.where, &d_where, err, errcap)) || (rc = p_up(c, H.pairs, &d_pairs, err, errcap)))
        return rc;
    S.ub = d_ub;
    SNK_HIP_TRY(snk_launch(p_seq_rows_kernel, snk_blocks(plan.n_unitig_pieces * ROW_WORDS, PB), PB, 0, st, d_ufirst, U, S.uoff, d_ub, (uint32_t)K, plan.n_unitig_pieces, (uint64_t)0, rows, lens));
    SNK_HIP_TRY(snk_launch(p_junction_rows_kernel, snk_blocks(plan.n_junctions * ROW_WORDS, PB), PB, 0, st, S, d_pairs, (uint32_t)K, plan.n_junctions, plan.n_unitig_pieces, rows, lens));
    SNK_HIP_TRY(snk_launch(p_seq_rows_kernel, snk_blocks(plan.n_closure_pieces * ROW_WORDS, PB), PB, 0, st, d_cfirst, C, d_coff, d_cb, (uint32_t)K, plan.n_closure_pieces,
                           plan.n_unitig_pieces + plan.n_junctions, rows, lens));
    // the k-mers of the K-base sequences: canonical, ascending, distinct
    uint64_t n_lonely = 0;
    const uint64_t nl = plan.n_lonely_max;
    if (nl) {
        pk *raw, *sorted;
        unsigned long long* d_count;
        if ((rc = c.alloc(nl, &raw)) || (rc = c.alloc(nl, &sorted)) || (rc = c.alloc(1, &d_count))) return rc;
        SNK_HIP_TRY(snk_launch(p_lonely_kernel<K>, snk_blocks(nl, PB), PB, 0, st, d_where, nl, d_ub, d_cb, raw));
        if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::merge_sort(tmp, tb, raw, sorted, (size_t)nl, pk_less(), st); }))) return rc;
        if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::unique(tmp, tb, sorted, lonely, d_count, (size_t)nl, pk_same(), st); }))) return rc;
        unsigned long long h_count = 0;
        SNK_HIP_TRY(hipMemcpyAsync(&h_count, d_count, 8, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        if (h_count > nl) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_patch_pieces: the list of K-base sequences is out of range");
        n_lonely = h_count;
    }
    SNK_HIP_TRY(c.stamp());
    SNK_HIP_TRY(snk_sync(st));
    out->n_pieces = plan.n_pieces;
    out->n_lonely = n_lonely;
    out->ms = c.ms(0, 1);
    return SNK_OK;
}

template <int K>
int merge_impl(snk_call& c, const snk_dev_result* res, const pk* lonely, uint64_t nl, snk_dev_patch_unitigs* out, char* err, size_t errcap) {
    const hipStream_t st = c.st;
    int rc;
    SNK_HIP_TRY(c.stamp());
    const uint64_t U = res->n_unitigs, total = res->unitig_total_bases;
    const uint64_t* uoff = (const uint64_t*)res->unitig_off;
    const uint8_t* ub = (const uint8_t*)res->unitig_bases;
    if (!U) {                                     // no piece at all: the offsets of no unitig
        uint64_t* zero;
        if ((rc = c.alloc(1, &zero))) return rc;
        SNK_HIP_TRY(hipMemsetAsync(zero, 0, 8, st));
        uoff = zero;
    }
    uint32_t* keep;
    uint64_t* rank;
    unsigned long long* pos;
    if ((rc = c.alloc(nl + 1, &keep)) || (rc = c.alloc(nl, &rank)) || (rc = c.alloc(nl + 1, &pos))) return rc;
    SNK_HIP_TRY(hipMemsetAsync(keep + nl, 0, 4, st));
    SNK_HIP_TRY(snk_launch(m_probe_kernel<K>, snk_blocks(nl, PB), PB, 0, st, lonely, nl, (const pk*)res->keys, res->n_kmers, uoff, ub, U, keep, rank));
    if ((rc = p_scan32(c, keep, pos, (size_t)(nl + 1)))) return rc;
    unsigned long long m = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&m, pos + nl, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    if (m > nl) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_patch_merge: the scan's total is out of range");
    if (!m) {                                     // every listed k-mer lies on the graph already: the count stage's arrays are the result
        out->n_unitigs = U; out->unitig_total_bases = total; out->unitig_off = uoff; out->unitig_bases = ub;
        return SNK_OK;
    }
    if (U + m >= (1ull << 31)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_patch_merge: too many unitigs");
    pk* kept;
    uint64_t *kept_rank, *noff;
    uint8_t* nb;
    if ((rc = c.alloc(m, &kept)) || (rc = c.alloc(m, &kept_rank)) || (rc = c.alloc(U + m + 1, &noff)) || (rc = c.alloc(total + (uint64_t)K * m, &nb))) return rc;
    SNK_HIP_TRY(snk_launch(m_compact_kernel, snk_blocks(nl, PB), PB, 0, st, lonely, nl, keep, pos, rank, kept, kept_rank));
    SNK_HIP_TRY(snk_launch(m_off_kernel, snk_blocks(std::max<uint64_t>(U + 1, m), PB), PB, 0, st, uoff, U, kept_rank, (uint64_t)m, (uint32_t)K, noff));
    SNK_HIP_TRY(snk_launch(m_bases_kernel, total ? snk_blocks_capped(total, PB, P_GRID_CAP) : 0, PB, 0, st, uoff, ub, U, total, kept_rank, (uint64_t)m, (uint32_t)K, nb));
    SNK_HIP_TRY(snk_launch(m_kept_bases_kernel<K>, snk_blocks(m, PB), PB, 0, st, kept, kept_rank, (uint64_t)m, uoff, nb));
    SNK_HIP_TRY(c.stamp());
    SNK_HIP_TRY(snk_sync(st));
    out->n_unitigs = U + m; out->unitig_total_bases = total + (uint64_t)K * m; out->unitig_off = noff; out->unitig_bases = nb; out->n_added = m;
    out->ms = c.ms(0, 1);
    return c.end(SNK_OK, {noff, nb});
}

struct paths_host {
    std::vector<int32_t> eu;
    std::vector<uint8_t> erc;
    path_host H;
};

template <int K>
int paths_impl(snk_call& c, paths_host& PH, uint64_t U_old, const uint64_t* d_uoff_old, const uint8_t* d_ub_old, const snk_hbv* h_old, uint64_t U_new, const uint64_t* d_uoff_new,
               const uint8_t* d_ub_new, const snk_hbv* h_new, const snk_dev_paths* paths, snk_dev_patched* out, char* err, size_t errcap) {
    const hipStream_t st = c.st;
    int rc;
    SNK_HIP_TRY(c.stamp());
    const uint64_t E_old = (uint64_t)(h_old->n_edges > 0 ? h_old->n_edges : 0), n = paths->n_reads, n_entries = paths->n_edges_total;
    uint32_t* flags;
    unsigned long long* counters;
    if ((rc = c.alloc(1, &flags)) || (rc = c.alloc(N_COUNTERS, &counters))) return rc;
    SNK_HIP_TRY(hipMemsetAsync(flags, 0, 4, st));
    SNK_HIP_TRY(hipMemsetAsync(counters, 0, N_COUNTERS * 8, st));
    t_args t;
    memset(&t, 0, sizeof t);
    t.n = n; t.n_entries = n_entries; t.E_old = E_old; t.K = K; t.flags = flags; t.counters = counters;
    t.in_start = (const unsigned long long*)paths->start; t.in_n = (const uint32_t*)paths->n_edges; t.in_off = (const int32_t*)paths->offset;
    t.in_edges = (const uint32_t*)paths->edges;
    // ---- the refusals that need the paths only
    SNK_HIP_TRY(snk_launch(t_check_kernel, snk_blocks_capped(std::max(n, n_entries), PB, P_GRID_CAP), PB, 0, st, t));
    uint32_t f = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&f, flags, 4, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    if (f & F_TABLE) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: start / n_edges do not add up to n_edges_total = %llu", (unsigned long long)n_entries);
    if (f & F_EDGE) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: a path holds an edge id outside the old graph's %llu edges", (unsigned long long)E_old);
    // ---- both graphs
    w_args w;
    memset(&w, 0, sizeof w);
    uint64_t total_new = 0;
    if ((rc = snk_path_graph_tables(c, PH.H, K, U_new, d_uoff_new, d_ub_new, h_new, &w.G, &total_new, "snk_dev_patch_paths", err, errcap))) return rc;
    edge_tables(h_old, PH.eu, PH.erc);
    w.old.uoff = d_uoff_old; w.old.ub = d_ub_old;
    if ((rc = p_up(c, PH.eu, &w.old.e_unitig, err, errcap)) || (rc = p_up(c, PH.erc, &w.old.e_rc, err, errcap))) return rc;
    w.E_old = E_old; w.U_new = U_new; w.flags = flags;
    // ---- where the first k-mer of every old edge lies
    pk *asked_raw, *asked_sorted, *asked;
    unsigned long long *land, *d_count;
    if ((rc = c.alloc(E_old, &asked_raw)) || (rc = c.alloc(E_old, &asked_sorted)) || (rc = c.alloc(E_old, &asked)) || (rc = c.alloc(E_old, &land)) || (rc = c.alloc(1, &d_count))) return rc;
    unsigned long long n_asked = 0;
    if (E_old) {
        SNK_HIP_TRY(snk_launch(w_query_kernel<K>, snk_blocks(E_old, PB), PB, 0, st, w.old, E_old, asked_raw));
        if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::merge_sort(tmp, tb, asked_raw, asked_sorted, (size_t)E_old, pk_less(), st); }))) return rc;
        if ((rc = c.with_temp([&](void* tmp, size_t& tb) { return rocprim::unique(tmp, tb, asked_sorted, asked, d_count, (size_t)E_old, pk_same(), st); }))) return rc;
        SNK_HIP_TRY(hipMemcpyAsync(&n_asked, d_count, 8, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(hipMemsetAsync(land, 0xFF, E_old * 8, st));
        SNK_HIP_TRY(snk_sync(st));
        if (n_asked > E_old) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_patch_paths: the list of first k-mers is out of range");
        SNK_HIP_TRY(snk_launch(w_land_kernel<K>, snk_blocks(snk_blocks(total_new, KM_RUN), PB), PB, 0, st, d_uoff_new, d_ub_new, U_new, total_new, asked, (uint64_t)n_asked, land));
    }
    w.asked = asked; w.n_asked = n_asked; w.land = land;
    // ---- to3 / left3: count, scan, write
    uint32_t* n3;
    int32_t *left3, *to3;
    unsigned long long* pos3;
    if ((rc = c.alloc(E_old + 1, &n3)) || (rc = c.alloc(E_old, &left3)) || (rc = c.alloc(E_old + 1, &pos3))) return rc;
    w.n3 = n3; w.left3 = left3;
    SNK_HIP_TRY(snk_launch((w_walk_kernel<K, false>), snk_blocks(E_old + 1, PB), PB, 0, st, w));
    if ((rc = p_scan32(c, n3, pos3, (size_t)(E_old + 1)))) return rc;
    unsigned long long n_to3 = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&n_to3, pos3 + E_old, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(hipMemcpyAsync(&f, flags, 4, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    if (f & F_MISS) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: the first k-mer of an old edge is not on the new graph (it was not built from the old one)");
    if (f & F_WALK) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: an old edge leaves the new graph (no out-edge carries its next k-mer)");
    if ((rc = c.alloc((size_t)n_to3, &to3))) return rc;
    w.pos = pos3; w.to3 = to3;
    SNK_HIP_TRY(snk_launch((w_walk_kernel<K, true>), snk_blocks(E_old + 1, PB), PB, 0, st, w));
    SNK_HIP_TRY(c.stamp());
    // ---- translate
    t.to3_off = pos3; t.to3 = to3; t.left3 = left3; t.G = w.G;
    uint32_t *need, *n_out;
    unsigned long long *qpos, *out_pos;
    int32_t *e_out, *off_out, *q, *edges_out;
    if ((rc = c.alloc(n + 1, &need)) || (rc = c.alloc(n + 1, &n_out)) || (rc = c.alloc(n + 1, &qpos)) || (rc = c.alloc(n + 1, &out_pos)) || (rc = c.alloc(n, &e_out)) ||
        (rc = c.alloc(n, &off_out)))
        return rc;
    t.need = need; t.n_out = n_out; t.e_out = e_out; t.off_out = off_out;
    const uint64_t grid = snk_blocks_capped(n + 1, PB, std::min<uint64_t>((uint64_t)c.ctx->n_cu * 64, P_GRID_CAP));
    SNK_HIP_TRY(snk_launch(t_first_kernel, grid, PB, 0, st, t));
    if ((rc = p_scan32(c, need, qpos, (size_t)(n + 1)))) return rc;
    unsigned long long q_total = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&q_total, qpos + n, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(hipMemcpyAsync(&f, flags, 4, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    if (f & F_LONG) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_patch_paths: a path whose new edges number 2^32 or more");
    if ((rc = c.alloc((size_t)q_total, &q))) return rc;
    t.qpos = qpos; t.q = q;
    if (q_total) SNK_HIP_TRY(snk_launch(t_later_kernel, grid, PB, 0, st, t));
    if ((rc = p_scan32(c, n_out, out_pos, (size_t)(n + 1)))) return rc;
    unsigned long long total = 0, h_cnt[N_COUNTERS];
    SNK_HIP_TRY(hipMemcpyAsync(&total, out_pos + n, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(hipMemcpyAsync(h_cnt, counters, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    if (total > n) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_patch_paths: the scan's total is out of range");
    if ((rc = c.alloc((size_t)total, &edges_out))) return rc;
    t.out_pos = out_pos; t.edges_out = edges_out;
    SNK_HIP_TRY(snk_launch(t_gather_kernel, grid, PB, 0, st, t));
    SNK_HIP_TRY(c.stamp());
    SNK_HIP_TRY(snk_sync(st));
    out->paths.n_reads = n; out->paths.n_edges_total = total; out->paths.offset = off_out; out->paths.n_edges = n_out; out->paths.start = out_pos; out->paths.edges = edges_out;
    out->paths.path_ms = c.ms(1, 2);
    out->n_old_edges = E_old; out->n_to3 = n_to3; out->to3_off = pos3; out->to3 = to3; out->left3 = left3;
    out->n_first = h_cnt[N_FIRST]; out->n_later = h_cnt[N_LATER]; out->n_cleared = h_cnt[N_CLEARED];
    out->map_ms = c.ms(0, 1); out->ms = c.ms(0, 2);
    return c.end(SNK_OK, {off_out, n_out, out_pos, edges_out, pos3, to3, left3});
}

}  // namespace

extern "C" int snk_patch_plan_sizes(uint32_t K, uint64_t n_unitigs, const uint64_t* unitig_off, const snk_hbv* h, uint64_t n_closures, const uint64_t* closure_off,
                                    snk_patch_plan* out, char* err, size_t errcap) {
    if (!out) return snk_fail(SNK_E_ARG, err, errcap, "snk_patch_plan_sizes: NULL argument");
    SNK_GUARD_AS("snk_patch_plan_sizes", return plan_sizes("snk_patch_plan_sizes", K, n_unitigs, unitig_off, h, n_closures, closure_off, out, err, errcap);)
}

extern "C" int snk_dev_patch_pieces(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const uint64_t* unitig_off, const void* d_unitig_bases, const snk_hbv* h, uint64_t n_closures,
                                    const uint64_t* closure_off, const void* d_closure_bases, uint64_t piece_capacity, void* d_rows, void* d_lens, uint64_t lonely_capacity,
                                    void* d_lonely, snk_dev_pieces* out, void* stream, char* err, size_t errcap) {
    if (!ctx || !out) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_pieces: NULL argument");
    memset(out, 0, sizeof *out);
    snk_patch_plan plan;
    pieces_host H;
    SNK_GUARD_AS("snk_dev_patch_pieces",
        const int rc0 = plan_sizes("snk_dev_patch_pieces", K, n_unitigs, unitig_off, h, n_closures, closure_off, &plan, err, errcap);
        if (rc0) return rc0;
        if (n_unitigs && !d_unitig_bases) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_pieces: NULL unitig arrays");
        if (n_closures && closure_off[n_closures] && !d_closure_bases) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_pieces: NULL closure bases");
        if (plan.n_pieces > piece_capacity || plan.n_lonely_max > lonely_capacity || (plan.n_pieces && (!d_rows || !d_lens)) || (plan.n_lonely_max && !d_lonely))
            return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_pieces: the caller's buffers hold %llu pieces and %llu k-mers, the plan needs %llu and %llu",
                            (unsigned long long)piece_capacity, (unsigned long long)lonely_capacity, (unsigned long long)plan.n_pieces, (unsigned long long)plan.n_lonely_max);
        H.uoff.assign(unitig_off, unitig_off + (n_unitigs ? n_unitigs + 1 : 0));
        if (!n_unitigs) H.uoff.assign(1, 0);
        H.coff.assign(closure_off, closure_off + (n_closures ? n_closures + 1 : 0));
        if (!n_closures) H.coff.assign(1, 0);
    )
    return snk_call_run(ctx, stream, "snk_dev_patch_pieces", out, err, errcap, [&](snk_call& c) -> int {
        return K == 48 ? pieces_impl<48>(c, H, n_unitigs, (const uint8_t*)d_unitig_bases, h, n_closures, (const uint8_t*)d_closure_bases, plan, (uint32_t*)d_rows, (uint16_t*)d_lens,
                                         (pk*)d_lonely, out, err, errcap)
                       : pieces_impl<60>(c, H, n_unitigs, (const uint8_t*)d_unitig_bases, h, n_closures, (const uint8_t*)d_closure_bases, plan, (uint32_t*)d_rows, (uint16_t*)d_lens,
                                         (pk*)d_lonely, out, err, errcap);
    });
}

extern "C" int snk_dev_patch_merge(snk_ctx* ctx, uint32_t K, const snk_dev_result* res, const void* d_lonely, uint64_t n_lonely, snk_dev_patch_unitigs* out, void* stream,
                                   char* err, size_t errcap) {
    if (!ctx || !res || !out) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_merge: NULL argument");
    memset(out, 0, sizeof *out);
    if (K != 48 && K != 60) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "K=%u is not supported (48 or 60)", K);
    if ((n_lonely && !d_lonely) || (res->n_unitigs && (!res->unitig_off || !res->unitig_bases)) || (res->n_kmers && !res->keys) || (!res->n_unitigs && res->unitig_total_bases))
        return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_merge: NULL argument");
    if (!n_lonely) {
        out->n_unitigs = res->n_unitigs; out->unitig_total_bases = res->unitig_total_bases; out->unitig_off = res->unitig_off; out->unitig_bases = res->unitig_bases;
        return SNK_OK;
    }
    return snk_call_run(ctx, stream, "snk_dev_patch_merge", out, err, errcap, [&](snk_call& c) -> int {
        return K == 48 ? merge_impl<48>(c, res, (const pk*)d_lonely, n_lonely, out, err, errcap) : merge_impl<60>(c, res, (const pk*)d_lonely, n_lonely, out, err, errcap);
    });
}

extern "C" int snk_dev_patch_paths(snk_ctx* ctx, uint32_t K, uint64_t n_old_unitigs, const void* d_old_unitig_off, const void* d_old_unitig_bases, const snk_hbv* h_old,
                                   uint64_t n_new_unitigs, const void* d_new_unitig_off, const void* d_new_unitig_bases, const snk_hbv* h_new, const snk_dev_paths* paths,
                                   snk_dev_patched* out, void* stream, char* err, size_t errcap) {
    if (!ctx || !h_old || !h_new || !paths || !out) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: NULL argument");
    memset(out, 0, sizeof *out);
    if (K != 48 && K != 60) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "K=%u is not supported (48 or 60)", K);
    const uint64_t n = paths->n_reads, n_entries = paths->n_edges_total;
    const snk_hbv* hs[2] = {h_old, h_new};
    const uint64_t Us[2] = {n_old_unitigs, n_new_unitigs};
    const void* arrs[4] = {d_old_unitig_off, d_old_unitig_bases, d_new_unitig_off, d_new_unitig_bases};
    for (int g = 0; g < 2; ++g) {
        const snk_hbv* h = hs[g];
        const uint64_t U = Us[g], E = (uint64_t)(h->n_edges > 0 ? h->n_edges : 0);
        if (U >= (1ull << 31)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_patch_paths: too many unitigs");
        if (U && (!arrs[2 * g] || !arrs[2 * g + 1])) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: NULL unitig arrays");
        if (E && (!h->v_left || !h->v_right || !h->src_unitig || !h->is_rc || !h->fwd_xlat || !h->rev_xlat)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: NULL argument");
        for (uint64_t u = 0; u < U; ++u)
            if (h->fwd_xlat[u] < 0 || h->rev_xlat[u] < 0 || (uint64_t)h->fwd_xlat[u] >= E || (uint64_t)h->rev_xlat[u] >= E ||
                (h->bvcomp_order && (h->bvcomp_order[u] < 0 || (uint64_t)h->bvcomp_order[u] >= U)))
                return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: inconsistent translation tables");
        for (uint64_t e = 0; e < E; ++e)
            if (h->src_unitig[e] < 0 || (uint64_t)h->src_unitig[e] >= U) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: edge %llu is out of range", (unsigned long long)e);
    }
    if (n && (!paths->start || !paths->n_edges || !paths->offset)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: paths without their device arrays");
    if (n_entries && !paths->edges) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: paths without their device arrays");
    if (!n && n_entries) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: start / n_edges do not add up to n_edges_total = %llu", (unsigned long long)n_entries);
    if (n_entries && h_old->n_edges <= 0) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_patch_paths: a path holds an edge id outside the old graph's 0 edges");
    if (n >= (1ull << 32) - 1) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_dev_patch_paths: too many reads");
    paths_host PH;
    return snk_call_run(ctx, stream, "snk_dev_patch_paths", out, err, errcap, [&](snk_call& c) -> int {
        return K == 48 ? paths_impl<48>(c, PH, n_old_unitigs, (const uint64_t*)d_old_unitig_off, (const uint8_t*)d_old_unitig_bases, h_old, n_new_unitigs,
                                        (const uint64_t*)d_new_unitig_off, (const uint8_t*)d_new_unitig_bases, h_new, paths, out, err, errcap)
                       : paths_impl<60>(c, PH, n_old_unitigs, (const uint64_t*)d_old_unitig_off, (const uint8_t*)d_old_unitig_bases, h_old, n_new_unitigs,
                                        (const uint64_t*)d_new_unitig_off, (const uint8_t*)d_new_unitig_bases, h_new, paths, out, err, errcap);
    });
}
