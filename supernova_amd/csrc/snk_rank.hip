// snk_rank.hip -- list ranking over the directed states of a degree<=2 link graph: the k-mer states of the global graph stage
// (snk_graph.hip: graph_impl), the fragment ends of the join on one GPU (snk_dist_join, snk_join_rank), and the fragment ends of the
// sharded step, partitioned over the ranks (snk_prank_*).
//
//   rank_lists_wyllie   plain pointer jumping over all states; cuts circles at their minimum node (the reference's cut at k-mer level)
//   the ruling set      splitters, walk records, first walk, jumping on the splitter list, second walk: ONE set-up (rank_setup), one walk
//                       step (walk_to_splitter / walk_step) and one jumping driver (jump_rounds) for the one-GPU and the partitioned form
//   cut_circles_sparse  circles cut from what the ruling set left, without the general algorithm
//   snk_rank_lists      the one-GPU ranking: ruling set, cut and retry, Wyllie where that does not do
//   snk_prank_*         the same ruling set with the two walks done for a 1/world share of the splitters per rank
#include <string.h>
#include <rocprim/rocprim.hpp>

#include <vector>

#include "snk_ctx.h"
#include "snk_call.h"
#include "snk_common.h"
#include "snk_graph.h"
#include "snk_rank.h"

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int TB = 256;

// ------------------------------------------------------------------ pointer jumping
__global__ void __launch_bounds__(TB) rank_init_kernel(const uint32_t* __restrict__ link, uint64_t ns,
                                                       uint32_t* __restrict__ nxt, uint32_t* __restrict__ dist,
                                                       uint32_t* __restrict__ tail) {
    uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (s >= ns) return;
    uint32_t l = link[s];
    if (l == NONE) { nxt[s] = NONE; dist[s] = 0; tail[s] = (uint32_t)s; }
    else { nxt[s] = l ^ 1u; dist[s] = 1; tail[s] = l ^ 1u; }
}
// weighted start of the ranking (fragment join): the distance counts k-mers, not hops
__global__ void __launch_bounds__(TB) rank_init_w_kernel(const uint32_t* __restrict__ link, const uint32_t* __restrict__ w,
                                                         uint64_t ns, uint32_t* __restrict__ nxt, uint32_t* __restrict__ dist,
                                                         uint32_t* __restrict__ tail) {
    uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (s >= ns) return;
    uint32_t l = link[s];
    if (l == NONE) { nxt[s] = NONE; dist[s] = 0; tail[s] = (uint32_t)s; }
    else { nxt[s] = l ^ 1u; dist[s] = w[l >> 1]; tail[s] = l ^ 1u; }
}
__global__ void __launch_bounds__(TB) rank_round_kernel(const uint32_t* __restrict__ nxt_in, const uint32_t* __restrict__ dist_in,
                                                        const uint32_t* __restrict__ tail_in, uint64_t ns,
                                                        uint32_t* __restrict__ nxt_out, uint32_t* __restrict__ dist_out,
                                                        uint32_t* __restrict__ tail_out, uint32_t* __restrict__ changed) {
    uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (s >= ns) return;
    uint32_t n1 = nxt_in[s];
    if (n1 == NONE) { nxt_out[s] = NONE; dist_out[s] = dist_in[s]; tail_out[s] = tail_in[s]; return; }
    nxt_out[s] = nxt_in[n1];
    dist_out[s] = dist_in[s] + dist_in[n1];
    tail_out[s] = tail_in[n1];
    *changed = 1u;
}
__global__ void __launch_bounds__(TB) rank_zip_kernel(const uint32_t* __restrict__ dist, const uint32_t* __restrict__ tail, uint64_t ns,
                                                      uint2* __restrict__ rk) {
    uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (s < ns) rk[s] = make_uint2(dist[s], tail[s]);
}
__global__ void __launch_bounds__(TB) unranked_check_kernel(const uint2* __restrict__ rk, uint64_t ns, uint32_t* __restrict__ flag) {
    uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (s < ns && rk[s].y == NONE) *flag = 1u;
}

// The jumping driver: (next, distance, tail) of `count` list elements in ping-pong buffers; [cur] holds them after `done` rounds.  The
// caller fills [0], clears its flag and says up to which round to enqueue; how many rounds go between two read-backs is its business.
struct jump_bufs {
    uint32_t *nxt[2], *dst[2], *tl[2];
    uint32_t* sink;                    // "changed" of the rounds that do not report
    uint64_t count;
    int max_rounds, cur, done;         // max_rounds: a list that still has successors after that many doublings is a cycle
};
int jump_alloc(snk_ctx* ctx, jump_bufs* J, uint64_t count, uint64_t slack, char* err, size_t errcap) {
    J->count = count;
    J->cur = J->done = 0;
    for (int b = 0; b < 2; ++b) { G_ALLOC(J->nxt[b], uint32_t, count + slack); G_ALLOC(J->dst[b], uint32_t, count + slack); G_ALLOC(J->tl[b], uint32_t, count + slack); }
    G_ALLOC(J->sink, uint32_t, 4);
    J->max_rounds = 2;
    while ((1ull << (J->max_rounds - 1)) < count + slack) ++J->max_rounds;
    return SNK_OK;
}
// rounds [done, upto): only the last one reports into *flag
int jump_rounds(hipStream_t st, jump_bufs* J, int upto, uint32_t* flag, char* err, size_t errcap) {
    for (; J->done < upto; ++J->done) {
        const int c = J->cur;
        SNK_HIP_TRY(snk_launch(rank_round_kernel, snk_blocks(J->count, TB), TB, 0, st, J->nxt[c], J->dst[c], J->tl[c], J->count, J->nxt[c ^ 1], J->dst[c ^ 1],
                               J->tl[c ^ 1], J->done + 1 == upto ? flag : J->sink));
        J->cur ^= 1;
    }
    return SNK_OK;
}

// smooth circles: states that still have a successor after ceil(log2(ns))+1 rounds
__global__ void __launch_bounds__(TB) cyc_init_kernel(const uint32_t* __restrict__ nxt_final, const uint32_t* __restrict__ link,
                                                      uint64_t ns, uint32_t* __restrict__ jump, uint32_t* __restrict__ mn) {
    uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (s >= ns) return;
    if (nxt_final[s] == NONE) { jump[s] = NONE; mn[s] = NONE; }
    else { jump[s] = link[s] ^ 1u; mn[s] = (uint32_t)(s >> 1); }
}
__global__ void __launch_bounds__(TB) cyc_round_kernel(const uint32_t* __restrict__ jump_in, const uint32_t* __restrict__ mn_in,
                                                       uint64_t ns, uint32_t* __restrict__ jump_out, uint32_t* __restrict__ mn_out) {
    uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (s >= ns) return;
    uint32_t j = jump_in[s];
    if (j == NONE) { jump_out[s] = NONE; mn_out[s] = NONE; return; }
    uint32_t a = mn_in[s], b = mn_in[j];
    mn_out[s] = a < b ? a : b;
    jump_out[s] = jump_in[j];
}
// cut the link out of s: both ends become terminals (circ, nullable, marks them as made by a cut)
__device__ __forceinline__ void cut_at(uint32_t* link, uint32_t s, uint8_t* circ, uint32_t* n_cut) {
    const uint32_t partner = link[s];
    link[s] = NONE;
    if (partner != NONE) link[partner] = NONE;
    if (circ) { circ[s] = 1; if (partner != NONE) circ[partner] = 1; }
    atomicAdd(n_cut, 1u);
}
// cut every circle at the left side of its minimum k-mer
__global__ void __launch_bounds__(TB) cyc_cut_kernel(const uint32_t* __restrict__ mn, uint64_t n, uint32_t* __restrict__ link,
                                                     uint32_t* __restrict__ n_cut, uint8_t* __restrict__ circ_state) {
    uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    if (mn[2 * i + 1] == (uint32_t)i) cut_at(link, (uint32_t)(2 * i + 1), circ_state, n_cut);
}

// Plain pointer jumping (Wyllie) over all states, one round per read-back.  Smooth circles are cut at the left side of their minimum
// node and ranked again.
int rank_lists_wyllie(snk_ctx* ctx, hipStream_t st, uint32_t* link, uint64_t n, const uint32_t* weights, uint8_t* circ /* per state, nullable */,
                      const uint2** rk_out, uint32_t* n_circles, uint32_t* rounds, char* err, size_t errcap) {
    const uint64_t ns = 2 * n;
    jump_bufs J;
    int rc = jump_alloc(ctx, &J, ns, 0, err, errcap);
    if (rc) return rc;
    uint32_t* flags;   // [0] changed, [1] circles cut
    G_ALLOC(flags, uint32_t, 4);
    SNK_HIP_TRY(hipMemsetAsync(flags, 0, 16, st));      // (flags[1] is read back as n_circles also when nothing was cut)
    uint32_t* h_flags = nullptr;
    SNK_HIP_TRY(hipHostMalloc((void**)&h_flags, 16, hipHostMallocDefault));
    uint32_t rounds_total = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        J.cur = J.done = 0;
        if (weights) SNK_HIP_TRY(snk_launch(rank_init_w_kernel, snk_blocks(ns, TB), TB, 0, st, link, weights, ns, J.nxt[0], J.dst[0], J.tl[0]));
        else SNK_HIP_TRY(snk_launch(rank_init_kernel, snk_blocks(ns, TB), TB, 0, st, link, ns, J.nxt[0], J.dst[0], J.tl[0]));
        bool converged = false;
        while (J.done < J.max_rounds && !converged) {
            SNK_HIP_TRY(hipMemsetAsync(flags, 0, 4, st));
            if ((rc = jump_rounds(st, &J, J.done + 1, flags, err, errcap))) { (void)hipHostFree(h_flags); return rc; }
            ++rounds_total;
            SNK_HIP_TRY(hipMemcpyAsync(h_flags, flags, 4, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(snk_sync(st));
            converged = h_flags[0] == 0;
        }
        if (converged) break;
        if (attempt == 1) { (void)hipHostFree(h_flags); return snk_fail(SNK_E_INTERNAL, err, errcap, "unitig ranking did not converge after the circle cut"); }
        // smooth circles: find each circle's minimum k-mer (index order == key order), cut there, rank again
        uint32_t *jump[2] = {J.dst[J.cur ^ 1], J.tl[J.cur ^ 1]};   // reuse the spare ranking buffers
        uint32_t* mn[2];
        G_ALLOC(mn[0], uint32_t, ns);
        G_ALLOC(mn[1], uint32_t, ns);
        SNK_HIP_TRY(snk_launch(cyc_init_kernel, snk_blocks(ns, TB), TB, 0, st, J.nxt[J.cur], link, ns, jump[0], mn[0]));
        int c2 = 0;
        for (int r = 0; r < J.max_rounds; ++r) {
            SNK_HIP_TRY(snk_launch(cyc_round_kernel, snk_blocks(ns, TB), TB, 0, st, jump[c2], mn[c2], ns, jump[c2 ^ 1], mn[c2 ^ 1]));
            c2 ^= 1;
        }
        SNK_HIP_TRY(hipMemsetAsync(flags + 1, 0, 4, st));
        SNK_HIP_TRY(snk_launch(cyc_cut_kernel, snk_blocks(n, TB), TB, 0, st, mn[c2], n, link, flags + 1, circ));
    }
    SNK_HIP_TRY(hipMemcpyAsync(h_flags, flags, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    *n_circles = h_flags[1];
    *rounds = rounds_total;
    (void)hipHostFree(h_flags);
    uint2* rkz;
    G_ALLOC(rkz, uint2, ns);
    SNK_HIP_TRY(snk_launch(rank_zip_kernel, snk_blocks(ns, TB), TB, 0, st, J.dst[J.cur], J.tl[J.cur], ns, rkz));
    *rk_out = rkz;
    return SNK_OK;
}

// ------------------------------------------------------------------ work-efficient ranking: sparse ruling set
// Wyllie's pointer jumping touches every state log2(len) times (21-28 rounds of random 12-byte gathers on the benchmark, 60% of the
// whole step); here every state is touched twice: list heads and a hashed 1/32 sample of the states are "splitters", each walks to
// the next splitter, the short splitter list is ranked by pointer jumping, and a second walk hands the ranks to the states in between.
__device__ __forceinline__ bool sampled_state(uint32_t s, uint32_t split_mask) { return ((snk_mix32(s >> 1) >> 7) & split_mask) == 0; }
// a splitter: nobody walks into s (it starts a list), or it was sampled
__device__ __forceinline__ bool is_splitter(const uint32_t* link, uint64_t s, uint32_t split_mask) {
    return link[s ^ 1ull] == NONE || sampled_state((uint32_t)s, split_mask);
}

// One 8-byte record per state for the walks: link (32) | splitter id (31) | is-splitter (1) -- a walk step is then ONE random HBM
// transaction instead of two (link[] and a mark): the walks are transaction bound (PMC: ~128 B fetched per step with separate arrays).
__device__ __forceinline__ unsigned long long wrec_plain(uint32_t link) { return link; }
__device__ __forceinline__ unsigned long long wrec_of_splitter(uint32_t link, uint32_t id) { return link | ((unsigned long long)id << 32) | (1ull << 63); }
__device__ __forceinline__ uint32_t wrec_link(unsigned long long rec) { return (uint32_t)rec; }
__device__ __forceinline__ bool wrec_is_splitter(unsigned long long rec) { return rec >> 63; }
__device__ __forceinline__ uint32_t wrec_splitter_id(unsigned long long rec) { return (uint32_t)(rec >> 32) & 0x7FFFFFFFu; }

// The walk of a splitter's own stretch, as the first walk takes it: from the splitter's state to the next splitter or the list's end
// -> (next splitter id or NONE, summed weight of the states stepped onto, last state -- the terminal when there is no next splitter --,
// states of the stretch where COUNT asks for them).  w == nullptr: every state weighs 1.
template <bool COUNT>
__device__ __forceinline__ uint4 walk_to_splitter(const unsigned long long* __restrict__ wrec, const uint32_t* __restrict__ w, uint32_t cur) {
    unsigned long long rec = wrec[cur];
    uint32_t d = 0, nx = NONE, steps = 1;
    for (;;) {
        const uint32_t l = wrec_link(rec);
        if (l == NONE) { nx = NONE; break; }
        cur = l ^ 1u;
        rec = wrec[cur];
        d += w ? w[cur >> 1] : 1u;
        if (wrec_is_splitter(rec)) { nx = wrec_splitter_id(rec); break; }
        if (COUNT) ++steps;
    }
    return make_uint4(nx, d, cur, steps);
}
// One step of a second walk, which visits the states of a stretch: false at the list's end or on the next splitter.
__device__ __forceinline__ bool walk_step(const unsigned long long* __restrict__ wrec, uint32_t& cur, unsigned long long& rec) {
    const uint32_t l = wrec_link(rec);
    if (l == NONE) return false;
    cur = l ^ 1u;
    rec = wrec[cur];
    return !wrec_is_splitter(rec);
}

// The splitter predicate is cheap to recompute from link[] and the hash, so no per-state mark array is kept: the scan reads the
// predicate through an iterator, and one pass writes the compacted splitter list and the walk records.
struct spl_flag_fn {
    const uint32_t* link;
    uint64_t ns;
    uint32_t split_mask;
    __device__ uint32_t operator()(uint64_t s) const {
        if (s >= ns) return 0u;                       // the scan's closing element: sid[ns] = number of splitters
        return is_splitter(link, s, split_mask) ? 1u : 0u;
    }
};
__global__ void __launch_bounds__(TB) spl_setup_kernel(const uint32_t* __restrict__ link, const uint32_t* __restrict__ sid, uint64_t ns, uint32_t split_mask,
                                                       uint32_t* __restrict__ spl_state, unsigned long long* __restrict__ wrec) {
    uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (s >= ns) return;
    const uint32_t l = link[s];
    unsigned long long r = wrec_plain(l);
    if (is_splitter(link, s, split_mask)) {
        const uint32_t id = sid[s];
        r = wrec_of_splitter(l, id);
        spl_state[id] = (uint32_t)s;
    }
    wrec[s] = r;
}
// The set-up of both forms: splitter ids by a scan over the predicate, one read-back of their number, then list and records.
int rank_setup(snk_ctx* ctx, hipStream_t st, const uint32_t* link, uint64_t ns, snk_rank_setup* S, char* err, size_t errcap) {
    S->ns = ns;
    S->split_mask = (1u << snk_opt_u32(ctx, SNK_OPT_split_log2)) - 1u;
    uint32_t* sid;
    G_ALLOC(sid, uint32_t, ns + 1);
    auto flag_it = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), spl_flag_fn{link, ns, S->split_mask});
    int rc = excl_scan<uint32_t>(ctx, st, flag_it, sid, (size_t)(ns + 1), err, errcap);
    if (rc) return rc;
    uint32_t m32 = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&m32, sid + ns, 4, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    S->m = m32;
    G_ALLOC(S->spl_state, uint32_t, S->m + 1);
    G_ALLOC(S->wrec, unsigned long long, ns + 1);
    SNK_HIP_TRY(snk_launch(spl_setup_kernel, snk_blocks(ns, TB), TB, 0, st, link, sid, ns, S->split_mask, S->spl_state, S->wrec));
    return SNK_OK;
}

__global__ void __launch_bounds__(TB) spl_walk1_kernel(const unsigned long long* __restrict__ wrec, const uint32_t* __restrict__ spl_state,
                                                       const uint32_t* __restrict__ w, uint64_t m, uint32_t* __restrict__ rnxt,
                                                       uint32_t* __restrict__ rdist, uint32_t* __restrict__ rtail) {
    uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= m) return;
    const uint4 v = walk_to_splitter<false>(wrec, w, spl_state[k]);
    rnxt[k] = v.x;
    rdist[k] = v.y;
    rtail[k] = v.z;        // the terminal state when there is no next splitter (overwritten by the jumping otherwise)
}
// The links are an involution: a list e_0 -> ... -> e_n also exists as its mirror e_n^1 -> ... -> e_0^1, and with
// rk[e_i] = (d_i, e_n), d_i = sum of w_j over j > i, the mirror's rank is rk[e_i ^ 1] = (W - d_i - w_i, e_0 ^ 1) with
// W = d_0 + w_0.  So only one list of each pair is walked a second time, and each visited state writes both ranks.
// After the jumping has converged every head splitter knows its terminal t; t ^ 1 is the mirror's head, a splitter, and its
// splitter id keys the pair (e_0, W): every entry that is read was written, so the table needs no clear.  (Before
// convergence the entries read may be stale: that walk's result is thrown away.)
__global__ void __launch_bounds__(TB) spl_head_info_kernel(const unsigned long long* __restrict__ wrec, const uint32_t* __restrict__ spl_state,
                                                           const uint32_t* __restrict__ w, const uint32_t* __restrict__ rdist,
                                                           const uint32_t* __restrict__ rtail, uint64_t m, uint2* __restrict__ info) {
    const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= m) return;
    const uint32_t h = spl_state[k];
    if (wrec_link(wrec[h ^ 1u]) != NONE) return;       // not a head
    const uint32_t t = rtail[k];
    const uint32_t id = wrec_splitter_id(wrec[t ^ 1u]);
    info[id] = make_uint2(h, rdist[k] + (w ? w[h >> 1] : 1u));
}
// The list whose terminal is the smaller of (t, e_0 ^ 1) is the one walked.  t == e_0 ^ 1: the list is its own mirror (it
// holds both states of every fragment on it), is walked as before and writes one rank per state.  *ranked counts the ranks
// written: a state no walk reaches (a circle without a splitter) shows as *ranked != ns.
__global__ void __launch_bounds__(TB) spl_walk2m_kernel(const unsigned long long* __restrict__ wrec, const uint32_t* __restrict__ spl_state,
                                                        const uint32_t* __restrict__ w, const uint32_t* __restrict__ rdist,
                                                        const uint32_t* __restrict__ rtail, const uint2* __restrict__ info, uint64_t m,
                                                        uint2* __restrict__ rk, uint32_t* __restrict__ ranked) {
    const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
    uint32_t cnt = 0;
    if (k < m) {
        uint32_t cur = spl_state[k];
        unsigned long long rec = wrec[cur];
        uint32_t d = rdist[k];
        const uint32_t t = rtail[k];
        const uint2 hw = info[wrec_splitter_id(wrec[t ^ 1u])];
        const uint32_t mt = hw.x ^ 1u;                // the mirror's terminal
        if (t <= mt) {
            const bool self = t == mt;
            uint32_t wc = w ? w[cur >> 1] : 1u;
            for (;;) {
                if (self) {
                    rk[cur] = make_uint2(d, t);
                    cnt += 1;
                } else {
                    const uint32_t dm = hw.y - d - wc;
                    // the two states of a fragment are neighbours in rk[]: one 16-byte store
                    ((uint4*)rk)[cur >> 1] = (cur & 1u) ? make_uint4(dm, mt, d, t) : make_uint4(d, t, dm, mt);
                    cnt += 2;
                }
                if (!walk_step(wrec, cur, rec)) break;
                wc = w ? w[cur >> 1] : 1u;
                d -= wc;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(ranked, cnt);
}

// ---- circles, cut without the general algorithm.  The ruling-set ranking sees a circle in one of two ways: its splitters form a
// cycle in the splitter list (the jumping does not converge), or it holds no splitter at all and no walk reaches it.  Round 2
// answered both with Wyllie's pointer jumping over ALL states (ceil(log2 ns) rounds of random gathers: ~50 ms at 35 M states,
// a second at 280 M -- for ONE plasmid in the data set).  Here: the minimum sampled FRAGMENT of every splitter cycle by
// pointer jumping on the splitter list only (1/32 of the states; both states of a fragment are sampled together, so the two
// directed cycles of a circle agree on it), and the minimum fragment of a splitter-free circle (a few hundred states at most)
// by walking it from every unreached odd state; the circle is cut at the odd state of that fragment -- one cut per circle --
// and the caller ranks again.  Where a circle is cut does not matter in the join: jcircle_kernel rotates it to the
// reference's cut (canonicalizeCircle, BuildReadQGraph48.cc:375-397).
__global__ void __launch_bounds__(TB) spl_reach_kernel(const unsigned long long* __restrict__ wrec, const uint32_t* __restrict__ spl_state, uint64_t m,
                                                       uint8_t* __restrict__ reach) {
    const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= m) return;
    uint32_t cur = spl_state[k];
    unsigned long long rec = wrec[cur];
    do reach[cur] = 1;
    while (walk_step(wrec, cur, rec));
}
__global__ void __launch_bounds__(TB) scyc_init_kernel(const uint32_t* __restrict__ rn_final, const uint32_t* __restrict__ rn_orig,
                                                       const uint32_t* __restrict__ spl_state, uint64_t m, uint32_t* __restrict__ jump, uint32_t* __restrict__ mn) {
    const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= m) return;
    const bool on = rn_final[k] != NONE;          // still has a successor after ceil(log2 m) + 1 doublings: on a cycle
    jump[k] = on ? rn_orig[k] : NONE;
    mn[k] = on ? spl_state[k] >> 1 : NONE;
}
__global__ void __launch_bounds__(TB) scyc_cut_kernel(const uint32_t* __restrict__ mn, const uint32_t* __restrict__ spl_state, uint64_t m,
                                                      uint32_t* __restrict__ link, uint32_t* __restrict__ n_cut, uint8_t* __restrict__ circ) {
    const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= m) return;
    const uint32_t s = spl_state[k];
    if (mn[k] != NONE && (s & 1u) && mn[k] == (s >> 1)) cut_at(link, s, circ, n_cut);
}
__global__ void __launch_bounds__(TB) free_circle_find_kernel(const uint8_t* __restrict__ reach, uint64_t ns, const uint32_t* __restrict__ link,
                                                              uint32_t* __restrict__ list, uint32_t cap, uint32_t* __restrict__ n_list, uint32_t* __restrict__ bad) {
    const uint64_t s0 = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (s0 >= ns || !(s0 & 1ull) || reach[s0]) return;
    // an unreached state lies on a circle without a splitter; every odd state of that circle walks it, the one of the minimum
    // fragment is where it will be cut.  Nothing is cut here: a cut also breaks the circle's OTHER direction, which other threads
    // are walking at this moment -- the states are listed and cut by the next kernel.
    const uint32_t s = (uint32_t)s0;
    uint32_t cur = s, mn = s >> 1;
    for (uint32_t steps = 0;; ++steps) {
        const uint32_t l = link[cur];
        if (l == NONE || steps > (1u << 22)) { atomicOr(bad, 1u); return; }      // not a circle / absurdly long: leave it to the general algorithm
        cur = l ^ 1u;
        if (cur == s) break;
        const uint32_t f = cur >> 1;
        mn = f < mn ? f : mn;
    }
    if (mn == (s >> 1)) { const uint32_t at = atomicAdd(n_list, 1u); if (at < cap) list[at] = s; else atomicOr(bad, 1u); }
}
__global__ void __launch_bounds__(TB) cut_list_kernel(const uint32_t* __restrict__ list, const uint32_t* __restrict__ n_list, uint32_t cap, uint32_t* __restrict__ link,
                                                      uint32_t* __restrict__ n_cut, uint8_t* __restrict__ circ) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    const uint32_t n = *n_list < cap ? *n_list : cap;
    if (i < n) cut_at(link, list[i], circ, n_cut);
}

// J: next splitter of every splitter after the jumping in [cur] (NONE unless on a cycle) and, put there again by the caller, as the
// first walk left it in the spare [cur ^ 1] (the jumping overwrites it, and only this rare path needs it: no copy is kept on every call).
// *n_cut = circles cut, *bad = 1: something the fast path does not understand (the caller uses the general algorithm).
int cut_circles_sparse(snk_ctx* ctx, hipStream_t st, uint32_t* link, const snk_rank_setup& S, const jump_bufs& J, bool jump_converged, uint8_t* circ,
                       uint32_t* n_cut, uint32_t* bad, char* err, size_t errcap) {
    const uint64_t ns = S.ns, m = S.m;
    uint32_t* d_flags;
    G_ALLOC(d_flags, uint32_t, 4);
    SNK_HIP_TRY(hipMemsetAsync(d_flags, 0, 16, st));
    // (the reach marks come from the links as they are BEFORE any cut)
    uint8_t* reach;
    G_ALLOC(reach, uint8_t, ns + 1);
    SNK_HIP_TRY(hipMemsetAsync(reach, 0, ns + 1, st));
    SNK_HIP_TRY(snk_launch(spl_reach_kernel, snk_blocks(m, TB), TB, 0, st, S.wrec, S.spl_state, m, reach));
    if (!jump_converged && m) {
        uint32_t *jump[2], *mn[2];
        for (int b = 0; b < 2; ++b) { G_ALLOC(jump[b], uint32_t, m + 1); G_ALLOC(mn[b], uint32_t, m + 1); }
        SNK_HIP_TRY(snk_launch(scyc_init_kernel, snk_blocks(m, TB), TB, 0, st, J.nxt[J.cur], J.nxt[J.cur ^ 1], S.spl_state, m, jump[0], mn[0]));
        int c2 = 0;
        for (int r = 0; r < J.max_rounds; ++r) {
            SNK_HIP_TRY(snk_launch(cyc_round_kernel, snk_blocks(m, TB), TB, 0, st, jump[c2], mn[c2], m, jump[c2 ^ 1], mn[c2 ^ 1]));
            c2 ^= 1;
        }
        SNK_HIP_TRY(snk_launch(scyc_cut_kernel, snk_blocks(m, TB), TB, 0, st, mn[c2], S.spl_state, m, link, d_flags, circ));
    }
    {
        const uint32_t cap = 1u << 18;
        uint32_t* list;
        G_ALLOC(list, uint32_t, cap);
        SNK_HIP_TRY(snk_launch(free_circle_find_kernel, snk_blocks(ns, TB), TB, 0, st, reach, ns, link, list, cap, d_flags + 2, d_flags + 1));
        SNK_HIP_TRY(snk_launch(cut_list_kernel, cap / TB, TB, 0, st, list, d_flags + 2, cap, link, d_flags, circ));
    }
    uint32_t h[2] = {0, 0};
    SNK_HIP_TRY(hipMemcpyAsync(h, d_flags, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    *n_cut = h[0];
    *bad = h[1];
    return SNK_OK;
}

// One attempt of the one-GPU ruling-set ranking.  *ranked: every state has its rank in *rk_out (and *rounds says what it took);
// else circles were seen -- T keeps what cutting them needs.
struct ruling_attempt {
    snk_rank_setup S;
    jump_bufs J;
    bool jump_converged;
};
int rank_ruling_set(snk_ctx* ctx, hipStream_t st, const uint32_t* link, uint64_t ns, const uint32_t* weights, ruling_attempt* T, const uint2** rk_out,
                    uint32_t* rounds, bool* ranked, char* err, size_t errcap) {
    snk_rank_setup& S = T->S;
    jump_bufs& J = T->J;
    int rc = rank_setup(ctx, st, link, ns, &S, err, errcap);
    if (rc) return rc;
    const uint64_t m = S.m;
    if ((rc = jump_alloc(ctx, &J, m, 1, err, errcap))) return rc;
    SNK_HIP_TRY(snk_launch(spl_walk1_kernel, snk_blocks(m, TB), TB, 0, st, S.wrec, S.spl_state, weights, m, J.nxt[0], J.dst[0], J.tl[0]));
    uint2* info;                       // (head state, list weight) of every list, keyed by the splitter id of its mirror's head
    G_ALLOC(info, uint2, m + 1);
    uint32_t* flags;                   // [0] the batch's last round changed something, [1] ranks the second walk wrote
    G_ALLOC(flags, uint32_t, 4);
    uint2* rk;
    G_ALLOC(rk, uint2, ns);
    // Rounds are issued in batches without asking the device whether the last one still changed anything (a round over the
    // ~n/32 splitters takes 10-15 us, a read-back 25-30 us of idle device): the first batch covers lists of 2^12 splitters
    // (128 k fragments), and its verdict comes back together with the walk's "every state ranked" check.
    const int batch0 = (int)snk_opt_u32(ctx, SNK_OPT_rank_round_batch0);
    bool converged = false, unranked = false;
    while (J.done < J.max_rounds && !converged) {
        const int upto = J.done == 0 && batch0 < J.max_rounds ? batch0 : J.max_rounds;
        SNK_HIP_TRY(hipMemsetAsync(flags, 0, 8, st));
        if ((rc = jump_rounds(st, &J, upto, flags, err, errcap))) return rc;
        // optimistic: rank the states from what the rounds left (harmless if they had not converged: it is redone)
        // (flags[1] was cleared with flags[0] above: a redone walk counts from zero)
        SNK_HIP_TRY(snk_launch(spl_head_info_kernel, snk_blocks(m, TB), TB, 0, st, S.wrec, S.spl_state, weights, J.dst[J.cur], J.tl[J.cur], m, info));
        SNK_HIP_TRY(snk_launch(spl_walk2m_kernel, snk_blocks(m, TB), TB, 0, st, S.wrec, S.spl_state, weights, J.dst[J.cur], J.tl[J.cur], info, m, rk, flags + 1));
        uint32_t h2[2] = {0, 0};
        SNK_HIP_TRY(hipMemcpyAsync(h2, flags, 8, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        converged = h2[0] == 0;
        unranked = h2[1] != ns;         // states no walk reached: a circle without a splitter
    }
    T->jump_converged = converged;
    *ranked = converged && !unranked;
    *rk_out = rk;
    *rounds = (uint32_t)J.done;
    return SNK_OK;
}

// ---- partitioned ranking (sharded runs, owner-side join).  Every rank holds the job's whole link structure (all-gathered),
// but ranking it in full on every rank would cost each of them what the rank-0 funnel cost one.  The ruling-set scheme
// splits naturally: the set-up is a streaming pass (replicated); the two walks -- the random access part -- are done for a
// 1/world share of the splitters per rank; what leaves a rank is 16 B per splitter after walk 1 (all-gather) and 16 B per
// visited state after walk 2 (to the state's owner).  The splitter list itself (1/32 of the states) is jumped on every rank.
// Circles are cut on every rank alike (the data is replicated) and the ranking begins again; what the fast cut refuses goes
// to the replicated ranking (snk_join_rank).
__global__ void __launch_bounds__(TB) spl_walk1p_kernel(const unsigned long long* __restrict__ wrec, const uint32_t* __restrict__ spl_state,
                                                        const uint32_t* __restrict__ w, uint64_t k0, uint64_t cnt, uint4* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i < cnt) out[i] = walk_to_splitter<true>(wrec, w, spl_state[k0 + i]);
}
__global__ void __launch_bounds__(TB) prank_unzip_kernel(const uint4* __restrict__ all, uint64_t m, uint32_t* __restrict__ rn, uint32_t* __restrict__ rd,
                                                         uint32_t* __restrict__ rt, unsigned long long* __restrict__ total_steps) {
    const uint64_t k = (uint64_t)blockIdx.x * TB + threadIdx.x;
    unsigned long long st = 0;
    if (k < m) { const uint4 v = all[k]; rn[k] = v.x; rd[k] = v.y; rt[k] = v.z; st = v.w; }
    for (int o = 32; o > 0; o >>= 1) st += __shfl_xor(st, o);
    if ((threadIdx.x & 63) == 0 && st) atomicAdd(total_steps, st);
}
__global__ void __launch_bounds__(TB) prank_steps_kernel(const uint4* __restrict__ all, uint64_t k0, uint64_t cnt, uint64_t* __restrict__ steps) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i <= cnt) steps[i] = i < cnt ? all[k0 + i].w : 0ull;
}
// second walk of this rank's share: one 16-byte record (state, distance, terminal, 0) per visited state, at positions known
// from the step counts of the first walk
__global__ void __launch_bounds__(TB) spl_walk2p_kernel(const unsigned long long* __restrict__ wrec, const uint32_t* __restrict__ spl_state,
                                                        const uint32_t* __restrict__ w, const uint32_t* __restrict__ rdist, const uint32_t* __restrict__ rtail,
                                                        uint64_t k0, uint64_t cnt, const uint64_t* __restrict__ pos, uint4* __restrict__ rec_out) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= cnt) return;
    uint32_t cur = spl_state[k0 + i];
    unsigned long long rec = wrec[cur];
    uint32_t d = rdist[k0 + i];
    const uint32_t t = rtail[k0 + i];
    uint64_t p = pos[i];
    for (;;) {
        rec_out[p++] = make_uint4(cur, d, t, 0u);
        if (!walk_step(wrec, cur, rec)) break;
        d -= w[cur >> 1];
    }
}
// records to the owners of their states: count / fill with the per-owner sums taken in LDS first, one reservation per owner and PR_TILES tiles
constexpr int PR_TILES = 16;
template <bool FILL>
__global__ void __launch_bounds__(256) prank_route_kernel(const uint4* __restrict__ rec, uint64_t n, const unsigned long long* __restrict__ frag_off, uint32_t world,
                                                          unsigned long long* __restrict__ cnt_or_cur, uint4* __restrict__ out) {
    extern __shared__ unsigned long long dynp[];          // [world] counts -> reserved bases, then [world] u32 local cursors
    uint32_t* lcur = reinterpret_cast<uint32_t*>(dynp + world);
    for (uint32_t r = threadIdx.x; r < world; r += 256) { dynp[r] = 0; lcur[r] = 0; }
    __syncthreads();
    const uint64_t i0 = (uint64_t)blockIdx.x * 256 * PR_TILES + threadIdx.x;
    auto owner_of = [&](unsigned long long g) { uint32_t o = 0; while (o + 1 < world && g >= frag_off[o + 1]) ++o; return o; };
    for (int t = 0; t < PR_TILES; ++t) {
        const uint64_t i = i0 + (uint64_t)t * 256;
        if (i < n) atomicAdd(&dynp[owner_of(rec[i].x >> 1)], 1ull);
    }
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < world; r += 256) { const unsigned long long c = dynp[r]; if (c) dynp[r] = atomicAdd(&cnt_or_cur[r], c); }
    if (!FILL) return;
    __syncthreads();
    for (int t = 0; t < PR_TILES; ++t) {
        const uint64_t i = i0 + (uint64_t)t * 256;
        if (i < n) {
            const uint4 v = rec[i];
            const uint32_t owner = owner_of(v.x >> 1);
            out[dynp[owner] + atomicAdd(&lcur[owner], 1u)] = v;
        }
    }
}
__global__ void __launch_bounds__(TB) prank_apply_kernel(const uint4* __restrict__ rec, uint64_t n, unsigned long long state_base, uint64_t n_local_states,
                                                         uint2* __restrict__ rk, uint32_t* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint4 v = rec[i];
    const unsigned long long s = (unsigned long long)v.x - state_base;
    if (s < n_local_states) rk[s] = make_uint2(v.y, v.z);
    else *bad = 1u;
}
}  // namespace

int snk_rank_lists(snk_ctx* ctx, hipStream_t st, uint32_t* link, uint64_t n, const uint32_t* weights, uint8_t* circ, const uint2** rk_out,
                   uint32_t* n_circles, uint32_t* rounds, char* err, size_t errcap, snk_rank_trace* trace) {
    snk_rank_trace unused;
    snk_rank_trace& tr = trace ? *trace : unused;
    tr = snk_rank_trace{};
    const uint64_t ns = 2 * n;
    if (ns < 4096 || snk_opt_u32(ctx, SNK_OPT_rank_wyllie)) {
        tr.source = SNK_RANK_WYLLIE;
        return rank_lists_wyllie(ctx, st, link, n, weights, circ, rk_out, n_circles, rounds, err, errcap);
    }
    uint32_t cut_total = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        ruling_attempt T;
        bool ranked = false;
        int rc = rank_ruling_set(ctx, st, link, ns, weights, &T, rk_out, rounds, &ranked, err, errcap);
        if (rc) return rc;
        tr.ruling_attempts = (uint32_t)attempt + 1;
        if (attempt == 0) tr.m_first = T.S.m;
        if (ranked) { *n_circles = cut_total; tr.source = SNK_RANK_RULING; return SNK_OK; }
        // circles.  In the join (circ given) they are cut here and the lists ranked once more; the k-mer level ranking of the global
        // graph stage needs the cut AT the minimum k-mer (it is the reference's cut there): the general algorithm does that.
        if (!circ || attempt == 1) break;
        // the cut wants every splitter's next splitter as the first walk left it: walk again (wrec[] is unchanged) into the spare buffers
        const jump_bufs& J = T.J;
        const int spare = J.cur ^ 1;
        SNK_HIP_TRY(snk_launch(spl_walk1_kernel, snk_blocks(T.S.m, TB), TB, 0, st, T.S.wrec, T.S.spl_state, weights, T.S.m, J.nxt[spare], J.dst[spare], J.tl[spare]));
        uint32_t n_cut = 0, bad = 0;
        if ((rc = cut_circles_sparse(ctx, st, link, T.S, J, T.jump_converged, circ, &n_cut, &bad, err, errcap))) return rc;
        // (the cuts are in link[] and circ[] whatever the verdict: a cut that gave up at its list's capacity has still made that many)
        cut_total += n_cut;
        tr.sparse_cut += n_cut;
        tr.bad |= bad;
        if (bad || n_cut == 0) break;
    }
    uint32_t nc2 = 0;
    int rcw = rank_lists_wyllie(ctx, st, link, n, weights, circ, rk_out, &nc2, rounds, err, errcap);
    *n_circles = cut_total + nc2;
    tr.source = SNK_RANK_RULING_THEN_WYLLIE;
    return rcw;
}

int snk_prank_begin(snk_ctx* ctx, hipStream_t st, uint64_t F, const uint32_t* nk, uint32_t* link, uint32_t rank, uint32_t world, snk_prank* P, char* err,
                    size_t errcap) {
    memset(P, 0, sizeof *P);
    P->w = nk; P->link = link;
    if (F >= (1ull << 31)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "more than 2^31 fragments at the join (%llu)", (unsigned long long)F);
    int rc = rank_setup(ctx, st, link, 2 * F, &P->set, err, errcap);
    if (rc) return rc;
    const uint64_t m = P->set.m;
    P->k0 = m * rank / world;
    P->k1 = m * (rank + 1) / world;
    const uint64_t cnt = P->k1 - P->k0;
    G_ALLOC(P->w1_share, uint4, cnt + 1);
    SNK_HIP_TRY(snk_launch(spl_walk1p_kernel, snk_blocks(cnt, TB), TB, 0, st, P->set.wrec, P->set.spl_state, nk, P->k0, cnt, P->w1_share));
    return SNK_OK;
}

// w1_all: the first walk's results of all ranks in splitter order.  *circles = 1: some list is a circle (the caller ranks the
// replicated way); else rec_out / n_rec = this rank's share of (state, distance, terminal) records.
int snk_prank_walk(snk_ctx* ctx, hipStream_t st, snk_prank* P, const uint4* w1_all, uint32_t* circles, uint32_t* rounds, char* err, size_t errcap,
                   uint8_t* circ, uint32_t* n_cut_out, snk_rank_trace* trace) {
    const snk_rank_setup& S = P->set;
    const uint64_t m = S.m;
    *circles = 0;
    *rounds = 0;
    P->n_rec = 0;
    jump_bufs J;
    int rc = jump_alloc(ctx, &J, m, 1, err, errcap);
    if (rc) return rc;
    unsigned long long* tot;           // [0] states the first walk reached, [1] the same again where the walk is unzipped a second time
    uint32_t* flags;
    G_ALLOC(tot, unsigned long long, 2);
    G_ALLOC(flags, uint32_t, 4);
    SNK_HIP_TRY(hipMemsetAsync(tot, 0, 16, st));
    SNK_HIP_TRY(snk_launch(prank_unzip_kernel, snk_blocks(m, TB), TB, 0, st, w1_all, m, J.nxt[0], J.dst[0], J.tl[0], tot));
    // pointer jumping over the splitter list in batches of rounds: one read-back per batch (flag of the batch's last round +,
    // the first time, the total the first walk reached), not per round; rounds past convergence change nothing
    unsigned long long h_tot = 0;
    uint32_t h_flag = 0;
    bool converged = false, first = true;
    const int batch = (int)snk_opt_u32(ctx, SNK_OPT_rank_round_batch);
    while (J.done < J.max_rounds && !converged) {
        if (m) {
            SNK_HIP_TRY(hipMemsetAsync(flags, 0, 4, st));
            if ((rc = jump_rounds(st, &J, J.done + batch < J.max_rounds ? J.done + batch : J.max_rounds, flags, err, errcap))) return rc;
            SNK_HIP_TRY(hipMemcpyAsync(&h_flag, flags, 4, hipMemcpyDeviceToHost, st));
        }
        if (first) SNK_HIP_TRY(hipMemcpyAsync(&h_tot, tot, 8, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        first = false;
        converged = m == 0 || h_flag == 0;
    }
    *rounds = (uint32_t)J.done;
    if (!converged || h_tot != S.ns) {
        // circles: splitters that form a cycle (the jumping did not converge) and / or states no walk reached (a circle without a
        // splitter).  Everything needed to cut them is replicated -- links, splitter list, the first walk of ALL ranks -- so every
        // rank makes the same cuts (cut_circles_sparse) and the caller starts the ranking again: *circles = 2.  1: fall back to the
        // replicated general algorithm (no circ array, or something the fast path does not understand).
        if (n_cut_out) *n_cut_out = 0;
        if (!circ) { *circles = 1; return SNK_OK; }
        // the cut wants every splitter's next splitter as the first walk left it: w1_all still holds it, unzipped into the spare buffers
        const int spare = J.cur ^ 1;
        SNK_HIP_TRY(snk_launch(prank_unzip_kernel, snk_blocks(m, TB), TB, 0, st, w1_all, m, J.nxt[spare], J.dst[spare], J.tl[spare], tot + 1));
        uint32_t n_cut = 0, bad = 0;
        if ((rc = cut_circles_sparse(ctx, st, P->link, S, J, converged, circ, &n_cut, &bad, err, errcap))) return rc;
        if (n_cut_out) *n_cut_out = n_cut;
        if (trace) { trace->sparse_cut += n_cut; trace->bad |= bad; }
        *circles = (bad || n_cut == 0) ? 1u : 2u;
        return SNK_OK;
    }
    const uint64_t cnt = P->k1 - P->k0;
    uint64_t *steps, *pos;
    G_ALLOC(steps, uint64_t, cnt + 1);
    G_ALLOC(pos, uint64_t, cnt + 1);
    SNK_HIP_TRY(snk_launch(prank_steps_kernel, snk_blocks(cnt + 1, TB), TB, 0, st, w1_all, P->k0, cnt, steps));
    if ((rc = excl_scan<uint64_t>(ctx, st, steps, pos, cnt + 1, err, errcap))) return rc;
    uint64_t n_rec = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&n_rec, pos + cnt, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    G_ALLOC(P->rec, uint4, n_rec + 1);
    SNK_HIP_TRY(snk_launch(spl_walk2p_kernel, snk_blocks(cnt, TB), TB, 0, st, S.wrec, S.spl_state, P->w, J.dst[J.cur], J.tl[J.cur], P->k0, cnt, pos, P->rec));
    P->n_rec = n_rec;
    return SNK_OK;
}

int snk_prank_route(snk_ctx* ctx, hipStream_t st, snk_prank* P, const unsigned long long* d_frag_off, uint32_t world,
                    unsigned long long* d_cursor, void* d_out, char* err, size_t errcap) {
    if (!P->n_rec) return SNK_OK;
    const uint64_t nb = snk_blocks(P->n_rec, 256 * PR_TILES);
    SNK_HIP_TRY(snk_launch(prank_route_kernel<true>, nb, 256, world * 12ull + 16, st, P->rec, P->n_rec, d_frag_off, world, d_cursor, (uint4*)d_out));
    return SNK_OK;
}

// the records that arrived -> rk of this rank's own states [state_base, state_base + n_local_states)
int snk_prank_apply(snk_ctx* ctx, hipStream_t st, const void* d_rec, uint64_t n, unsigned long long state_base, uint64_t n_local_states,
                    const uint2** rk_out, char* err, size_t errcap) {
    uint2* rk;
    uint32_t* flag;
    G_ALLOC(rk, uint2, n_local_states + 1);
    G_ALLOC(flag, uint32_t, 4);
    SNK_HIP_TRY(hipMemsetAsync(rk, 0xFF, (n_local_states + 1) * 8, st));
    SNK_HIP_TRY(hipMemsetAsync(flag, 0, 8, st));
    SNK_HIP_TRY(snk_launch(prank_apply_kernel, snk_blocks(n, TB), TB, 0, st, (const uint4*)d_rec, n, state_base, n_local_states, rk, flag));
    SNK_HIP_TRY(snk_launch(unranked_check_kernel, snk_blocks(n_local_states, TB), TB, 0, st, rk, n_local_states, flag + 1));
    uint32_t h[2] = {0, 0};
    SNK_HIP_TRY(hipMemcpyAsync(h, flag, 8, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    if (h[0] || h[1]) return snk_fail(SNK_E_INTERNAL, err, errcap, "partitioned ranking: %s", h[0] ? "a record for a foreign state arrived" : "a local state was not ranked");
    *rk_out = rk;
    return SNK_OK;
}

// ---- the ranking on its own (include/snk.h: snk_dev_rank_lists): an entry for the tests.  Host code only: the input is judged on the
// host, the one-GPU form is snk_rank_lists as the join calls it, and the partitioned form is the attempt loop of the sharded step
// (snk_shard_step.hip) with the collectives replaced by copies inside this context.
namespace {
// Every rank of the sharded step holds its own replica of links and marks and cuts it; rank 0 works on the caller's arrays here, the
// others on copies taken at the start of the attempt.
int prank_emulated(snk_call& c, uint64_t n, uint32_t* link, const uint32_t* w, uint8_t* circ, uint32_t world, const uint64_t* frag_off, uint2* rk_out,
                   snk_rank_evidence* ev, char* err, size_t errcap) {
    snk_ctx* ctx = c.ctx;
    const hipStream_t st = c.st;
    const uint64_t ns = 2 * n;
    int rc;
    std::vector<unsigned long long> h_off(frag_off, frag_off + world + 1);
    unsigned long long* d_frag_off;
    G_ALLOC(d_frag_off, unsigned long long, world + 1);
    SNK_HIP_TRY(hipMemcpyAsync(d_frag_off, h_off.data(), (world + 1) * 8ull, hipMemcpyHostToDevice, st));
    SNK_HIP_TRY(snk_sync(st));         // (h_off does not outlive an early return)
    std::vector<uint32_t*> r_link(world, link);
    std::vector<uint8_t*> r_circ(world, circ);
    for (uint32_t r = 1; r < world; ++r) { G_ALLOC(r_link[r], uint32_t, ns + 4); G_ALLOC(r_circ[r], uint8_t, ns + 16); }
    uint32_t join_circles = 0;
    snk_rank_trace tr;
    bool ranked = false;
    std::vector<snk_prank> P(world);
    for (int attempt = 0; !ranked && attempt < 3; ++attempt) {
        ev->part_attempts = (uint32_t)attempt + 1;
        for (uint32_t r = 1; r < world; ++r) {
            SNK_HIP_TRY(hipMemcpyAsync(r_link[r], link, ns * 4, hipMemcpyDeviceToDevice, st));
            SNK_HIP_TRY(hipMemcpyAsync(r_circ[r], circ, ns, hipMemcpyDeviceToDevice, st));
        }
        for (uint32_t r = 0; r < world; ++r)
            if ((rc = snk_prank_begin(ctx, st, n, w, r_link[r], r, world, &P[r], err, errcap))) return rc;
        const uint64_t m = P[0].set.m;
        if (attempt == 0) ev->splitters = m;
        uint4* w1_all;                 // (the step's all-gather of the shares, in rank order)
        G_ALLOC(w1_all, uint4, m + 2);
        for (uint32_t r = 0; r < world; ++r) {
            if (P[r].set.m != m || P[r].k0 != m * r / world || P[r].k1 != m * (r + 1) / world)
                return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_rank_lists: the ranks' splitter shares do not tile the splitter list");
            if (P[r].k1 > P[r].k0) SNK_HIP_TRY(hipMemcpyAsync(w1_all + P[r].k0, P[r].w1_share, (P[r].k1 - P[r].k0) * 16, hipMemcpyDeviceToDevice, st));
        }
        uint32_t verdict = 0, n_cut = 0;
        for (uint32_t r = 0; r < world; ++r) {
            uint32_t v = 0, nc = 0, rounds = 0;
            if ((rc = snk_prank_walk(ctx, st, &P[r], w1_all, &v, &rounds, err, errcap, r_circ[r], &nc, r == 0 ? &tr : nullptr))) return rc;
            if (r == 0) { verdict = v; n_cut = nc; ev->rounds = rounds; }
            else if (v != verdict || nc != n_cut)
                return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_rank_lists: rank %u says circles = %u (%u cut), rank 0 says %u (%u cut)", r, v, nc, verdict, n_cut);
        }
        join_circles += n_cut;
        if (verdict == 1) break;
        if (verdict == 2) continue;
        // the records of every rank's walks into per-owner regions, then every owner's regions into its slice of rk
        std::vector<uint4*> rsend(world);
        std::vector<std::vector<unsigned long long>> ends(world, std::vector<unsigned long long>(world));
        for (uint32_t r = 0; r < world; ++r) {
            const uint64_t rcap = P[r].n_rec + 1;
            for (uint32_t q = 0; q < world; ++q) ends[r][q] = (unsigned long long)q * rcap;
            if (!P[r].n_rec) continue;          // (no records: the fill is not launched)
            unsigned long long* d_cur;
            G_ALLOC(rsend[r], uint4, (uint64_t)world * rcap + 2);
            G_ALLOC(d_cur, unsigned long long, world + 1);
            SNK_HIP_TRY(hipMemcpyAsync(d_cur, ends[r].data(), world * 8ull, hipMemcpyHostToDevice, st));
            SNK_HIP_TRY(snk_sync(st));          // (ends[r] is written next)
            if ((rc = snk_prank_route(ctx, st, &P[r], d_frag_off, world, d_cur, rsend[r], err, errcap))) return rc;
            SNK_HIP_TRY(hipMemcpyAsync(ends[r].data(), d_cur, world * 8ull, hipMemcpyDeviceToHost, st));
            SNK_HIP_TRY(snk_sync(st));
        }
        for (uint32_t q = 0; q < world; ++q) {
            uint64_t n_in = 0;
            for (uint32_t r = 0; r < world; ++r) {
                const unsigned long long base = (unsigned long long)q * (P[r].n_rec + 1);
                if (ends[r][q] < base || ends[r][q] - base > P[r].n_rec) return snk_fail(SNK_E_INTERNAL, err, errcap, "snk_dev_rank_lists: a record region overran");
                n_in += ends[r][q] - base;
            }
            uint4* rk_in;
            G_ALLOC(rk_in, uint4, n_in + 2);
            uint64_t at = 0;
            for (uint32_t r = 0; r < world; ++r) {
                const unsigned long long base = (unsigned long long)q * (P[r].n_rec + 1), cnt = ends[r][q] - base;
                if (cnt) SNK_HIP_TRY(hipMemcpyAsync(rk_in + at, rsend[r] + base, cnt * 16, hipMemcpyDeviceToDevice, st));
                at += cnt;
            }
            const uint64_t s0 = 2 * frag_off[q], nl = 2 * (frag_off[q + 1] - frag_off[q]);
            const uint2* rk_q = nullptr;
            if ((rc = snk_prank_apply(ctx, st, rk_in, n_in, s0, nl, &rk_q, err, errcap))) return rc;
            if (nl) SNK_HIP_TRY(hipMemcpyAsync(rk_out + s0, rk_q, nl * 8, hipMemcpyDeviceToDevice, st));
        }
        ranked = true;
    }
    ev->sparse_cut = tr.sparse_cut;
    ev->bad = tr.bad;
    ev->n_circles = join_circles;
    ev->partitioned = ranked ? 1u : 0u;
    ev->source = SNK_RANK_RULING;
    if (!ranked) {
        // a circle the fast cut refuses, or no attempt left: the replicated ranking on the links as the cuts left them, marks kept
        const uint2* rk = nullptr;
        uint8_t* circ_out = nullptr;
        uint32_t nc = 0;
        snk_rank_trace tf;
        if ((rc = snk_join_rank(ctx, st, n, w, link, &rk, &circ_out, &nc, &ev->rounds, err, errcap, circ, &tf))) return rc;
        SNK_HIP_TRY(hipMemcpyAsync(rk_out, rk, ns * 8, hipMemcpyDeviceToDevice, st));
        ev->n_circles += nc;
        ev->source = tf.source;
        ev->ruling_attempts = tf.ruling_attempts;
        ev->sparse_cut += tf.sparse_cut;
        ev->bad |= tf.bad;
    }
    return SNK_OK;
}
}  // namespace

extern "C" int snk_dev_rank_lists(snk_ctx* ctx, uint64_t n, void* d_link, const void* d_weights, void* d_circ, uint32_t world, const uint64_t* frag_off,
                                  void* d_rk, snk_rank_evidence* out, void* stream, char* err, size_t errcap) {
    if (!ctx || !out) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_rank_lists: NULL argument");
    memset(out, 0, sizeof *out);
    if (n == 0) return SNK_OK;
    if (!d_link || !d_rk) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_rank_lists: NULL device array");
    if (n >= (1ull << 31)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_rank_lists: %llu nodes (2n must stay below 2^32)", (unsigned long long)n);
    if (world) {
        if (!d_weights || !d_circ) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_rank_lists: the partitioned ranking needs weights and circ");
        if (!frag_off || frag_off[0] != 0 || frag_off[world] != n) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_rank_lists: frag_off does not run from 0 to n");
        for (uint32_t q = 0; q < world; ++q)
            if (frag_off[q] > frag_off[q + 1]) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_rank_lists: frag_off descends at owner %u", q);
    }
    const uint64_t ns = 2 * n;
    return snk_call_run(ctx, stream, "snk_dev_rank_lists", out, err, errcap, [&](snk_call& c) -> int {
        const hipStream_t st = c.st;
        // the links are an involution, or no walk over them need end: judged on the host before anything is launched
        std::vector<uint32_t> h_link(ns);
        SNK_HIP_TRY(hipMemcpyAsync(h_link.data(), d_link, ns * 4, hipMemcpyDeviceToHost, st));
        SNK_HIP_TRY(snk_sync(st));
        for (uint64_t s = 0; s < ns; ++s) {
            const uint32_t l = h_link[s];
            if (l == NONE) continue;
            if (l >= ns) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_rank_lists: link[%llu] = %u lies outside the %llu states", (unsigned long long)s, l, (unsigned long long)ns);
            if (h_link[l] != s) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_rank_lists: link[link[%llu]] != %llu: not an involution", (unsigned long long)s, (unsigned long long)s);
        }
        uint32_t* link = (uint32_t*)d_link;
        const uint32_t* w = (const uint32_t*)d_weights;
        uint8_t* circ = (uint8_t*)d_circ;
        if (world) return prank_emulated(c, n, link, w, circ, world, frag_off, (uint2*)d_rk, out, err, errcap);
        const uint2* rk = nullptr;
        snk_rank_trace tr;
        int rc2 = snk_rank_lists(ctx, st, link, n, w, circ, &rk, &out->n_circles, &out->rounds, err, errcap, &tr);
        if (rc2) return rc2;
        SNK_HIP_TRY(hipMemcpyAsync(d_rk, rk, ns * 8, hipMemcpyDeviceToDevice, st));
        out->source = tr.source;
        out->ruling_attempts = tr.ruling_attempts;
        out->splitters = tr.m_first;
        out->sparse_cut = tr.sparse_cut;
        out->bad = tr.bad;
        return SNK_OK;
    });
}
