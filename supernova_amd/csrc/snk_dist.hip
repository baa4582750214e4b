// snk_dist.hip -- the minimiser-sharded (multi-GPU) path: the session state of a step, its read intake, and the phases of the step that
// do more than forward to the bucket-local stage (snk_local.hip), the join (snk_graph.hip) or the list ranking (snk_rank.hip).  snk_shard_step.hip drives everything and
// runs the exchanges (snk_comm.hip: RCCL over xGMI, or in-process ranks).  SURVEY.md 8(e); the reference's counterpart is the shardio
// exchange + per-shard processing + global join of tada
// (lib/tada/external/rust-shardio/src/shard.rs:184-211,488-493; cmd_shard_asm.rs:37-94; cmd_main_asm.rs:25-89)
// and the thread swizzle of MapReduceEngine.h:362-385.
//
// One process (or host thread) per GPU.  The k-mer space is cut into NB_total minimiser buckets; rank r owns buckets
// [r*NB_total/world, (r+1)*NB_total/world).  Every rank runs, with [..] an exchange:
//   snk_shard_begin (or the slabs' snk_shard_job_*)  trim + one-pass partition over all buckets
//   -> [histograms] -> [records of the buckets other ranks own, in bucket ranges] -> snk_stage_count_table (own buckets in place)
//   -> snk_shard_prune_plan / snk_bl_dist_fill -> [membership queries] -> snk_dist_answer -> [answers] -> snk_dist_apply
//   -> snk_bl_dist_fragments -> snk_dist_links_query -> [link queries] -> snk_dist_links_answer -> [answers] -> snk_dist_links_apply_regions
//   -> [links + k-mer counts of all fragments] -> snk_shard_prank_begin -> [splitters] -> snk_prank_walk / snk_prank_route (snk_rank.hip) -> [ranks]
//   -> snk_shard_place_ranked  (or snk_shard_place: the ranking replicated, when a list is a circle)
//   -> snk_shard_route_fill -> [fragments to the owners of their unitigs' heads] -> snk_shard_emit: this rank's unitigs.
// There is no rank-0 funnel: every rank writes the unitigs whose head fragment it owns.
#include <string.h>

#include <vector>

#include "snk_ctx.h"
#include "snk_common.h"
#include "snk_graph.h"
#include "snk_kernels.h"
#include "snk_stages.h"
#include "snk_shard.h"

void snk_shard_state_free(void* p) { delete static_cast<snk_shard_state*>(p); }
void snk_shard_state_invalidate_job(void* p) { if (p) static_cast<snk_shard_state*>(p)->job_open = false; }

// a new step on this context: everything the last one held goes back
static snk_shard_state* step_reset(snk_ctx* ctx, const snk_params* p, uint32_t rank, uint32_t world, uint32_t NB_total) {
    snk_ctx_release_scratch(ctx);
    snk_shard_state* S = snk_shard_state_of(ctx);
    S->params = *p;
    S->rank = rank; S->world = world; S->NB_total = NB_total; S->NBl = NB_total / world;
    S->circ_all = nullptr; S->join_circles = 0;
    ctx->last_bl_attempts = ctx->last_bl_big_chunks = 0; ctx->last_bl_circles = 0;
    return S;
}

// (its refusals carry the name of the round-2 entry point this was the first half of: callers of snk_shard_step have seen it since,
// and the texts stay as they are)
static const char* const BEGIN_WHO = "snk_shard_hist";
int snk_shard_begin(snk_ctx* ctx, const snk_dev_reads* in, const snk_params* p, uint32_t rank, uint32_t world, uint32_t NB_total,
                    uint64_t* n_instances, hipStream_t st, char* err, size_t errcap) {
    if (!ctx || !in || !p) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument", BEGIN_WHO);
    int rc;
    if ((rc = snk_intake_check_params(p, err, errcap))) return rc;
    if (world == 0 || rank >= world || NB_total == 0 || NB_total % world) return snk_fail(SNK_E_ARG, err, errcap, "%s: NB_total must be a positive multiple of world", BEGIN_WHO);
    if (world > 0x7FFF) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "world > 32767");
    if (snk_intake_reads_fault(in)) return snk_fail(SNK_E_ARG, err, errcap, "%s: bad reads", BEGIN_WHO);
    SNK_HIP_TRY(snk_enter(ctx));
    snk_shard_state* S = step_reset(ctx, p, rank, world, NB_total);
    const uint16_t* good_len;
    snk_fused_trim ft;
    bool fused;
    if ((rc = snk_intake_trim(ctx, st, in, p, &good_len, &ft, &fused, err, errcap))) return rc;
    if ((rc = snk_intake_status(ctx, st, &S->status, err, errcap))) return rc;
    // one partition pass into fixed-capacity bucket slots (as on one GPU); the histogram is its cursor array
    // the slots are sized from what the untrimmed reads could hold at most (a few per cent above what the trim leaves: the
    // capacity is 2.5 x the mean anyway); the exact instance count comes back with the partition's own read-back
    unsigned long long h_plan[2] = {0, 0};
    unsigned long long* d_plan = nullptr;
    if (!fused && (rc = snk_stage_partition_plan(ctx, st, p->K, good_len, in->n_reads, h_plan, err, errcap, &d_plan))) return rc;
    const unsigned long long kpr = in->read_len >= p->K ? in->read_len - p->K + 1 : 0;
    if ((rc = snk_stage_partition(ctx, st, p->K, in, good_len, NB_total, in->n_reads * kpr, in->n_reads, false, S->status, &S->part, err, errcap, d_plan, h_plan,
                                  fused ? &ft : nullptr))) return rc;
    if (n_instances) *n_instances = h_plan[0];
    return SNK_OK;
}

// ---- streamed step: the partition runs slab by slab while the next slab is decoded / uploaded (lib/tada/src/cmd_msp.rs:55-69 streams its
// FASTQ chunks into the partitioner the same way); everything behind the partition is the resident step's
int snk_shard_job_open(snk_ctx* ctx, const snk_params* p, uint32_t rank, uint32_t world, uint32_t NB_total, uint32_t read_len, uint64_t reads_ub,
                       uint64_t total_reads, int has_bc, hipStream_t st, char* err, size_t errcap) {
    if (!ctx || !p) return snk_fail(SNK_E_ARG, err, errcap, "snk_shard_stream_begin: NULL argument");
    int rc;
    if ((rc = snk_intake_check_params(p, err, errcap))) return rc;
    if (world == 0 || rank >= world || NB_total == 0 || NB_total % world) return snk_fail(SNK_E_ARG, err, errcap, "snk_shard_stream_begin: NB_total must be a positive multiple of world");
    if (read_len == 0 || read_len > 256 || reads_ub == 0) return snk_fail(SNK_E_ARG, err, errcap, "snk_shard_stream_begin: read_len 1..256 and an upper bound of this rank's reads are needed");
    SNK_HIP_TRY(snk_enter(ctx));
    snk_shard_state* S = step_reset(ctx, p, rank, world, NB_total);
    S->job_open = false; S->job_read_len = read_len; S->job_has_bc = has_bc; S->job_reads_ub = reads_ub; S->job_total_reads = total_reads;
    if ((rc = snk_intake_status(ctx, st, &S->status, err, errcap))) return rc;
    void* q;
    if ((rc = snk_ctx_alloc(ctx, reads_ub * 2 + 64, &q, err, errcap))) return rc; S->job_good_len = (uint16_t*)q;
    const unsigned long long kpr = read_len >= p->K ? read_len - p->K + 1 : 0;
    if ((rc = snk_partition_open(ctx, st, p->K, NB_total, reads_ub * kpr, reads_ub, false, S->status, &S->job, err, errcap))) return rc;
    S->job_open = true;
    return SNK_OK;
}
int snk_shard_job_add(snk_ctx* ctx, const snk_dev_reads* slab, hipStream_t st, char* err, size_t errcap) {
    if (!ctx || !ctx->shard || !slab) return snk_fail(SNK_E_ARG, err, errcap, "snk_shard_stream_append: NULL argument / no open step");
    snk_shard_state* S = snk_shard_state_of(ctx);
    if (!S->job_open) return snk_fail(SNK_E_ARG, err, errcap, "snk_shard_stream_append: no open step (snk_shard_stream_begin)");
    if (slab->n_reads == 0) return SNK_OK;
    int rc = snk_intake_check_slab(slab, S->job_read_len, S->job_has_bc != 0, S->job.n_reads, S->job_reads_ub, "snk_shard_stream_append", "step's", "rank's", err, errcap);
    if (rc) return rc;
    SNK_HIP_TRY(snk_enter(ctx));
    return snk_intake_add_slab(ctx, st, &S->job, slab, S->params.min_qual, S->job_good_len + S->job.n_reads, err, errcap);
}
int snk_shard_job_adopt(snk_ctx* ctx, uint64_t* n_instances, hipStream_t st, char* err, size_t errcap) {
    snk_shard_state* S = snk_shard_state_of(ctx);
    if (!S->job_open) return snk_fail(SNK_E_ARG, err, errcap, "snk_shard_stream_finish: no open step");
    S->job_open = false;
    unsigned long long h_plan[2] = {0, 0};
    int rc = snk_partition_close(ctx, st, &S->job, &S->part, h_plan, err, errcap);
    if (rc) return rc;
    if (n_instances) *n_instances = h_plan[0];
    return SNK_OK;
}

int snk_shard_prune_plan(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, char* err, size_t errcap) {
    // bucket-local prune (snk_local.hip); only neighbours owned by another rank become queries
    snk_bl_state& B = S.bl;
    memset(&B, 0, sizeof B);
    B.tab = &S.tab;
    B.K = S.params.K; B.rank = S.rank; B.world = S.world; B.NB_total = S.NB_total; B.NBl = S.NBl;
    B.do_prune = S.params.min_freq > 1 ? 1u : 0u;
    int rc = snk_bl_dist_plan(ctx, st, &B, err, errcap);      // (the counts stay on the device: B.qcount)
    if (rc) return rc;
    // the answering / applying kernels of the global sharded stage work on the same arrays
    snk_dist_graph& g = S.g;
    memset(&g, 0, sizeof g);
    g.K = B.K; g.rank = B.rank; g.world = B.world; g.NB_total = B.NB_total; g.NBl = B.NBl; g.do_prune = B.do_prune;
    g.n = S.tab.n; g.keys = S.tab.keys; g.vals = S.tab.vals;
    g.index = B.index; g.index_mask = B.index_mask;
    g.ctx = B.ctx; g.counts = B.counts; g.rq_idx = B.rq_idx; g.rq_meta = B.rq_meta;
    return SNK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Owner-side join (no rank-0 funnel).  tada's MAIN_ASM_SN is one process (lib/tada/src/cmd_main_asm.rs:25-89,184-193) and so
// was the first version of this path: every fragment travelled to rank 0, which ranked and wrote all unitigs -- serial in
// the size of the job.  Now the only thing every rank sees of the whole job is the LINK structure (8 + 4 bytes per fragment,
// all-gathered): it ranks the fragment lists, places its own fragments (unitig = the smaller terminal state, offset,
// strand) and sends each fragment's bases to the rank that owns the unitig's head fragment, which writes the unitig.
//   snk_shard_place*      links + k-mer counts of all ranks -> placement of my fragments
//   snk_shard_route_fill  32-byte headers + bases grouped by owner (the two send buffers of one all-to-all each)
//   snk_shard_emit        headers + bases received -> this rank's unitigs (canonical, circles rotated, ordered)
namespace {
constexpr unsigned long long RT_RC = 1ull, RT_CIRC = 2ull, RT_HEAD = 4ull;
__device__ __forceinline__ uint32_t owner_of_frag(const unsigned long long* __restrict__ frag_off, uint32_t world, unsigned long long g) {
    uint32_t r = 0;
    while (r + 1 < world && g >= frag_off[r + 1]) ++r;
    return r;
}
// FILL = false: count fragments and base bytes per owner; true: write header and bases at reserved positions (the step routes in one
// pass into per-owner regions and launches FILL = true only).
// header (4 x u64): pid | gfid << 32;  nk | flags << 32;  koff (heads: N);  offset of the bases inside the owner's segment.
// One fragment per thread for the bookkeeping: the workgroup adds up its fragments and bytes per owner in LDS and goes to
// the `world` device counters once per owner (2 M fragments on the same few addresses, one device atomic each, took 100 ms);
// then the bases are copied by 8 lanes per fragment.
constexpr int ROUTE_TILES = 16;      // tiles of 256 fragments per workgroup: ONE reservation per owner for all of them (see jlink_query_kernel, snk_graph.hip)
template <bool FILL>
__global__ void __launch_bounds__(256) route_kernel(uint64_t Fl, unsigned long long f0, const uint32_t* __restrict__ nk, const uint32_t* __restrict__ pl_pid,
                                                    const unsigned long long* __restrict__ pl_koff, const unsigned long long* __restrict__ pl_N,
                                                    const uint8_t* __restrict__ pl_circ, const unsigned long long* __restrict__ frag_off, uint32_t world,
                                                    uint32_t K, const uint64_t* __restrict__ boff, const uint8_t* __restrict__ bases,
                                                    unsigned long long* __restrict__ cnt_or_cur /* [2][world] */, unsigned long long* __restrict__ hdr,
                                                    uint8_t* __restrict__ bout, const unsigned long long* __restrict__ base_seg /* [world] byte offset of every owner's segment */) {
    extern __shared__ unsigned long long dynr[];          // [world] fragments -> reserved first header, [world] bytes -> reserved first byte, [2][world] running cursors
    __shared__ unsigned long long c_src[256], c_dst[256];
    __shared__ uint32_t c_len[256];
    unsigned long long* lfr = dynr;
    unsigned long long* lby = dynr + world;
    unsigned long long* cfr = dynr + 2 * world;
    unsigned long long* cby = dynr + 3 * world;
    for (uint32_t r = threadIdx.x; r < 4 * world; r += 256) dynr[r] = 0;
    __syncthreads();
    const uint64_t fbase = (uint64_t)blockIdx.x * 256 * ROUTE_TILES + threadIdx.x;
    for (int t = 0; t < ROUTE_TILES; ++t) {
        const uint64_t f = fbase + (uint64_t)t * 256;
        if (f < Fl) {
            const uint32_t owner = owner_of_frag(frag_off, world, pl_pid[f] >> 1);
            atomicAdd(&lfr[owner], 1ull);
            atomicAdd(&lby[owner], (unsigned long long)((uint64_t)nk[f] + K - 1));
        }
    }
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < world; r += 256) {
        const unsigned long long cf = lfr[r], cb = lby[r];
        if (cf) {
            const unsigned long long a = atomicAdd(&cnt_or_cur[r], cf), b = atomicAdd(&cnt_or_cur[world + r], cb);
            lfr[r] = a; lby[r] = b;
        }
    }
    if (!FILL) return;
    for (int t = 0; t < ROUTE_TILES; ++t) {
        __syncthreads();       // the reservations are in LDS / the copy of the tile before is through with c_src, c_dst, c_len
        const uint64_t f = fbase + (uint64_t)t * 256;
        c_len[threadIdx.x] = 0;
        if (f < Fl) {
            const uint32_t pid = pl_pid[f];
            const uint32_t owner = owner_of_frag(frag_off, world, pid >> 1);
            const uint64_t len = (uint64_t)nk[f] + K - 1;
            const unsigned long long slot = lfr[owner] + atomicAdd(&cfr[owner], 1ull), bo = lby[owner] + atomicAdd(&cby[owner], (unsigned long long)len);
            const unsigned long long ko = pl_koff[f];
            const unsigned long long g = f0 + f;
            const bool head = (ko & ~(1ull << 63)) == 0 && (pid >> 1) == (uint32_t)g;
            const unsigned long long flags = ((ko >> 63) ? RT_RC : 0ull) | (pl_circ[f] ? RT_CIRC : 0ull) | (head ? RT_HEAD : 0ull);
            hdr[4 * slot + 0] = (unsigned long long)pid | (g << 32);
            hdr[4 * slot + 1] = (unsigned long long)nk[f] | (flags << 32);
            hdr[4 * slot + 2] = head ? pl_N[f] : (ko & ~(1ull << 63));
            hdr[4 * slot + 3] = bo - base_seg[owner];
            c_src[threadIdx.x] = boff[f];
            c_dst[threadIdx.x] = bo;
            c_len[threadIdx.x] = (uint32_t)len;
        }
        __syncthreads();
        const uint32_t sub = threadIdx.x & 7u;
        for (uint32_t i = threadIdx.x >> 3; i < 256; i += 32) {
            const uint32_t n = c_len[i];
            const uint8_t* src = bases + c_src[i];
            uint8_t* dst = bout + c_dst[i];
            // bytes up to dst's first 4-byte boundary, dwords (read at byte alignment), the last bytes -- a byte per lane and instruction
            // made the copy instruction-bound (snk_graph.hip, jemit_kernel)
            struct __attribute__((packed)) u32_any { uint32_t v; };
            uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
            if (head > n) head = n;
            if (sub < head) dst[sub] = src[sub];
            const uint32_t ndw = (n - head) >> 2;
            for (uint32_t j = sub; j < ndw; j += 8) *reinterpret_cast<uint32_t*>(dst + head + 4 * j) = reinterpret_cast<const u32_any*>(src + head + 4 * j)->v;
            const uint32_t t0 = head + 4 * ndw;
            if (sub < n - t0) dst[t0 + sub] = src[t0 + sub];
        }
    }
}
// received headers -> the arrays snk_join_emit wants; hdr_seg / base_seg: first header / first base byte of every source rank
__global__ void __launch_bounds__(256) unroute_kernel(const unsigned long long* __restrict__ hdr, uint64_t F, const unsigned long long* __restrict__ hdr_seg,
                                                      const unsigned long long* __restrict__ base_seg, uint32_t world, uint32_t* __restrict__ nk,
                                                      uint32_t* __restrict__ gfid, uint32_t* __restrict__ pid, unsigned long long* __restrict__ koff,
                                                      unsigned long long* __restrict__ N, uint8_t* __restrict__ circ, uint64_t* __restrict__ boff) {
    const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    uint32_t src = 0;
    while (src + 1 < world && f >= hdr_seg[src + 1]) ++src;
    const unsigned long long w0 = hdr[4 * f], w1 = hdr[4 * f + 1], w2 = hdr[4 * f + 2], w3 = hdr[4 * f + 3];
    const unsigned long long flags = w1 >> 32;
    pid[f] = (uint32_t)w0;
    gfid[f] = (uint32_t)(w0 >> 32);
    nk[f] = (uint32_t)w1;
    const bool head = flags & RT_HEAD;
    koff[f] = (head ? 0ull : w2) | ((flags & RT_RC) ? (1ull << 63) : 0ull);
    N[f] = head ? w2 : 0ull;
    circ[f] = (flags & RT_CIRC) ? 1 : 0;
    boff[f] = base_seg[src] + w3;
}
}  // namespace

// placement of this rank's fragments from a ranking (whole list: rk_f0 = 0; own states only: rk_f0 = my_frag_off), and the cursors of the
// one-pass routing into per-owner regions (snk_shard_route_fill)
static int place(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, const uint2* rk, uint64_t rk_f0, const uint8_t* circ, const uint32_t* nk_all, char* err,
                 size_t errcap) {
    int rc;
    if ((rc = snk_join_place(ctx, st, rk, nk_all, circ, S.my_frag_off, S.frags.n_frags, &S.pl, err, errcap, rk_f0))) return rc;
    void* q;
    if ((rc = snk_ctx_alloc(ctx, 2ull * (S.world + 1) * 8, &q, err, errcap))) return rc; S.rt_cursor = (unsigned long long*)q;
    return SNK_OK;
}

int snk_shard_place(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, uint64_t n_frags_total, const uint32_t* nk_all, uint32_t* flink_all,
                    uint64_t my_frag_off, char* err, size_t errcap) {
    if (2 * n_frags_total >= (1ull << 32)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "more than 2^31 fragments in the job");
    S.my_frag_off = my_frag_off;
    const uint2* rk = nullptr;
    uint8_t* circ = nullptr;
    uint32_t nc = 0;
    int rc = snk_join_rank(ctx, st, n_frags_total, nk_all, flink_all, &rk, &circ, &nc, &S.join_rounds, err, errcap, S.circ_all);
    if (rc) return rc;
    S.join_circles += nc;
    return place(ctx, S, st, rk, 0, circ, nk_all, err, errcap);
}

// ---- the ranking partitioned over the ranks (snk_rank.hip: snk_prank_*)
int snk_shard_prank_begin(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, uint64_t n_frags_total, const uint32_t* nk_all, uint32_t* flink_all,
                          uint64_t my_frag_off, char* err, size_t errcap) {
    if (2 * n_frags_total >= (1ull << 32)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "more than 2^31 fragments in the job");
    S.my_frag_off = my_frag_off;
    S.nk_all = nk_all;
    if (!S.circ_all) {          // first ranking attempt of this step (a second one follows a circle cut and keeps the marks)
        void* q;
        int rc0 = snk_ctx_alloc(ctx, 2 * n_frags_total + 16, &q, err, errcap);
        if (rc0) return rc0;
        S.circ_all = (uint8_t*)q;
        SNK_HIP_TRY(hipMemsetAsync(S.circ_all, 0, 2 * n_frags_total + 16, st));
    }
    // (the share S.pr.w1_share is consumed by a collective on the same stream: nothing to wait for here)
    return snk_prank_begin(ctx, st, n_frags_total, nk_all, flink_all, S.rank, S.world, &S.pr, err, errcap);
}
int snk_shard_place_ranked(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, const void* d_recs, uint64_t n_recs, char* err, size_t errcap) {
    const uint2* rk = nullptr;
    int rc = snk_prank_apply(ctx, st, d_recs, n_recs, 2ull * S.my_frag_off, 2ull * S.frags.n_frags, &rk, err, errcap);
    if (rc) return rc;
    return place(ctx, S, st, rk, S.my_frag_off, S.join_circles ? S.circ_all : nullptr, S.nk_all, err, errcap);
}

int snk_shard_route_fill(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, uint32_t K, const unsigned long long* d_frag_off, const unsigned long long* d_hdr_off,
                         const unsigned long long* d_base_off, void* d_hdr, void* d_bases, char* err, size_t errcap) {
    const uint64_t Fl = S.frags.n_frags;
    SNK_HIP_TRY(hipMemcpyAsync(S.rt_cursor, d_hdr_off, S.world * 8ull, hipMemcpyDeviceToDevice, st));
    SNK_HIP_TRY(hipMemcpyAsync(S.rt_cursor + S.world, d_base_off, S.world * 8ull, hipMemcpyDeviceToDevice, st));
    SNK_HIP_TRY(snk_launch(route_kernel<true>, snk_blocks(Fl, 256 * ROUTE_TILES), 256, 4ull * S.world * 8, st, Fl, (unsigned long long)S.my_frag_off, S.frags.nk, S.pl.pid, S.pl.koff,
                           S.pl.N, S.pl.circ, d_frag_off, S.world, K, S.frags.boff, S.frags.bases, S.rt_cursor, (unsigned long long*)d_hdr, (uint8_t*)d_bases, d_base_off));
    return SNK_OK;
}

int snk_shard_emit(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, uint32_t K, uint64_t n_recv, const void* d_hdr, const unsigned long long* d_hdr_seg,
                   const unsigned long long* d_base_seg, const uint8_t* d_bases, snk_join_out* out, char* err, size_t errcap) {
    uint32_t *nk, *gfid, *pid;
    unsigned long long *koff, *N;
    uint8_t* circ;
    uint64_t* boff;
    void* q;
    int rc;
    if ((rc = snk_ctx_alloc(ctx, (n_recv + 1) * 4, &q, err, errcap))) return rc; nk = (uint32_t*)q;
    if ((rc = snk_ctx_alloc(ctx, (n_recv + 1) * 4, &q, err, errcap))) return rc; gfid = (uint32_t*)q;
    if ((rc = snk_ctx_alloc(ctx, (n_recv + 1) * 4, &q, err, errcap))) return rc; pid = (uint32_t*)q;
    if ((rc = snk_ctx_alloc(ctx, (n_recv + 1) * 8, &q, err, errcap))) return rc; koff = (unsigned long long*)q;
    if ((rc = snk_ctx_alloc(ctx, (n_recv + 1) * 8, &q, err, errcap))) return rc; N = (unsigned long long*)q;
    if ((rc = snk_ctx_alloc(ctx, (n_recv + 1), &q, err, errcap))) return rc; circ = (uint8_t*)q;
    if ((rc = snk_ctx_alloc(ctx, (n_recv + 2) * 8, &q, err, errcap))) return rc; boff = (uint64_t*)q;
    SNK_HIP_TRY(snk_launch(unroute_kernel, snk_blocks(n_recv, 256), 256, 0, st, (const unsigned long long*)d_hdr, n_recv, d_hdr_seg, d_base_seg, S.world, nk, gfid, pid, koff, N,
                           circ, boff));
    // every pid received here is a terminal state of one of this rank's own fragments
    return snk_join_emit(ctx, st, K, n_recv, nk, gfid, pid, koff, N, circ, (uint32_t)(2 * S.my_frag_off), 2 * S.frags.n_frags, boff, d_bases, nullptr, out, err, errcap);
}

// ---- fragment bases on the wire: 2 bits per base (the gather to rank 0 is the only place where bases cross xGMI)
namespace {
__global__ void __launch_bounds__(256) pack2_kernel(const uint8_t* __restrict__ in, uint64_t n, uint8_t* __restrict__ out) {
    // one thread per 16 bases -> one 32-bit word (base j of a byte at bits 2*(j%4), as in the .bv packing)
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t b0 = t * 16;
    if (b0 >= n) return;
    uint32_t w = 0;
    if (b0 + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(in + b0);
        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) w |= ((q[k] >> (8 * j)) & 3u) << (2 * (4 * k + j));
    } else {
        for (uint64_t j = 0; b0 + j < n; ++j) w |= (uint32_t)(in[b0 + j] & 3u) << (2 * j);
    }
    reinterpret_cast<uint32_t*>(out)[t] = w;
}
__global__ void __launch_bounds__(256) unpack2_kernel(const uint8_t* __restrict__ in, uint64_t n, uint8_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t b0 = t * 16;
    if (b0 >= n) return;
    const uint32_t w = reinterpret_cast<const uint32_t*>(in)[t];
    if (b0 + 16 <= n && ((uintptr_t)(out + b0) & 15u) == 0) {
        uint32_t q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            q[k] = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) q[k] |= ((w >> (2 * (4 * k + j))) & 3u) << (8 * j);
        }
        *reinterpret_cast<uint4*>(out + b0) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
        for (uint64_t j = 0; j < 16 && b0 + j < n; ++j) out[b0 + j] = (uint8_t)((w >> (2 * j)) & 3u);
    }
}
}  // namespace

extern "C" uint64_t snk_pack2_bytes(uint64_t n_bases) { return ((n_bases + 15) / 16) * 4; }

extern "C" int snk_dev_pack2(snk_ctx* ctx, const void* d_bases, uint64_t n_bases, void* d_packed, void* stream) {
    char* err = nullptr;
    size_t errcap = 0;
    if (!ctx || (n_bases && (!d_bases || !d_packed))) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_pack2: NULL argument");
    if (((uintptr_t)d_bases & 15u) || ((uintptr_t)d_packed & 3u)) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_pack2: bases must be 16-byte, packed 4-byte aligned");
    if (n_bases == 0) return SNK_OK;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    ctx->cur_stream = st;
    const uint64_t nt = (n_bases + 15) / 16;
    SNK_HIP_TRY(snk_launch(pack2_kernel, snk_blocks(nt, 256), 256, 0, st, (const uint8_t*)d_bases, n_bases, (uint8_t*)d_packed));
    return SNK_OK;
}

extern "C" int snk_dev_unpack2(snk_ctx* ctx, const void* d_packed, uint64_t n_bases, void* d_bases, void* stream) {
    char* err = nullptr;
    size_t errcap = 0;
    if (!ctx || (n_bases && (!d_bases || !d_packed))) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_unpack2: NULL argument");
    if ((uintptr_t)d_packed & 3u) return snk_fail(SNK_E_ARG, err, errcap, "snk_dev_unpack2: packed input must be 4-byte aligned");
    if (n_bases == 0) return SNK_OK;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    ctx->cur_stream = st;
    const uint64_t nt = (n_bases + 15) / 16;
    SNK_HIP_TRY(snk_launch(unpack2_kernel, snk_blocks(nt, 256), 256, 0, st, (const uint8_t*)d_packed, n_bases, (uint8_t*)d_bases));
    return SNK_OK;
}
