// snk_shard.h -- the minimiser-sharded step's per-context session state and the phases snk_shard_step.hip runs between its exchanges
// (snk_dist.hip implements those that do more than forward to snk_local.hip / snk_graph.hip / snk_rank.hip).  Library-internal: the multi-GPU surface
// of include/snk.h is snk_shard_step / snk_shard_stream_* / snk_shard_gather_unitigs.
#pragma once
#include "snk_ctx.h"
#include "snk_graph.h"
#include "snk_rank.h"
#include "snk_kernels.h"
#include "snk_stages.h"

struct snk_shard_state {
    snk_params params;
    uint32_t rank = 0, world = 1, NB_total = 0, NBl = 0;
    uint32_t* status = nullptr;
    snk_partition part{};
    snk_table tab{};
    snk_dist_graph g{};
    snk_bl_state bl{};
    snk_frag_out frags{};              // this rank's fragments (valid from snk_bl_dist_fragments on)
    const unsigned long long* d_node_off = nullptr;      // u64[world+1] exclusive scan of the ranks' retained k-mers (global node numbering)
    unsigned long long my_node_off = 0, my_end_base = 0;
    unsigned long long* lq_cursor = nullptr;   // [world+1] cursors of the link queries' regions and, behind them, this rank's fragment count
    // owner-side join: placement of this rank's fragments, route cursors
    snk_placement pl{};
    unsigned long long* rt_cursor = nullptr;   // [2][world]: fragments, base bytes
    unsigned long long my_frag_off = 0;
    uint32_t join_circles = 0, join_rounds = 0;
    snk_prank pr{};
    uint8_t* circ_all = nullptr;               // [2 * fragments of the job] terminals made by cutting circles (replicated; reset per step)
    const uint32_t* nk_all = nullptr;
    // a streamed step (snk_shard_stream_*): the rank's reads arrive slab by slab and are partitioned as they come
    snk_partition_job job{};
    bool job_open = false;
    uint32_t job_read_len = 0;
    int job_has_bc = 0;
    uint64_t job_reads_ub = 0, job_total_reads = 0;
    uint16_t* job_good_len = nullptr;
};

inline snk_shard_state* snk_shard_state_of(snk_ctx* ctx) {
    if (!ctx->shard) ctx->shard = new snk_shard_state();
    return static_cast<snk_shard_state*>(ctx->shard);
}

// ---- the step's reads: trim + one-pass minimiser partition over all NB_total buckets of the job (S->part) ...
int snk_shard_begin(snk_ctx* ctx, const snk_dev_reads* in, const snk_params* p, uint32_t rank, uint32_t world, uint32_t NB_total,
                    uint64_t* n_instances, hipStream_t st, char* err, size_t errcap);
// ... or slab by slab: open (sizes the job's slots), add a slab, adopt (closes the job: S->part as snk_shard_begin leaves it)
int snk_shard_job_open(snk_ctx* ctx, const snk_params* p, uint32_t rank, uint32_t world, uint32_t NB_total, uint32_t read_len, uint64_t reads_ub,
                       uint64_t total_reads, int has_bc, hipStream_t st, char* err, size_t errcap);
int snk_shard_job_add(snk_ctx* ctx, const snk_dev_reads* slab, hipStream_t st, char* err, size_t errcap);
int snk_shard_job_adopt(snk_ctx* ctx, uint64_t* n_instances, hipStream_t st, char* err, size_t errcap);

// ---- the phases behind the count (S.tab).  Device pointers; what a phase leaves in S stays valid until the context's next step.
// (Not in the library's dynamic symbol table, as little as the round-2 entry points they were until they became plain functions.)
#pragma GCC visibility push(hidden)
// Bucket-local prune, first half: only neighbours owned by another rank become membership queries (24 bytes each, answers 4 bytes);
// their counts per rank stay on the device (S.bl.qcount).  snk_bl_dist_fill -> [queries] -> snk_dist_answer -> [answers] -> snk_dist_apply.
int snk_shard_prune_plan(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, char* err, size_t errcap);
// Owner-side join (replaces the rank-0 funnel of tada's MAIN_ASM_SN, lib/tada/src/cmd_main_asm.rs:25-89,184-193; its build_edges is
// lib/tada/src/debruijn.rs:733-776): every rank holds the LINKS (u32[2F] global end ids) and k-mer counts (u32[F]) of all fragments,
// ranks the lists, places its own fragments and sends each to the rank that owns its unitig's head fragment, which writes the unitig.
// snk_shard_place: the ranking replicated on every rank (a list is a circle, or the option asks for it).
int snk_shard_place(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, uint64_t n_frags_total, const uint32_t* nk_all, uint32_t* flink_all,
                    uint64_t my_frag_off, char* err, size_t errcap);
// The ranking partitioned over the ranks (snk_rank.hip; a rank walks 1/world of the splitters of the ruling-set scheme; only the streaming
// set-up, which is the one-GPU ranking's, and the short splitter list are replicated): snk_shard_prank_begin -> all-gather of S.pr.w1_share (16 B per splitter, shares
// [m*r/world, m*(r+1)/world)) -> snk_prank_walk (circles = 1: some list is a circle, rank the replicated way; 2: circles were cut in the
// replicated links, begin again) -> snk_prank_route -> all-to-all (16 B per state) -> snk_shard_place_ranked.
int snk_shard_prank_begin(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, uint64_t n_frags_total, const uint32_t* nk_all, uint32_t* flink_all,
                          uint64_t my_frag_off, char* err, size_t errcap);
int snk_shard_place_ranked(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, const void* d_recs, uint64_t n_recs, char* err, size_t errcap);
// 32-byte headers and the bases of this rank's fragments, grouped by owner from the given first header / first base byte of every
// owner's region (u64[world] each; two all-to-alls follow; S.rt_cursor holds the regions' ends afterwards) ...
int snk_shard_route_fill(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, uint32_t K, const unsigned long long* d_frag_off, const unsigned long long* d_hdr_off,
                         const unsigned long long* d_base_off, void* d_hdr, void* d_bases, char* err, size_t errcap);
// ... and what arrived (d_hdr_seg / d_base_seg: first header / first base byte of every source rank, u64[world+1]) -> this rank's unitigs
int snk_shard_emit(snk_ctx* ctx, snk_shard_state& S, hipStream_t st, uint32_t K, uint64_t n_recv, const void* d_hdr, const unsigned long long* d_hdr_seg,
                   const unsigned long long* d_base_seg, const uint8_t* d_bases, snk_join_out* out, char* err, size_t errcap);
#pragma GCC visibility pop
