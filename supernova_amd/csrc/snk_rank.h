// snk_rank.h -- internal interface of the list ranking (snk_rank.hip): the k-mer states of the global graph stage, the fragment ends
// of the join on one GPU, and the fragment ends of the sharded step partitioned over the ranks.
#pragma once
#include "snk_ctx.h"

// List ranking over the 2n directed states (node, exit side) of a degree<=2 link graph: for every state the number of steps (or summed
// weights) to the end of its path and the terminal state.  Smooth circles are cut and the lists ranked again; link[] is modified by the
// cut, circ (per state, nullable) marks the terminals a cut made.  Sparse ruling set, or plain pointer jumping (small inputs, rank_wyllie,
// circles the fast cut refuses).
// trace (nullable; NULL on the production callers): which way the call went, for snk_dev_rank_lists (include/snk.h: snk_rank_evidence)
struct snk_rank_trace {
    uint32_t source = 0;           // SNK_RANK_*: what produced rk
    uint32_t ruling_attempts = 0;  // ruling-set attempts of snk_rank_lists
    uint32_t sparse_cut = 0;       // circles the sparse cut cut (added up over the attempts)
    uint32_t bad = 0;              // the sparse cut met something it leaves to the general algorithm
    uint64_t m_first = 0;          // splitters of the first attempt
};
int snk_rank_lists(snk_ctx* ctx, hipStream_t st, uint32_t* link, uint64_t n, const uint32_t* weights, uint8_t* circ, const uint2** rk_out,
                   uint32_t* n_circles, uint32_t* rounds, char* err, size_t errcap, snk_rank_trace* trace = nullptr);

// the ruling set of a link structure: its splitters (list heads and a hashed 1 / 2^split_log2 sample of the states) and the walk records
struct snk_rank_setup {
    uint64_t ns, m;            // states, splitters
    uint32_t split_mask;
    uint32_t* spl_state;       // [m + 1] state of every splitter, in state order
    unsigned long long* wrec;  // [ns + 1] walk record of every state (snk_rank.hip: wrec_*)
};

// partitioned ranking of the job's fragment lists (sharded runs): replicated streaming set-up, walks for a 1/world share
struct snk_prank {
    snk_rank_setup set;
    uint64_t k0, k1, n_rec;    // this rank's splitters [k0, k1), records of its second walk
    const uint32_t* w;
    uint32_t* link;
    uint4* w1_share;           // [k1-k0] first walk of this rank's splitters: next splitter, distance, tail, states
    uint4* rec;                // [n_rec] second walk: state, distance, terminal, 0
};
int snk_prank_begin(snk_ctx* ctx, hipStream_t st, uint64_t F, const uint32_t* nk, uint32_t* link, uint32_t rank, uint32_t world, snk_prank* P, char* err,
                    size_t errcap);
int snk_prank_walk(snk_ctx* ctx, hipStream_t st, snk_prank* P, const uint4* w1_all, uint32_t* circles, uint32_t* rounds, char* err, size_t errcap,
                   uint8_t* circ = nullptr /* [ns]: given = circles are cut here (*circles = 2: begin again) */, uint32_t* n_cut = nullptr,
                   snk_rank_trace* trace = nullptr /* adds the cut's count and its verdict */);
int snk_prank_route(snk_ctx* ctx, hipStream_t st, snk_prank* P, const unsigned long long* d_frag_off, uint32_t world,
                    unsigned long long* d_cursor /* [world]: first record of every owner's region; the regions' ends afterwards */, void* d_out, char* err, size_t errcap);
int snk_prank_apply(snk_ctx* ctx, hipStream_t st, const void* d_rec, uint64_t n, unsigned long long state_base, uint64_t n_local_states,
                    const uint2** rk_out, char* err, size_t errcap);
