// snk_plan.h -- the sizing policy of the count path as plain host code: how many minimiser buckets a job gets, whether the count kernel
// books its table slots (count_tight), whether the bit filter goes in front of the table (count_screen), and from those the usable
// table slots a context reports after the call (last_count_limit).  One rule for the resident call (snk_dev_count_graph), the streamed
// job (snk_dev_stream_begin) and the sharded step (snk_shard_step, snk_shard_stream_begin): a caller fills snk_plan_in, applies
// snk_plan_out.  No HIP, no context, no I/O, no state: tests/plan_host.cc links it with the host compiler alone.
//
// The sizing HISTORY the rule feeds on (distinct and retained k-mers per instance of the previous call on the same data) is
// snk_sizing_history: one instance in a context, one in a communicator (the group's, snk_comm.h).
#pragma once
#include <stdint.h>

#include "snk_opts.h"

// the mode a history was made in: 2 K + grouped + 256 x minimiser length
inline uint32_t snk_sizing_key(uint32_t K, bool grouped, uint32_t mlen) { return K * 2 + (grouped ? 1u : 0u) + 256u * mlen; }

struct snk_sizing_history {
    double ratio = 0.0;          // distinct k-mers per k-mer instance the count kernel saw in the last call ...
    double retain = 0.0;         // ... and retained k-mers per instance
    double screen_ratio = 0.0;   // the distinct-per-instance ratio a screened call was decided on (what such a call reports is the table's view: the decision keeps its ratio)
    uint64_t reads = 0;          // ... over this many reads (a context) or instances of the job (a communicator) ...
    uint32_t key = 0;            // ... in this mode (snk_sizing_key)
    bool lookup(uint32_t k, uint64_t r) const { return key == k && reads == r; }       // is this the history of such a call?
    void store(uint32_t k, uint64_t r, double ratio_, double retain_ = 0.0) { key = k; reads = r; ratio = ratio_; retain = retain_; }
};

struct snk_plan_in {
    uint32_t K = 48;
    bool grouped = false;        // per-barcode groups (SNK_F_GROUPED)
    bool has_bc = false;         // the reads carry barcodes
    uint32_t min_freq = 0, min_bc = 0;
    uint32_t n_buckets = 0;      // the caller's forced bucket count (0: the rule's)
    uint64_t inst_ub = 0;        // upper bound of the job's k-mer instances
    uint32_t world = 1;          // ranks the buckets are dealt to (1 off the sharded path)
    double ratio = 0.0;          // hint: distinct k-mers per instance (history or pilot; 0 = none)
    double retain = 0.0;         // hint: retained k-mers per instance (0 = none)
    bool may_adapt = false;      // the bucket target may follow `ratio`
    const snk_opts* opts = nullptr;
    // the count kernel's geometry (snk_count_slots, snk_count_limit(K, 0, 0) = SLOTS - THREADS - 64, snk_count_screen_limit)
    uint32_t slots = 0, plain_limit = 0, screen_limit = 0;

    // ---- Where the callers differ today.  None of these differences is argued for anywhere: the rule was written three times and the
    // copies drifted.  They are kept as they are -- every caller computes what it computed -- and named, so that a later change can
    // decide each of them here.
    //                           resident (snk_dev_count_graph)   streamed (snk_dev_stream_begin)   sharded (snk_shard_step)   sharded, streamed open
    //   nb_max                  2^25                             2^23                              2^26                       2^26
    //   use_retain              yes                              no                                no                         no
    //   may_book                yes                              no                                yes                        no
    //   book_only_adapting      no                               -                                 yes                        -
    //   screen_needs_tight      no                               -                                 yes                        -
    //   fill_unclamped          no                               yes                               no                         no
    //   may_adapt               no forced bucket count or        whenever there is a ratio         as resident, without the   as sharded
    //                           target, not grouped, option      (the option adaptive_buckets      grouped clause
    //                           adaptive_buckets                 is not asked)
    // nb_max: 2^23 until round 6 everywhere: at 800 M reads that is 9700 instances per bucket, a third of the buckets split; 1.2 B reads as
    // per-barcode graphs want 23.5 M.  Raised in the resident copy only; the sharded copy had 2^26 from the start.
    uint64_t nb_max = 1ull << 25;
    bool use_retain = false;          // the retained-share rule (option chunk_kmers) takes part
    bool may_book = true;             // the call may choose booked slots and the bit filter at all: a streamed job cannot partition again and keeps the default kernel and its bucket rule
    bool book_only_adapting = false;  // ... but only where the target follows the ratio (no forced bucket count or target, may_adapt, ratio > 0), and count_tight = n is only asked "0?"
    bool screen_needs_tight = false;  // the bit filter goes on only if the ratio has chosen booked slots first (else: the filter brings booked slots with it)
    bool fill_unclamped = false;      // the bucket_fill_pct target is not cut at the default target (only matters above bucket_fill_pct = 65)
};

struct snk_plan_out {
    uint32_t NB = 0;             // buckets: a multiple of world, at least (inst_ub >> 20) + 1
    uint32_t tight = 0;          // count_tight: usable slots in the low half, tight_tries << 16; 0 = the margin kernel
    uint32_t screen = 0;         // count_screen: the filter's level, 0 = off
    uint32_t count_limit = 0;    // usable table slots of the count launches
    uint32_t target = 0;         // k-mer instances per bucket the rule aimed at (0: the bucket count was forced)
};

snk_plan_out snk_bucket_plan(const snk_plan_in& in);
