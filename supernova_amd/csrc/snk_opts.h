// snk_opts.h -- per-context options: every choice the library makes by itself, and every hook its tests use, is a named option of the
// CONTEXT, set through the C ABI (snk_ctx_set_tuning for the documented knobs, snk_ctx_set_option by name; SNK_TUNING="name=value,..." is
// read once when a context is created, for shell tools).  Nothing in the product path reads the process environment any more except the
// tracing switches (SNK_SYNC_TRACE, SNK_ARENA_TRACE, SNK_ARENA_POISON, SNK_INGEST_TRACE, SNK_HBV_DEPTH), SNK_RCCL_LIB and the host
// decoder's two (SNK_FASTH_LIBDEFLATE, SNK_FASTH_WHOLE_MAX_MB: no context there).
// SNK_OPTIONS is the one registry: name, default, range, doc, in the order snk_option_name / snk_option_doc list them.  A stage reads an
// option of the context it was handed by id (snk_opt_u32(ctx, SNK_OPT_hot)); a NULL context reads the defaults.  Names are looked up only
// by the by-name C ABI and SNK_TUNING.  Where the default depends on the data (count_tight, target_inst, msp_sigmas_x10, msp_site_records,
// chunk_merge, path_index, path_edge_cap, path_redo_cap, path_ubc_cap) the entry's 0 is never read: the call site asks snk_opt_is_set and
// chooses itself.
// The range is what every setter accepts (snk_opt_valid: snk_ctx_set_option, snk_option_check, SNK_TUNING, snk_ctx_set_tuning).  It comes
// from the call sites: no value a setter lets through is undefined, divides by zero, skips work or loses bits there.  snk_option_doc
// shows it in brackets behind the text.  The forms:
//   SNK_SW              a switch, 0 or 1
//   SNK_R(lo, hi)       lo .. hi
//   SNK_R0(lo, hi)      0 (off / never), or lo .. hi
//   SNK_RS(lo, hi, s)   lo, lo + s, ... hi;  SNK_RS0: the same, or 0
// Nothing is negative, and nothing goes above SNK_U32 (most options are read through snk_opt_u32, which would cut it to 32 bits).
#pragma once
#include <stdint.h>

#define SNK_SW 0, 1, 1, false
#define SNK_R(lo, hi) lo, hi, 1, false
#define SNK_R0(lo, hi) lo, hi, 1, true
#define SNK_RS(lo, hi, step) lo, hi, step, false
#define SNK_RS0(lo, hi, step) lo, hi, step, true
#define SNK_U32 4294967295ll

#define SNK_OPTIONS(X) \
    /* ---- which count kernel runs, how full its tables may get, how large a bucket is (snk_pipeline.hip, snk_shard_step.hip) */ \
    /* (1984 = the 2048 LDS table slots of snk_count.hip - 64; the one-GPU call site clamps to the build's slots, the sharded one only asks "0?") */ \
    X(count_tight, 0, SNK_R0(256, 1984), "count kernel with booked table slots: 0 never, n = always, n usable slots of the table (256 .. slots - 64); unset: chosen from the data") \
    X(count_screen, 1, SNK_R(0, 2), "per-barcode groups: bit filter in front of the table: 0 off, 1 on for min_freq >= 3 (default), 2 on for min_freq >= 2") \
    X(count_screen_ng, 1, SNK_R(0, 2), "ungrouped reads: bit filter in front of a 1024-slot table: 0 never, 1 when the tables run full (default), 2 always") \
    X(screen_ratio_pct, 30, SNK_R(0, 100), "count_screen_ng = 1: distinct k-mers per 100 instances above which the filter goes on (30)") \
    /* (bucket targets divide the instance count: at least the ~100 instances of one read, at most the 2^20 one workgroup is handed) */ \
    X(screen_target, 4000, SNK_R(100, 1048576), "k-mer instances per bucket behind the ungrouped filter (4000)") \
    /* (the count rides in the high half of the 32-bit word whose low half is the slot limit) */ \
    X(tight_tries, 48, SNK_R(1, 65535), "booked slots: how often a wave looks again before it gives the pass up (48)") \
    X(target_inst, 0, SNK_R(100, 1048576), "k-mer instances per minimiser bucket; unset: 5000 (K=48) / 3500 (K=60), adapted to the data") \
    X(bucket_fill_pct, 50, SNK_R(1, 100), "adaptive buckets aim at this share of the table's usable slots (50)") \
    X(adaptive_buckets, 1, SNK_SW, "look at the first buckets of unknown data and partition a second time if their tables run full (1)") \
    X(chunk_kmers, 180, SNK_R(1, 65536), "retained k-mers per bucket the bucket count aims at when the data retain many (180)") \
    X(count_persist, 32, SNK_R(0, 1024), "residency waves of count workgroups (32; 0 = 1)") \
    X(input_fp, 1, SNK_SW, "fingerprint the reads so that other data of the same size do not inherit sizing history (1)") \
    X(pilot_est, 1, SNK_SW, "size the count regions from the pilot launch (1)") \
    X(minimiser_len, 0, SNK_RS0(16, 20, 4), "16 or 20: overrides SNK_F_LONG_MINIMISER (tools, tests)") \
    X(global_graph, 0, SNK_SW, "1: the global graph stage (as SNK_F_GLOBAL_GRAPH)") \
    /* ---- partition */ \
    X(partition_passes, 0, SNK_R(0, 64), "bucket-range passes of the partition: 0 = as many as the device needs (default)") \
    X(msp_cap_pct, 100, SNK_R(1, 100), "bucket slot capacity in percent of the occupancy model's (100; tests shrink it to force the overflow segment)") \
    X(msp_sigmas_x10, 0, SNK_R(0, 100), "bucket slot capacity = mean + this/10 sigma of the occupancy model; unset: 5, or 3 / 1.5 when the slots would take more than 30 % of the device") \
    X(msp_site_records, 0, SNK_R(1, 65536), "supermers per minimiser site in the occupancy model (48; groups 3)") \
    X(msp_dense, 0, SNK_SW, "1: reservation-free partition (dense records + sorted index list)") \
    X(msp_hot_factor, 32, SNK_R(0, 65536), "a bucket is noted hot at this multiple of its capacity (32; 0 never)") \
    X(msp_hot_min, 4096, SNK_R(1, SNK_U32), "... and at least this many reservations (4096)") \
    X(trim_fused, 1, SNK_SW, "quality trim inside the partition kernel (1)") \
    X(trim_rowwise, 0, SNK_SW, "1: the row-wise trim kernel for every layout") \
    X(defer_compact, 1, SNK_SW, "leave the count regions in place until the prune reads them (1)") \
    /* ---- hot minimiser buckets */ \
    X(hot, 1, SNK_SW, "re-partition hot minimiser buckets by k-mer hash (1)") \
    X(hot_min, 8192, SNK_R(1, SNK_U32), "a bucket is hot above this many records (8192) ...") \
    X(hot_factor, 8, SNK_R(1, 65536), "... and this multiple of the slot capacity (8)") \
    X(hot_class_inst, 6000, SNK_R(100, 1048576), "k-mer instances per hash class of a hot bucket (6000)") \
    /* ---- bucket-local graph, join */ \
    X(chunk_merge, 0, SNK_R(0, 65536), "graph chunks are merged up to this many k-mers (256, which is also the most; 0 off)") \
    X(bl_cpw, 4, SNK_R(1, 1024), "graph chunks per workgroup of the prune (4)") \
    X(bl_index_fused, 1, SNK_SW, "boundary index built by the prune (1)") \
    X(bl_noclassify, 0, SNK_SW, "1: every miss of the prune is pending (no neighbour classification)") \
    X(bl_pool, 4096, SNK_R(0, 1048576), "slots of the in-chunk circle pool (4096; 0 forces the exact re-run)") \
    /* (snk_rank.hip: sampled_state makes a state a splitter when the low split_log2 bits of a 25-bit hash are zero, and a splitter's walk to the  \
       next one is one thread's serial work: 2^12 dependent loads on average at 12; a circle that drew no splitter is walked in full  \
       by each of its odd states, quadratic in the spacing.  At 0 every state is a splitter: pointer jumping over all states with three \
       times its memory, which rank_wyllie does better.  From 32 on the mask's shift is undefined.) */ \
    X(split_log2, 5, SNK_R(1, 12), "log2 of the ranking's splitter spacing (5: one state in 32)") \
    X(rank_wyllie, 0, SNK_SW, "1: plain pointer jumping instead of the sparse ruling set") \
    X(emit_grid_log2, 22, SNK_R(0, 22), "log2 of the largest grid of the join's fragment copy (22; tests make it small: the kernel strides)") \
    X(lean_cold, 1, SNK_SW, "0: a context whose arena has not mapped the memory yet still sizes its record slots at 5 sigma (1: 1.5 sigma until the arena has the slack)") \
    X(plan_mem_mb, 0, SNK_R(0, 16777216), "the memory (MB) the slot / pass / region plans of a call divide instead of what the device has free (tests: bucket-range passes and their region probe at fixture size)") \
    X(hbv_huge_pages, 1, SNK_SW, "0: the host tables of a14's flood are plain malloc memory (1: 2-MB aligned with MADV_HUGEPAGE)") \
    X(hbv_short_queue, 1, SNK_SW, "0: the host flood of a14 prefetches 16 / 8 / 4 queue places ahead only (1: also at push time and one / two places ahead: the bulk of a genome graph has a short queue)") \
    X(join_dbg, 0, SNK_SW, "1: the join counts the bytes of its unitig buffers that nothing wrote (stderr; debugging aid)") \
    /* (a batch of 0 rounds reports "nothing changed" without having looked; 2^32 splitters converge in 33 rounds) */ \
    X(rank_round_batch, 8, SNK_R(1, 64), "jumping rounds per read-back, sharded ranking (8)") \
    X(rank_round_batch0, 12, SNK_R(1, 64), "jumping rounds before the first read-back, one-GPU ranking (12)") \
    /* ---- sharded step */ \
    X(exchange_ranges, 4, SNK_R(1, 64), "bucket ranges of the record exchange (4; never more than a rank has buckets)") \
    X(join_replicated, 0, SNK_SW, "1: replicated list ranking instead of the partitioned one") \
    X(dbg_fake_segs, 0, SNK_R(0, 32), "count kernel: see the slots as this many record segments (measurement of the N-rank read pattern)") \
    /* ---- read pathing, duplicates, HBV */ \
    X(path_index, 0, SNK_SW, "look-ups through the minimiser index: 1 always, 0 never; unset: when the k-mer dictionary does not fit") \
    X(path_dict_max_kb, 0, SNK_R(0, SNK_U32), "a k-mer dictionary above this size 'does not fit' (tests)") \
    /* (the dictionary gets nk * x / 10 + 1024 slots for nk unitig k-mers, and its insertion probes until it finds a free one: below 11 there may be none) */ \
    X(path_slots_x10, 30, SNK_R(11, 1000), "dictionary slots per unitig k-mer x 10 (30; at least 11: the table must keep free slots)") \
    X(path_two_pass, 1, SNK_SW, "second pass with 16 lanes per read (1)") \
    /* (the two lane counts the first pass is instantiated for; 0 = 16: "no fast pass", as callers have always been able to say) */ \
    X(path_fast_gs, 8, SNK_RS0(8, 16, 8), "lanes per read of the first pass: 8 = the fast first pass, 16 or 0 = the second pass's kernel first (8)") \
    X(path_fused, 0, SNK_SW, "1: one kernel for both passes") \
    X(path_redo_all, 0, SNK_SW, "1: every read takes the second pass (tests)") \
    X(path_fp_mask, 0, SNK_R(0, 1073741823), "mask of the dictionary's 30-bit fingerprints (tests: collisions; 0 = all of them)") \
    X(path_edge_cap, 0, SNK_R(0, SNK_U32), "first capacity of the pather's list of second and later path edges (tests: the re-run with a longer list; unset: n/4 + 65536)") \
    X(path_redo_cap, 0, SNK_R(0, SNK_U32), "first capacity of the pather's list of reads for the full-capacity pass (tests: the re-run; unset: n/64 + 65536)") \
    X(path_ubc_cap, 0, SNK_R(0, SNK_U32), "first capacity of the (unitig, barcode) keys beyond a read's first (tests: the re-run; unset: n/4 + 65536)") \
    X(path_idx_dbg, 0, SNK_R(0, 255), "index look-up debug mode") \
    X(unitig_bc_cut, 20000, SNK_R(1, SNK_U32), "entries a unitig's barcode list is cut at (20000)") \
    X(dups_two_sorts, 0, SNK_SW, "1: the two-pass sort of MarkDups") \
    X(hbv_dev_min, 65536, SNK_R(0, SNK_U32), "graphs below this many unitigs take the host id hand-out (65536)") \
    X(hbv_big, 1024, SNK_R(0, SNK_U32), "components above this many nodes take the host flood (1024)") \
    X(hbv_strict, 0, SNK_SW, "1: fail instead of falling back when the device flood gives up") \
    X(df_stream, 0, SNK_R(0, 2), "stage-input files -> unitigs: 2 = through a streamed job (the reads never resident in any form); else the compact resident form (rows + good lengths + barcode ids, the adaptive resident step)") \
    /* ---- memory */ \
    X(arena_vmm, 1, SNK_SW, "growing virtual-memory arena (1); 0 = cached hipMalloc blocks") \
    /* ---- kernel debug modes (results invalid unless stated) */ \
    X(count_dbg, 0, SNK_R(0, 255), "count kernel probe mode") \
    X(msp_dbg, 0, SNK_R(0, 255), "partition kernel probe mode") \
    X(overlap_probe, 0, SNK_R(0, 255), "builds with -DSNK_PROBES: a second kernel next to the count kernel (tools/overlap_probe*.py)") \
    X(overlap_probe_dbg, 0, SNK_R(0, 255), "... which probe")

enum snk_opt_id : int {
#define X(name, dflt, range, doc) SNK_OPT_##name,
    SNK_OPTIONS(X)
#undef X
    SNK_OPT_COUNT
};
struct snk_opts {
    long long v[SNK_OPT_COUNT];
    bool set[SNK_OPT_COUNT];
};
struct snk_opt_def { const char* name; long long dflt; long long lo, hi, step; bool zero; const char* doc; };      // lo, lo + step, ... hi; zero: and 0
extern const snk_opt_def snk_opt_defs[SNK_OPT_COUNT];
int snk_opt_index(const char* name);                 // -1: no such option
void snk_opts_init(snk_opts* o);                     // nothing set
int snk_opts_parse(snk_opts* o, const char* text, char* bad, unsigned badcap);      // "name=value,name=value"; 0 ok, else the offending item in `bad`
bool snk_opt_valid(int id, long long value);         // the option's range; every setter refuses what lies outside
const char* snk_opt_doc(int id);                     // the registry's text and, in brackets, the range
// the value that was set, else the registry's default: over a set of options (host code without HIP: snk_opts.hip with SNK_OPTS_NO_CTX) ...
bool snk_opts_is_set(const snk_opts& o, snk_opt_id id);
unsigned long long snk_opts_u64(const snk_opts& o, snk_opt_id id);
inline uint32_t snk_opts_u32(const snk_opts& o, snk_opt_id id) { return (uint32_t)snk_opts_u64(o, id); }
// ... and over a context's (ctx NULL: the defaults)
struct snk_ctx;
bool snk_opt_is_set(const snk_ctx* ctx, snk_opt_id id);
uint32_t snk_opt_u32(const snk_ctx* ctx, snk_opt_id id);
unsigned long long snk_opt_u64(const snk_ctx* ctx, snk_opt_id id);
