// snk_opts.h -- per-context options: every choice the library makes by itself, and every hook its tests use, is a named option of the
// CONTEXT, set through the C ABI (snk_ctx_set_tuning for the documented knobs, snk_ctx_set_option by name; SNK_TUNING="name=value,..." is
// read once when a context is created, for shell tools).  Nothing in the product path reads the process environment any more except the
// tracing switches (SNK_SYNC_TRACE, SNK_ARENA_TRACE, SNK_ARENA_POISON, SNK_INGEST_TRACE, SNK_HBV_DEPTH), SNK_RCCL_LIB and the host
// decoder's two (SNK_FASTH_LIBDEFLATE, SNK_FASTH_WHOLE_MAX_MB: no context there).
// SNK_OPTIONS is the one registry: name, default, doc, in the order snk_option_name / snk_option_doc list them.  A stage reads an option of
// the context it was handed by id (snk_opt_u32(ctx, SNK_OPT_hot)); a NULL context reads the defaults.  Names are looked up only by the
// by-name C ABI and SNK_TUNING.  Where the default depends on the data (count_tight, target_inst, msp_sigmas_x10, msp_site_records,
// chunk_merge, path_index, path_edge_cap, path_redo_cap, path_ubc_cap) the entry's 0 is never read: the call site asks snk_opt_is_set and
// chooses itself.
#pragma once
#include <stdint.h>

#define SNK_OPTIONS(X) \
    /* ---- which count kernel runs, how full its tables may get, how large a bucket is (snk_pipeline.hip, snk_shard_step.hip) */ \
    X(count_tight, 0, "count kernel with booked table slots: 0 never, n = always, n usable slots of the table (256 .. slots - 64); unset: chosen from the data") \
    X(count_screen, 1, "per-barcode groups: bit filter in front of the table: 0 off, 1 on for min_freq >= 3 (default), 2 on for min_freq >= 2") \
    X(count_screen_ng, 1, "ungrouped reads: bit filter in front of a 1024-slot table: 0 never, 1 when the tables run full (default), 2 always") \
    X(screen_ratio_pct, 30, "count_screen_ng = 1: distinct k-mers per 100 instances above which the filter goes on (30)") \
    X(screen_target, 4000, "k-mer instances per bucket behind the ungrouped filter (4000)") \
    X(tight_tries, 48, "booked slots: how often a wave looks again before it gives the pass up (48)") \
    X(target_inst, 0, "k-mer instances per minimiser bucket; unset: 5000 (K=48) / 3500 (K=60), adapted to the data") \
    X(bucket_fill_pct, 50, "adaptive buckets aim at this share of the table's usable slots (50)") \
    X(adaptive_buckets, 1, "look at the first buckets of unknown data and partition a second time if their tables run full (1)") \
    X(chunk_kmers, 180, "retained k-mers per bucket the bucket count aims at when the data retain many (180)") \
    X(count_persist, 32, "residency waves of count workgroups (32)") \
    X(input_fp, 1, "fingerprint the reads so that other data of the same size do not inherit sizing history (1)") \
    X(pilot_est, 1, "size the count regions from the pilot launch (1)") \
    X(minimiser_len, 0, "16 or 20: overrides SNK_F_LONG_MINIMISER (tools, tests)") \
    X(global_graph, 0, "1: the global graph stage (as SNK_F_GLOBAL_GRAPH)") \
    /* ---- partition */ \
    X(partition_passes, 0, "bucket-range passes of the partition: 0 = as many as the device needs (default)") \
    X(msp_cap_pct, 100, "bucket slot capacity in percent of the occupancy model's (100; tests shrink it to force the overflow segment)") \
    X(msp_sigmas_x10, 0, "bucket slot capacity = mean + this/10 sigma of the occupancy model; unset: 5, or 3 / 1.5 when the slots would take more than 30 % of the device") \
    X(msp_site_records, 0, "supermers per minimiser site in the occupancy model (48; groups 3)") \
    X(msp_dense, 0, "1: reservation-free partition (dense records + sorted index list)") \
    X(msp_hot_factor, 32, "a bucket is noted hot at this multiple of its capacity (32)") \
    X(msp_hot_min, 4096, "... and at least this many reservations (4096)") \
    X(trim_fused, 1, "quality trim inside the partition kernel (1)") \
    X(trim_rowwise, 0, "1: the row-wise trim kernel for every layout") \
    X(defer_compact, 1, "leave the count regions in place until the prune reads them (1)") \
    /* ---- hot minimiser buckets */ \
    X(hot, 1, "re-partition hot minimiser buckets by k-mer hash (1)") \
    X(hot_min, 8192, "a bucket is hot above this many records (8192) ...") \
    X(hot_factor, 8, "... and this multiple of the slot capacity (8)") \
    X(hot_class_inst, 6000, "k-mer instances per hash class of a hot bucket (6000)") \
    /* ---- bucket-local graph, join */ \
    X(chunk_merge, 0, "graph chunks are merged up to this many k-mers (256; 0 off)") \
    X(bl_cpw, 4, "graph chunks per workgroup of the prune (4)") \
    X(bl_index_fused, 1, "boundary index built by the prune (1)") \
    X(bl_noclassify, 0, "1: every miss of the prune is pending (no neighbour classification)") \
    X(bl_pool, 4096, "slots of the in-chunk circle pool (4096; 0 forces the exact re-run)") \
    X(split_log2, 5, "log2 of the ranking's splitter spacing + 1 (5)") \
    X(rank_wyllie, 0, "1: plain pointer jumping instead of the sparse ruling set") \
    X(emit_grid_log2, 22, "log2 of the largest grid of the join's fragment copy (22; tests make it small: the kernel strides)") \
    X(lean_cold, 1, "0: a context whose arena has not mapped the memory yet still sizes its record slots at 5 sigma (1: 1.5 sigma until the arena has the slack)") \
    X(plan_mem_mb, 0, "the memory (MB) the slot / pass / region plans of a call divide instead of what the device has free (tests: bucket-range passes and their region probe at fixture size)") \
    X(hbv_huge_pages, 1, "0: the host tables of a14's flood are plain malloc memory (1: 2-MB aligned with MADV_HUGEPAGE)") \
    X(hbv_short_queue, 1, "0: the host flood of a14 prefetches 16 / 8 / 4 queue places ahead only (1: also at push time and one / two places ahead: the bulk of a genome graph has a short queue)") \
    X(join_dbg, 0, "1: the join counts the bytes of its unitig buffers that nothing wrote (stderr; debugging aid)") \
    X(rank_round_batch, 8, "jumping rounds per read-back, sharded ranking (8)") \
    X(rank_round_batch0, 12, "jumping rounds before the first read-back, one-GPU ranking (12)") \
    /* ---- sharded step */ \
    X(exchange_ranges, 4, "bucket ranges of the record exchange (4)") \
    X(join_replicated, 0, "1: replicated list ranking instead of the partitioned one") \
    X(dbg_fake_segs, 0, "count kernel: see the slots as this many record segments (measurement of the N-rank read pattern)") \
    /* ---- read pathing, duplicates, HBV */ \
    X(path_index, 0, "look-ups through the minimiser index: 1 always, 0 never; unset: when the k-mer dictionary does not fit") \
    X(path_dict_max_kb, 0, "a k-mer dictionary above this size 'does not fit' (tests)") \
    X(path_slots_x10, 30, "dictionary slots per unitig k-mer x 10 (30; at least 11: the table must keep free slots)") \
    X(path_two_pass, 1, "second pass with 16 lanes per read (1)") \
    X(path_fast_gs, 8, "lanes per read of the first pass (8)") \
    X(path_fused, 0, "1: one kernel for both passes") \
    X(path_redo_all, 0, "1: every read takes the second pass (tests)") \
    X(path_fp_mask, 0, "mask of the dictionary's fingerprints (tests: collisions)") \
    X(path_edge_cap, 0, "first capacity of the pather's list of second and later path edges (tests: the re-run with a longer list; unset: n/4 + 65536)") \
    X(path_redo_cap, 0, "first capacity of the pather's list of reads for the full-capacity pass (tests: the re-run; unset: n/64 + 65536)") \
    X(path_ubc_cap, 0, "first capacity of the (unitig, barcode) keys beyond a read's first (tests: the re-run; unset: n/4 + 65536)") \
    X(path_idx_dbg, 0, "index look-up debug mode") \
    X(unitig_bc_cut, 20000, "entries a unitig's barcode list is cut at (20000)") \
    X(dups_two_sorts, 0, "1: the two-pass sort of MarkDups") \
    X(hbv_dev_min, 65536, "graphs below this many unitigs take the host id hand-out (65536)") \
    X(hbv_big, 1024, "components above this many nodes take the host flood (1024)") \
    X(hbv_strict, 0, "1: fail instead of falling back when the device flood gives up") \
    X(df_stream, 0, "stage-input files -> unitigs: 2 = through a streamed job (the reads never resident in any form); else the compact resident form (rows + good lengths + barcode ids, the adaptive resident step)") \
    /* ---- memory */ \
    X(arena_vmm, 1, "growing virtual-memory arena (1); 0 = cached hipMalloc blocks") \
    /* ---- kernel debug modes (results invalid unless stated) */ \
    X(count_dbg, 0, "count kernel probe mode") \
    X(msp_dbg, 0, "partition kernel probe mode") \
    X(overlap_probe, 0, "builds with -DSNK_PROBES: a second kernel next to the count kernel (tools/overlap_probe*.py)") \
    X(overlap_probe_dbg, 0, "... which one")

enum snk_opt_id : int {
#define X(name, dflt, doc) SNK_OPT_##name,
    SNK_OPTIONS(X)
#undef X
    SNK_OPT_COUNT
};
struct snk_opts {
    long long v[SNK_OPT_COUNT];
    bool set[SNK_OPT_COUNT];
};
struct snk_opt_def { const char* name; long long dflt; const char* doc; };
extern const snk_opt_def snk_opt_defs[SNK_OPT_COUNT];
int snk_opt_index(const char* name);                 // -1: no such option
void snk_opts_init(snk_opts* o);                     // nothing set
int snk_opts_parse(snk_opts* o, const char* text, char* bad, unsigned badcap);      // "name=value,name=value"; 0 ok, else the offending item in `bad`
bool snk_opt_valid(int id, long long value);         // the option's range (path_slots_x10: at least 11); every setter refuses what lies outside
// the context's value if it set one, else the registry's default (ctx NULL: the defaults)
struct snk_ctx;
bool snk_opt_is_set(const snk_ctx* ctx, snk_opt_id id);
uint32_t snk_opt_u32(const snk_ctx* ctx, snk_opt_id id);
unsigned long long snk_opt_u64(const snk_ctx* ctx, snk_opt_id id);
