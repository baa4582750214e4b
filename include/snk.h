/* snk.h -- C ABI of libsnk: MI355X-native k-mer count + de Bruijn unitig graph (Supernova hot path).
 *
 * This is the drop-in boundary of SURVEY.md section 8(b), row b5.  The reference has no C ABI on this
 * path; its seams are
 *   - the C++ entry  buildReadQGraph48(...)            lib/assembly/src/paths/long/BuildReadQGraph48.h:24-34
 *   - its tail       buildHBVFromEdges(...)            lib/assembly/src/paths/long/HBVFromEdges.h:27-28
 *   - the unitig hand-off file (.bv) tada -> DF        lib/tada/src/debruijn.rs:895-929,
 *                                                      lib/assembly/src/paths/long/BuildReadQGraph48.cc:1640-1642
 *   - the stage argv/MRO contracts (ASSEMBLER_DF, MSP/SHARD_ASM/MAIN_ASM_SN)
 *                                                      mro/_assembler_stages.mro:24-39, lib/tada/mro/_asm_stages.mro:53-80
 * Every entry point below names the reference interface it replaces.  Plain pointers and sizes only.
 *
 * Conventions
 *   - return value: 0 = SNK_OK, negative = error; the message is left in the caller's `err` buffer
 *     (NUL terminated, truncated to errcap) and is also retrievable with snk_last_error().
 *   - base codes A=0 C=1 G=2 T=3; every non-ACGT input character maps to A
 *     (lib/tada/src/kmer/mod.rs:311-319, lib/assembly/src/10X/ParseBarcodedFastqs.cc:87-88).
 *   - packed read rows: `row_words` u32 words per read, base i of a read in word i>>4, bits
 *     31-2*(i&15)..30-2*(i&15) (MSB first; the same order as KMer<K>'s storage words, kmers/KMer.h:153-160).
 *   - k-mer keys are 4 u32 words MSB-first (K=48 uses words 0..2, word 3 = 0; K=60 uses all four with
 *     the low 8 bits of word 3 zero); lexicographic order on words == order on bases (KMer.h:305-311).
 *   - context byte = pred one-hot << 4 | succ one-hot in the k-mer's canonical orientation
 *     (kmers/KMerContext.h:27-28), after the adjacency prune (kmers/ReadPather.h:346-385).
 *   - barcode ids: int32 per read, 0 = no barcode, -1 = "ignore the barcode rule for this read"
 *     (BuildReadQGraph48.cc:108-114,158-159), >0 = barcode ordinal.
 *   - "dev" entry points take device pointers (HBM resident) and a hipStream_t passed as void*.
 */
#ifndef SNK_H_
#define SNK_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNK_OK 0
#define SNK_E_ARG (-1)      /* bad argument */
#define SNK_E_HIP (-2)      /* HIP runtime error (message carries hipGetErrorString) */
#define SNK_E_NOGPU (-3)    /* no gfx950 device visible: the product path never falls back to the CPU */
#define SNK_E_NOMEM (-4)    /* device/host allocation failed (adapter maps it to exit 99, system/RunTime.cc:195-221) */
#define SNK_E_IO (-5)
#define SNK_E_UNSUPPORTED (-6)
#define SNK_E_INTERNAL (-7)

typedef struct snk_ctx snk_ctx; /* one per process per GPU: owns streams, arena, scratch */

/* thresholds of the path; defaults = CS-build constants K=48 MIN_FREQ=3 MIN_BC=2 MIN_QUAL=7
 * (lib/assembly/src/10X/DF.cc:138-141,181-184; mro/_assembler.mro:44; lib/tada/mro/_asm_sn.mro:15) */
typedef struct snk_params {
    uint32_t K;            /* 48 or 60 */
    uint32_t min_qual;     /* 7 */
    uint32_t min_freq;     /* 3 */
    uint32_t min_bc;       /* 0..8 distinct barcodes a k-mer needs (2 = reference default; the count kernel tells up to eight apart
                              per k-mer in LDS: > 8 is SNK_E_UNSUPPORTED) */
    uint32_t n_buckets;    /* 0 = choose from the k-mer instance count */
    uint32_t flags;        /* SNK_F_* */
} snk_params;
#define SNK_F_NO_GRAPH 1u      /* stop after the retained k-mer table (count only) */
#define SNK_F_UNSORTED_TABLE 2u /* leave the retained table in bucket order (the reference's dictionary is an unordered
                                  hash set, kmers/ReadPather.h:189-245); default: keys ascending */
#define SNK_F_GROUPED 8u        /* per-group graphs (BASELINE config 5: per-barcode local graphs): reads carry a group id
                                  (snk_dev_reads.group); k-mers are counted, pruned and walked per (group, k-mer); every
                                  unitig reports its group.  K=48, frequency rule only.  The group id is returned in the
                                  32 low bits of every key. */
#define SNK_F_NO_TABLE 16u      /* snk_count_graph (host pointers): do not download the retained table (kmers/counts/ctx stay
                                  NULL, n_kmers is still reported) -- callers at the .bv seam only need the unitigs */
#define SNK_F_BV_IMAGE 32u      /* snk_count_graph (host pointers): return the unitigs as the bytes of the .bv hand-off file
                                   (snk_result.bv_image, packed on the device) instead of unitig_off / unitig_bases */
#define SNK_F_LONG_MINIMISER 64u /* minimisers of 20 bases instead of 16: for genomes whose minimiser sites outnumber the 2.1 G canonical 16-mers
                                   (human: 3.1 G) -- sites that share a minimiser share a bucket, and at 1-2 sites per value the step loses
                                   5-25 %.  11 % more supermers: slower on small genomes.  Same results, bit for bit. */
#define SNK_F_GLOBAL_GRAPH 4u   /* use the global graph stage (sort + HBM index + list ranking over all k-mers) instead
                                  of the bucket-local one; same results, kept as a cross-check */

const char* snk_version(void);
const char* snk_last_error(void);
void snk_params_default(snk_params* p);

/* ---- context ------------------------------------------------------------------------------------ */
int snk_ctx_create(int device, snk_ctx** out, char* err, size_t errcap);
void snk_ctx_destroy(snk_ctx* ctx);
/* Give the context's cached, currently unused device memory back to the device (results of the last call stay valid).  The
 * context keeps its scratch between calls so that a steady stream of equal-sized calls never allocates; a caller that shares
 * the GPU with another allocator calls this when it changes problem size.  Blocks unused for two calls are dropped anyway. */
void snk_ctx_trim(snk_ctx* ctx);
/* Map `bytes` of device memory into the context's scratch arena now and keep that much mapped between calls (until snk_ctx_trim).  A call
 * that needs more scratch than the context has mapped so far pays the driver for the new memory inside the call (~25-30 ms per GB: 100 M
 * error-rich reads after 100 M clean ones: +20 GB, 745 instead of 228 ms for that one call); a host that owns the GPU reserves its share
 * once, at start-up.  Returns SNK_E_NOMEM when the device cannot give that much (what could be mapped stays usable).  The reservation
 * outlives the arena's own resets (a sealed range, a shrink after much larger calls): it is mapped again at the start of the next call; only a
 * multi-rank step (plain device blocks for the xGMI buffers) runs without it, and the call after that step maps it again. */
int snk_ctx_reserve(snk_ctx* ctx, uint64_t bytes, char* err, size_t errcap);

/* ---- tuning (round 6) ------------------------------------------------------------------------------------------------------------
 * Every choice the library makes by itself -- which count kernel runs, how large a minimiser bucket is, how many partition passes, the
 * minimiser length, the thresholds of the hot-bucket path, how reads are looked up -- can be pinned per context, and read back together
 * with what the context's last call chose.  Nothing on the product path reads the process environment (tracing switches aside); a Martian
 * stage sets what it wants here and logs snk_ctx_get_tuning.  A zero field = the library's own choice.  Results never depend on any of it.
 * The long tail (test hooks, probe modes) is reachable by name: snk_ctx_set_option / snk_option_name enumerate them with a one-line
 * description each; SNK_TUNING="name=value,name=value" in the environment is applied once, when a context is created (shell tools). */
#define SNK_COUNT_KERNEL_AUTO 0u     /* from the data: the distinct-k-mers-per-instance ratio of the first buckets / the previous call */
#define SNK_COUNT_KERNEL_MARGIN 1u   /* 1216 of 2048 table slots usable, no bookkeeping (clean, deep data: the bench's operating point) */
#define SNK_COUNT_KERNEL_BOOKED 2u   /* waves book their slots: count_tight_slots (1920) usable -- error-rich reads, per-barcode groups */
#define SNK_COUNT_KERNEL_SCREEN 3u   /* bit filter in front of a 1024-slot table with booked slots -- reads whose k-mers are mostly singletons */
typedef struct snk_tuning {
    uint32_t count_kernel;            /* SNK_COUNT_KERNEL_* */
    uint32_t count_tight_slots;       /* BOOKED: usable slots (256 .. 1984), 0 = 1920 */
    uint32_t count_screen_ratio_pct;  /* AUTO: the filter goes on above this many distinct k-mers per 100 instances (0 = 30) */
    uint32_t target_inst;             /* k-mer instances per minimiser bucket (0 = 5000 at K=48 / 3500 at K=60, adapted to the data) */
    uint32_t bucket_fill_pct;         /* adaptive buckets aim at this share of the usable slots (0 = 50) */
    uint32_t adaptive_buckets;        /* 0 default (on), 1 on, 2 off: look at the first buckets of unknown data, partition again if their tables run full */
    uint32_t chunk_kmers;             /* retained k-mers per bucket aimed at when the data retain many (0 = 180) */
    uint32_t minimiser_len;           /* 0 = from snk_params.flags (SNK_F_LONG_MINIMISER), else 16 | 20 */
    uint32_t partition_passes;        /* bucket-range passes (0 = as many as the device needs) */
    uint32_t hot_buckets;             /* 0 default (on), 1 on, 2 off: re-partition hot minimiser buckets by k-mer hash */
    uint32_t hot_min, hot_factor, hot_class_inst;   /* 0 = 8192 records, 8 x the slot capacity, 6000 instances per class */
    uint32_t exchange_ranges;         /* sharded step: bucket ranges of the record exchange (0 = 4) */
    uint32_t join_ranking;            /* sharded step: 0 default (partitioned), 1 partitioned, 2 replicated */
    uint32_t path_lookup;             /* read pathing: 0 = dictionary when it fits, 1 minimiser index, 2 dictionary */
    uint32_t unitig_bc_cut;           /* entries a unitig's barcode list is cut at (0 = 20000, cmd_main_asm.rs:115) */
    uint32_t hbv_dev_min, hbv_big;    /* graph ids: below hbv_dev_min unitigs (0 = 65536) / above hbv_big nodes per component (0 = 1024) on the host */
    uint32_t reserved[9];
    /* filled by snk_ctx_get_tuning: what the context's last call ran with */
    uint32_t last_count_kernel, last_count_limit, last_partition_passes, last_minimiser_len;
} snk_tuning;
void snk_tuning_default(snk_tuning* t);
int snk_ctx_set_tuning(snk_ctx* ctx, const snk_tuning* t, char* err, size_t errcap);
void snk_ctx_get_tuning(const snk_ctx* ctx, snk_tuning* t);
int snk_ctx_set_option(snk_ctx* ctx, const char* name, long long value, char* err, size_t errcap);   /* SNK_E_ARG: no such option, or a value out of its range (snk_option_doc ends with it) */
int snk_option_check(const char* name, long long value, char* err, size_t errcap);                    /* no context: would snk_ctx_set_option take it? */
int snk_ctx_clear_option(snk_ctx* ctx, const char* name);                    /* NULL: every option back to the library's choice */
int snk_ctx_get_option(const snk_ctx* ctx, const char* name, long long* value);   /* 1 set, 0 not set, < 0 no such option */
const char* snk_option_name(uint32_t i);                                      /* NULL past the last one */
const char* snk_option_doc(uint32_t i);                                       /* "... [lo..hi]", "[0 or lo..hi]", "[lo..hi step s]": what the setters accept */

/* ---- synthetic linked reads; counter-based, bit-identical host vs device ---------- */
typedef struct snk_synth_params {
    uint64_t seed;
    uint64_t n_reads;          /* total reads of the data set (pairs are reads 2q, 2q+1) */
    uint64_t genome_len;       /* 0 -> n_reads*read_len/56 (56x coverage)              */
    uint32_t read_len;         /* 150 */
    uint32_t mol_len;          /* 50000 (clamped to genome_len) */
    uint32_t mols_per_bc;      /* 10 */
    uint32_t pairs_per_bc;     /* 400 (=> 800 reads per barcode) */
    uint32_t insert_min;       /* 300 */
    uint32_t insert_span;      /* 101 (insert uniform in [300,400]) */
    uint32_t sub_ppm;          /* substitution probability per base, parts per million (2000) */
    uint32_t unbarcoded_ppm;   /* pairs with bc=0 (20000) */
    uint32_t lowq_tail_ppm;    /* reads with a Q2 tail (50000) */
    uint32_t tail_max;         /* tail length uniform in [0,tail_max] (40) */
    uint32_t err_cdf[4];       /* filled by snk_synth_default: P(#errors<=j)*2^32 for j=0..3 (snk_synth_set_errors refills it) */
    uint32_t repeat_mode;      /* 0: i.i.d. uniform genome.  Bit mask (15 = all) of a repeat-rich genome, every structure a pure function of the
                                  position (csrc/snk_synth.h): bit 0 four interspersed families (a 300-bp element in 60 % of the 4-kb
                                  blocks, 1-3 % divergence from its consensus: ~10^4 copies each at the bench's genome size), bit 1 5-kb
                                  segmental duplications (exact copies, one in four odd 64-kb superblocks), bit 2 short tandem repeats
                                  (unit 1-6 bp, 40-200 bp, 3 % of the blocks), bit 3 poly-A runs (20-80 bp, 2 %); bit 4 (16, not part of 15): every
                                  fifth base is A -- a minimiser space as crowded as a human genome's at a fraction of its size */
    uint32_t reserved[3];
} snk_synth_params;
/* substitution rate of the model: sub_ppm and the error-count table that goes with it */
void snk_synth_set_errors(snk_synth_params* sp, uint32_t sub_ppm);
void snk_synth_default(snk_synth_params* sp, uint64_t n_reads, uint64_t seed, int error_free);
/* host generator: reads [first, first+n).  rows: n*row_words u32; quals: n*qstride bytes (raw phred);
 * bc: n int32.  Any output pointer may be NULL. */
int snk_synth_host(const snk_synth_params* sp, uint64_t first, uint64_t n, uint32_t* rows, uint32_t row_words,
                   uint8_t* quals, uint32_t qstride, int32_t* bc);
int snk_synth_dev(snk_ctx* ctx, const snk_synth_params* sp, uint64_t first, uint64_t n, void* d_rows,
                  uint32_t row_words, void* d_quals, uint32_t qstride, void* d_bc, void* stream);


/* ---- device-resident path -------------------------------------------------------------------------- */
/* K1: replaces GoodLenTailFinder (BuildReadQGraph48.cc:65-89) / find_trim_len (lib/tada/src/cmd_msp.rs:129-146).
 * d_quals: n_reads rows of qstride bytes (raw phred, no +33); d_lens: u16 per read or NULL (= read_len);
 * d_good_len: u16 per read out. */
int snk_dev_trim(snk_ctx* ctx, const void* d_quals, uint32_t qstride, const void* d_lens, uint32_t read_len,
                 uint64_t n_reads, uint32_t K, uint32_t min_qual, void* d_good_len, void* stream);
/* K2: replaces base_to_bits (lib/tada/src/kmer/mod.rs:311-319): ASCII rows -> packed 2-bit rows. */
int snk_dev_pack_ascii(snk_ctx* ctx, const void* d_ascii, uint32_t astride, uint32_t read_len, uint64_t n_reads,
                       void* d_rows, uint32_t row_words, void* stream);

typedef struct snk_dev_reads {
    uint64_t n_reads;
    const void* rows;         /* u32[n_reads*row_words] packed bases (HBM) */
    uint32_t row_words;
    uint32_t read_len;        /* <= 256 */
    const void* lens;         /* u16[n_reads] or NULL (all reads are read_len long) */
    const void* quals;        /* u8[n_reads*qstride] raw phred, or NULL if good_len is given */
    uint32_t qstride;
    uint32_t reserved0;
    const void* good_len;     /* u16[n_reads] precomputed trim, or NULL */
    const void* bc;           /* i32[n_reads] barcode ids, or NULL (no barcode rule) */
    int64_t ign_bc_below;     /* reads with global index < this get bc = -1 (BuildReadQGraph48.cc:158-159) */
    uint64_t read_index_base; /* global index of read 0 of this slab (multi-GPU slabs) */
    const void* group;        /* u32[n_reads] group id per read (SNK_F_GROUPED), or NULL */
} snk_dev_reads;

/* All pointers are device pointers owned by the context; they stay valid until the next
 * snk_dev_count_graph call on the same context or snk_ctx_destroy. */
typedef struct snk_dev_result {
    uint64_t n_reads;
    uint64_t n_instances;        /* sum over reads of max(0, good_len-K+1), reads with good_len < K+1 excluded */
    uint64_t n_supermers;
    uint64_t n_buckets;
    const void* good_len;        /* u16[n_reads] */
    uint64_t n_kmers;            /* retained canonical k-mers */
    const void* keys;            /* n_kmers x 16 bytes: little-endian 128-bit value = {u64 lo, u64 hi}; base i of the
                                    k-mer at bits 127-2i..126-2i; ascending unless SNK_F_UNSORTED_TABLE */
    const void* counts;          /* u32[n_kmers] */
    const void* ctx;             /* u8[n_kmers] pruned context bytes */
    const void* spectrum;        /* u64[spectrum_bins]: retained k-mers per count (histogram_kmer_count.json) */
    uint32_t spectrum_bins;
    uint32_t n_circles;
    uint64_t n_unitigs;
    uint64_t unitig_total_bases;
    const void* unitig_off;      /* u64[n_unitigs+1] */
    const void* unitig_bases;    /* u8 base codes, canonical orientation, unitigs ordered by their first K bases */
    uint32_t rank_rounds;
    uint32_t buckets_split;
    uint32_t max_slots_used;
    uint32_t n_overflow;         /* supermers that did not fit their bucket's fixed capacity (second count segment) */
    uint64_t scratch_bytes;
    float phase_ms[8];           /* trim, partition plan, minimiser partition, count, sort, prune+unitigs, -, total */
    float kernel_ms[4];          /* HIP-event time of single launches: -, minimiser partition, count (LDS reduce), - */
    uint64_t n_boundary;         /* bucket-local graph: k-mers with a neighbour outside their bucket chunk */
    uint64_t n_fragments;        /* bucket-local graph: local unitig fragments joined at the end */
    const void* unitig_group;    /* u32[n_unitigs] group of every unitig (SNK_F_GROUPED; unitigs ordered by group, then by
                                    their first K bases), else NULL */
    float graph_ms[8];           /* bucket-local graph: local prune, boundary resolve, fragments, join, table sort+spectrum */
    uint32_t repartitioned;      /* 1: the first buckets overflowed their tables (error-rich / shallow data) and the reads were
                                    partitioned a second time into smaller buckets; later calls on the context start there */
    uint32_t n_hot_buckets;      /* minimiser buckets far above their capacity (repeat families, homopolymer runs) whose k-mer instances
                                    were re-partitioned by k-mer hash and counted class by class */
} snk_dev_result;

/* Replaces the body of buildReadQGraph48 (BuildReadQGraph48.cc:1688-1774, pPaths==nullptr) up to and
 * including buildEdges; == tada MSP -> SHARD_ASM -> MAIN_ASM_SN.  Inputs already resident in HBM. */
int snk_dev_count_graph(snk_ctx* ctx, const snk_dev_reads* in, const snk_params* p, snk_dev_result* out, void* stream,
                        char* err, size_t errcap);
int snk_dev_download(snk_ctx* ctx, const void* d_src, void* h_dst, size_t bytes, void* stream);

/* Streamed input: the same job with its reads arriving slab by slab (as a FASTH decoder delivers them).  The reference streams its
 * FASTQ chunks through the partitioner (lib/tada/src/cmd_msp.rs:55-69) and re-scans in passes when the keys do not fit
 * (MapReduceEngine.h:452-468); here every slab is partitioned into the job's minimiser buckets as it arrives -- the launch is
 * asynchronous, so the decode / upload of the next slab overlaps it -- and the slab's buffers may be reused once the stream has passed
 * the call (an event, or a synchronise).  The job's reads are never resident as a whole.
 *   begin : total_reads_ub = an upper bound of the job's reads (it sizes the bucket slots; reads beyond it are refused),
 *           has_bc = the slabs carry barcode ids (all of them or none).  Per-group graphs (SNK_F_GROUPED) are not streamed.
 *   append: slab->read_index_base = global index of its first read (ign_bc_below); 0 = numbered in arrival order.
 *   finish: count + graph over everything appended; result as snk_dev_count_graph's (good_len covers the reads in arrival order),
 *           bit-identical to one resident call on the concatenated slabs.
 * A job that cannot look at its first buckets and partition again (its slabs are gone): error-rich data without the context's
 * history of an earlier job of the same size are counted in hash-split sub-passes -- slower, same result. */
int snk_dev_stream_begin(snk_ctx* ctx, const snk_params* p, uint32_t read_len, uint64_t total_reads_ub, int has_bc, void* stream, char* err, size_t errcap);
int snk_dev_stream_append(snk_ctx* ctx, const snk_dev_reads* slab, void* stream, char* err, size_t errcap);
int snk_dev_stream_finish(snk_ctx* ctx, snk_dev_result* out, void* stream, char* err, size_t errcap);

/* ---- minimiser-sharded multi-GPU path: ONE entry point, snk_shard_step (below); its phases are internal
 * (supernova_amd/csrc/snk_shard_phases.h) since the step moved behind the C ABI in round 3. */
/* fragment bases on the wire (the gather to rank 0): 2 bits per base, 16 bases per 32-bit word, base j at bits 2j --
 * the .bv byte packing (lib/tada/src/debruijn.rs:895-929).  snk_pack2_bytes(n) = size of the packed buffer. */
uint64_t snk_pack2_bytes(uint64_t n_bases);
int snk_dev_pack2(snk_ctx* ctx, const void* d_bases, uint64_t n_bases, void* d_packed, void* stream);
int snk_dev_unpack2(snk_ctx* ctx, const void* d_packed, uint64_t n_bases, void* d_bases, void* stream);


/* ---- the sharded step behind ONE call (round 3) ------------------------------------------------------------------------
 * A communicator carries the exchanges; the step itself -- partition, histogram and record exchange (in bucket ranges,
 * overlapped with the count), count, cross-rank prune, fragments, fragment links, owner-side join -- runs inside
 * snk_shard_step, so a C++ host (supernova_amd/csrc/host/snk_asm_sn.cc) runs the N-GPU job without any scripting layer.
 * Replaces tada's MSP -> SHARD_ASM -> MAIN_ASM_SN with its shard files (lib/tada/src/cmd_msp.rs:38-80, cmd_shard_asm.rs:37-94,
 * cmd_main_asm.rs:25-89; lib/tada/external/rust-shardio/src/shard.rs:184-211,488-493) and MapReduceEngine.h:362-385.
 *   snk_comm_unique_id      rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the other ranks (file, socket, ...)
 *   snk_comm_create_rccl    every rank: ncclCommInitRank on the context's device; librccl is bound at run time
 *                           (snk_comm_set_rccl_path / $SNK_RCCL_LIB / librccl.so.1 / $ROCM_PATH/lib)
 *   snk_comm_from_nccl      adopt the caller's ncclComm_t (not destroyed by snk_comm_destroy)
 *   snk_comm_create_local   `world` in-process ranks on ONE device (tests): out[r] is rank r's handle, every rank runs on its
 *                           own host thread with its own context; the wire is a device copy */
typedef struct snk_comm snk_comm;
int snk_comm_set_rccl_path(const char* path);
int snk_comm_unique_id(void* id128, char* err, size_t errcap);
int snk_comm_create_rccl(snk_ctx* ctx, const void* id128, uint32_t rank, uint32_t world, snk_comm** out, char* err, size_t errcap);
int snk_comm_from_nccl(snk_ctx* ctx, void* nccl_comm, uint32_t rank, uint32_t world, snk_comm** out, char* err, size_t errcap);
int snk_comm_create_local(uint32_t world, snk_comm** out /* [world] */, char* err, size_t errcap);
/* the exchanges through callbacks of the host (its own transport: MPI, sockets, torch.distributed, ...): a2a moves scnt[p] bytes
 * at send + sbeg[p] to rank p and delivers rcnt[s] bytes from rank s at recv + rbeg[s]; gather collects k u64 of every rank
 * (mine and all are HOST memory: device counters are read back by the library first) into all[world * k].  a2a's buffers are
 * whatever memory the step hands over -- DEVICE memory inside snk_shard_step, not ordered with any stream: the callback
 * synchronises the device before it reads and after it writes.
 * Both return 0 or an error code.  snk_comm_selftest runs the step's exchange patterns on HOST memory with synthetic contents
 * over any communicator whose buffers may be host memory (the CPU tests use it over gloo, world_size 2). */
typedef int (*snk_comm_a2a_fn)(void* user, const void* send, const uint64_t* sbeg, const uint64_t* scnt, void* recv, const uint64_t* rbeg,
                               const uint64_t* rcnt, uint32_t world);
typedef int (*snk_comm_gather_fn)(void* user, const void* mine, uint32_t k, unsigned long long* all, uint32_t world);
int snk_comm_create_callbacks(uint32_t rank, uint32_t world, snk_comm_a2a_fn a2a, snk_comm_gather_fn gather, void* user, snk_comm** out,
                              char* err, size_t errcap);
int snk_comm_selftest(snk_comm* c, uint64_t seed, uint32_t buckets_per_rank, uint32_t ranges, char* err, size_t errcap);
void snk_comm_destroy(snk_comm* c);
void snk_comm_abort(snk_comm* c);          /* in-process ranks: release the others after a failure outside snk_shard_step */
uint32_t snk_comm_rank(const snk_comm* c);
uint32_t snk_comm_world(const snk_comm* c);
const char* snk_comm_kind(const snk_comm* c);   /* "rccl" | "local" */

/* Device pointers owned by the context, valid until its next top-level call.  The table share is in bucket order; the
 * unitigs are the ones whose head fragment this rank owns, ordered by their first K bases (the union over the ranks is the
 * job's unitig set; snk_shard_gather_unitigs brings it to one rank in BVComp order). */
typedef struct snk_shard_result {
    uint32_t rank, world;
    uint64_t n_reads, n_instances, n_supermers, n_buckets_total;
    uint64_t n_kmers;
    const void* keys;
    const void* counts;
    const void* ctx;
    const void* spectrum;
    uint32_t spectrum_bins, n_circles;
    uint64_t n_unitigs, unitig_total_bases;
    const void* unitig_off;          /* u64[n_unitigs+1] */
    const void* unitig_bases;
    const void* unitig_circular;
    uint64_t n_frags, n_frags_total, n_queries, n_link_queries;
    uint64_t exchanged_bytes[8];     /* sent to OTHER ranks: records, prune queries+answers, link queries+answers, link structure,
                                        splitters, ranks, fragments, everything the transport carried */
    uint32_t host_syncs;             /* host waits for the stream during the step (the read-backs of sizes) */
    uint32_t ranking;                /* 1 = the list ranking ran partitioned over the ranks, 0 = replicated */
    uint32_t buckets_split, max_slots_used;
    float phase_ms[8];               /* trim+partition, histograms+compaction, exchange issue, count, prune, fragments, join, total */
    float join_ms[8];                /* links, link structure, rank+place, route, emit */
    float count_kernel_ms;
    uint32_t repartitioned;          /* 1: the first buckets overflowed the count kernel's tables and the step partitioned and exchanged a
                                        second time into smaller buckets (a job-wide decision); later steps on the context start there */
    uint32_t n_hot_buckets;          /* this rank's minimiser buckets far above their capacity (repeat families, homopolymer runs): re-partitioned
                                        by k-mer hash and counted by a launch of their own, like snk_dev_result.n_hot_buckets */
    uint32_t reserved_u;
    uint64_t pair_max_bytes[8];      /* per exchange (the order of exchanged_bytes): the most this rank sent to ONE other rank.  xGMI is point to
                                        point: an exchange takes as long as its fullest pair, so max against exchanged_bytes / (world - 1) is the
                                        link balance of the step */
} snk_shard_result;
/* Bucket-range passes of the last snk_dev_count_graph on the context (1 = the one-pass partition).  A job whose supermer slots would not
 * fit the device is partitioned and counted range by range over one slot array, the reads scanned once per pass -- what the reference
 * does when its k-mer records do not fit (lib/assembly/src/MapReduceEngine.h:452-468, lib/tada/src/utils.rs:329-341).  Same results. */
uint32_t snk_ctx_last_partition_passes(const snk_ctx* ctx);
/* Distinct k-mers one pass over a bucket could hold in the count kernel's table in the last snk_dev_count_graph on the context: 1216 of the 2048
 * slots with the default kernel, 1920 when the call's data run the tables full (error-rich reads, per-barcode groups) and the waves book
 * their slots instead of keeping a round's worth free (DESIGN.md 4 "round 5").  Same results either way. */
uint32_t snk_ctx_last_count_limit(const snk_ctx* ctx);
/* total_reads: reads of the whole job (sizes the bucket count without an exchange; 0 = the ranks exchange their slab sizes,
 * ignored when p->n_buckets is set).  in->read_index_base = global index of the slab's first read. */
int snk_shard_step(snk_ctx* ctx, snk_comm* comm, const snk_dev_reads* in, const snk_params* p, uint64_t total_reads, uint32_t flags,
                   snk_shard_result* out, void* stream, char* err, size_t errcap);
/* The same step with the rank's reads arriving slab by slab (what snk_dev_stream_* is to snk_dev_count_graph; tada streams its FASTQ
 * chunks into the partitioner, lib/tada/src/cmd_msp.rs:55-69): begin sizes the job's buckets -- total_reads = reads of the whole job, the
 * same on every rank -- and this rank's slots (rank_reads_ub: an upper bound of what it will append); append partitions one slab (nothing
 * is waited for; slab->read_index_base = global index of its first read); finish runs the rest of the step.  A streamed step cannot
 * partition twice: without the group's history of a previous step, error-rich data are counted in hash-split sub-passes. */
int snk_shard_stream_begin(snk_ctx* ctx, snk_comm* comm, const snk_params* p, uint32_t read_len, uint64_t rank_reads_ub, uint64_t total_reads,
                           int has_bc, void* stream, char* err, size_t errcap);
int snk_shard_stream_append(snk_ctx* ctx, const snk_dev_reads* slab, void* stream, char* err, size_t errcap);
int snk_shard_stream_finish(snk_ctx* ctx, snk_comm* comm, uint32_t flags, snk_shard_result* out, void* stream, char* err, size_t errcap);
/* ---- host-pointer convenience + graph hand-off -------------- */
typedef struct snk_reads {
    uint64_t n_reads;
    uint32_t read_len;          /* row length in bases (<= 256); per-read lengths in `lens` */
    uint32_t reserved;
    const uint8_t* ascii;       /* n_reads*read_len base characters (non-ACGT -> A), or NULL if rows given */
    const uint32_t* rows;       /* packed rows (row_words = ceil(read_len/16)), or NULL if ascii given */
    const uint16_t* lens;       /* per-read length or NULL */
    const uint8_t* quals;       /* n_reads*read_len raw phred (no +33), or NULL if good_len given */
    const uint16_t* good_len;   /* precomputed trim or NULL */
    const int32_t* bc;          /* barcode ids or NULL */
    int64_t ign_bc_below;
} snk_reads;

typedef struct snk_result {
    uint64_t n_instances;
    uint64_t n_kmers;
    uint32_t* kmers;            /* n_kmers*4 words MSB-first, ascending */
    uint32_t* counts;
    uint8_t* ctx;
    uint64_t n_unitigs;
    uint64_t* unitig_off;       /* n_unitigs+1 */
    uint8_t* unitig_bases;      /* base codes; unitigs canonical, ordered by BVComp (len desc, lexicographic;
                                   lib/assembly/src/paths/long/HBVFromEdges.cc:106-111) */
    uint64_t* spectrum;         /* spectrum_bins */
    uint32_t spectrum_bins;
    uint32_t reserved;
    float phase_ms[8];
    uint8_t* bv_image;          /* SNK_F_BV_IMAGE: the .bv file ("BINWRITE", u64 count, per unitig u32 length + ceil(len/4)
                                   bytes; lib/tada/src/debruijn.rs:895-929), unitigs in BVComp order; else NULL */
    uint64_t bv_bytes;
} snk_result;

/* Replaces buildReadQGraph48(..., pPaths=nullptr) up to the unitigs for host-resident inputs
 * (BuildReadQGraph48.h:24-34).  Uploads over PCIe, runs snk_dev_count_graph, downloads and orders the result.
 * Outputs are malloc'ed by the library and released by snk_free. */
int snk_count_graph(snk_ctx* ctx, const snk_reads* in, const snk_params* p, snk_result* out, char* err, size_t errcap);
void snk_free(snk_result* r);

/* The job's unitig set on ONE rank in the reference's order -- what MAIN_ASM_SN writes to asm_graph.bv
 * (lib/tada/src/cmd_main_asm.rs:184-193, debruijn.rs:895-929): every rank (all must call) ships the unitigs it wrote at 2 bits
 * per base to `root`, which orders the union by BVComp (HBVFromEdges.cc:106-111) on its device.  On root, out holds n_unitigs +
 * unitig_off / unitig_bases, or with flags & SNK_F_BV_IMAGE the file's bytes (bv_image / bv_bytes); release with snk_free.
 * Other ranks get an empty result. */
int snk_shard_gather_unitigs(snk_ctx* ctx, snk_comm* comm, const snk_shard_result* res, uint32_t K, uint32_t root, uint32_t flags,
                             snk_result* out, void* stream, char* err, size_t errcap);

/* Page-locked host memory for the inputs of snk_count_graph (the reference keeps reads/quals in plain vectors, vecbvec /
 * VecPQVec, BuildReadQGraph48.h:24-34; a host that fills pinned buffers instead saves the staging copy: the DMA engine
 * reads them in place).  Pageable inputs are accepted just the same. */
int snk_host_alloc_pinned(size_t bytes, void** out, char* err, size_t errcap);
void snk_host_free_pinned(void* p);

/* a13: the unitig hand-off file tada writes and DF reads through MSPEDGES= ("BINWRITE", u64 count, per entry u32
 * length + ceil(len/4) bytes, base j at bits 2*(j%4)): writer TempGraph::write_to_sn_format
 * lib/tada/src/debruijn.rs:895-929, reader BuildReadQGraph48.cc:1640-1642. */
int snk_write_bv(const char* path, uint64_t n_unitigs, const uint64_t* unitig_off, const uint8_t* unitig_bases,
                 char* err, size_t errcap);
int snk_read_bv(const char* path, uint64_t* n_unitigs, uint64_t** unitig_off, uint8_t** unitig_bases, char* err,
                size_t errcap);   /* outputs malloc'ed; free() them */

/* a13 on the device: the bytes of that file from the device-resident unitigs of snk_dev_count_graph -- BVComp order (length
 * descending, then lexicographic: HBVFromEdges.cc:106-111), 2-bit packing and the "BINWRITE" header all in HBM; *d_image is context
 * memory (valid until the next top-level call), ready for one download or a GPU-direct write.  by_first_kmer: the unitigs are ordered
 * by their first K bases (how snk_dev_count_graph leaves them): one stable sort by length does. */
int snk_dev_bv_image(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, int by_first_kmer,
                     const void** d_image, uint64_t* image_bytes, void* stream, char* err, size_t errcap);

/* a14: buildHBVFromEdges (lib/assembly/src/paths/long/HBVFromEdges.cc:244-296): vertices = distinct (K-1)-mer
 * unitig ends, HBV edges = every unitig and its reverse complement (palindromes once), ids assigned by the
 * reference's deterministic flood fill over the BVComp edge order.  Unitigs must be in BVComp order.
 * snk_hbv_from_unitigs takes host arrays in BVComp order.  snk_dev_hbv takes the device-resident unitigs of
 * snk_dev_count_graph (any order): BVComp ranking, the
 * (K-1)-mer end keys, their sort and the vertex classes are computed on the device (what the reference runs through
 * its MapReduce engine, HBVFromEdges.cc:136-168,257-262); the id hand-out, a breadth-first flood whose ids ARE the
 * visiting order (:170-238), runs per connected component: components and their id blocks on the device, one thread per
 * component; a component above SNK_HBV_BIG (1024) nodes, and any graph below SNK_HBV_DEV_MIN (65536) unitigs, on the host.
 * snk_ctx_last_hbv_flood says which of the two ran.  The input must be the unitig set of a de Bruijn graph (no K-mer twice, at most 8
 * ends per (K-1)-mer); other input is not refused. */
typedef struct snk_hbv {
    int32_t n_vertices, n_edges;
    int32_t* v_left;            /* per HBV edge */
    int32_t* v_right;
    int32_t* src_unitig;        /* per HBV edge: unitig it is a copy (or reverse complement) of */
    uint8_t* is_rc;
    int32_t* fwd_xlat;          /* per unitig: HBV edge id of the forward / reverse-complement copy */
    int32_t* rev_xlat;
    int32_t* bvcomp_order;      /* snk_dev_hbv: per BVComp rank (the unitig numbering above) the index of that unitig
                                   in the caller's device arrays; NULL from snk_hbv_from_unitigs (input already ranked) */
} snk_hbv;
int snk_hbv_from_unitigs(uint32_t K, uint64_t n_unitigs, const uint64_t* unitig_off, const uint8_t* unitig_bases,
                         snk_hbv* out, char* err, size_t errcap);
/* Which id flood the last snk_dev_hbv on the context ran: 0 = the host flood (the graph was below hbv_dev_min unitigs), 1 = the device
 * flood, 2 = the device flood gave up and the host flood redid the graph (never with hbv_strict, which fails the call instead).
 * *device_components / *host_components (either may be NULL): the connected components of the (unitig, strand) graph that device threads
 * flooded (one thread each: those of at most hbv_big nodes) and those that host threads flooded (all of them after 0 and 2).  After a
 * call that failed or had no unitigs: 0 and no components. */
uint32_t snk_ctx_last_hbv_flood(const snk_ctx* ctx, uint64_t* device_components, uint64_t* host_components);
/* What the bucket-local graph stage did in the context's last count-and-graph call (snk_dev_count_graph, the streamed and the sharded
 * forms): returns the attempts of its fragment pass -- 1, or 2 when the circles closed inside single chunks needed more fragment slots than
 * the pool held (bl_pool + F/256 for F open paths) and the pass ran again with the exact number -- or 0 when the stage did not run
 * (global_graph, SNK_F_NO_GRAPH, an empty table, a failed call).  *in_chunk_circles: those circles; *big_chunks: the chunks that went to
 * the large-chunk kernels (either may be NULL).  A NULL context answers 0 everywhere.  Read-only; for tests and diagnostics. */
uint32_t snk_ctx_last_local_graph(const snk_ctx* ctx, uint64_t* in_chunk_circles, uint32_t* big_chunks);
/* The device stages that run after snk_dev_count_graph -- snk_dev_hbv, snk_dev_path_reads2, snk_dev_mark_dups, snk_dev_paths_index,
 * snk_dev_edge_barcodes, snk_dev_paths_zip, snk_dev_paths_unzip, snk_dev_extend_paths, snk_dev_patch_pieces, snk_dev_patch_merge, snk_dev_patch_paths, snk_dev_mark_bads, snk_dev_mark_bads_df, snk_dev_edge_pairs, snk_dev_close_gaps, snk_dev_delete_edges, snk_dev_hanging_ends, snk_dev_mow_lawn and snk_dev_check_graph -- share one result rule: after ANY non-zero return *out is all
 * zero (nothing to free, no device pointer to use; a snk_check_report keeps its struct_size), the call's work on the stream has
 * ended and its scratch is back in the context. */
/* device_ms (optional): time of the device part, HIP events */
int snk_dev_hbv(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases,
                snk_hbv* out, float* device_ms, void* stream, char* err, size_t errcap);
void snk_hbv_free(snk_hbv* h);
/* f1: read pathing on the device -- pathReads with the new aligner (paths/long/BuildReadQGraph48.cc:1441-1469):
 * Pather::path (:705-748), HBVPather::algorithmTwo (:1217-1336), pathPartsToReadPath (:1393-1428) and
 * ExtendReadPath::attemptLeftRightExtension (paths/long/ExtendReadPath.cc:108-358), over a k-mer -> (edge, offset) dictionary
 * built from the unitigs (:1656-1664).  Reads are pathed untrimmed (packed rows + quality rows + lengths of snk_dev_reads;
 * good_len / bc are not used).  The unitigs are the device arrays of snk_dev_count_graph, h their graph from snk_dev_hbv
 * (bvcomp_order maps its unitig numbering to the device arrays; NULL = the arrays are already in BVComp order).
 * Result (device memory of the context, valid until its next top-level call): per read the offset of the read on its first
 * edge (ReadPath::mOffset, may be negative), its number of edges and their HBV edge ids (start[r] .. start[r] + n_edges[r]). */
typedef struct snk_dev_paths {
    uint64_t n_reads, n_edges_total;
    const void* offset;        /* i32[n_reads] */
    const void* n_edges;       /* u32[n_reads] */
    const void* start;         /* u64[n_reads + 1] */
    const void* edges;         /* i32[n_edges_total] */
    uint64_t dict_slots;
    float dict_ms, path_ms;    /* HIP events: graph tables + packed unitigs + dictionary; pathing + gather */
    /* SNK_PATH_UNITIG_BCS (snk_dev_path_reads2): per unitig (device numbering) the sorted distinct barcodes > 0 of the reads that
     * have a k-mer on it -- the edge -> barcode sets of tada's MAIN_ASM_SN (lib/tada/src/cmd_main_asm.rs:91-151,
     * debruijn.rs:115-131), cut at 20 000 entries per unitig like cmd_main_asm.rs:115 -- the smallest ids are kept; the reference keeps
     * what its shard order delivers first, which needs its shard layout: parity unpinned (Rust) */
    const void* unitig_bc_off; /* u64[n_unitigs + 1] */
    const void* unitig_bcs;    /* u32[n_unitig_bcs] */
    uint64_t n_unitig_bcs;
    float bcs_ms;              /* HIP events: key sort + run heads + per-unitig lists (SNK_PATH_UNITIG_BCS) */
    uint32_t lookup_index;     /* 1: the look-ups went through the minimiser index (the k-mer dictionary did not fit, or SNK_PATH_INDEX=1); dict_slots then counts its places */
    uint64_t n_slow;           /* reads the fast pass left to the full algorithm (a miss, or an exact-match run that ended inside the read) */
    uint32_t retries;          /* lists that overflowed and made the call run the pass again with a longer one: bit 0 the reads for the
                                  full-capacity pass, bit 1 the second and later path edges, bit 2 the (unitig, barcode) keys */
} snk_dev_paths;
#define SNK_PATH_UNITIG_BCS 1u
#define SNK_PATH_UNITIG_BCS_EXHAUSTIVE 2u   /* (with SNK_PATH_UNITIG_BCS) derive the lists the slow, literal way -- every k-mer of every barcoded
                                               read looked up, barcodes_for_sedge (debruijn.rs:115-131) -- instead of from the path parts: a
                                               second, independent derivation the tests compare the fast one with */
#define SNK_PATH_UNITIG_BCS_NOCUT 4u        /* do not apply the 20 000-entry cut (cmd_main_asm.rs:115; here: a unitig keeps its 20 000 smallest ids) */
int snk_dev_path_reads(snk_ctx* ctx, uint32_t K, const snk_dev_reads* in, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases,
                       const snk_hbv* h, snk_dev_paths* out, void* stream, char* err, size_t errcap);
int snk_dev_path_reads2(snk_ctx* ctx, uint32_t K, const snk_dev_reads* in, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases,
                        const snk_hbv* h, uint32_t flags, snk_dev_paths* out, void* stream, char* err, size_t errcap);
/* f2: hbv.Involution (paths/HyperBasevector.cc:685-697; 10X/runstages/RunStages.cc:418): inv[e] = edge that is e's reverse
 * complement -- and the files DF keeps the graph in: a.hbv = BinaryWriter::writeFile(HyperBasevector)
 * (paths/HyperBasevector.cc:121-125, graph/DigraphTemplate.h:3092-3097) and a.inv (vec<int>), byte for byte.  The unitig arrays
 * are the ones the snk_hbv was built from (BVComp order); path_inv may be NULL. */
int snk_hbv_involution(const snk_hbv* h, uint64_t n_unitigs, int32_t* inv /* [n_edges] */, char* err, size_t errcap);
int snk_write_hbv(const char* path_hbv, const char* path_inv, uint32_t K, uint64_t n_unitigs, const uint64_t* unitig_off,
                  const uint8_t* unitig_bases, const snk_hbv* h, char* err, size_t errcap);

/* ---- f4: duplicate marking over the read paths --------------------------------------------------
 * MarkDups, lib/assembly/src/10X/SecretOps.cc:413-593 (10X/DF.cc:597-600 runs it on the paths just made and writes a.dup):
 * placed reads that share (first edge, offset on it, first five bases of the mate) are duplicates of each other; the one with
 * the largest quality sum over both mates -- the earliest read among equals -- survives, every other member flags its PAIR.
 *   in     the reads the paths were made from (untrimmed rows, quality rows, lens, bc: the raw barcode ids; NULL = all 0);
 *          reads 2q and 2q+1 are mates
 *   dup    u8[n_reads / 2] on the device (owned by the context, valid until its next call): vec<Bool> dup of the reference
 *   interdup_rate   duplicate reads whose group spans more than one barcode / duplicate reads (the reference's rule: a group's
 *          barcode is its first member's, or while that is 0 the next member's)
 *   n_art_pairs     pairs the reference counts as artifactual duplicates (identical bases AND qualities to another member of a
 *          group with a quality-sum tie); it only logs their percentage */
typedef struct snk_dev_dups {
    uint64_t n_pairs;
    const void* dup;
    uint64_t n_placed;            /* reads with a path */
    uint64_t n_dup_reads;         /* sum over groups of (size - 1) */
    uint64_t n_interdup_reads;
    uint64_t n_dup_pairs;         /* pairs flagged */
    uint64_t n_art_pairs;
    double interdup_rate;
    float ms;                     /* HIP events around the whole call */
} snk_dev_dups;
int snk_dev_mark_dups(snk_ctx* ctx, const snk_dev_reads* in, const snk_dev_paths* paths, snk_dev_dups* out, void* stream, char* err, size_t errcap);

/* ---- the paths index and the rest of a.48/ ------------------------------------------------------------------------
 * writePathsIndex, lib/assembly/src/10X/PathsIndex.cc:23-145 (10X/DF.cc:588 runs it on the paths just made): per HBV edge the ids of
 * the reads whose path holds it -- what every later stage of the reference opens first (a.paths.inv; StageFindPatch, DF.cc:636-638) --
 * and the read support per edge (a.countsb).  The reference writes one (edge, read id) pair per path entry into 15 temporary chunk files,
 * reads them back and comparison-sorts each (:38-114); here the entries of snk_dev_paths, already ordered by read id, go through one
 * stable radix sort over the ceil(log2 n_hbv_edges) bits an edge id has.
 *   paths        of snk_dev_path_reads (edge ids = HBV edge ids); it must stay valid across the call, and does: the call takes its
 *                memory from the context's arena behind it and hands its scratch back on return
 *   inv          HOST array, int32[n_hbv_edges], of snk_hbv_involution
 *   index_off    u64[n_hbv_edges + 1], index_ids u64[n_entries]: the reads of edge e are index_ids[index_off[e] .. index_off[e + 1]),
 *                ascending, a read repeated as often as its path holds e (the reference keeps the duplicates of its sorted pairs,
 *                :51-57,90,104-107: a path through a tandem repeat visits an edge many times)
 *   counts       i32[n_hbv_edges]: entries of e, and for every pair e != inv[e] both replaced by their sum; a self-inverse edge keeps
 *                its own (:122-133).  A sum above 2^31 - 1 is refused (SNK_E_UNSUPPORTED): the file holds int
 * Device memory of the context, valid until its next top-level call.  SNK_E_ARG: an edge id outside [0, n_hbv_edges), an inv that is not
 * an involution, start / n_edges that do not add up to n_edges_total.  The result is bit-identical from call to call and depends on no
 * tuning option. */
typedef struct snk_dev_pidx {
    uint64_t n_hbv_edges, n_entries;     /* n_entries = paths->n_edges_total */
    const void* index_off;
    const void* index_ids;
    const void* counts;
    uint64_t n_empty_edges;              /* edges no read's path holds (the reference writes an empty entry for them, :101-102) */
    float ms;                            /* HIP events around the whole call (the upload of inv included) */
    uint32_t key_bits;                   /* bits of an edge id the sort looked at */
    uint64_t reserved[6];
} snk_dev_pidx;
int snk_dev_paths_index(snk_ctx* ctx, const snk_dev_paths* paths, uint64_t n_hbv_edges, const int32_t* inv, snk_dev_pidx* out, void* stream,
                        char* err, size_t errcap);
/* The files (host arrays; no GPU needed), byte for byte what the reference leaves in a.48/:
 *   snk_write_paths        a.paths = the tmp.paths of pathReads (BuildReadQGraph48.cc:1441-1469, renamed at DF.cc:584): feudal
 *                          MasterVec<ReadPath> -- control block, per read i32 offset, u32 last skip (always 0: :1408-1418 is commented
 *                          out) and its edge ids (paths/long/ReadPath.h:61-63), then the table of n_reads + 1 file offsets.
 *                          start may be NULL: the paths follow each other in `edges`
 *   snk_write_paths_index  a.paths.inv = IncrementalWriter<ULongVec> (PathsIndex.cc:76,100-108): feudal, per edge its read ids as u64;
 *                          a.countsb = BinaryWriter::writeFile(vec<vec<int>>) with one inner vector (:75,135).  Either path may be NULL
 *   snk_write_dup          a.dup = BinaryWriter::writeFile(vec<Bool>) (DF.cc:599-600): "BINWRITE", u64 count, one byte per pair */
int snk_write_paths(const char* path, uint64_t n_reads, const int32_t* offset, const uint32_t* n_edges, const uint64_t* start, const int32_t* edges,
                    char* err, size_t errcap);
int snk_write_paths_index(const char* path_inv, const char* path_countsb, uint64_t n_hbv_edges, const uint64_t* index_off, const uint64_t* index_ids,
                          const int32_t* counts, char* err, size_t errcap);
int snk_write_dup(const char* path, uint64_t n_pairs, const uint8_t* dup, char* err, size_t errcap);

/* ---- the compressed read paths: a.pathsX and a.hbx ------------------------------------------------------------------
 * Right after StageBuildGraph the reference turns the graph into a HyperBasevectorX and the paths into a ReadPathVecX (10X/DF.cc:573-583,
 * InitializePathsXFromPaths, 10X/DfTools.cc:24-69); every later consumer takes that form, and a DF entered at START=patch opens a.hbv,
 * a.hbx, a.inv, a.pathsX and a.dup (DF.cc:612-630).  Per read, in read order, the record is (RPParser::LLzip,
 * 10X/paths/ReadPathParser.cc:18-51,184-198):
 *     u8 n = number of edges | n > 0: i16 offset (static_cast<int16_t>: beyond +-32767 it wraps), u32 first edge id,
 *                              (n - 1 + 3) / 4 bytes of 2-bit branch ids, least significant bits first
 * The branch id of a step e -> e' is the position of e' in From(ToRight(e)).  A step whose e' is not among them encodes nothing and does
 * not move the bit cursor; the record's size still comes from n (the bytes left over are 0).  ZipIndex: the byte offset of every 10th
 * read.
 *   paths        of snk_dev_path_reads (edge ids = HBV edge ids); it stays valid across the call, as for snk_dev_paths_index
 *   h            HOST: the graph the paths were made on.  Its From / To lists are derived by the function that snk_write_hbv takes them
 *                from, in the order a.hbv has them
 *   data         u8[n_bytes], index i64[n_index], n_index = ceil(n_reads / 10): device memory of the context, valid until its next
 *                top-level call
 * Refused: a path of more than 255 edges (SNK_E_UNSUPPORTED: the reference's own record is self-inconsistent there: one byte holds the
 * count), a vertex with more than four out-edges (SNK_E_UNSUPPORTED: a branch id has two bits), an edge id outside the graph (SNK_E_ARG),
 * start / n_edges that do not add up to n_edges_total (SNK_E_ARG: start must be the exclusive scan of n_edges -- no gaps, no overlaps -- and
 * start[n_reads] = n_edges_total, as snk_dev_path_reads leaves them).  The result is bit-identical from call to call and depends on no
 * tuning option. */
typedef struct snk_dev_pathsx {
    uint64_t n_reads, n_bytes, n_index;
    const void* data;
    const void* index;
    uint64_t n_empty;                    /* reads without a path (one byte each) */
    uint64_t n_steps_not_found;          /* steps e -> e' with e' not in From(ToRight(e)): nothing encoded for them */
    uint64_t n_offsets_wrapped;          /* reads with a path whose offset does not fit an int16 */
    float ms;                            /* time between two HIP events at the start and the end of the call's device work: not kernel time
                                            alone -- it spans the upload of the per-edge arrays, one wait of the host in the middle (largest
                                            edge id, flags and n_bytes come down before data is allocated) and that allocation.  The
                                            host's derivation of the per-edge arrays from h comes before the first event */
    uint32_t reserved0;
    uint64_t reserved[6];
} snk_dev_pathsx;
int snk_dev_paths_zip(snk_ctx* ctx, const snk_dev_paths* paths, const snk_hbv* h, snk_dev_pathsx* out, void* stream, char* err, size_t errcap);
/* The inverse (ReadPathVecX::unzip, LLunzip, ReadPathParser.cc:106-132): how a consumer starts from an a.pathsX file.  in->data and
 * in->index are device memory (n_reads, n_bytes, n_index filled in; the counters are not read).  out: offset, n_edges, start, edges as
 * from snk_dev_path_reads (context memory, valid until its next top-level call; path_ms = time of the call, the other fields 0); an
 * offset comes back as the int16 it was stored as.  SNK_E_ARG: n_index is not ceil(n_reads / 10), the records do not follow the index or
 * do not end exactly at n_bytes, a first edge outside the graph, a branch id that addresses no out-edge of its vertex. */
int snk_dev_paths_unzip(snk_ctx* ctx, const snk_dev_pathsx* in, const snk_hbv* h, snk_dev_paths* out, void* stream, char* err, size_t errcap);
/* The files (host arrays; no GPU needed), byte for byte what the reference writes:
 *   snk_write_pathsx   a.pathsX = ReadPathVecX::writeBinary(std::string) (10X/paths/ReadPathVecX.cc:976-996), raw: skip = 10, start_rid = 0,
 *                      next_start_rid = n_reads, the index size and the data size as int64, the index, the data
 *   snk_read_pathsx    the same file back; *index and *data are malloc'ed (snk_host_free).  SNK_E_IO: a header that does not fit the file
 *   snk_write_hbx      a.hbx = BinaryWriter::writeFile(HyperBasevectorX) (paths/HyperBasevector.cc:133-137, graph/DigraphTemplate.h:3107-3113):
 *                      "BINWRITE", int K, from_, to_ (per vertex a u32 count and the vertices at the other end), from_edge_obj_,
 *                      to_edge_obj_ (the edge ids), edges_ (as in a.hbv), to_left_, to_right_ (u64 count + ints).  The unitig arrays are
 *                      the ones the snk_hbv was built from (BVComp order), as for snk_write_hbv */
int snk_write_pathsx(const char* path, uint64_t n_reads, const int64_t* index, uint64_t n_index, const uint8_t* data, uint64_t n_bytes, char* err, size_t errcap);
int snk_read_pathsx(const char* path, uint64_t* n_reads, uint64_t* n_index, int64_t** index, uint64_t* n_bytes, uint8_t** data, char* err, size_t errcap);
int snk_write_hbx(const char* path, uint32_t K, uint64_t n_unitigs, const uint64_t* unitig_off, const uint8_t* unitig_bases, const snk_hbv* h, char* err,
                  size_t errcap);

/* ---- path extension: StageExtension ---------------------------------------------------------------------------------
 * ExtendPathsNew, lib/assembly/src/10X/Extend.cc:14-177 (StageExtension, 10X/runstages/RunStages.cc:159-174, called at 10X/DF.cc:676; DF
 * writes its second paths index from the result, DF.cc:690), with the HyperBasevectorX overload of ExtendPath
 * (paths/long/large/GapToyTools4.cc:477-555; min_gain 5, mode 1).  A function of (graph, reads, paths): the graph may be the one the
 * paths were made on or one a host has patched since.  Three legs per read, in this order, each on the result of the one before:
 *   1 backward, only with SNK_EXT_BACK (Extend.cc:25-61): while offset < 0 and To(ToLeft(p[0])) is not empty, the first in-edge e, in
 *     To-list order, whose bases agree with the read at every position l with l - offset - Kmers(e) >= 0 is put in front and Kmers(e)
 *     added to the offset; it stops when none agrees
 *   2 quality-aware (:63-95): the path is cut to its first edge, then ExtendPath runs.  It changes nothing when the offset is negative,
 *     the read does not reach beyond the first edge, or From(ToRight) is empty.  Otherwise it lists the continuations breadth-first in
 *     From-list order (GapToyTools4.cc:495-515): entries of len >= ext are not expanded but count, and reaching list index 101 fails
 *     (expanding entries 0..100 left more than 101).  Only entries with len >= ext are kept (:517-523); qsum = the read's raw quality
 *     summed over the mismatches against the edges' bases from K-1 on (:527-538); the best is taken iff it is the only one or beats
 *     the runner-up by at least 5 (:539-543) -- ties never decide, so the order among equals does not matter.  A read that is declined
 *     keeps the one-edge path
 *   3 exact (Extend.cc:97-177): the path is walked against the read; only if the walk runs off the path's last edge without a mismatch
 *     and before the read ends does it go on, base by base, stepping at an edge's end to the out-edge whose base K-1 equals the read's
 *     base.  The reference's loop has no break: several matching out-edges are all pushed.  That is refused here (below)
 * Arguments: the graph as for snk_dev_path_reads (bvcomp_order, NULL = the arrays are in BVComp order); of `in` the rows, lens (NULL =
 * read_len) and quals; the From / To lists are the ones a.hbv has.  paths stays valid and unchanged, as do the count result and earlier
 * stage results.  out->paths: offset / n_edges / start / edges as from snk_dev_path_reads (context memory, valid until the context's next
 * top-level call; path_ms = time of this call, the other fields 0).  The result depends on no tuning option and is bit-identical from
 * call to call.
 * SNK_E_ARG -- the reference would read outside a read or an edge: offset <= -len(read), offset >= Bases(p[0]), a path on a read of length
 * 0, and with SNK_EXT_BACK a read that ends inside the K-1 bases its first edge shares with its in-edges while leg 1 would run; further
 * an edge id outside the graph, start / n_edges that do not add up to n_edges_total, quals == NULL, read_len above 256, unknown flags.
 * SNK_E_UNSUPPORTED: an offset outside +-32767, given or made by leg 1 (the reference keeps the paths in a ReadPathVecX, on entry and
 * between its legs: an in-edge of more than 32767 k-mers put in front would wrap the offset), a path of more than 255 edges (given or made), a
 * vertex with more than four out-edges (the list of continuations is sized 1 + 101 x 4 = 405 entries; a.pathsX has two bits per branch),
 * two out-edges of one vertex with the same base at K-1 met by leg 3. */
typedef struct snk_dev_extend {
    snk_dev_paths paths;
    uint64_t n_back_extended;     /* reads whose path gained an edge in front (SNK_EXT_BACK) */
    uint64_t n_cut_to_first;      /* reads whose path of two or more edges left leg 2 as its first edge alone: ExtendPath did not re-extend it */
    uint64_t n_quality_extended;  /* reads ExtendPath extended (leg 2) */
    uint64_t n_ambiguous;         /* ... declined: runner-up within MIN_GAIN */
    uint64_t n_too_many;          /* ... declined: more than max_exts extensions */
    uint64_t n_exact_extended;    /* reads the exact-match leg (leg 3) extended */
    float ms;                     /* HIP events around the call's device work (graph tables included) */
    uint32_t reserved0;
    uint64_t n_enumerated;        /* reads that reached ExtendPath's enumeration (the listed, slow pass) */
    uint64_t reserved[5];
} snk_dev_extend;
#define SNK_EXT_BACK 1u
int snk_dev_extend_paths(snk_ctx* ctx, uint32_t K, const snk_dev_reads* in, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases,
                         const snk_hbv* h, const snk_dev_paths* paths, uint32_t flags, snk_dev_extend* out, void* stream, char* err, size_t errcap);

/* ---- pairs that disagree with the graph: MarkBads, a.bad ----------------------------------------------------------------
 * MarkBads, lib/assembly/src/10X/SecretOps.cc:70-107 (ReadPath) and :22-59 (ReadPathVecX): the first step of StageFindPatch
 * (10X/runstages/RunStages.cc:261; also :52).  DF keeps the result as a.bad (10X/DF.cc:644) and FindEdgePairs drops such pairs from its
 * "rights" (10X/Closomatic.cc:293,316).  For every read with a path p on the graph:
 *   m      = hb.Cat(p) (paths/HyperBasevector.cc:631-635), a chain of TrimCat (feudal/BaseVec.h:550-558): every edge but the last gives its
 *            first Kmers(e) bases, the last all of its own.  The edges need not be adjacent: where two disagree inside the K-1 bases
 *            they would share, m shows the LATER edge's
 *   badsum = the raw quality q[l] summed over the read positions l with 0 <= offset + l < |m| and read[l] != m[offset + l]; positions in
 *            front of m or behind it are skipped, not counted
 *   bad[i] = badsum > 150 for read 2i or read 2i + 1 (a read without a path contributes nothing; MAX_BAD and MIN_HQ of the source are unused)
 * flags = 0: offset is the path's int (the ReadPath overload).  SNK_BADS_X: the ReadPathVecX overload, which is what DF runs and what the
 * a.bad of a stock run holds -- the path has been through zip / unzip, so the offset is static_cast<int16_t>(offset): beyond +-32767 it
 * wraps and the read is compared where it does not lie.  That is reproduced (every position is range-checked: nothing is read out of
 * bounds); n_offsets_wrapped counts such reads in either mode.  With SNK_BADS_X the paths must be what snk_dev_paths_zip accepts and
 * snk_dev_paths_unzip gives back unchanged: at most 255 edges and no vertex with more than four out-edges (SNK_E_UNSUPPORTED), every
 * step e -> e' with e' in From(ToRight(e)) (SNK_E_ARG).
 * Arguments as for snk_dev_extend_paths: of `in` the rows, lens (NULL = read_len) and quals.  bad: u8[n_reads / 2], context memory,
 * valid until the context's next top-level call.  in, paths, the count result and earlier stage results stay valid and unchanged.  The
 * result is bit-identical from call to call and depends on no tuning option.
 * SNK_E_ARG: an odd n_reads (the reference asserts dup.size( ) * 2 == bases.size( )), paths->n_reads != n_reads, an edge id outside the
 * graph, an edge of fewer than K bases, start / n_edges that do not add up to n_edges_total, quals == NULL, read_len above 256, unknown
 * flags.  After any failure *out is all zero. */
#define SNK_BADS_X 1u     /* offsets as a ReadPathVecX holds them (int16): what DF's a.bad has */
typedef struct snk_dev_bads {
    uint64_t n_pairs;
    const void* bad;              /* u8[n_pairs] */
    uint64_t n_placed;            /* reads with a path */
    uint64_t n_mismatch_reads;    /* ... with at least one mismatch inside m, whatever its quality */
    uint64_t n_bad_reads;         /* ... with badsum > 150 */
    uint64_t n_bad_pairs;         /* pairs flagged */
    uint64_t n_offsets_wrapped;   /* reads with a path whose offset does not fit an int16 */
    float ms;                     /* HIP events around the device work, graph tables included (_df: the whole call, host clock) */
    uint32_t n_slabs;             /* launches of the comparison kernel: 1, or the slabs of the _df form */
    float tables_ms, kernel_ms;   /* the resident form's two parts: graph tables + the checks of the paths; the comparison kernel.  They take
                                     one of the reserved slots; the _df form leaves them 0 (its kernels run between the slabs' copies) */
    uint64_t reserved[5];
} snk_dev_bads;
int snk_dev_mark_bads(snk_ctx* ctx, uint32_t K, const snk_dev_reads* in, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases,
                      const snk_hbv* h, const snk_dev_paths* paths, uint32_t flags, snk_dev_bads* out, void* stream, char* err, size_t errcap);
/* The same over reads [first, first + n) of an opened reads.fastb / reads.qualp (snk_df_open), for a job whose quality rows are not
 * resident (the ASSEMBLER_DF ingest keeps 46 bytes per read): the files are decoded again slab by slab, the kernel runs on every slab
 * as it is decoded, and no more than the ring's slabs of quality rows ever exist.  paths: of reads [first, first + n), on the device.
 * first and slab_reads (0 = 262144; the ring takes 16 at least) must be even, so that mates never straddle slabs (SNK_E_ARG);
 * read_len, threads as for snk_dev_ingest_df.  The graph tables are built once per call.  The result is byte for byte the resident
 * form's; file errors as snk_dev_ingest_df's.  A slab whose quality bytes do not fit its slot is decoded in pieces cut where the bytes
 * say; a cut inside a pair is refused (SNK_E_UNSUPPORTED: more than 192 quality bytes per read on average over a slab). */
struct snk_df_files;      /* (snk_df_open, below) */
int snk_dev_mark_bads_df(snk_ctx* ctx, uint32_t K, struct snk_df_files* f, uint64_t first, uint64_t n, uint32_t read_len, uint32_t threads, uint64_t slab_reads,
                         uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, const snk_hbv* h, const snk_dev_paths* paths, uint32_t flags,
                         snk_dev_bads* out, char* err, size_t errcap);

/* ---- gap-patch candidates: FindEdgePairs, a.hops -------------------------------------------------------------------------
 * FindEdgePairs, lib/assembly/src/10X/Closomatic.cc:17-354: the second step of StageFindPatch (10X/runstages/RunStages.cc:263-266).
 * DF keeps the result as a.hops (10X/DF.cc:642-643); the closures that snk_dev_patch_pieces takes are made for these pairs.  The
 * result is the sorted set of (e1, e2) that three rules give.  Kmers(e) = bases - K + 1; a read's barcode class is its bc value (10x data:
 * bidc = N + bc, all bc == 0 reads are one class); `entries of e` are the reads of the paths index entry of e.
 *   sink(e)     every edge leaving ToRight(e) has at most 120 k-mers and ends in a vertex with no out-edge and one in-edge (an e with
 *               nothing behind it is a sink); source(e) is the mirror image over the edges entering ToLeft(e)
 *   keys        for every entry r of a sink e1 whose mate has a path: e2 = inv[last edge of the mate's path], e2 != e1, class of r
 *   part 1      (e1, e2) with keys of two classes or more, and source(e2) unless SNK_HOPS_ONE_GOOD
 *   part 2      for an e1 that is the first element of no part-1 pair: (e1, e2) with keys of two classes or more,
 *               Kmers(e2) >= 100 and ToRight(e1) != ToLeft(e2)
 *   part 3      for every e of K + 1 k-mers or more whose entries, with those of inv[e], are of two classes or more.  X = the path suffixes
 *               from every occurrence of e, the mates' paths reversed and inverted, the reversed and inverted prefixes up to every
 *               occurrence of inv[e].  From the members that begin with e, a sequence x grows by a member y that holds x's last edge
 *               at a place that is not its last and agrees with x wherever the two overlap; e is `extended` when some reachable x has 100
 *               k-mers or more behind its first edge.  If it is not: over the entries of pairs with bad == 0, too_easy = the edges behind e
 *               on the same path, can = (edge, class) of the mates' inverted paths and of the inverted prefixes ending in inv[e],
 *               both only edges of 40 k-mers or more other than e and inv[e]; (e, f) for every f of two classes in can that is
 *               not in too_easy
 * The closure of part 3 runs on the device over the set of sequences reached so far, at most ext_budget of them per edge (0 = the
 * default and the most, 128; a larger value counts as 128) in 4 096 ints; an edge that needs more, or that has more than 65 536 index
 * entries with a member of two edges or more, is finished by a host routine without a bound (n_ext_host counts them).  No result depends on the budget.  SNK_HOPS_EXT_HOST sends every closure to the host routine (tests).
 * paths: of snk_dev_path_reads or a later stage, and what snk_dev_paths_zip accepts and gives back unchanged (the reference reads a
 * ReadPathVecX): the refusals of SNK_BADS_X.  px: the paths index of these paths, or NULL (made inside the call).  d_bc: i32 per read;
 * d_bad: u8 per pair (snk_dev_mark_bads).  pairs: i32[2 * n_pairs], ascending by (first, second), context memory valid until the
 * context's next top-level call.  The result is bit-identical from call to call and depends on no tuning option.
 * SNK_E_ARG: an odd read count, an edge id outside the graph, an inv that is not an involution, a px whose n_hbv_edges or n_entries
 * do not match, unknown flags, NULL d_bc / d_bad with reads.  After any failure *out is all zero. */
#define SNK_HOPS_ONE_GOOD 1u   /* DF's ONE_GOOD=True; DF's default is False */
#define SNK_HOPS_EXT_HOST 2u   /* tests: every closure of part 3 on the host leg */
typedef struct snk_dev_hops {
    uint64_t n_pairs;
    const void* pairs;                         /* i32[2 * n_pairs], ascending (first, second) */
    uint64_t n_part1, n_part2, n_part3;        /* distinct pairs each part contributed, before the final unique */
    uint64_t n_sink_edges;                     /* edges with sink(e) */
    uint64_t n_long_edges;                     /* edges of K + 1 k-mers or more */
    uint64_t n_two_class;                      /* ... whose entries are of two classes or more = the next three */
    uint64_t n_ext_round0;                     /* ... extended by a member of X as it stands */
    uint64_t n_ext_closure;                    /* ... extended by the closure */
    uint64_t n_ext_host;                       /* closures the host routine finished (extended or not) */
    uint64_t n_not_extended;
    float ms, tables_ms;                       /* HIP events: the whole call; graph tables, checks of the paths and the index */
    uint32_t ext_budget;                       /* the budget the call ran with */
    float part12_ms, part3_ms;
    uint64_t reserved[4];
} snk_dev_hops;
int snk_dev_edge_pairs(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, const snk_hbv* h,
                       const int32_t* inv /* host */, const snk_dev_paths* paths, const snk_dev_pidx* px /* NULL: made inside */,
                       const void* d_bc /* i32 per read */, const void* d_bad /* u8 per pair */, uint32_t flags, uint32_t ext_budget /* 0 = default */,
                       snk_dev_hops* out, void* stream, char* err, size_t errcap);
/* a.hops = BinaryWriter::writeFile(vec<pair<int,int>>) (10X/DF.cc:642-643): "BINWRITE", u64 count, two i32 per pair.  snk_read_hops:
 * *pairs is malloc'ed (snk_host_free). */
int snk_write_hops(const char* path, uint64_t n_pairs, const int32_t* pairs, char* err, size_t errcap);
int snk_read_hops(const char* path, uint64_t* n_pairs, int32_t** pairs, char* err, size_t errcap);

/* ---- gap closures: CloseGap and CloseGap2, closures.fastb ---------------------------------------------------------------------
 * CloseGap2 / CloseGap, lib/assembly/src/10X/Closomatic.cc:480-657 / :356-459: the third step of StageFindPatch
 * (10X/runstages/RunStages.cc:334-384), run for every pair of a.hops.  The result is EXACTLY what DF writes as closures.fastb
 * (10X/DF.cc:645) with STACKSTER=False: Stackster, which adds more closures for the same pairs with DF's default STACKSTER=True, is not
 * part of this library.  Per pair (e1, e2), sides es = { e1, inv[e2] }:
 *   rows        of side e: for every index entry of e, in index order, every place j with p[j] == e -- pos = offset - sum Kmers(p[l < j]),
 *               forward; then the same over inv[e], the row reverse-complemented.  A read that visits the edge twice, or that the index
 *               lists twice, gives its rows as often.  Forward cells in front of the edge are dropped; nothing is cut at its end.
 *               M = the largest column over all rows; the stack keeps its last max_width columns and loses the rows without a cell
 *               there; the stack of inv[e2] is reversed (both are when e1 == inv[e2])
 *   CloseGap2   in front of that: followers = the (edge, distance) behind e along the paths (those on inv[e] through inv); a group of 5
 *               or more identical ones gives every 32-mer of that edge with its position; the partner of a forward read of side ei that is
 *               no forward row of side 1 - ei, and whose 32-mers are found there at exactly one distinct position - place, becomes a
 *               forward row at the END of side 1 - ei (ei = 0 first, ids ascending; the ids are taken before any partner is added)
 *   offsets     GetOffsets1 (paths/long/ReadStack.cc:1192-1512) on the two seed consensuses (quality sums as doubles in row order, Q0
 *               counts 0.1, Q1 and Q2 0.2; the LOWEST base on a tie): none if either has 1000 columns or more; 8-mer seeds; per offset
 *               bits = -10/6 x the minimum of log10(BinomialSum(n, k, 0.75)) over its windows, bad windows as written; bits >= 25; the
 *               invalidation with its flank of 10; big near small.  The table of log binomial sums is made once per context ON THE HOST with
 *               the reference's arithmetic (long double, pow, log10); the device only reads it
 *   closures    for at most two surviving offsets (more: none): stack 1's rows, then stack 2's shifted by the offset; per column the
 *               HIGHEST base on a tie (an empty column: T)
 * The result is in pair order, then offset order -- the order closures.fastb has.  Qualities are phred values of at most 63 (what the reference's PQVec holds).
 * in: packed rows, quality rows, lengths.  paths: plain ReadPaths (the reference reads a.paths here, RunStages.cc:326): offsets are ints,
 * nothing wraps, the refusals of SNK_BADS_X do not apply.  px: the paths index of these paths, or NULL (made inside the call).  d_pairs:
 * device i32[2 * n_pairs], the pairs of snk_dev_hops.  max_width: 0 = 400, DF's constant.
 * CloseGap2's 32-mers live in a hash table of device scratch per pair, sized by what the pair needs: bod_budget of them per side at most (0 = the default and the most, 262 144); a pair with a side over the budget
 * is finished by a host routine without a bound (n_place_host counts them).  No result depends on the budget.  SNK_CLOSE_PLACE_HOST sends
 * every pair's placement to the host routine (tests).
 * closure_off / bases are what snk_dev_patch_pieces and snk_patch_plan_sizes take (closure_off after a download).  Context memory valid
 * until the context's next top-level call.  The result is bit-identical from call to call and depends on no tuning option.
 * SNK_E_ARG: an odd read count, a pair id outside the graph, an inv that is not an involution, a px whose n_hbv_edges or n_entries do
 * not match, unknown flags, NULL reads with n_pairs > 0.  After any failure *out is all zero. */
#define SNK_CLOSE_CG1 1u          /* CloseGap (DF's CG2=False); without it CloseGap2, DF's default */
#define SNK_CLOSE_PLACE_HOST 2u   /* tests: every partner placement on the host leg */
typedef struct snk_dev_closures {
    uint64_t n_closures, n_bases, n_pairs;
    const void* closure_off;                   /* u64[n_closures + 1] */
    const void* bases;                         /* u8[n_bases]: base codes 0 .. 3 */
    const void* pair_first;                    /* u64[n_pairs + 1]: the closures of pair p are pair_first[p] .. pair_first[p + 1] */
    uint64_t n_pairs_0, n_pairs_1, n_pairs_2, n_pairs_many;   /* pairs by surviving offsets; more than two gives no closure (Closomatic.cc:647) */
    uint64_t n_rows;                           /* stack rows kept, both sides of every pair */
    uint64_t n_partners_tried, n_partners_placed;
    uint64_t n_followers;                      /* (edge, distance) groups of 5 or more */
    uint64_t n_cons_too_long;                  /* pairs with a consensus of 1000 columns or more */
    uint64_t n_place_host;                     /* pairs whose placement the host routine did */
    float ms, tables_ms;                       /* HIP events: the whole call; graph tables, checks, the index */
    float gather_ms, close_ms;                 /* rows and placement; offsets and closures */
    uint32_t max_width, bod_budget;            /* what the call ran with */
    uint64_t reserved[4];
} snk_dev_closures;
int snk_dev_close_gaps(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, const snk_hbv* h,
                       const int32_t* inv /* host */, const snk_dev_reads* in, const snk_dev_paths* paths, const snk_dev_pidx* px /* NULL: made inside */,
                       uint64_t n_pairs, const void* d_pairs /* i32[2 * n_pairs] */, uint32_t max_width /* 0 = 400 */, uint32_t flags,
                       uint32_t bod_budget /* 0 = default */, snk_dev_closures* out, void* stream, char* err, size_t errcap);
/* closures.fastb = BinaryWriter::writeFile(vec<basevector>) (10X/DF.cc:645) is the layout snk_write_bv writes and snk_read_bv reads. */

/* ---- gap patches into the graph: StageInsertPatch ---------------------------------------------------------------------
 * StageInsertPatch, lib/assembly/src/10X/runstages/RunStages.cc:176-230 (10X/DF.cc:656): the graph is rebuilt from its own edges, the
 * junction (K+1)-mers and the closure sequences that StageFindPatch found (BuildAll, paths/long/large/GapToyTools4.cc:187-214;
 * readsToHBV_Sleek, kmers/BigKPather.cc:1528-1647: every k-mer, no frequency, barcode or quality rule, no prune), every old edge is
 * pathed over the new graph (Pather_sleek, :594-630 -> to3, left3, RunStages.cc:207-214) and every read path moved onto it
 * (TranslatePaths, GapToyTools4.cc:220-266).  The result is the graph StageExtension (snk_dev_extend_paths) and the second paths index
 * work on.  The graph itself is built by snk_dev_count_graph and snk_dev_hbv; the calls here stand around them:
 *
 *   snk_patch_plan_sizes   host only: the rows snk_dev_patch_pieces will write.
 *   snk_dev_patch_pieces   the sequences as rows for the count stage (row_words 16, read_len 256, lens = good_len = the piece's length, no
 *                          quality rows, no barcodes): the old unitigs (an edge and its reverse complement hold the same k-mers), one
 *                          (K+1)-mer per pair e1 in To(v), e2 in From(v) -- the last K bases of e1 and base K-1 of e2 --, the closures.  A
 *                          sequence of more than K bases becomes pieces of at most 256 bases, consecutive ones overlapping by K: each of
 *                          its (K+1)-mers lies in one piece and every piece has K+1 bases at least.  A sequence of fewer than K bases is
 *                          skipped.  One of exactly K bases has no piece; its canonical k-mer is listed in d_lonely (ascending, distinct,
 *                          16 bytes each as snk_dev_result.keys).
 *   snk_dev_count_graph    on the rows with min_freq = 1, min_bc = 0, bc = NULL, flags 0.
 *   snk_dev_patch_merge    a listed k-mer that the new table does not hold is a one-k-mer unitig (an isolated old edge of K bases, a
 *                          closure of K bases that is new): merged into the count result's unitigs in their order (by first K bases).
 *                          Without such a k-mer the result IS the count result's arrays.
 *   snk_dev_hbv            on those unitigs: the new edge numbering is the library's own.
 *   snk_dev_patch_paths    to3 / left3 per OLD edge and the translated paths.  TranslatePaths per read: an empty path stays empty;
 *                          start = offset + left3[p[0]]; to3[p[0]] empty: cleared; start < Bases(to3[p[0]][0]): that edge at start (a
 *                          negative start lands here); else q = OverlapAppend over the to3[p[j]] up to the first empty one (the LONGEST
 *                          suffix / prefix overlap is not repeated, Vec.h:604-619), and while start >= Bases(q[trim]) start -= Kmers(q[trim]),
 *                          ++trim: q[trim] at start, or cleared when trim runs off q.  A translated path has at most ONE edge.
 *
 * MEMORY.  snk_dev_count_graph is a top-level call: at its start everything the context handed out before is free again.  So the rows, the
 * lengths and the k-mer list are written into buffers the CALLER owns, and whatever a later step reads -- the old unitig arrays, the
 * closures, the paths -- must by then live in caller-owned memory too (a copy of the earlier count result's unitigs, not the result).
 * The results of snk_dev_patch_merge and snk_dev_patch_paths are context memory, valid until the context's next top-level call; they,
 * the count result and the caller's arrays stay valid and unchanged across the calls here.
 *
 * Arguments.  unitig_off / closure_off are HOST arrays (u64[n + 1], from 0): the sizes come from them without a device round trip;
 * d_unitig_bases / d_closure_bases the base codes on the device.  h: HOST, the graph of the old unitigs (bvcomp_order maps its unitig
 * numbering to the arrays, NULL = they are in BVComp order; the From / To lists are those of the function snk_write_hbv uses).
 * piece_capacity / lonely_capacity: what d_rows (u32[16 x pieces]), d_lens (u16[pieces]) and d_lonely hold; less than the plan: SNK_E_ARG.
 * paths: on the OLD graph, offset as int32.  out->paths.offset is int32 (snk_dev_paths_zip does the int16 wrap, as pathsX.append does).
 * SNK_E_ARG: a closure base code above 3 (pieces); an edge id outside the old graph, start / n_edges that do not add up to n_edges_total,
 * an old edge whose k-mers are not on the new graph (paths).  The result rule and the call frame of the stages after the graph apply:
 * after any non-zero return *out is all zero.  Results are bit-identical from call to call and depend on no tuning option. */
typedef struct snk_patch_plan {
    uint64_t n_pieces;            /* rows: n_unitig_pieces + n_junctions + n_closure_pieces, in this order */
    uint64_t n_unitig_pieces, n_junctions, n_closure_pieces;
    uint64_t n_lonely_max;        /* sequences of exactly K bases: the most k-mers d_lonely can get */
    uint64_t reserved[3];
} snk_patch_plan;
int snk_patch_plan_sizes(uint32_t K, uint64_t n_unitigs, const uint64_t* unitig_off, const snk_hbv* h, uint64_t n_closures, const uint64_t* closure_off,
                         snk_patch_plan* out, char* err, size_t errcap);
typedef struct snk_dev_pieces {
    uint64_t n_pieces, n_lonely;
    float ms;                     /* HIP events around the call's device work */
    uint32_t reserved0;
    uint64_t reserved[5];
} snk_dev_pieces;
int snk_dev_patch_pieces(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const uint64_t* unitig_off, const void* d_unitig_bases, const snk_hbv* h, uint64_t n_closures,
                         const uint64_t* closure_off, const void* d_closure_bases, uint64_t piece_capacity, void* d_rows, void* d_lens, uint64_t lonely_capacity,
                         void* d_lonely, snk_dev_pieces* out, void* stream, char* err, size_t errcap);
typedef struct snk_dev_patch_unitigs {
    uint64_t n_unitigs, unitig_total_bases;
    const void* unitig_off;       /* u64[n_unitigs + 1] */
    const void* unitig_bases;     /* as snk_dev_result's: canonical, ordered by their first K bases */
    uint64_t n_added;             /* one-k-mer unitigs merged in */
    float ms;
    uint32_t reserved0;
    uint64_t reserved[4];
} snk_dev_patch_unitigs;
int snk_dev_patch_merge(snk_ctx* ctx, uint32_t K, const snk_dev_result* res, const void* d_lonely, uint64_t n_lonely, snk_dev_patch_unitigs* out, void* stream,
                        char* err, size_t errcap);
typedef struct snk_dev_patched {
    snk_dev_paths paths;          /* translated: n_edges is 0 or 1; path_ms = the translation */
    uint64_t n_old_edges, n_to3;
    const void* to3_off;          /* u64[n_old_edges + 1] */
    const void* to3;              /* i32[n_to3] new edge ids */
    const void* left3;            /* i32[n_old_edges] */
    uint64_t n_first;             /* reads kept on the first new edge of their first old edge */
    uint64_t n_later;             /* reads moved to a later edge of q */
    uint64_t n_cleared;           /* reads whose path was cleared */
    float ms, map_ms;             /* HIP events: the whole call; the graph tables, the look-ups and to3 / left3 */
    uint64_t reserved[4];
} snk_dev_patched;
int snk_dev_patch_paths(snk_ctx* ctx, uint32_t K, uint64_t n_old_unitigs, const void* d_old_unitig_off, const void* d_old_unitig_bases, const snk_hbv* h_old,
                        uint64_t n_new_unitigs, const void* d_new_unitig_off, const void* d_new_unitig_bases, const snk_hbv* h_new, const snk_dev_paths* paths,
                        snk_dev_patched* out, void* stream, char* err, size_t errcap);

/* ---- graph edits: DeleteEdges + Cleanup, and the hanging-end trim ------------------------------------------------------
 * Every simplification step of the reference after DF picks edges, deletes them (hbv.DeleteEdgesParallel(dels)) and cleans up
 * (Cleanup, lib/assembly/src/paths/long/large/GapToyTools.cc:1287-1302).  snk_dev_delete_edges is that pair; snk_dev_hanging_ends is
 * the first selection the reference runs through it, the hanging-end rule of StageTrim (10X/runstages/RunStages.cc:91-146).
 *
 * snk_dev_delete_edges, in the reference's order:
 *   1 the edges of dels (any order, duplicates allowed, closed under inv) leave the From / To lists;
 *   2 every path is cut at its first deleted edge (GapToyTools.cc:1290-1297); a path cut to nothing keeps its offset;
 *   3 RemoveUnneededVertices2 (GapToyTools3.cc:487-667): a vertex with one in-edge and one out-edge whose predecessor and successor
 *     vertices differ (:520-527) is unneeded; from the highest such vertex down (:541-563) the maximal chain through it gives a run
 *     eleft .. eright; a run is merged with its reverse complement when eleft < inv[eright] (:571) -- a run that is its own reverse
 *     complement never is -- and a circle made only of unneeded vertices comes out as eleft == eright = the edge that leaves its highest
 *     vertex, which is created again under a new id when it is smaller than its inverse.  The runs are taken from the back of the list
 *     (:607-633): pair i gives the inverse run E_old + 2 i and the canonical run E_old + 2 i + 1; a new edge's bases are the TrimCat of
 *     its run; offsets[e] = the k-mers of the run in front of e.  Paths (:653-664): offset += offsets[first edge], every edge renumbered,
 *     consecutive equal ids collapse to one;
 *   4 CleanupCore (GapToyTools.cc:1253-1285): the surviving edges are compacted in id order (new edges behind the old ones), inv and
 *     the paths renumbered, vertices without an edge removed and the rest compacted in id order.
 * The From / To lists of the result are those snk_hbv_lists_build derives (AddEdge inserts by upper_bound, deletions keep the order), so
 * snk_write_hbv / snk_write_hbx on the result write the reference's files.
 *
 * Arguments: the graph as every stage after the graph takes it (d_unitig_off u64[n_unitigs + 1] and d_unitig_bases on the device, h on
 * the host with bvcomp_order or NULL), inv i32[h->n_edges] on the host, the paths on the device, dels on the host.  flags must be 0.
 * Result: device unitig arrays with ONE unitig per pair {e, inv[e]} of the new graph, numbered by the pair's smaller edge id and stored as
 * that edge reads (a self-inverse edge once); out->h over them (bvcomp_order NULL), out->inv, out->edge_map / edge_koff per OLD edge (its
 * new id or -1; its k-mer offset inside the new edge) on the host -- all four freed by snk_dev_edit_free --; the rewritten paths on the
 * device.  The device arrays are context memory, valid until the context's next top-level call; the result goes into a second
 * snk_dev_delete_edges, snk_dev_paths_zip, snk_dev_paths_index and snk_dev_extend_paths as it is.
 * The path rewrite and the copy of the bases run on the device; the vertex classes, the runs and the id hand-out run on the host (one
 * pass over the edges, the reference's own walk).
 * SNK_E_ARG: an edge id in dels or in a path outside [0, E) (the reference cuts such a path; every stage here refuses the id), inv that
 * is not an involution, dels not closed under inv, start / n_edges that do not add up, a path whose consecutive edges do not meet at
 * a vertex (the reference's Validate asserts), flags other than 0.  The result rule of the stages after the graph applies. */
typedef struct snk_dev_edit {
    uint64_t n_unitigs, unitig_total_bases;
    const void* unitig_off;       /* u64[n_unitigs + 1], device */
    const void* unitig_bases;     /* u8 codes, device */
    snk_hbv h;                    /* host */
    int32_t* inv;                 /* host i32[h.n_edges] */
    snk_dev_paths paths;          /* device; path_ms = the rewrite */
    uint64_t n_old_edges;
    int32_t* edge_map;            /* host i32[n_old_edges]: new id, -1 = deleted */
    int32_t* edge_koff;           /* host i32[n_old_edges]: k-mers of the new edge in front of the old one */
    uint64_t n_deleted;           /* distinct edges of dels */
    uint64_t n_runs;              /* new edges made (a run and its inverse count as two) */
    uint64_t n_absorbed;          /* old edges that went into them */
    uint64_t max_run;             /* edges of the longest run */
    uint64_t n_truncated;         /* paths cut at a deleted edge */
    uint64_t n_emptied;           /* ... of which cut to nothing */
    uint64_t n_collapsed;         /* path entries dropped because they repeat the new edge in front of them */
    float ms, graph_ms;           /* HIP events: the whole call; wall clock of the host's part inside it */
    uint64_t reserved[4];
} snk_dev_edit;
int snk_dev_delete_edges(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, const snk_hbv* h, const int32_t* inv,
                         const snk_dev_paths* paths, const int32_t* dels, uint64_t n_dels, uint32_t flags, snk_dev_edit* out, void* stream, char* err, size_t errcap);
void snk_dev_edit_free(snk_dev_edit* r);      /* the host arrays; the device arrays are the context's */
/* snk_dev_hanging_ends: rs[e] = over all path entries x, (x == e) + (inv[x] == e) (RunStages.cc:94-119: a self-inverse edge counts
 * twice per entry, unlike a.countsb); an edge with rs[e] == 0 and at most max_kmers k-mers (the reference: 200) is deleted together
 * with inv[e] when its left vertex has no in-edge and exactly one out-edge, or its right vertex has no out-edge and exactly one
 * in-edge (:128-141).  The counts are made without atomics on global memory: up to SNK_HANG_LDS_MAX edges every workgroup counts its
 * share of the entries in LDS and the per-workgroup tables are summed; above that the entries are sorted and every edge finds its run.
 * The call chooses by size; flags may force either leg (tests).  support: i32[E] on the device (context memory); dels: ascending,
 * distinct, on the host, freed by snk_host_free.  SNK_E_ARG as for snk_dev_delete_edges (the entries' ids, inv, the path table; the LDS
 * leg forced above SNK_HANG_LDS_MAX edges). */
#define SNK_HANG_LDS 1u
#define SNK_HANG_SORT 2u
#define SNK_HANG_LDS_MAX 16384u
typedef struct snk_dev_hanging {
    uint64_t n_hbv_edges, n_entries;
    const void* support;          /* i32[n_hbv_edges], device */
    uint64_t n_dels;
    int32_t* dels;                /* host */
    uint64_t n_unsupported;       /* edges with rs == 0 */
    uint32_t leg;                 /* SNK_HANG_LDS or SNK_HANG_SORT: the one that ran */
    float ms;
    uint64_t reserved[4];
} snk_dev_hanging;
int snk_dev_hanging_ends(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, const snk_hbv* h, const int32_t* inv,
                         const snk_dev_paths* paths, uint32_t max_kmers, uint32_t flags, snk_dev_hanging* out, void* stream, char* err, size_t errcap);
/* snk_dev_mow_lawn: MowLawn (10X/Lawnmower.cc:301-554, the ReadPathVecX overload StageTrim calls at 10X/runstages/RunStages.cc:84), the
 * weak-branch rule that picks StageTrim's first batch of deletions.  Kmers(e) = bases - K + 1.
 *   candidate   (v, e1, e2): To(v) = {e1, e2} (both orders are tried), From(v) has one edge, Kmers(e2) <= Kmers(e1), and the left vertex of
 *               e2 has no in-edge and exactly one out-edge;
 *   read limit  npe = the path entries equal to e2 plus those equal to inv[e2] (a self-inverse e2 counts twice per entry), over reads
 *               whose pair is not dup; a candidate with npe > 2 is dropped;
 *   windows     n = Kmers(e2), del = Kmers(e1) - n; x1 = bases [del, del + n) of e1, x2 = bases [0, n) of e2;
 *   records     for e = e1 (pass 1), then e = e2 (pass 2): every entry of e at a path position l that is not the last (fw) and every
 *               entry of inv[e] at a position l >= 1 (not fw), of a read whose pair is not dup and that has fewer than 5 mismatches of
 *               quality >= 30 against hb.Cat(path) at the path's offset (positions off the sequence are skipped; the offset is the
 *               ReadPathVecX's, static_cast<int16_t>).  offset_l = the offset minus the k-mers of the edges in front of l.  A fw read has
 *               base m at epos = offset_l + m; a read that is not fw is reverse-complemented, its qualities reversed, and starts at
 *               epos = Bases(e) - offset_l - len.  In pass 1 epos is lowered by del.  Over 0 <= epos < n, q1 sums the qualities where
 *               the read differs from x1 and q2 where it differs from x2; (fw, offset_l, q1 - q2) is a record when q1 != q2;
 *   decision    the records are grouped by (fw, offset_l); a group whose smallest and largest difference have the same sign is worth
 *               min(largest magnitude, 50), to z2 when positive, to z1 when negative; qss1 / qss2 = the sum of z1 / z2 without its
 *               largest value; e2 and inv[e2] are deleted when qss1 >= 300 and qss2 <= 30.
 * An entry whose read does not reach the window makes no record, and a group keeps only its extremes, so every path entry is
 * visited once and the window test -- arithmetic on offset, length, del and n -- runs before a base or a quality is loaded.
 *
 * Arguments: the graph as for snk_dev_delete_edges; the reads as for snk_dev_mark_bads (rows, quality rows, lens); d_dup the u8 per PAIR
 * that snk_dev_mark_dups returns; the paths of these reads, which must be what snk_dev_paths_zip accepts and gives back unchanged (the
 * refusals of SNK_BADS_X).  flags must be 0.
 * Result: dels on the host, ascending and distinct, freed by snk_host_free; scored, i32[4 * n_scored] on the device (context memory):
 * (e1, e2, qss1, qss2) ascending by (e2, e1), one row per candidate that passed the read limit -- what the reference prints when it is
 * given a `tests` list.  The candidates and the two thresholds are edge-sized work and run on the host; the read limit, the work items,
 * the scoring, the sort and the group reductions run on the device.  No atomic decides anything but an integer sum: the result is the
 * same bytes from call to call.
 * SNK_E_ARG: as for snk_dev_hanging_ends and snk_dev_mark_bads with SNK_BADS_X, an odd read count, NULL d_dup with reads, flags != 0. */
typedef struct snk_dev_mow {
    uint64_t n_dels;
    int32_t* dels;                /* host */
    uint64_t n_scored;
    const void* scored;           /* i32[4 * n_scored], device */
    uint64_t n_candidates;        /* (v, e1, e2) that pass the graph's part of the rule */
    uint64_t n_too_many_reads;    /* ... dropped by the read limit */
    uint64_t n_entries_on_candidates; /* (path entry, role) of a non-dup read on e1, e2 or an inverse of a candidate that passed the read
                                         limit, at a position the rule takes */
    uint64_t n_entries_in_window; /* ... whose read reaches the window: the work items */
    uint64_t n_reads_hq_excluded; /* work items whose read has 5 or more mismatches of quality >= 30 */
    uint64_t n_records;           /* work items with q1 != q2 that pass the filter */
    uint64_t n_groups;            /* distinct (candidate, fw, offset_l) among them */
    uint64_t n_groups_mixed_sign; /* groups that count for nothing */
    uint64_t n_deleted_candidates;
    float ms, tables_ms;          /* HIP events: the whole call; the graph tables and the checks of the paths */
    float phase_ms[6];            /* candidates (host, wall clock), read limit, work items, scoring, sort, decision */
    uint64_t reserved[4];
} snk_dev_mow;
int snk_dev_mow_lawn(snk_ctx* ctx, uint32_t K, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases, const snk_hbv* h, const int32_t* inv /* host */,
                     const snk_dev_reads* in, const snk_dev_paths* paths, const void* d_dup /* u8 per pair */, uint32_t flags, snk_dev_mow* out, void* stream, char* err,
                     size_t errcap);

/* ---- the edge -> barcode lists: a.ebcx ------------------------------------------------------------------------------
 * computeEdgeToBarcodeX, lib/assembly/src/10X/PathsIndex.cc:297-358 (StageEBC, 10X/runstages/RunStages.cc:31-38): per HBV edge the
 * barcodes whose reads visit it -- stored as a.ebcx, the file every scaffolding step of the reference opens first.  The reference takes
 * the reads one barcode's run at a time (bci: the start of every run; reads sorted by barcode), collects {e, inv[e]} over the path
 * entries of a run whose first read has bc > 0, UniqueSorts them (:313-322) and appends the run's barcode to the list of every edge of
 * that set, run by run (:344-355).  Here every path entry of a read with bc > 0 gives the two keys (e, bc) and (inv[e], bc); one stable
 * radix sort and a distinct step leave the lists.
 *   paths        of snk_dev_path_reads (edge ids = HBV edge ids; edges 4-byte aligned); it stays valid across the call, as for
 *                snk_dev_paths_index
 *   d_bc         DEVICE array, int32[n_reads]: the barcode of every read (<= 0: none, the read contributes nothing)
 *   inv          HOST array, int32[n_hbv_edges], of snk_hbv_involution
 *   flags        0 or SNK_EBC_GENERAL_SORT
 * Contract: the list of edge e is the ascending set of the distinct bc[r] > 0 over the reads r whose path holds e or inv[e].  It is a
 * pure function of (paths, bc, inv): independent of the order of the reads, of `flags` and of every tuning option, and bit-identical
 * from call to call.
 *   - On reads sorted by barcode with one value per run (what 10X/DF.cc:464-469 makes: bc is the run's ordinal) this IS the reference's
 *     output, list by list.
 *   - Two separate runs that carry the same value: the reference would list the value twice, here it is listed once.  DF never makes
 *     that input.
 *   - An empty run contributes nothing (there are no runs here, only reads).  The reference reads bc[bci[b]] of an empty last run out of
 *     bounds (:311,345).
 * Device memory of the context, valid until its next top-level call.  SNK_E_ARG: a NULL argument, an inv that is not an involution, an
 * edge id outside [0, n_hbv_edges), start / n_edges that do not add up to n_edges_total (a read outside the entry table, or more entries
 * in the reads with a barcode than the table has), unknown flag bits.  SNK_E_UNSUPPORTED: n_edges_total >= 2^31 (two keys are sorted per
 * path entry).  *out is all zero after any refusal. */
typedef struct snk_dev_ebcx {
    uint64_t n_hbv_edges, n_ebc;         /* n_ebc = sum of the list lengths */
    const void* ebc_off;                 /* u64[n_hbv_edges + 1] */
    const void* ebc;                     /* i32[n_ebc]: the barcodes of edge e are ebc[ebc_off[e] .. ebc_off[e + 1]), strictly ascending */
    uint64_t n_keys;                     /* (edge, barcode) keys that went into the sort: two per path entry of a read with bc > 0 */
    uint64_t n_empty_edges, max_list;    /* edges without a barcode; the longest list */
    uint32_t bc_sorted;                  /* 1: bc was non-decreasing over the reads with bc > 0 */
    uint32_t general_sort;               /* 1: the full (edge, barcode) key was sorted; 0: the edge bits only (bc_sorted and no flag) */
    uint32_t key_bits;                   /* bits of an edge id the sort looked at */
    float ms;                            /* HIP events around the whole call (the upload of inv and the sizing read-back included) */
    uint64_t reserved[6];
} snk_dev_ebcx;
#define SNK_EBC_GENERAL_SORT 1u          /* take the full-key sort even when bc is sorted */
int snk_dev_edge_barcodes(snk_ctx* ctx, const snk_dev_paths* paths, const void* d_bc, uint64_t n_hbv_edges, const int32_t* inv, uint32_t flags,
                          snk_dev_ebcx* out, void* stream, char* err, size_t errcap);
/* The file (host arrays; no GPU needed), byte for byte what VecIntVec::WriteAll leaves:
 *   snk_write_ebcx   a.ebcx = feudal MasterVec<SerfVec<int>> in its single-file form (the family of a.paths.inv): control block (count,
 *                    flags 1, no fixed-length data, sizeof(SerfVec<int>) = 16, sizeof(int) = 4), the lists back to back as int32, the
 *                    table of n_hbv_edges + 1 file offsets
 *   snk_read_ebcx    the same file back; *ebc_off and *ebc are malloc'ed (snk_host_free).  SNK_E_IO: a file that does not add up (control
 *                    block, offset table and size disagree, or the offsets decrease or leave the data) */
int snk_write_ebcx(const char* path, uint64_t n_hbv_edges, const uint64_t* ebc_off, const int32_t* ebc, char* err, size_t errcap);
int snk_read_ebcx(const char* path, uint64_t* n_hbv_edges, uint64_t** ebc_off, int32_t** ebc, char* err, size_t errcap);

/* ---- f3: barcode ids on the device --------------------------------------------------------------
 * BcIndexer, lib/tada/src/utils.rs:101-164: whitelist line -> index (identical lines: the last one wins); a read's
 * barcode field "SEQ[-gg][,raw]" (FASTH line 6, lib/tada/src/multifastq.rs:72-126) gets
 *     id = index(SEQ) + 1 + (gg - 1) * lines(whitelist),   gg = 1 without a "-gg" suffix,   0 = not on the whitelist.
 * snk_bc_index_create takes the bytes of the whitelist file (lines of at most 32 bytes, any characters);
 * snk_dev_bc_ids reads n_reads fields of `stride` bytes each (zero padded, resident in HBM) and writes int32 ids.
 * Errors follow the reference's panics: a gem group that is not a decimal u8 ("invalid gem group string", :138),
 * an id beyond 2^31 ("BC id overflowed", :157). */
typedef struct snk_bc_index snk_bc_index;
int snk_bc_index_create(snk_ctx* ctx, const char* whitelist, size_t bytes, snk_bc_index** out, char* err, size_t errcap);
void snk_bc_index_destroy(snk_bc_index* ix);
uint32_t snk_bc_index_lines(const snk_bc_index* ix);
int snk_dev_bc_ids(snk_ctx* ctx, const snk_bc_index* ix, const void* d_fields, uint32_t stride, uint64_t n_reads, void* d_ids,
                   void* stream, char* err, size_t errcap);

/* ---- stage-input formats of ASSEMBLER_DF (mro/_assembler_stages.mro:24-39) ----------- */
/* reads.fastb = feudal MasterVec<BaseVec>: 24-byte control block (feudal/FeudalControlBlock.h:157-166), the packed
 * bases (2 bits, base j at bits 2*(j%4), feudal/FieldVec.h:586-603), (N+1) u64 file offsets, N u32 lengths.
 * Output: packed rows in libsnk's layout (row_words = ceil(max_len/16)), lengths; malloc'ed, free() them. */
int snk_read_fastb(const char* path, uint64_t* n_reads, uint32_t* max_len, uint16_t** lens, uint32_t** rows, char* err,
                   size_t errcap);
/* reads.qualp = feudal MasterVec<PQVec>: per read a chain of byte-aligned blocks [nQs:8][nBits:3][minQ:6][nQs x nBits]
 * ended by a 0 byte (feudal/PQVec.cc:86-127).  quals: caller buffer n_reads*qstride (raw phred). */
int snk_read_qualp(const char* path, uint64_t n_reads, uint32_t qstride, uint8_t* quals, char* err, size_t errcap);
/* reads.bci = BINWRITE vec<int64_t>: bci[b]..bci[b+1] = read range of barcode ordinal b, b = 0 unbarcoded
 * (10X/ParseBarcodedFastqs.cc:284-293); expanded to one barcode id per read as DF does (10X/DF.cc:464-469). */
int snk_read_bci(const char* path, uint64_t n_reads, int32_t* bc_per_read, uint64_t* n_barcodes, char* err, size_t errcap);

/* The same three files decoded ON THE DEVICE, at the rate the bytes can be moved (supernova_amd/csrc/snk_dfin.hip): the reference loads
 * reads.fastb with bases.ReadAll and walks reads.qualp through VirtualMasterVec<PQVec> (10X/DF.cc:265-272,345,595-597; block codec
 * feudal/PQVec.cc:86-200; barcode index expansion DF.cc:464-469) -- offset-indexed, uncompressed files.  Here the raw byte ranges of a
 * slab of reads go from the page cache into a page-locked ring (a pool of `threads` pread workers, 0 = chosen from the CPU budget), up in
 * one copy per section, and three kernels make packed rows, quality rows, lengths and barcode ids of them; the host parses nothing but the
 * control blocks and the barcode index.
 *   snk_df_open       control blocks + the barcode index (bci may be NULL: no ids); nothing else is read
 *   snk_dev_ingest_df reads [first, first + n) -> resident device arrays as snk_dev_ingest_fasth's (release: snk_dev_ingest_free).  A rank
 *                     of the N-GPU job passes ITS range and touches only those bytes.  read_len = row length in bases, 0 = the longest
 *                     read of the file (one scan of its length table, on the device; snk_df_max_len does the scan for a range);
 *                     slab_reads: reads per slab, 0 = 262144
 *   snk_dev_ingest_df_count_graph   the slabs -> unitigs.  Default: a slab's quality rows are trimmed as soon as they are decoded and dropped;
 *                     packed rows, good lengths and barcode ids of the job stay (46 bytes per read, owned by the context) and the resident
 *                     step runs on them -- with its look at the first buckets, its second partition and its choice of count kernel, which
 *                     is what real (error-rich) reads need from the first call of a process on.  Option df_stream = 2: the slabs are
 *                     appended to a streamed job instead (snk_dev_stream_*: partitioned as they arrive, the reads never resident in any
 *                     form).  res as snk_dev_count_graph's, bit-identical either way.  stats: rows / quals / lens / bc stay NULL;
 *                     text_bytes = file bytes moved; n_files = 4 compact, 3 streamed.
 * Errors follow the host readers': SNK_E_IO for a bad offset / length / truncated quality block, SNK_E_ARG for a quality chain longer
 * than a row (the message names the first offending read). */
typedef struct snk_df_files snk_df_files;
typedef struct snk_df_info {
    uint64_t n_reads, n_barcodes;                 /* n_barcodes = entries of the index - 1 (ordinal 0 = unbarcoded), 0 without one */
    uint64_t fastb_bytes, qualp_bytes, bci_bytes;
    uint64_t reserved[3];
} snk_df_info;
struct snk_dev_ingest;
int snk_df_open(const char* fastb, const char* qualp, const char* bci, snk_df_files** out, snk_df_info* info, char* err, size_t errcap);
void snk_df_close(snk_df_files* f);
int snk_df_max_len(snk_ctx* ctx, snk_df_files* f, uint64_t first, uint64_t n, uint32_t* max_len, char* err, size_t errcap);
int snk_dev_ingest_df(snk_ctx* ctx, snk_df_files* f, uint64_t first, uint64_t n, uint32_t read_len, uint32_t threads, uint64_t slab_reads,
                      struct snk_dev_ingest* out, char* err, size_t errcap);
/* reads [first, first + n) in their compact form: packed rows, GOOD LENGTHS (the trim at K / min_qual runs on every slab as it is decoded, the
 * quality rows are never resident) and barcode ids: 46 instead of 204 bytes per 150-base read, all that count + graph needs (snk_dev_reads.good_len) */
int snk_dev_ingest_df_trimmed(snk_ctx* ctx, snk_df_files* f, uint64_t first, uint64_t n, uint32_t read_len, uint32_t threads, uint64_t slab_reads, uint32_t K,
                              uint32_t min_qual, struct snk_dev_ingest* out, char* err, size_t errcap);
int snk_dev_ingest_df_count_graph(snk_ctx* ctx, snk_df_files* f, uint64_t first, uint64_t n, uint32_t read_len, uint32_t threads, uint64_t slab_reads,
                                  const snk_params* p, int64_t ign_bc_below, snk_dev_result* res, struct snk_dev_ingest* stats, char* err, size_t errcap);
/* Writers of the triple (tests, bench.py's df_seam row, tools): feudal/FeudalFileWriter.cc:18-140, PQVec.cc:86-127,
 * BinaryWriter::writeFile(vec<int64_t>).  The reads must be ordered by barcode id (>= 0) -- the index holds one read range per ordinal
 * (10X/ParseBarcodedFastqs.cc:284-293).  The quality block choice is the writer's own (any chain of valid blocks decodes alike);
 * adversarial != 0 seeds random block cuts and wider-than-needed values, 1 = a block per value (decoder tests).  snk_synth_df_write: reads [first, first + n) of
 * the synthetic model (sp->unbarcoded_ppm must be 0); qual_jitter > 1 spreads the model's Q30 over [30, 30 + jitter) -- the same trim,
 * a quality file of realistic entropy. */
int snk_write_df(const char* head, uint64_t n, const uint32_t* rows, uint32_t row_words, const uint16_t* lens, uint32_t read_len, const uint8_t* quals,
                 uint32_t qstride, const int32_t* bc, uint32_t threads, uint64_t adversarial, char* err, size_t errcap);
int snk_synth_df_write(const char* head, const snk_synth_params* sp, uint64_t first, uint64_t n, uint32_t qual_jitter, uint32_t threads, char* err,
                       size_t errcap);

/* FASTH = the barcode-sorted read-pair text format of the tada stages (MultiFastqIter, lib/tada/src/multifastq.rs:69-127):
 * gzip, 9 lines per pair (header, R1, Q1, R2, Q2, barcode field, 3 ignored lines).  Returns malloc'ed arrays (free with
 * snk_host_free): ASCII bases and raw phred values in rows of `stride` bytes (read 2q = R1, 2q+1 = R2, cmd_msp.rs:160-181),
 * lengths, and one zero-padded 64-byte barcode field per PAIR (part before the first ',') for snk_dev_bc_ids. */
int snk_read_fasth(const char* path, uint32_t stride, uint64_t* n_reads, uint32_t* max_len, uint8_t** ascii, uint8_t** quals,
                   uint16_t** lens, uint8_t** bc_fields, char* err, size_t errcap);
void snk_host_free(void* p);

/* f3 at rate: many FASTH files decoded concurrently (the reference: one decode thread per two files, lib/tada/src/cmd_msp.rs:55-69,
 * over MultiFastqIter, multifastq.rs:69-127; like it, a file that is not gzip is refused).  A pool of `threads` workers
 * (0 = one per file up to the host's hardware threads) takes whole files, inflates with zlib's streaming API and parses the
 * records in place into batches of `batch_pairs` read pairs (0 = 32768); snk_fasth_next hands out full batches in any order
 * (file / first_pair say where a batch belongs), n_pairs == 0 = every file has been read to its end.  flags bit 0: the batches
 * live in page-locked memory (needs a GPU).  Rows of `stride` bytes: bases 'A'-padded, raw phred 0-padded. */
typedef struct snk_fasth_stream snk_fasth_stream;
typedef struct snk_fasth_batch {
    uint64_t n_pairs;           /* reads 2q, 2q+1 of the batch = R1, R2 of its pair q (cmd_msp.rs:160-181) */
    uint64_t first_pair;        /* index of the batch's first pair inside its file */
    uint32_t file, max_len;
    const uint8_t* ascii;       /* 2*n_pairs rows */
    const uint8_t* quals;
    const uint16_t* lens;       /* 2*n_pairs */
    const uint8_t* bc_fields;   /* n_pairs x 64 bytes, zero padded: the barcode field up to its first ',' */
    uint64_t text_bytes;        /* inflated bytes this batch was parsed from */
    uint64_t token;
} snk_fasth_batch;
/* CPUs this process may use: the cgroup CPU quota (cpu.max) when there is one, else the affinity mask / the hardware threads.  The
 * default number of decode threads is this minus two (threads = 0). */
uint32_t snk_host_cpu_budget(void);
int snk_fasth_open(const char* const* paths, uint32_t n_files, uint32_t stride, uint32_t batch_pairs, uint32_t threads, uint32_t flags,
                   snk_fasth_stream** out, char* err, size_t errcap);
int snk_fasth_next(snk_fasth_stream* s, snk_fasth_batch* out, char* err, size_t errcap);
void snk_fasth_release(snk_fasth_stream* s, snk_fasth_batch* b);      /* the batch's buffers go back to the workers */
uint64_t snk_fasth_file_pairs(snk_fasth_stream* s, uint32_t file);   /* known once the file has been read to its end */
void snk_fasth_close(snk_fasth_stream* s);
/* ... and into HBM: packed rows (snk_dev_pack_ascii), quality rows, lengths and -- with a whitelist index -- barcode ids
 * (snk_dev_bc_ids, one per read), in file-major order; uploads, pack and id lookup overlap the decode.  The arrays are plain
 * device allocations (not the context's arena: they are the INPUT of snk_dev_count_graph); snk_dev_ingest_free releases them.
 *   read_len  1..256: the row length in bases, i.e. the longest read the lane may hold.  Rows are padded to 16 bases (row_words =
 *             ceil(read_len / 16), qstride = 16 * row_words); shorter reads are fine (lens[] has their lengths, packed codes and
 *             quality bytes behind a read's own length are 0).  A read LONGER than read_len is refused by both entry points:
 *             SNK_E_UNSUPPORTED, the message names the file, the record, the read's length and read_len.  Nothing is ever cut:
 *             every kernel downstream takes min(lens[], read_len) as a read's length, so a cut read would lose its last k-mers
 *             silently.  (snk_fasth_open itself takes whatever fits its stride.)
 *   SNK_INGEST_TRACE=1 prints where the consumer thread's time went, the number of batches, how many times the device arrays had
 *             to grow (their first size is a guess from the compressed sizes) and whether the batches had to be put into file-major
 *             order afterwards (1) or arrived in it (0). */
typedef struct snk_dev_ingest {
    uint64_t n_reads;
    uint32_t read_len, row_words, qstride, max_len;
    const void* rows;
    const void* quals;
    const void* lens;
    const void* bc;             /* NULL without an index */
    uint64_t text_bytes, compressed_bytes;
    double seconds, decode_wait_seconds;   /* whole call; of it, time the consumer waited for a decoded batch */
    uint32_t n_files, n_batches;
    double setup_seconds;                  /* of `seconds`: page-locked batch pool + device arrays allocated, workers started */
    const void* good_len;                  /* u16 per read: set by snk_dev_ingest_df_trimmed (quals and lens are NULL there), else NULL */
} snk_dev_ingest;
int snk_dev_ingest_fasth(snk_ctx* ctx, const char* const* paths, uint32_t n_files, uint32_t read_len, const snk_bc_index* ix, uint32_t threads,
                         uint32_t batch_pairs, snk_dev_ingest* out, char* err, size_t errcap);
void snk_dev_ingest_free(snk_dev_ingest* r);
/* FASTH files -> unitigs with the reads never resident as a whole: every decoded batch is uploaded, packed, given its barcode ids and
 * appended to a streamed job (snk_dev_stream_*) -- partitioned while the next batches are being inflated; the wall time is
 * max(ingest, partition) + count + graph.  res: as snk_dev_count_graph's (good_len in arrival order: batches arrive in any order).
 * read_len and the refusal of longer reads: as snk_dev_ingest_fasth.
 * total_reads_hint: an upper bound of the job's reads (sizes the bucket slots).  A lane with more reads than the hint is refused
 * (SNK_E_ARG) as soon as a batch crosses it; the message names total_reads_hint and the reads decoded so far.  0 = the library's own
 * guess from the compressed sizes and the gzip trailers.  It is a guess: files of several gzip members (cat a.gz b.gz), lanes of
 * reads much shorter than read_len and lanes that deflate unusually well hold more reads than it.  Then nothing more is uploaded, the
 * decode runs to the end to count the reads, and the job is run again from the files with that count: the same result, at the price
 * of decoding the lane twice (and the device work done up to the crossing).  Callers that know the read count should pass it.
 * stats: rows / quals / lens / bc stay NULL; seconds covers both passes.  The reading half + MSP of tada in one pass
 * (lib/tada/src/cmd_msp.rs:55-69,100-190). */
int snk_dev_ingest_count_graph(snk_ctx* ctx, const char* const* paths, uint32_t n_files, uint32_t read_len, const snk_bc_index* ix, uint32_t threads,
                               uint32_t batch_pairs, uint64_t total_reads_hint, const snk_params* p, snk_dev_result* res, snk_dev_ingest* stats, char* err,
                               size_t errcap);
/* synthetic FASTH (tests, bench.py --ingest): pairs [first_pair, first_pair + n_pairs) of the synthetic read model as one gzip
 * file; barcode field = snk_synth_bc_seq(id) + "-1" (",raw" appended on every third pair), an off-whitelist sequence for id 0 */
int snk_synth_fasth_write(const char* path, const snk_synth_params* sp, uint64_t first_pair, uint64_t n_pairs, int level, uint64_t* text_bytes,
                          char* err, size_t errcap);
void snk_synth_bc_seq(uint32_t id, char* out16);

/* ---- the graph verifier (supernova_amd/csrc/snk_check.hip) ------------------------------------------------------------------------
 * The reference's reassembly invariants (lib/tada/src/sim_tests.rs:297-404; EdgeBuilder, BuildReadQGraph48.cc:327-541), checked on the
 * device over raw arrays -- any producer's, or a corrupted copy -- at any size (entry ids up to 2^32 - 2; 64-bit positions and counters).
 * The verifier shares the key layout and the context plumbing with the rest of libsnk, nothing of the count or graph code: its own
 * canonical form, its own hash index, its own trim.  Its scratch (about 8.25 B per entry, 5 B more for the reads level) comes from
 * the context's arena after the arrays under test and is handed back on return: the snk_dev_result it checks stays valid.
 *
 * Graph level (unless SNK_CHECK_DIGEST_ONLY): every counter below counts violations, first[] holds the first offender (table row,
 * unitig or read index; UINT64_MAX = none).
 *   table_duplicate_keys   two rows share a key
 *   table_not_sorted       SNK_CHECK_SORTED_TABLE: a key below the one before it
 *   count_below_min_freq   a count < min_freq
 *   bad_unitig             a unitig shorter than K, a base code > 3, offsets that do not start at 0 or decrease
 *   unitig_kmer_missing    a k-mer of a unitig, canonicalised (group included), is not in the table
 *   kmer_repeated          a table entry hit by more than one unitig k-mer (a k-mer belongs to exactly one unitig, :492-504)
 *   kmer_uncovered         a table entry no unitig k-mer hits
 *   ctx_dangling           a context bit (pred << 4 | succ, canonical orientation) names a neighbour that is not in the table
 *   ctx_not_reciprocal     ... that is, but does not carry the reciprocal bit (ReadPather.h:356-381)
 *   interior_break         a step x -> y inside a unitig breaks the walk rule: x has one successor, y's last base; y has one
 *                          predecessor; neither is a palindrome (EdgeBuilder::extend, :445-464)
 *   end_extendable         an end of a non-circular unitig the walk rule would extend (up/downstreamExtensionPossible, :408-428)
 *   not_canonical          a linear unitig not in FWD form; a circle that does not start at its smallest canonical k-mer, in that
 *                          k-mer's FWD form, before addEdge orients the whole sequence (:348-397,478-486).  A palindrome k-mer is a
 *                          unitig of its own.  A circle's last K-1 bases repeat its first
 *   not_ordered            SNK_CHECK_ORDERED: unitigs not ascending by their first K bases (group-major when grouped)
 *   group_mismatch         grouped runs: a k-mer of a unitig is not in the table under the unitig's group but is under another one
 *                          (the index hashes the k-mer without its group, so every group's copy lies on one probe chain)
 *   key_padding            key bits below the K bases that are not zero where no group belongs there (ungrouped runs, K=60)
 * Reads level (reads != NULL): the k-mers of every read with good length >= K+1 at positions 0 .. good_len-K (Kmerizer::map,
 * :155-172), looked up in the verifier's index:
 *   count_mismatch         min(recount, 2^24-1) != min(stored count, 2^24-1)
 *   ctx_mismatch           (min_freq > 1) the context the reads give -- neighbours both retained -- != the stored byte
 *   good_len_mismatch      reads->quals given: the trim recomputed (App. A.4, min_qual) != reads->good_len
 *   instances_mismatch     sum of max(0, good_len-K+1) over reads with good_len >= K+1 != in->n_instances (when that is not 0)
 * Not re-derived: which k-mers the min_freq / min_bc rules drop.
 *
 * Digests (always; mod 2^64, mix = the splitmix64 finaliser z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
 * z *= 0x94D049BB133111EB, z ^= z >> 31): order-independent across rows and unitigs, additive over disjoint shares, position-sensitive
 * inside a unitig:
 *   table_digest  = sum over rows     mix(key_lo ^ mix(key_hi ^ mix((min(count, 2^24-1) << 8) | ctx)))
 *   unitig_digest = sum over unitigs  mix(h_u ^ mix(len_u ^ (group_u << 40))),  h_u = sum over i mix((i << 2) | base_{u,i})
 * (group_u = 0 outside grouped runs). */
#define SNK_CHECK_SORTED_TABLE 1u   /* the table must be ascending */
#define SNK_CHECK_ORDERED 2u        /* unitigs ordered by their first K bases, group-major when grouped (snk_dev_result) */
#define SNK_CHECK_GROUPED 4u        /* per-group run: the group in the 32 low key bits (K=48); unitig_group and reads->group given */
#define SNK_CHECK_DIGEST_ONLY 8u    /* digests only: a rank's share of a sharded step, where unitigs cross table shares */
#define SNK_CHECK_N_COUNTERS 24
/* counter indices (count[] / first[]) */
#define SNK_CHECK_TABLE_DUPLICATE_KEYS 0
#define SNK_CHECK_TABLE_NOT_SORTED 1
#define SNK_CHECK_COUNT_BELOW_MIN_FREQ 2
#define SNK_CHECK_BAD_UNITIG 3
#define SNK_CHECK_UNITIG_KMER_MISSING 4
#define SNK_CHECK_KMER_REPEATED 5
#define SNK_CHECK_KMER_UNCOVERED 6
#define SNK_CHECK_CTX_DANGLING 7
#define SNK_CHECK_CTX_NOT_RECIPROCAL 8
#define SNK_CHECK_INTERIOR_BREAK 9
#define SNK_CHECK_END_EXTENDABLE 10
#define SNK_CHECK_NOT_CANONICAL 11
#define SNK_CHECK_NOT_ORDERED 12
#define SNK_CHECK_GROUP_MISMATCH 13
#define SNK_CHECK_COUNT_MISMATCH 14
#define SNK_CHECK_CTX_MISMATCH 15
#define SNK_CHECK_GOOD_LEN_MISMATCH 16
#define SNK_CHECK_INSTANCES_MISMATCH 17
#define SNK_CHECK_KEY_PADDING 18          /* 19 .. 23 reserved */
typedef struct snk_check_input {   /* raw device arrays, so any producer (and a corrupted copy in a test) can be checked */
    uint32_t K, flags;             /* SNK_CHECK_* */
    uint32_t min_freq;
    uint32_t min_qual;             /* reads level, the trim recomputed from reads->quals (0 = 7) */
    uint64_t n_instances;          /* what the producer reported (snk_dev_result.n_instances); 0 = not checked */
    uint64_t n_kmers;
    const void* keys;              /* as snk_dev_result */
    const void* counts;
    const void* ctx;
    uint64_t n_unitigs;
    const void* unitig_off;        /* u64[n_unitigs + 1] */
    const void* unitig_bases;
    const void* unitig_group;      /* u32[n_unitigs] with SNK_CHECK_GROUPED, else ignored */
} snk_check_input;
typedef struct snk_check_report {
    uint32_t struct_size;          /* the caller sets sizeof(snk_check_report) = 600; the library refuses a smaller one */
    uint32_t levels;               /* what ran: 1 graph level, 2 reads level (0: digests only) */
    uint64_t n_kmers, n_unitigs, n_circles, n_palindromes, n_bases;
    uint64_t n_instances;          /* reads level: the instances the reads give */
    uint64_t table_digest, unitig_digest;
    uint64_t count[SNK_CHECK_N_COUNTERS];
    uint64_t first[SNK_CHECK_N_COUNTERS];
    uint64_t peak_bytes;           /* verifier scratch */
    float graph_ms, reads_ms;      /* HIP events: digests + graph level; reads level + the per-entry comparison */
    uint64_t reserved[16];
} snk_check_report;
/* reads: NULL = graph level only (ignored with SNK_CHECK_DIGEST_ONLY).  Returns SNK_OK whatever it found: the report says. */
int snk_dev_check_graph(snk_ctx* ctx, const snk_check_input* in, const snk_dev_reads* reads, snk_check_report* out, void* stream,
                        char* err, size_t errcap);

/* ---- the list ranking on its own (an entry for the tests, like snk_comm_selftest and the snk_ctx_last_* witnesses).
 * The join's ranking (csrc/snk_rank.hip) over a link structure the caller made: n nodes, 2n directed states (node, exit side).
 *   d_link[2n]    u32: link[s] = the state that s is joined to, or 0xFFFFFFFF (none); an involution (link[link[s]] == s; link[s] == s is
 *                 a turn).  Circles are cut in place: both states of ONE pair of every circle become 0xFFFFFFFF.
 *   d_weights[n]  u32 or NULL (every node weighs 1)
 *   d_circ[2n]    u8, zeroed by the caller, or NULL: 1 on the states whose link a cut removed
 *   d_rk[2n]      two u32 per state: (summed weight of the nodes stepped onto after the state up to the end of its list, terminal state)
 * world == 0: the one-GPU ranking exactly as the join calls it (frag_off is ignored).  world >= 1: the partitioned ranking of the
 * sharded step with every rank emulated in this context -- its attempt loop without a communicator, owner q holding the nodes
 * [frag_off[q], frag_off[q + 1]) --; it needs d_weights and d_circ.
 * SNK_E_ARG, before anything is launched and with *out zeroed: links that are no involution or point outside [0, 2n), 2n >= 2^32, a
 * frag_off[world + 1] that does not ascend from 0 to n, world >= 1 without weights or circ.  n == 0: SNK_OK, nothing written. */
#define SNK_RANK_WYLLIE 1               /* plain pointer jumping over all states */
#define SNK_RANK_RULING 2               /* the sparse ruling set */
#define SNK_RANK_RULING_THEN_WYLLIE 3   /* the ruling set met circles it left to pointer jumping, which ranked */
typedef struct snk_rank_evidence {
    uint32_t n_circles, rounds;    /* as snk_dev_result reports them */
    uint32_t source;               /* SNK_RANK_*: what produced rk */
    uint32_t ruling_attempts;      /* ruling-set attempts of the one-GPU ranking (also where it ran as the partitioned form's fallback) */
    uint64_t splitters;            /* splitters of the first ruling-set attempt (partitioned: of the first partitioned attempt) */
    uint32_t sparse_cut;           /* circles cut by the sparse cut */
    uint32_t bad;                  /* the sparse cut gave up on something */
    uint32_t part_attempts;        /* world >= 1: partitioned attempts made */
    uint32_t partitioned;          /* world >= 1: 1 = rk is the partitioned ranking's, 0 = the replicated fallback's */
    uint64_t reserved[4];
} snk_rank_evidence;
int snk_dev_rank_lists(snk_ctx* ctx, uint64_t n, void* d_link, const void* d_weights, void* d_circ, uint32_t world, const uint64_t* frag_off,
                       void* d_rk, snk_rank_evidence* out, void* stream, char* err, size_t errcap);

#ifdef __cplusplus
}
#endif
#endif /* SNK_H_ */
