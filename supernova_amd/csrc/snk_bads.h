// snk_bads.h -- MarkBads in pieces (snk_bads.hip), for its two entry points: snk_dev_mark_bads runs one launch over resident reads,
// snk_dev_mark_bads_df (snk_dfin.hip, where the slab ring lives) one launch per decoded slab.  Both go begin -> slab ... -> finish inside
// ONE call frame, so the graph tables are built and the paths checked once per call and the flags of a call are one array.
#pragma once
#include <stdint.h>

#include "snk_call.h"
#include "snk_pathgraph.h"

struct bads_job {
    path_graph G;
    int K;
    uint32_t x;                        // SNK_BADS_X: offsets as a ReadPathVecX holds them
    uint64_t n_reads;                  // of the call (even)
    const unsigned long long* start;   // the paths of the call's reads (device)
    const uint32_t* n_edges;
    const int32_t* offset;
    const uint32_t* edges;
    uint8_t* bad;                      // [n_reads / 2], zeroed by begin
    unsigned long long* counters;      // [8]
};

// The arguments that need no device (call it before the frame is made: nothing has run when it refuses).  read_len / have_quals: of the
// reads the slabs will bring.
int snk_bads_check_args(const char* who, uint32_t K, uint64_t n_reads, uint32_t read_len, bool have_quals, uint64_t n_unitigs, const void* d_unitig_off,
                        const void* d_unitig_bases, const snk_hbv* h, const snk_dev_paths* paths, uint32_t flags, char* err, size_t errcap);
// The graph tables, the refusals that need the device (the path table, the edge ids, and with SNK_BADS_X what snk_dev_paths_zip
// refuses or would not give back unchanged), the zeroed flags and counters.  H is declared in front of the frame.
int snk_bads_begin(snk_call& c, path_host& H, const char* who, uint32_t K, uint64_t n_reads, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases,
                   const snk_hbv* h, const snk_dev_paths* paths, uint32_t flags, bads_job* job, char* err, size_t errcap);
// Reads [first, first + R.n) of the call (both even), given as the device arrays of a slab: enqueues the kernel on st.
hipError_t snk_bads_slab(const bads_job& job, uint64_t first, const snk_reads_view& R, hipStream_t st);
// Waits for the stream, brings the counters down and fills *out (all but ms and n_slabs).  The caller keeps job.bad (c.end).
int snk_bads_finish(snk_call& c, const bads_job& job, snk_dev_bads* out, char* err, size_t errcap);
