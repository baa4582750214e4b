// snk_call.h -- the call frame of the device stages that run after the graph (snk_dev_hbv, snk_dev_check_graph, snk_dev_path_reads2,
// snk_dev_mark_dups, snk_dev_paths_index, snk_dev_edge_barcodes, snk_dev_paths_zip, snk_dev_paths_unzip, snk_dev_extend_paths, snk_dev_patch_pieces, snk_dev_patch_merge, snk_dev_patch_paths, snk_dev_mark_bads, snk_dev_mark_bads_df, snk_dev_edge_pairs, snk_dev_close_gaps, snk_dev_delete_edges, snk_dev_hanging_ends, snk_dev_mow_lawn).
//
// One protocol, one owner.  Such an entry point checks the arguments that need no device, zeroes *out and hands its body to
// snk_call_run.  The frame makes the context's device current, picks the stream, remembers where the call's scratch begins, and on
// EVERY way out -- c.end(), a plain `return rc`, an exception -- waits for the stream (nothing of the call is still running when
// its scratch is handed back, or when the caller's host buffers die), returns the scratch to the arena except what the caller
// keeps, and destroys the timing events.  After a failure *out is all zero.
//
// Host memory that an asynchronous copy of the body reads or writes is declared BEFORE snk_call_run, so that it outlives the
// frame's final wait.
#pragma once
#include <string.h>

#include <exception>
#include <initializer_list>
#include <new>

#include "snk_ctx.h"

// No C++ exception leaves an extern "C" entry point: a failed host allocation maps to SNK_E_NOMEM (the caller's exit code 99,
// system/RunTime.cc:195-221), anything else to SNK_E_INTERNAL.  `who` is "" or the entry point's name.
#define SNK_GUARD_AS(who, body)                                                                                                      \
    try { body } catch (const std::bad_alloc&) {                                                                                     \
        return snk_fail(SNK_E_NOMEM, err, errcap, "%s%shost allocation failed", (who), (who)[0] ? ": " : "");                        \
    } catch (const std::exception& ex) { return snk_fail(SNK_E_INTERNAL, err, errcap, "%s", ex.what()); }                            \
    catch (...) { return snk_fail(SNK_E_INTERNAL, err, errcap, "unexpected exception"); }
#define SNK_GUARD(body) SNK_GUARD_AS("", body)

// a scratch block that several two-step primitives share (snk_call::temp)
struct snk_temp { void* p = nullptr; size_t bytes = 0; };

struct snk_call {
    snk_ctx* ctx;
    hipStream_t st;
    char* err;
    size_t errcap;
    uint64_t mark;              // the call's scratch = the blocks handed out after this serial
    size_t bytes = 0;           // ... and their sum (the verifier reports it)
    hipEvent_t ev[8];
    int n_ev = 0;
    hipError_t entered;
    bool done = false;

    snk_call(snk_ctx* c, void* stream, char* e, size_t ecap) : ctx(c), st(stream ? (hipStream_t)stream : c->stream), err(e), errcap(ecap) {
        entered = snk_enter(ctx);
        ctx->cur_stream = st;
        mark = ctx->alloc_serial;
    }
    snk_call(const snk_call&) = delete;
    snk_call& operator=(const snk_call&) = delete;
    ~snk_call() { end(SNK_E_INTERNAL); }

    // the one allocator: n elements (an empty array is still a block) + 16 bytes of slack for the kernels that read whole words
    template <typename T>
    int alloc(size_t n, T** out) {
        void* q = nullptr;
        const size_t b = (n ? n : 1) * sizeof(T) + 16;
        const int rc = snk_ctx_alloc(ctx, b, &q, err, errcap);
        if (!rc) bytes += b;
        *out = (T*)q;
        return rc;
    }
    // rocPRIM's two steps.  Every f(tmp, bytes) wraps one primitive; with tmp == NULL it only asks for its size.  temp() sizes ONE block
    // for all of them (the callers run them one after the other, each as f(t.p, t.bytes)); with_temp() is the usual case of one
    // primitive that runs right away.
    template <typename F>
    static hipError_t temp_size(snk_temp* t, F& f) {
        size_t tb = 0;
        const hipError_t e = f((void*)nullptr, tb);
        if (tb > t->bytes) t->bytes = tb;
        return e;
    }
    template <typename... F>
    int temp(snk_temp* t, F... f) {
        for (hipError_t e : {temp_size(t, f)...}) SNK_HIP_TRY(e);
        return alloc(t->bytes, (uint8_t**)&t->p);
    }
    template <typename F>
    int with_temp(F f) {
        snk_temp t;
        const int rc = temp(&t, f);
        if (rc) return rc;
        SNK_HIP_TRY(f(t.p, t.bytes));
        return SNK_OK;
    }
    // timing: stamp() records the next event on the stream (events are made on demand and belong to the frame); ms(a, b) is the time
    // between the a-th and the b-th stamp, once the stream has been waited for
    hipError_t stamp() {
        if (n_ev == (int)(sizeof ev / sizeof ev[0])) return hipErrorInvalidValue;
        const hipError_t e = hipEventCreate(&ev[n_ev]);
        return e != hipSuccess ? e : hipEventRecord(ev[n_ev++], st);
    }
    float ms(int a, int b) const {
        float t = 0.f;
        if (a < n_ev && b < n_ev) (void)hipEventElapsedTime(&t, ev[a], ev[b]);
        return t;
    }
    // the way out: keep[] stays with the caller until the context's next top-level call -- after a failure nothing does
    int end(int rc, std::initializer_list<const void*> keep = {}) {
        if (done) return rc;
        done = true;
        (void)hipStreamSynchronize(st);
        snk_ctx_release_since(ctx, mark, keep.begin(), rc ? 0 : keep.size());
        for (int i = 0; i < n_ev; ++i) (void)hipEventDestroy(ev[i]);
        return rc;
    }
};

template <typename Body>
int snk_call_guarded(snk_ctx* ctx, void* stream, const char* who, char* err, size_t errcap, Body body) {
    SNK_GUARD_AS(who,
        snk_call c(ctx, stream, err, errcap);
        SNK_HIP_TRY(c.entered);
        return c.end(body(c));
    )
}
// runs body(frame) -> rc; *out is zero after any failure
template <typename Out, typename Body>
int snk_call_run(snk_ctx* ctx, void* stream, const char* who, Out* out, char* err, size_t errcap, Body body) {
    const int rc = snk_call_guarded(ctx, stream, who, err, errcap, body);
    if (rc) memset(out, 0, sizeof *out);
    return rc;
}

// the largest edge id of a path table, compared as unsigned (a negative id is the largest), into the 256 slots of `range` (zeroed by
// the caller; the result is their maximum).  Any 4-byte-aligned pointer.  Shared by the paths index and the compressed paths
// (snk_pidx.hip), which refuse an id outside the graph before they index with it.
hipError_t snk_max_edge_id(const uint32_t* edges, uint64_t n, uint32_t* range, hipStream_t st);
// Row r of a path table of n reads adds up: start[0] = 0, start[r + 1] = start[r] + n_edges[r], start[n] = n_entries (no gaps, no
// overlaps; start has n + 1 entries).  Every stage that indexes with start / n_edges asks this of every row first, in its own check
// kernel, and refuses the table under its own flag and message.
__device__ __forceinline__ bool snk_paths_row_ok(const unsigned long long* start, const uint32_t* n_edges, uint64_t r, uint64_t n, uint64_t n_entries) {
    const uint64_t s = start[r], m = n_edges[r];
    if (s > n_entries || m > n_entries - s || start[r + 1] != s + m || (r == 0 && s != 0) || (r + 1 == n && s + m != n_entries)) return false;
    return true;
}
// The lists of the paths index inside a frame (snk_pidx.hip): off[E + 1], ids[n_edges_total] and, with_counts, room for counts[E] (the
// caller fills it), all scratch of c.  Refuses, as `who`, a path table that does not add up and an edge id outside [0, E).  What
// snk_dev_paths_index is made of, and what snk_dev_edge_pairs runs when it is given no index.
int snk_pidx_lists(snk_call& c, const struct snk_dev_paths* paths, uint64_t E, const char* who, bool with_counts, unsigned long long** off, unsigned long long** ids,
                   int32_t** counts, uint32_t* key_bits, char* err, size_t errcap);
