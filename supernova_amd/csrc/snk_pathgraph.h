// snk_pathgraph.h -- the per-edge and per-unitig device tables of a graph that the stages working on (reads, graph, paths) share:
// the pather (snk_path.hip), which adds its k-mer dictionary or minimiser index to them, and the path extension (snk_extend.hip),
// which needs nothing else.  One function fills them (snk_path.hip); the From / To lists are those of snk_hbv_lists_build.  One set of
// device accessors reads them (pg_*, below the struct): the pather, the extension, MarkBads, the patch insertion, FindEdgePairs and the
// gap closures use these and keep no copy of their own.  (The verifier, snk_check.hip, shares nothing with what it verifies.)
#pragma once
#include <stdint.h>

#include <vector>

#include "snk_call.h"
#include "snk_common.h"

constexpr uint64_t UPAD = 512;      // bases of slack in front of (and behind) the packed unitigs: a window may start 270 bases before a hit or run 270 past it

struct path_graph {            // device arrays
    const uint64_t* uoff;      // [U+1] unitig offsets into ubases (device order)
    const uint8_t* ubases;     // 1 byte per base
    const uint32_t* upack;     // the same bases, 2 bits each, 16 per word, first base in the top bits (one word of slack at either end): what the
                               //     seed check and the exact-match extension read (a read's whole window is 40 bytes instead of 150 byte loads)
    const uint4* uinfo;        // [U] x 2: {offset lo, offset hi, bases, flags}, {fwd edge, rev edge, 0, 0}; flags bit 0 / 1: a seed on the
                               //     forward / reverse-complement copy is dropped (hanging edge rule, BuildReadQGraph48.cc:1240-1247)
    const int32_t *fwd, *rev;  // [U] HBV edge of the unitig read forward / reverse-complemented
    const int32_t *vleft, *vright;         // [E]
    const int32_t *e_unitig;               // [E] device index of the unitig the edge is a copy of
    const uint8_t* e_rc;                   // [E]
    const int32_t *to_off, *to_v, *to_e;   // [N+1], [E], [E]: in-edges of a vertex, AddEdge order (graph/DigraphTemplate.h:2572-2582)
    const int32_t *from_off, *from_v, *from_e;
    const unsigned long long* dslot;   // dictionary, 8 bytes per slot: fingerprint (30 bits) | strand (1) | position (33 bits: first base of
                               //   the k-mer in the concatenated unitigs); all ones: empty.  strand: the unitig holds the reverse complement
                               //   of the canonical form.  A probe is one 8-byte access, a claim ONE 64-bit compare-and-swap; a fingerprint
                               //   match is VERIFIED against the unitig's bases, so look-ups stay exact (2^-30 false candidates per probe of
                               //   an occupied slot: a few reads per 10^8 take the verified path).  24 bytes per unitig k-mer.
    const uint32_t* ublk;      // unitig that holds base 256 b of the concatenation (position -> unitig: this entry, then a step or two along uoff)
    uint64_t dcap;             // slots: 3 per k-mer, not a power of two
    unsigned long long fp_mask; // 30 ones; SNK_PATH_FP_MASK (tests) narrows the fingerprint so that false matches happen and the verified path runs
    // Minimiser index (round 4; ment != NULL: the look-ups go through it and dslot is not built).  A k-mer lies on the graph iff its
    // minimiser -- the 16-mer with the smallest ordering key among its K-15, the leftmost on ties -- occurs in a unitig at the matching
    // place and the K bases around it agree.  The index lists the places a unitig k-mer's window picks (its leftmost AND its rightmost
    // minimum: a read may run against the unitig's strand), ~2 / (K-14) of the unitig bases: 8 bytes each, sorted by key behind a
    // directory over the key's top bits -- 0.14 GB for the bench graph's 0.27 G k-mers where the k-mer dictionary takes 6.4 GB, small
    // enough to live in the 256 MB Infinity Cache together with the packed unitigs the candidates are verified against.
    const unsigned long long* ment;    // [n_ment] key low 30 bits << 34 | the unitig's 16-mer is the reverse complement of the canonical one << 33 | position
    const uint32_t* mdir;      // [(1 << mdir_bits) + 1] first entry of every key prefix
    uint32_t mdir_bits;
    uint32_t idx_dbg;          // SNK_PATH_IDX_DBG (timing aid, results invalid): 1 = window minimum only, 2 = + directory and entries, 3 = + base comparison (no unitig-bounds check)
};

#if defined(__HIPCC__)
// ---- how a kernel reads the tables.  An HBV edge is a unitig read forward or reverse-complemented: edge-keyed accessors go through
// e_unitig / e_rc, unitig-keyed ones take the orientation as an argument.  Every stage reads the graph through these.
struct pg_edge { uint64_t o; uint32_t len; uint32_t rc; };      // where the unitig starts in the concatenation, its bases, read backwards and complemented

// (I: the edge id as the caller holds it -- int32_t from the graph's lists, uint32_t from a path table whose ids were checked as
// unsigned.  It indexes as that type, so no caller pays for a conversion.)
template <typename I>
__device__ __forceinline__ pg_edge pg_edge_load(const path_graph& G, I e) {
    const uint4 q = G.uinfo[2 * (uint64_t)(uint32_t)G.e_unitig[e]];
    pg_edge x;
    x.o = ((uint64_t)q.y << 32) | q.x; x.len = q.z; x.rc = G.e_rc[e];
    return x;
}
__device__ __forceinline__ uint32_t pg_unitig_len(const path_graph& G, uint32_t u) { return G.uinfo[2 * (uint64_t)u].z; }
template <typename I>
__device__ __forceinline__ uint32_t pg_edge_len(const path_graph& G, I e) { return pg_unitig_len(G, (uint32_t)G.e_unitig[e]); }      // bases; k-mers: - K + 1
// bases i .. i + 15 of an edge in its orientation, first base in the top bits, i <= len (behind its end: whatever the packed array
// holds there; the callers mask).  The reverse-complement branch reads the 16 bases that END at base len - i of the unitig, so for
// i > len - 16 it starts up to 16 bases IN FRONT of the unitig: of the first unitig that is in front of the array's first base, which
// is why upack has UPAD bases of slack in front (and why the position is UPAD + ..., never below zero).  Reversed as 2-bit groups
// (brev, then the bits of every pair swapped back) and complemented.
__device__ __forceinline__ uint32_t pg_edge16(const path_graph& G, const pg_edge& x, uint32_t i) {
    if (!x.rc) return snk_packed16(G.upack, UPAD + x.o + i);
    uint32_t w = __brev(snk_packed16(G.upack, UPAD + x.o + x.len - 16 - i));
    w = ((w >> 1) & 0x55555555u) | ((w & 0x55555555u) << 1);
    return ~w;
}
// base i of an edge in its orientation, from the byte array through uoff
__device__ __forceinline__ uint32_t pg_edge_base(const path_graph& G, int32_t e, uint32_t i) {
    const uint32_t u = (uint32_t)G.e_unitig[e];
    const uint64_t o = G.uoff[u], len = G.uoff[u + 1] - o;
    return G.e_rc[e] ? 3u - (G.ubases[o + len - 1 - i] & 3u) : G.ubases[o + i] & 3u;
}
// base i of unitig u read forward (rc = 0) or reverse-complemented, through the uinfo record: what the pather's sequential part reads
// (it holds (unitig, rc) in its path parts and has the record in cache)
__device__ __forceinline__ uint32_t pg_unitig_base(const path_graph& G, uint32_t u, uint32_t rc, uint32_t i) {
    const uint4 q = G.uinfo[2 * (uint64_t)u];
    const uint8_t* b = G.ubases + (((uint64_t)q.y << 32) | q.x);
    return rc ? (uint32_t)(b[q.z - 1 - i] ^ 3u) & 3u : (uint32_t)b[i] & 3u;
}
__device__ __forceinline__ int pg_to_size(const path_graph& G, int32_t v) { return G.to_off[v + 1] - G.to_off[v]; }            // in-edges of a vertex
__device__ __forceinline__ int pg_from_size(const path_graph& G, int32_t v) { return G.from_off[v + 1] - G.from_off[v]; }      // out-edges
#endif

// the graph tables on the host: what the asynchronous uploads read.  The entry point declares them in front of the frame, which waits
// for the stream before they are let go of, whichever way the call ends.
struct path_host {
    std::vector<int32_t> fwd, rev, eu, off_to, v_to, e_to, off_from, v_from, e_from, vl, vr;
    std::vector<uint8_t> erc, drop;
};

// Fills, from the unitigs on the device and their graph h (bvcomp_order as for snk_dev_path_reads), every field of G in front of
// `dslot`: the unitig offsets and bases, the packed bases, the per-unitig records, the edge tables and the From / To lists.  The
// look-up structures are the pather's own and stay as they are.  Everything is scratch of the frame c; H holds what the uploads read
// and must be declared in front of the frame.  *total_bases = the bases of all unitigs.  `who` names the entry point in messages.
int snk_path_graph_tables(snk_call& c, path_host& H, uint32_t K, uint64_t U, const uint64_t* d_uoff, const uint8_t* d_ubases, const snk_hbv* h, path_graph* G,
                          uint64_t* total_bases, const char* who, char* err, size_t errcap);
