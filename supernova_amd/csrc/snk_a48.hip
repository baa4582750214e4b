// snk_a48.hip -- host writers for the files DF leaves in a.48/ beside a.hbv and a.inv (those: snk_hbv.hip).  No device code.
//   a.paths      feudal MasterVec<ReadPath>   paths/long/ReadPath.h:61-63 (writeFeudal: offset, last skip, the edge ids),
//                                             IncrementalWriter, feudal/FeudalFileWriter.cc:18-140; written as tmp.paths by pathReads
//                                             (BuildReadQGraph48.cc:1441-1469), renamed at 10X/DF.cc:584
//   a.paths.inv  feudal MasterVec<ULongVec>   10X/PathsIndex.cc:76,100-108
//   a.countsb    BINWRITE vec<vec<int>>       10X/PathsIndex.cc:75,135 (one inner vector)
//   a.dup        BINWRITE vec<Bool>           10X/DF.cc:599-600
// A feudal file: 24-byte control block (feudal/FeudalControlBlock.h:157-166), the elements' variable-length data back to back, the
// table of N + 1 file offsets, then the fixed-length data (none for these element types).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "snk_ctx.h"

namespace {

#pragma pack(push, 1)
struct fcb_t {          // FeudalControlBlock, 24 bytes
    uint32_t n;         // elements modulo 2^32 (readers take the count from the offsets)
    uint8_t flags, sizeof_fixed, sizeof_x, sizeof_a;
    uint64_t var_offset, fixed_offset;
};
#pragma pack(pop)
static_assert(sizeof(fcb_t) == 24, "feudal control block is 24 bytes");

struct out_file {
    FILE* f = nullptr;
    bool ok = true;
    std::vector<uint8_t> buf;
    explicit out_file(const char* path) { f = fopen(path, "wb"); ok = f != nullptr; buf.reserve(1u << 20); }
    ~out_file() { if (f) fclose(f); }
    void flush() {
        if (ok && !buf.empty()) ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
        buf.clear();
    }
    void put(const void* p, size_t bytes) {
        if (bytes >= (1u << 20)) { flush(); if (ok && bytes) ok = fwrite(p, 1, bytes, f) == bytes; return; }
        if (buf.size() + bytes > (1u << 20)) flush();
        const uint8_t* b = (const uint8_t*)p;
        buf.insert(buf.end(), b, b + bytes);
    }
    bool close() {
        flush();
        if (f) { ok = fclose(f) == 0 && ok; f = nullptr; }
        return ok;
    }
};

}  // namespace

extern "C" int snk_write_paths(const char* path, uint64_t n_reads, const int32_t* offset, const uint32_t* n_edges, const uint64_t* start, const int32_t* edges,
                               char* err, size_t errcap) {
    if (!path || (n_reads && (!offset || !n_edges))) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_paths: NULL argument");
    uint64_t total = 0;
    for (uint64_t r = 0; r < n_reads; ++r) total += n_edges[r];
    if (total && !edges) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_paths: NULL argument");
    out_file o(path);
    if (!o.ok) return snk_fail(SNK_E_IO, err, errcap, "snk_write_paths: cannot create %s", path);
    const uint64_t var = sizeof(fcb_t) + n_reads * 8 + total * 4;
    const fcb_t h = {(uint32_t)n_reads, 1, 0, 24, 4, var, var + (n_reads + 1) * 8};     // sizeof(ReadPath) = 24, sizeof(int) = 4
    o.put(&h, sizeof h);
    uint64_t pos = 0;
    for (uint64_t r = 0; r < n_reads; ++r) {
        const uint32_t head[2] = {(uint32_t)offset[r], 0u};
        o.put(head, 8);
        const uint64_t s = start ? start[r] : pos;
        if (n_edges[r]) o.put(edges + s, (size_t)n_edges[r] * 4);
        pos += n_edges[r];
    }
    uint64_t at = sizeof(fcb_t);
    for (uint64_t r = 0; r <= n_reads; ++r) {
        o.put(&at, 8);
        if (r < n_reads) at += 8 + (uint64_t)n_edges[r] * 4;
    }
    if (!o.close()) return snk_fail(SNK_E_IO, err, errcap, "snk_write_paths: write error on %s", path);
    return SNK_OK;
}

extern "C" int snk_write_paths_index(const char* path_inv, const char* path_countsb, uint64_t E, const uint64_t* index_off, const uint64_t* index_ids,
                                     const int32_t* counts, char* err, size_t errcap) {
    if ((!path_inv && !path_countsb) || (path_inv && !index_off) || (path_countsb && E && !counts))
        return snk_fail(SNK_E_ARG, err, errcap, "snk_write_paths_index: NULL argument");
    if (path_inv) {
        if (index_off[0] != 0) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_paths_index: index_off does not start at 0");
        for (uint64_t e = 0; e < E; ++e)
            if (index_off[e + 1] < index_off[e]) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_paths_index: index_off decreases at edge %llu", (unsigned long long)e);
        const uint64_t n = index_off[E];
        if (n && !index_ids) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_paths_index: NULL argument");
        out_file o(path_inv);
        if (!o.ok) return snk_fail(SNK_E_IO, err, errcap, "snk_write_paths_index: cannot create %s", path_inv);
        const uint64_t var = sizeof(fcb_t) + n * 8;
        const fcb_t h = {(uint32_t)E, 1, 0, 16, 8, var, var + (E + 1) * 8};               // sizeof(ULongVec) = 16, sizeof(unsigned long) = 8
        o.put(&h, sizeof h);
        o.put(index_ids, (size_t)n * 8);
        for (uint64_t e = 0; e <= E; ++e) {
            const uint64_t at = sizeof(fcb_t) + index_off[e] * 8;
            o.put(&at, 8);
        }
        if (!o.close()) return snk_fail(SNK_E_IO, err, errcap, "snk_write_paths_index: write error on %s", path_inv);
    }
    if (path_countsb) {
        out_file o(path_countsb);
        if (!o.ok) return snk_fail(SNK_E_IO, err, errcap, "snk_write_paths_index: cannot create %s", path_countsb);
        const uint64_t one = 1;
        o.put("BINWRITE", 8);
        o.put(&one, 8);
        o.put(&E, 8);
        o.put(counts, (size_t)E * 4);
        if (!o.close()) return snk_fail(SNK_E_IO, err, errcap, "snk_write_paths_index: write error on %s", path_countsb);
    }
    return SNK_OK;
}

extern "C" int snk_write_dup(const char* path, uint64_t n_pairs, const uint8_t* dup, char* err, size_t errcap) {
    if (!path || (n_pairs && !dup)) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_dup: NULL argument");
    out_file o(path);
    if (!o.ok) return snk_fail(SNK_E_IO, err, errcap, "snk_write_dup: cannot create %s", path);
    o.put("BINWRITE", 8);
    o.put(&n_pairs, 8);
    o.put(dup, (size_t)n_pairs);
    if (!o.close()) return snk_fail(SNK_E_IO, err, errcap, "snk_write_dup: write error on %s", path);
    return SNK_OK;
}
