// snk_a48.hip -- host writers for the files DF leaves in a.48/ beside a.hbv and a.inv (those: snk_hbv.hip), and for a.ebcx.  No device code.
//   a.paths      feudal MasterVec<ReadPath>   paths/long/ReadPath.h:61-63 (writeFeudal: offset, last skip, the edge ids),
//                                             IncrementalWriter, feudal/FeudalFileWriter.cc:18-140; written as tmp.paths by pathReads
//                                             (BuildReadQGraph48.cc:1441-1469), renamed at 10X/DF.cc:584
//   a.paths.inv  feudal MasterVec<ULongVec>   10X/PathsIndex.cc:76,100-108
//   a.countsb    BINWRITE vec<vec<int>>       10X/PathsIndex.cc:75,135 (one inner vector)
//   a.dup        BINWRITE vec<Bool>           10X/DF.cc:599-600
//   a.pathsX     raw ReadPathVecX             10X/paths/ReadPathVecX.cc:976-996 (five int64, the ZipIndex, the zipped data)
//   a.hbx        BINWRITE HyperBasevectorX    paths/HyperBasevector.cc:133-137, graph/DigraphTemplate.h:3107-3113; 10X/DF.cc:573-576
//   a.ebcx       feudal MasterVec<SerfVec<int>> VecIntVec::WriteAll of computeEdgeToBarcodeX's result (10X/PathsIndex.cc:297-358); not in a.48/
// A feudal file: 24-byte control block (feudal/FeudalControlBlock.h:157-166), the elements' variable-length data back to back, the
// table of N + 1 file offsets, then the fixed-length data (none for these element types).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include <vector>

#include "snk_ctx.h"
#include "snk_hbvadj.h"

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

extern "C" int snk_write_pathsx(const char* path, uint64_t n_reads, const int64_t* index, uint64_t n_index, const uint8_t* data, uint64_t n_bytes, char* err, size_t errcap) {
    if (!path || (n_index && !index) || (n_bytes && !data)) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_pathsx: NULL argument");
    if (n_index != (n_reads + 9) / 10)
        return snk_fail(SNK_E_ARG, err, errcap, "snk_write_pathsx: %llu index entries for %llu reads (one per 10)", (unsigned long long)n_index, (unsigned long long)n_reads);
    out_file o(path);
    if (!o.ok) return snk_fail(SNK_E_IO, err, errcap, "snk_write_pathsx: cannot create %s", path);
    const int64_t head[5] = {10, 0, (int64_t)n_reads, (int64_t)n_index, (int64_t)n_bytes};      // skip, start_rid, next_start_rid, sizes
    o.put(head, sizeof head);
    o.put(index, (size_t)n_index * 8);
    o.put(data, (size_t)n_bytes);
    if (!o.close()) return snk_fail(SNK_E_IO, err, errcap, "snk_write_pathsx: write error on %s", path);
    return SNK_OK;
}

extern "C" int snk_read_pathsx(const char* path, uint64_t* n_reads, uint64_t* n_index, int64_t** index, uint64_t* n_bytes, uint8_t** data, char* err, size_t errcap) {
    if (!path || !n_reads || !n_index || !index || !n_bytes || !data) return snk_fail(SNK_E_ARG, err, errcap, "snk_read_pathsx: NULL argument");
    *n_reads = *n_index = *n_bytes = 0;
    *index = nullptr;
    *data = nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) return snk_fail(SNK_E_IO, err, errcap, "snk_read_pathsx: cannot open %s", path);
    int64_t head[5];
    bool ok = fread(head, 8, 5, f) == 5 && fseek(f, 0, SEEK_END) == 0;
    const long long size = ok ? (long long)ftell(f) : -1;
    // skip 10 and reads from 0: what DF writes; the sizes must be the file's
    // (every count is bounded by the file's size before it is multiplied: a hostile header cannot overflow the sums)
    ok = ok && head[0] == 10 && head[1] == 0 && head[2] >= 0 && head[2] <= size && head[3] >= 0 && head[3] <= size / 8 && head[4] >= 0 && head[4] <= size &&
         head[3] == (head[2] + 9) / 10 && head[4] >= head[2] && head[4] <= head[2] * 71 && size == 40 + head[3] * 8 + head[4] && fseek(f, 40, SEEK_SET) == 0;
    if (!ok) { fclose(f); return snk_fail(SNK_E_IO, err, errcap, "snk_read_pathsx: %s is not an a.pathsX file (header and size disagree)", path); }
    int64_t* ix = (int64_t*)malloc((size_t)head[3] * 8 + 8);
    uint8_t* d = (uint8_t*)malloc((size_t)head[4] + 8);
    if (!ix || !d) { free(ix); free(d); fclose(f); return snk_fail(SNK_E_NOMEM, err, errcap, "snk_read_pathsx: host allocation failed"); }
    ok = fread(ix, 8, (size_t)head[3], f) == (size_t)head[3] && fread(d, 1, (size_t)head[4], f) == (size_t)head[4];
    fclose(f);
    if (!ok) { free(ix); free(d); return snk_fail(SNK_E_IO, err, errcap, "snk_read_pathsx: short read from %s", path); }
    *n_reads = (uint64_t)head[2];
    *n_index = (uint64_t)head[3];
    *n_bytes = (uint64_t)head[4];
    *index = ix;
    *data = d;
    return SNK_OK;
}

extern "C" int snk_write_ebcx(const char* path, uint64_t E, const uint64_t* ebc_off, const int32_t* ebc, char* err, size_t errcap) {
    if (!path || !ebc_off) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_ebcx: NULL argument");
    if (ebc_off[0] != 0) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_ebcx: ebc_off does not start at 0");
    for (uint64_t e = 0; e < E; ++e)
        if (ebc_off[e + 1] < ebc_off[e]) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_ebcx: ebc_off decreases at edge %llu", (unsigned long long)e);
    const uint64_t n = ebc_off[E];
    if (n && !ebc) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_ebcx: NULL argument");
    out_file o(path);
    if (!o.ok) return snk_fail(SNK_E_IO, err, errcap, "snk_write_ebcx: cannot create %s", path);
    const uint64_t var = sizeof(fcb_t) + n * 4;
    const fcb_t h = {(uint32_t)E, 1, 0, 16, 4, var, var + (E + 1) * 8};                   // sizeof(SerfVec<int>) = 16, sizeof(int) = 4
    o.put(&h, sizeof h);
    o.put(ebc, (size_t)n * 4);
    for (uint64_t e = 0; e <= E; ++e) {
        const uint64_t at = sizeof(fcb_t) + ebc_off[e] * 4;
        o.put(&at, 8);
    }
    if (!o.close()) return snk_fail(SNK_E_IO, err, errcap, "snk_write_ebcx: write error on %s", path);
    return SNK_OK;
}

extern "C" int snk_read_ebcx(const char* path, uint64_t* n_hbv_edges, uint64_t** ebc_off, int32_t** ebc, char* err, size_t errcap) {
    if (!path || !n_hbv_edges || !ebc_off || !ebc) return snk_fail(SNK_E_ARG, err, errcap, "snk_read_ebcx: NULL argument");
    *n_hbv_edges = 0;
    *ebc_off = nullptr;
    *ebc = nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) return snk_fail(SNK_E_IO, err, errcap, "snk_read_ebcx: cannot open %s", path);
    fcb_t h;
    bool ok = fread(&h, sizeof h, 1, f) == 1 && fseek(f, 0, SEEK_END) == 0;
    const long long size = ok ? (long long)ftell(f) : -1;
    // the control block of a MasterVec<SerfVec<int>> without fixed-length data, and sizes that are the file's: the lists fill
    // [24, var_offset), the table of E + 1 offsets [var_offset, fixed_offset = size)
    ok = ok && h.flags == 1 && h.sizeof_fixed == 0 && h.sizeof_x == 16 && h.sizeof_a == 4 && h.fixed_offset == (uint64_t)size && h.var_offset >= sizeof(fcb_t) &&
         h.var_offset <= h.fixed_offset - 8 && (h.var_offset - sizeof(fcb_t)) % 4 == 0 && (h.fixed_offset - h.var_offset) % 8 == 0;
    const uint64_t E = ok ? (h.fixed_offset - h.var_offset) / 8 - 1 : 0, n = ok ? (h.var_offset - sizeof(fcb_t)) / 4 : 0;
    ok = ok && (uint32_t)E == h.n && fseek(f, sizeof(fcb_t), SEEK_SET) == 0;
    if (!ok) { fclose(f); return snk_fail(SNK_E_IO, err, errcap, "snk_read_ebcx: %s is not an a.ebcx file (control block and size disagree)", path); }
    uint64_t* off = (uint64_t*)malloc((size_t)(E + 1) * 8);
    int32_t* d = (int32_t*)malloc((size_t)n * 4 + 8);
    if (!off || !d) { free(off); free(d); fclose(f); return snk_fail(SNK_E_NOMEM, err, errcap, "snk_read_ebcx: host allocation failed"); }
    ok = fread(d, 4, (size_t)n, f) == (size_t)n && fread(off, 8, (size_t)(E + 1), f) == (size_t)(E + 1);
    fclose(f);
    if (!ok) { free(off); free(d); return snk_fail(SNK_E_IO, err, errcap, "snk_read_ebcx: short read from %s", path); }
    // file offsets -> entries: they start at the control block's end, end at the table, never decrease and fall on whole ints
    ok = off[0] == sizeof(fcb_t) && off[E] == h.var_offset;
    for (uint64_t e = 0; ok && e < E; ++e) ok = off[e + 1] >= off[e] && off[e + 1] <= h.var_offset && (off[e + 1] - sizeof(fcb_t)) % 4 == 0;
    if (!ok) { free(off); free(d); return snk_fail(SNK_E_IO, err, errcap, "snk_read_ebcx: the offset table of %s does not add up", path); }
    for (uint64_t e = 0; e <= E; ++e) off[e] = (off[e] - sizeof(fcb_t)) / 4;
    *n_hbv_edges = E;
    *ebc_off = off;
    *ebc = d;
    return SNK_OK;
}

static int write_hbx_impl(const char* path, uint32_t K, uint64_t U, const uint64_t* off, const uint8_t* bases, const snk_hbv* h, char* err, size_t errcap) {
    const int32_t N = h->n_vertices, E = h->n_edges;
    for (int32_t e = 0; e < E; ++e)
        if (h->src_unitig[e] < 0 || (uint64_t)h->src_unitig[e] >= U) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_hbx: edge %d is out of range", e);
    snk_hbv_lists ls;
    const int rc = snk_hbv_lists_build(h, &ls, "snk_write_hbx", err, errcap);
    if (rc) return rc;
    out_file o(path);
    if (!o.ok) return snk_fail(SNK_E_IO, err, errcap, "snk_write_hbx: cannot create %s", path);
    o.put("BINWRITE", 8);
    const int32_t k32 = (int32_t)K;
    o.put(&k32, 4);
    // VecIntVec = MasterVec<SerfVec<int>>: u64 count, per element a u32 count and its ints (feudal/OuterVec.h:377-379, SmallVec.h:355-357)
    auto put_lists = [&](const std::vector<uint64_t>& loff, const std::vector<int32_t>& vals) {
        const uint64_t n = (uint64_t)N;
        o.put(&n, 8);
        for (int32_t v = 0; v < N; ++v) {
            const uint32_t m = (uint32_t)(loff[(size_t)v + 1] - loff[v]);
            o.put(&m, 4);
            if (m) o.put(vals.data() + loff[v], (size_t)m * 4);
        }
    };
    put_lists(ls.from_off, ls.from_v);
    put_lists(ls.to_off, ls.to_v);
    put_lists(ls.from_off, ls.from_e);
    put_lists(ls.to_off, ls.to_e);
    const uint64_t e64 = (uint64_t)E;
    o.put(&e64, 8);
    std::vector<uint8_t> buf;
    for (int32_t e = 0; e < E; ++e) {
        const uint64_t len64 = snk_hbv_edge_image(h, e, off, bases, buf);
        if (len64 > 0xFFFFFFFFull) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "snk_write_hbx: edge longer than 2^32 bases");
        const uint32_t len = (uint32_t)len64;
        o.put(&len, 4);
        o.put(buf.data(), buf.size());
    }
    o.put(&e64, 8);
    o.put(h->v_left, (size_t)E * 4);
    o.put(&e64, 8);
    o.put(h->v_right, (size_t)E * 4);
    if (!o.close()) return snk_fail(SNK_E_IO, err, errcap, "snk_write_hbx: write error on %s", path);
    return SNK_OK;
}

extern "C" int snk_write_hbx(const char* path, uint32_t K, uint64_t n_unitigs, const uint64_t* unitig_off, const uint8_t* unitig_bases, const snk_hbv* h, char* err,
                             size_t errcap) {
    if (!path || !h || (n_unitigs && (!unitig_off || !unitig_bases))) return snk_fail(SNK_E_ARG, err, errcap, "snk_write_hbx: NULL argument");
    try { return write_hbx_impl(path, K, n_unitigs, unitig_off, unitig_bases, h, err, errcap); }
    catch (const std::bad_alloc&) { return snk_fail(SNK_E_NOMEM, err, errcap, "snk_write_hbx: host allocation failed"); }
}
