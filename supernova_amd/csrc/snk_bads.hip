// snk_bads.hip -- MarkBads on the device: the first step of StageFindPatch (10X/runstages/RunStages.cc:261, and :52), whose result DF
// keeps as a.bad (10X/DF.cc:644) and FindEdgePairs reads to drop pairs from its "rights" (10X/Closomatic.cc:293,316).
//
// What it replaces: both overloads of MarkBads, lib/assembly/src/10X/SecretOps.cc:70-107 (ReadPath: the int offset) and :22-59
// (ReadPathVecX: the path has been through zip / unzip, so its offset is static_cast<int16_t>(offset) -- SNK_BADS_X).  For a read with a
// path p:  m = hb.Cat(p) (paths/HyperBasevector.cc:631-635), a chain of TrimCat (feudal/BaseVec.h:550-558): what is there loses its last
// K-1 bases and the next edge is appended WHOLE, adjacent or not -- so where two edges disagree inside the K-1 bases they would share,
// m shows the LATER edge's;  badsum = the raw quality summed over the read positions l with 0 <= offset + l < |m| and
// read[l] != m[offset + l]; a pair is bad iff badsum > 150 for either mate.  MAX_BAD and MIN_HQ of the source are unused.
//
// m is never made.  With S_j = the k-mers of the edges in front of edge j, edge j supplies m[S_j, b_j), b_j = S_j + Kmers(p[j]) = S_(j+1)
// for every edge but the last, which supplies all its bases: the pieces follow each other without a gap, and position t of piece j is
// base t - S_j of the edge.
//
// Passes.
//   b_table_kernel   one lane per read: start / n_edges add up (before anything indexes with them)
//   b_edges_kernel   one lane per read, once the edge ids are known to lie inside the graph: an edge shorter than K; with SNK_BADS_X a
//                    path of more than 255 edges and a step e -> e' with e' not in From(ToRight(e))
//   b_bads_kernel    8 lanes per PAIR, 4 per mate.  Lane q of a mate takes the read's row words q, q + 4, ...: a word's 16 bases are
//                    XORed, piece by piece, against 16 bases of the edge taken from the packed unitigs (pg_edge16: a reverse-complement edge is
//                    read backwards).  A zero XOR loads no quality byte; a mismatch is found with clz and fetches its own.  A lane's
//                    words rise, so its place in the path only moves forward: a path is walked once per lane.  The mate's sum is two
//                    shuffles, the pair's flag a third: no atomic decides a result, and the counters are summed per workgroup before
//                    five atomics.
// The common read -- one edge, no mismatch -- costs per lane its path record, the edge record and, per word, one row word and two words
// of unitig.
#include <string.h>

#include "snk_bads.h"
#include "snk_common.h"
#include "snk_hbvadj.h"

namespace {

constexpr unsigned BB = 256;                 // lanes of a workgroup
constexpr unsigned LPM = 4, LPP = 2 * LPM;   // lanes per mate, per pair
constexpr unsigned PPB = BB / LPP;           // pairs per workgroup and step
constexpr int MAX_BAD_SUM = 150;             // SecretOps.cc:29,77
constexpr uint64_t B_GRID_CAP = 1u << 20;
constexpr uint32_t F_TABLE = 1, F_LONG = 2, F_STEP = 4, F_SHORT = 8;
enum { N_PLACED, N_MISMATCH, N_BAD_READS, N_BAD_PAIRS, N_WRAPPED, N_COUNTED, N_COUNTERS = 8 };

struct b_paths {                             // of the launch's reads: read r of the launch is entry r (edges: the whole array, start indexes it)
    const unsigned long long* start;
    const uint32_t* n_edges;
    const int32_t* offset;
    const uint32_t* edges;
};

__global__ void __launch_bounds__(BB) b_table_kernel(uint64_t n, const unsigned long long* __restrict__ start, const uint32_t* __restrict__ n_edges, uint64_t n_entries,
                                                     uint32_t* __restrict__ flags) {
    for (uint64_t r = (uint64_t)blockIdx.x * BB + threadIdx.x; r < n; r += (uint64_t)gridDim.x * BB) {
        if (!snk_paths_row_ok(start, n_edges, r, n, n_entries)) atomicOr(flags, F_TABLE);
    }
}

__global__ void __launch_bounds__(BB) b_edges_kernel(path_graph G, int K, uint32_t xmode, uint64_t n, const unsigned long long* __restrict__ start,
                                                     const uint32_t* __restrict__ n_edges, const uint32_t* __restrict__ edges, uint32_t* __restrict__ flags) {
    for (uint64_t r = (uint64_t)blockIdx.x * BB + threadIdx.x; r < n; r += (uint64_t)gridDim.x * BB) {
        const uint64_t s = start[r], m = n_edges[r];
        if (!m) continue;
        uint32_t f = 0;
        if (xmode && m > 255) { atomicOr(flags, F_LONG); continue; }
        uint32_t e = edges[s];
        for (uint64_t j = 0; j < m; ++j) {
            if (pg_edge_len(G, e) < (uint32_t)K) f |= F_SHORT;
            if (j + 1 == m) break;
            const uint32_t e2 = edges[s + j + 1];
            if (xmode) {
                const int32_t v = G.vright[e];
                bool found = false;
                for (int l = G.from_off[v]; l < G.from_off[v + 1]; ++l) found |= (uint32_t)G.from_e[l] == e2;
                if (!found) f |= F_STEP;
            }
            e = e2;
        }
        if (f) atomicOr(flags, f);
    }
}

__global__ void __launch_bounds__(BB) b_bads_kernel(path_graph G, snk_reads_view R, b_paths P, int K, uint32_t xmode, uint8_t* __restrict__ bad,
                                                    unsigned long long* __restrict__ counters) {
    __shared__ uint32_t l_cnt[BB / 64][N_COUNTED];
    const uint32_t tid = threadIdx.x, q = tid & (LPM - 1), mate = (tid / LPM) & 1u;
    const uint64_t n_pairs = R.n / 2;
    uint32_t cnt[N_COUNTED] = {0, 0, 0, 0, 0};
    // every lane of a workgroup makes the same number of steps: the shuffles below are reached by whole waves
    for (uint64_t base = (uint64_t)blockIdx.x * PPB; base < n_pairs; base += (uint64_t)gridDim.x * PPB) {
        const uint64_t pair = base + tid / LPP;
        const bool on = pair < n_pairs;
        const uint64_t r = 2 * pair + mate;
        const uint32_t m = on ? P.n_edges[r] : 0u;
        int badsum = 0, nmis = 0;
        bool wrapped = false;
        if (m) {
            const int len = (int)snk_read_len(R, r);
            const int off0 = P.offset[r];
            const int off = xmode ? (int)(int16_t)off0 : off0;          // (ReadPathParser.cc:184-198: the record holds static_cast<int16_t>)
            wrapped = (int)(int16_t)off0 != off0;
            const uint64_t s = P.start[r];
            const uint32_t* row = R.rows + r * R.row_words;
            const uint8_t* qual = R.quals + r * R.qstride;
            // the lane's place in the path: piece j = m[S, b), S = the k-mers in front of it
            uint32_t j = 0;
            pg_edge x = pg_edge_load(G, P.edges[s]);
            long long S = 0, b = m > 1 ? (long long)x.len - (K - 1) : (long long)x.len;
            for (int w = (int)q; 16 * w < len && j < m; w += (int)LPM) {
                long long lo = (long long)off + 16 * w;
                const long long hi = lo + min(16, len - 16 * w);
                if (hi <= 0) continue;                                  // in front of m: skipped, not counted
                if (lo < 0) lo = 0;
                const uint32_t word = row[w];
                while (lo < hi) {
                    while (b <= lo && ++j < m) {
                        S = b;
                        x = pg_edge_load(G, P.edges[s + j]);
                        b = S + (j + 1 < m ? (long long)x.len - (K - 1) : (long long)x.len);
                    }
                    if (j >= m) break;                                  // behind m: skipped
                    const long long top = hi < b ? hi : b;
                    const int rp = (int)(lo - off);
                    uint32_t d = (word << (2 * (rp - 16 * w))) ^ pg_edge16(G, x, (uint32_t)(lo - S));
                    d = (d | (d << 1)) & 0xAAAAAAAAu;
                    const uint32_t c = (uint32_t)(top - lo);
                    if (c < 16) d &= ~(0xFFFFFFFFu >> (2 * c));
                    while (d) {                                         // only a mismatch fetches its quality
                        const int g = __clz((int)d) >> 1;
                        badsum += (int)qual[rp + g];
                        ++nmis;
                        d &= ~(0x80000000u >> (2 * g));
                    }
                    lo = top;
                }
            }
        }
        badsum += __shfl_xor(badsum, 1); badsum += __shfl_xor(badsum, 2);
        nmis += __shfl_xor(nmis, 1); nmis += __shfl_xor(nmis, 2);
        const int mine = badsum > MAX_BAD_SUM ? 1 : 0;
        const int either = mine | __shfl_xor(mine, (int)LPM);
        if (q == 0) {
            cnt[N_PLACED] += m ? 1u : 0u;
            cnt[N_MISMATCH] += nmis ? 1u : 0u;
            cnt[N_BAD_READS] += (uint32_t)mine;
            cnt[N_WRAPPED] += wrapped ? 1u : 0u;
        }
        if (on && (tid & (LPP - 1)) == 0) {
            bad[pair] = (uint8_t)either;
            cnt[N_BAD_PAIRS] += (uint32_t)either;
        }
    }
#pragma unroll
    for (int k = 0; k < N_COUNTED; ++k) {
        uint32_t v = cnt[k];
        for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
        if ((tid & 63) == 0) l_cnt[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < N_COUNTED) {
        uint32_t v = 0;
        for (unsigned w = 0; w < BB / 64; ++w) v += l_cnt[w][tid];
        if (v) atomicAdd(&counters[tid], (unsigned long long)v);
    }
}

}  // namespace

int snk_bads_check_args(const char* who, uint32_t K, uint64_t n, uint32_t read_len, bool have_quals, uint64_t n_unitigs, const void* d_unitig_off,
                        const void* d_unitig_bases, const snk_hbv* h, const snk_dev_paths* paths, uint32_t flags, char* err, size_t errcap) {
    if (K != 48 && K != 60) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "K=%u is not supported (48 or 60)", K);
    if (flags & ~SNK_BADS_X) return snk_fail(SNK_E_ARG, err, errcap, "%s: unknown flag bits 0x%x", who, flags & ~SNK_BADS_X);
    if (n & 1) return snk_fail(SNK_E_ARG, err, errcap, "%s: %llu reads are not pairs (reads 2q and 2q + 1 are mates)", who, (unsigned long long)n);
    const uint64_t n_entries = paths->n_edges_total, E = (uint64_t)(h->n_edges > 0 ? h->n_edges : 0);
    if (paths->n_reads != n) return snk_fail(SNK_E_ARG, err, errcap, "%s: %llu paths for %llu reads", who, (unsigned long long)paths->n_reads, (unsigned long long)n);
    if (n && !have_quals) return snk_fail(SNK_E_ARG, err, errcap, "%s: quals == NULL (a mismatch counts with its raw quality)", who);
    if (read_len > 256) return snk_fail(SNK_E_ARG, err, errcap, "%s: reads of at most 256 bases (read_len = %u)", who, read_len);
    if (n_unitigs && (!d_unitig_off || !d_unitig_bases)) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL unitig arrays", who);
    if (n_unitigs >= (1ull << 31)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: too many unitigs", who);
    if (E && (!h->v_left || !h->v_right || !h->src_unitig || !h->is_rc || !h->fwd_xlat || !h->rev_xlat)) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument", who);
    if (n && (!paths->start || !paths->n_edges || !paths->offset)) return snk_fail(SNK_E_ARG, err, errcap, "%s: paths without their device arrays", who);
    if (n_entries && !paths->edges) return snk_fail(SNK_E_ARG, err, errcap, "%s: paths without their device arrays", who);
    if (n_entries && !E) return snk_fail(SNK_E_ARG, err, errcap, "%s: %llu path entries on a graph without edges", who, (unsigned long long)n_entries);
    if (!n && n_entries) return snk_fail(SNK_E_ARG, err, errcap, "%s: start / n_edges do not add up to n_edges_total = %llu", who, (unsigned long long)n_entries);
    if (n >= (1ull << 40)) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: too many reads", who);
    for (uint64_t u = 0; u < n_unitigs; ++u)
        if (h->fwd_xlat[u] < 0 || h->rev_xlat[u] < 0 || (uint64_t)h->fwd_xlat[u] >= E || (uint64_t)h->rev_xlat[u] >= E ||
            (h->bvcomp_order && (h->bvcomp_order[u] < 0 || (uint64_t)h->bvcomp_order[u] >= n_unitigs)))
            return snk_fail(SNK_E_ARG, err, errcap, "%s: inconsistent translation tables", who);
    for (uint64_t e = 0; e < E; ++e)
        if (h->src_unitig[e] < 0 || (uint64_t)h->src_unitig[e] >= n_unitigs) return snk_fail(SNK_E_ARG, err, errcap, "%s: edge %llu is out of range", who, (unsigned long long)e);
    return SNK_OK;
}

int snk_bads_begin(snk_call& c, path_host& H, const char* who, uint32_t K, uint64_t n, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases,
                   const snk_hbv* h, const snk_dev_paths* paths, uint32_t flags, bads_job* job, char* err, size_t errcap) {
    const hipStream_t st = c.st;
    int rc;
    memset(job, 0, sizeof *job);
    const uint64_t n_entries = paths->n_edges_total, E = (uint64_t)(h->n_edges > 0 ? h->n_edges : 0);
    uint64_t total_bases = 0;
    if ((rc = snk_path_graph_tables(c, H, K, n_unitigs, (const uint64_t*)d_unitig_off, (const uint8_t*)d_unitig_bases, h, &job->G, &total_bases, who, err, errcap))) return rc;
    job->K = (int)K; job->x = flags & SNK_BADS_X; job->n_reads = n;
    job->start = (const unsigned long long*)paths->start; job->n_edges = (const uint32_t*)paths->n_edges; job->offset = (const int32_t*)paths->offset;
    job->edges = (const uint32_t*)paths->edges;
    uint32_t* range;
    if ((rc = c.alloc(256 + 1, &range)) || (rc = c.alloc(N_COUNTERS, &job->counters)) || (rc = c.alloc(n / 2, &job->bad))) return rc;
    SNK_HIP_TRY(hipMemsetAsync(range, 0, 257 * 4, st));
    SNK_HIP_TRY(hipMemsetAsync(job->counters, 0, N_COUNTERS * 8, st));
    SNK_HIP_TRY(hipMemsetAsync(job->bad, 0, n / 2 + 1, st));
    uint32_t* d_flags = range + 256;
    // ---- the refusals: the table and the edge ids first, then what indexes with them
    SNK_HIP_TRY(snk_launch(b_table_kernel, snk_blocks_capped(n, BB, B_GRID_CAP), BB, 0, st, n, job->start, job->n_edges, n_entries, d_flags));
    if (n_entries) SNK_HIP_TRY(snk_max_edge_id(job->edges, n_entries, range, st));
    uint32_t h_range[257];
    SNK_HIP_TRY(hipMemcpyAsync(h_range, range, sizeof h_range, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    uint32_t emax = 0;
    for (int q = 0; q < 256; ++q) emax = emax > h_range[q] ? emax : h_range[q];
    if (h_range[256] & F_TABLE) return snk_fail(SNK_E_ARG, err, errcap, "%s: start / n_edges do not add up to n_edges_total = %llu", who, (unsigned long long)n_entries);
    if (n_entries && emax >= E) return snk_fail(SNK_E_ARG, err, errcap, "%s: a path holds edge id %lld, the graph has %llu edges", who, (long long)(int32_t)emax, (unsigned long long)E);
    if (job->x)
        for (int32_t v = 0; v < h->n_vertices; ++v)
            if (H.off_from[(size_t)v + 1] - H.off_from[v] > 4)
                return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: vertex %d has more than four out-edges (SNK_BADS_X: a ReadPathVecX has two bits per branch)", who, v);
    SNK_HIP_TRY(snk_launch(b_edges_kernel, snk_blocks_capped(n, BB, B_GRID_CAP), BB, 0, st, job->G, job->K, job->x, n, job->start, job->n_edges, job->edges, d_flags));
    uint32_t f = 0;
    SNK_HIP_TRY(hipMemcpyAsync(&f, d_flags, 4, hipMemcpyDeviceToHost, st));
    SNK_HIP_TRY(snk_sync(st));
    if (f & F_LONG) return snk_fail(SNK_E_UNSUPPORTED, err, errcap, "%s: a path of more than 255 edges (SNK_BADS_X: the record's edge count is one byte)", who);
    if (f & F_SHORT) return snk_fail(SNK_E_ARG, err, errcap, "%s: a path holds an edge of fewer than K = %u bases", who, K);
    if (f & F_STEP)
        return snk_fail(SNK_E_ARG, err, errcap, "%s: a path steps to an edge that does not leave the vertex its predecessor ends in (SNK_BADS_X: zip / unzip would not return it)", who);
    return SNK_OK;
}

hipError_t snk_bads_slab(const bads_job& job, uint64_t first, const snk_reads_view& R, hipStream_t st) {
    const uint64_t n = R.n;
    if (!n) return hipSuccess;
    if ((first & 1) || (n & 1) || first > job.n_reads || n > job.n_reads - first) return hipErrorInvalidValue;
    b_paths P;
    P.start = job.start + first; P.n_edges = job.n_edges + first; P.offset = job.offset + first; P.edges = job.edges;
    return snk_launch(b_bads_kernel, snk_blocks_capped(n / 2, PPB, B_GRID_CAP), BB, 0, st, job.G, R, P, job.K, job.x, job.bad + first / 2, job.counters);
}

int snk_bads_finish(snk_call& c, const bads_job& job, snk_dev_bads* out, char* err, size_t errcap) {
    unsigned long long h_cnt[N_COUNTERS];
    SNK_HIP_TRY(hipMemcpyAsync(h_cnt, job.counters, sizeof h_cnt, hipMemcpyDeviceToHost, c.st));
    SNK_HIP_TRY(snk_sync(c.st));
    out->n_pairs = job.n_reads / 2;
    out->bad = job.bad;
    out->n_placed = h_cnt[N_PLACED];
    out->n_mismatch_reads = h_cnt[N_MISMATCH];
    out->n_bad_reads = h_cnt[N_BAD_READS];
    out->n_bad_pairs = h_cnt[N_BAD_PAIRS];
    out->n_offsets_wrapped = h_cnt[N_WRAPPED];
    return SNK_OK;
}

extern "C" int snk_dev_mark_bads(snk_ctx* ctx, uint32_t K, const snk_dev_reads* in, uint64_t n_unitigs, const void* d_unitig_off, const void* d_unitig_bases,
                                 const snk_hbv* h, const snk_dev_paths* paths, uint32_t flags, snk_dev_bads* out, void* stream, char* err, size_t errcap) {
    static const char who[] = "snk_dev_mark_bads";
    if (!ctx || !in || !h || !paths || !out) return snk_fail(SNK_E_ARG, err, errcap, "%s: NULL argument", who);
    memset(out, 0, sizeof *out);
    const uint64_t n = in->n_reads;
    int rc = snk_bads_check_args(who, K, n, in->read_len, in->quals != nullptr, n_unitigs, d_unitig_off, d_unitig_bases, h, paths, flags, err, errcap);
    if (rc) return rc;
    if (n && (!in->rows || in->read_len == 0 || in->row_words * 16 < in->read_len || in->row_words > 16))
        return snk_fail(SNK_E_ARG, err, errcap, "%s: need packed rows of at most 256 bases that hold read_len", who);
    if (n && in->qstride < in->read_len) return snk_fail(SNK_E_ARG, err, errcap, "%s: quality rows shorter than read_len", who);
    path_host H;           // (the uploads read it: declared in front of the frame)
    return snk_call_run(ctx, stream, who, out, err, errcap, [&](snk_call& c) -> int {
        int rc2;
        SNK_HIP_TRY(c.stamp());
        bads_job job;
        if ((rc2 = snk_bads_begin(c, H, who, K, n, n_unitigs, d_unitig_off, d_unitig_bases, h, paths, flags, &job, err, errcap))) return rc2;
        SNK_HIP_TRY(c.stamp());
        SNK_HIP_TRY(snk_bads_slab(job, 0, snk_reads_view_of(in, n), c.st));
        SNK_HIP_TRY(c.stamp());
        if ((rc2 = snk_bads_finish(c, job, out, err, errcap))) return rc2;
        out->ms = c.ms(0, 2);
        out->tables_ms = c.ms(0, 1);
        out->kernel_ms = c.ms(1, 2);
        out->n_slabs = n ? 1 : 0;
        return c.end(SNK_OK, {job.bad});
    });
}
