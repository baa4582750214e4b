// closures_driver.cc -- TEST INFRASTRUCTURE ONLY: runs the reference's own CloseGap and CloseGap2 (10X/Closomatic.cc:356-657) for
// tests/golden/make_closures_golden.py, over the pairs of an a.hops file, the way StageFindPatch does with STACKSTER=False
// (10X/runstages/RunStages.cc:334-384).
//
//   closures_driver in.snkrd a.hbv a.inv in.paths a.paths.inv in.hops CG2 MAX_WIDTH out.fastb out.pair_first
//
// in.snkrd is the read file of oracle/ref/ref_driver.cc (tests/refio.py), a.hbv / a.inv the graph as DF writes it, in.paths a feudal
// MasterVec<ReadPath> (what snk_write_paths wrote), a.paths.inv the paths index as this library's writer makes it (byte-equal to the
// reference's), in.hops a BINWRITE vec<pair<int,int>>.  Everything is handed over as MasterVecs (the explicit instantiations at
// Closomatic.cc:461-465 and :659-663).  The pairs run in the reference's 1000 batches under `omp parallel for`; the closures are appended
// batch by batch and written with BinaryWriter::writeFile(vec<basevector>), the way DF writes closures.fastb (10X/DF.cc:645).
// out.pair_first: u64[n_pairs + 1], the first closure of every pair.  The thread count comes from OMP_NUM_THREADS.
// Built by the maker in a scratch directory against the reference's headers and objects; nothing compiled from it is kept.
#include <omp.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "10X/Closomatic.h"
#include "feudal/BinaryStream.h"
#include "feudal/PQVec.h"
#include "paths/HyperBasevector.h"
#include "paths/long/ReadPath.h"
#include "system/RunTime.h"

int main(int argc, char** argv) {
    RunTime();
    if (argc != 11) {
        std::cerr << "usage: closures_driver in.snkrd a.hbv a.inv in.paths a.paths.inv in.hops CG2 MAX_WIDTH out.fastb out.pair_first" << std::endl;
        return 2;
    }
    // ---- the reads (SNKRD001: magic, u64 n, u32 stride, u32 has_bc, i64 ign_bc_below, u16 len[n], ASCII bases, raw qualities)
    FILE* f = fopen(argv[1], "rb");
    if (!f) { std::cerr << "cannot open " << argv[1] << std::endl; return 2; }
    char magic[8];
    uint64_t n = 0;
    uint32_t stride = 0, has_bc = 0;
    int64_t ign = 0;
    bool ok = fread(magic, 1, 8, f) == 8 && fread(&n, 8, 1, f) == 1 && fread(&stride, 4, 1, f) == 1 && fread(&has_bc, 4, 1, f) == 1 && fread(&ign, 8, 1, f) == 1;
    std::vector<uint16_t> len(n);
    std::vector<uint8_t> bs(n * stride), qs(n * stride);
    ok = ok && fread(len.data(), 2, n, f) == n && fread(bs.data(), 1, bs.size(), f) == bs.size() && fread(qs.data(), 1, qs.size(), f) == qs.size();
    fclose(f);
    if (!ok) { std::cerr << "short read file" << std::endl; return 2; }
    vecbasevector bases;
    VecPQVec quals;
    bvec b;
    qvec q;
    for (uint64_t r = 0; r < n; ++r) {
        const unsigned L = len[r];
        b.resize(L);
        q.resize(L);
        for (unsigned i = 0; i < L; ++i) {
            unsigned c = 0;
            switch (bs[r * stride + i]) { case 'C': c = 1; break; case 'G': c = 2; break; case 'T': c = 3; break; }
            b.Set(i, c);
            q[i] = qs[r * stride + i];
        }
        bases.push_back(b);
        quals.push_back(PQVec(q));
    }
    // ---- the graph, the paths, their index, the pairs
    HyperBasevector hbv;
    BinaryReader::readFile(argv[2], &hbv);
    HyperBasevectorX hb(hbv);
    vec<int> inv;
    BinaryReader::readFile(argv[3], &inv);
    ReadPathVec paths(argv[4]);
    VecULongVec paths_index(argv[5]);
    vec<std::pair<int, int>> pairs;
    BinaryReader::readFile(argv[6], &pairs);
    if (paths.size() != n || paths_index.size() != (size_t)hb.E() || inv.size() != (size_t)hb.E()) {
        std::cerr << paths.size() << " paths for " << n << " reads, " << paths_index.size() << " index entries and " << inv.size() << " inv entries for " << hb.E() << " edges"
                  << std::endl;
        return 2;
    }
    const bool CG2 = atoi(argv[7]) != 0;
    const int max_width = atoi(argv[8]);
    // ---- RunStages.cc:339-367 and :381-382
    const int batches = 1000;
    vec<vec<basevector>> closuresi(batches);
    std::vector<uint64_t> per_pair(pairs.size() + 1, 0);
    const int64_t NP = pairs.size();
    const double t0 = WallClockTime();
    #pragma omp parallel for
    for (int bi = 0; bi < batches; bi++) {
        for (int pi = bi * NP / batches; pi < (bi + 1) * NP / batches; pi++) {
            int e1 = pairs[pi].first, e2 = pairs[pi].second;
            vec<basevector> fc;
            if (CG2) CloseGap2(hb, inv, bases, quals, paths, paths_index, e1, e2, fc, False, pi, max_width);
            else CloseGap(hb, inv, bases, quals, paths, paths_index, e1, e2, fc, False, pi, max_width);
            per_pair[pi] = fc.size();
            closuresi[bi].append(fc);
        }
    }
    const double secs = WallClockTime() - t0;
    vec<basevector> closures;
    for (int bi = 0; bi < batches; bi++) closures.append(closuresi[bi]);
    BinaryWriter::writeFile(argv[9], closures);
    std::vector<uint64_t> first(pairs.size() + 1, 0);
    for (size_t i = 0; i < pairs.size(); ++i) first[i + 1] = first[i] + per_pair[i];
    f = fopen(argv[10], "wb");
    ok = f && fwrite(first.data(), 8, first.size(), f) == first.size();
    if (f) ok = fclose(f) == 0 && ok;
    if (!ok) { std::cerr << "cannot write " << argv[10] << std::endl; return 2; }
    std::cout << "CLOSURES_DRIVER K " << hb.K() << " threads " << omp_get_max_threads() << " reads " << n << " E " << hb.E() << " cg2 " << (CG2 ? 1 : 0) << " max_width " << max_width
              << " pairs " << pairs.size() << " closures " << closures.size() << " seconds " << secs << std::endl;
    return 0;
}
