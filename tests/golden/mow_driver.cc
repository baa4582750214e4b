// mow_driver.cc -- TEST INFRASTRUCTURE ONLY: runs the reference's own MowLawn (10X/Lawnmower.cc:301-554, the ReadPathVecX overload that
// StageTrim calls, 10X/runstages/RunStages.cc:70) behind its own MarkDups version 2 (10X/SecretOps.cc:599), for
// tests/golden/make_mow_golden.py.
//
//   mow_driver in.snkrd a.hbv a.inv in.paths WORK ALL_TESTS out.dup out.dels
//
// in.snkrd is the read file of oracle/ref/ref_driver.cc (tests/refio.py) with barcodes, a.hbv / a.inv the graph as DF writes it,
// in.paths a feudal MasterVec<ReadPath> (what snk_write_paths wrote).  The files MowLawn opens by name are made in WORK by the
// reference's own writers: a.paths.inv by writePathsIndex (10X/PathsIndex.cc:23-145, as 10X/DF.cc:588 calls it) and the .qualp by
// VecPQVec::WriteAll.  The paths are zipped by the reference's own ReadPathVecX::append.  ALL_TESTS = 0: `tests` is empty, the way
// StageTrim calls it; 1: `tests` names every edge, which takes the one-thread branch and prints e1, e2, qss1, qss2 for every
// candidate that passed the read limit (PRINT4, Lawnmower.cc:536).  out.dup is written with BinaryWriter::writeFile(vec<Bool>), out.dels
// as text, one edge id per line.  The thread count comes from OMP_NUM_THREADS.
// Built by the maker in a scratch directory against the reference's headers and objects; nothing compiled from it is kept.
#include <omp.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "10X/Lawnmower.h"
#include "10X/PathsIndex.h"
#include "10X/SecretOps.h"
#include "10X/paths/ReadPathVecX.h"
#include "feudal/BinaryStream.h"
#include "feudal/ObjectManager.h"
#include "feudal/PQVec.h"
#include "paths/HyperBasevector.h"
#include "paths/long/ReadPath.h"
#include "system/RunTime.h"

int main(int argc, char** argv) {
    RunTime();
    if (argc != 9) {
        std::cerr << "usage: mow_driver in.snkrd a.hbv a.inv in.paths WORK ALL_TESTS out.dup out.dels" << std::endl;
        return 2;
    }
    // ---- the reads (SNKRD001: magic, u64 n, u32 stride, u32 has_bc, i64 ign_bc_below, u16 len[n], ASCII bases, raw qualities, i32 bc[n])
    FILE* f = fopen(argv[1], "rb");
    if (!f) { std::cerr << "cannot open " << argv[1] << std::endl; return 2; }
    char magic[8];
    uint64_t n = 0;
    uint32_t stride = 0, has_bc = 0;
    int64_t ign = 0;
    bool ok = fread(magic, 1, 8, f) == 8 && fread(&n, 8, 1, f) == 1 && fread(&stride, 4, 1, f) == 1 && fread(&has_bc, 4, 1, f) == 1 && fread(&ign, 8, 1, f) == 1;
    std::vector<uint16_t> len(n);
    std::vector<uint8_t> bs(n * stride), qs(n * stride);
    std::vector<int32_t> bcs(n, 0);
    ok = ok && has_bc && fread(len.data(), 2, n, f) == n && fread(bs.data(), 1, bs.size(), f) == bs.size() && fread(qs.data(), 1, qs.size(), f) == qs.size() &&
         fread(bcs.data(), 4, n, f) == n;
    fclose(f);
    if (!ok) { std::cerr << "short read file, or one without barcodes" << std::endl; return 2; }
    vecbasevector bases;
    VecPQVec quals;
    vec<int32_t> bc(n);
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
        bc[r] = bcs[r];
    }
    // ---- the graph, the paths and the two files MowLawn opens
    const String work(argv[5]);
    HyperBasevector hbv;
    BinaryReader::readFile(argv[2], &hbv);
    HyperBasevectorX hb(hbv);
    vec<int> inv;
    BinaryReader::readFile(argv[3], &inv);
    ReadPathVec paths(argv[4]);
    if (paths.size() != n || (int)inv.size() != hb.E()) { std::cerr << "the inputs do not fit each other" << std::endl; return 2; }
    writePathsIndex(paths, inv, work, "a.paths.inv", "a.countsb", 15, false);
    quals.WriteAll(work + "/reads.qualp");
    ReadPathVecX px;
    px.append(paths, hb);
    vec<Bool> dup;
    double interdup = 0;
    MarkDups(bases, quals, px, hb, bc, dup, interdup);
    ObjectManager<VecPQVec> quals_om(work + "/reads.qualp");
    vec<int> dels, tests;
    if (atoi(argv[6]))
        for (int e = 0; e < hb.E(); ++e) tests.push_back(e);
    MowLawn(hb, inv, bases, quals_om, px, work + "/a.paths.inv", bc, dup, interdup, dels, tests);
    BinaryWriter::writeFile(argv[7], dup);
    std::ofstream out(argv[8]);
    for (int i = 0; i < dels.isize(); ++i) out << dels[i] << "\n";
    out.close();
    std::cout << "MOW_DRIVER K " << hb.K() << " threads " << omp_get_max_threads() << " reads " << n << " E " << hb.E() << " tests " << tests.size() << " sum_dup " << Sum(dup)
              << " dels " << dels.size() << std::endl;
    return 0;
}
