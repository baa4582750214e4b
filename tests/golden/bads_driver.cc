// bads_driver.cc -- TEST INFRASTRUCTURE ONLY: runs the reference's own MarkBads (10X/SecretOps.cc:22-59 and :70-107) for
// tests/golden/make_bads_golden.py.
//
//   bads_driver in.snkrd a.hbv in.paths MODES out.bad_plain out.bad_x
//
// in.snkrd is the read file of oracle/ref/ref_driver.cc (tests/refio.py), a.hbv the graph as DF writes it, in.paths a feudal
// MasterVec<ReadPath> (what snk_write_paths wrote).  MODES: bit 0 = the ReadPath overload (:70-107) on the paths as they are, bit 1 = the
// ReadPathVecX overload (:22-59) on the paths zipped by the reference's own ReadPathVecX::append.  Both are reached through the explicit
// instantiations at SecretOps.cc:64-65 and :112-113.  Each result is written with BinaryWriter::writeFile(vec<Bool>), the way DF writes
// a.bad (10X/DF.cc:644).  The thread count comes from OMP_NUM_THREADS.
// Built by the maker in a scratch directory against the reference's headers and objects; nothing compiled from it is kept.
#include <omp.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "10X/SecretOps.h"
#include "10X/paths/ReadPathVecX.h"
#include "feudal/BinaryStream.h"
#include "feudal/PQVec.h"
#include "paths/HyperBasevector.h"
#include "paths/long/ReadPath.h"
#include "system/RunTime.h"

int main(int argc, char** argv) {
    RunTime();
    if (argc != 7) {
        std::cerr << "usage: bads_driver in.snkrd a.hbv in.paths MODES out.bad_plain out.bad_x" << std::endl;
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
    // ---- the graph and the paths
    HyperBasevector hbv;
    BinaryReader::readFile(argv[2], &hbv);
    HyperBasevectorX hb(hbv);
    ReadPathVec paths(argv[3]);
    if (paths.size() != n) { std::cerr << paths.size() << " paths for " << n << " reads" << std::endl; return 2; }
    const int modes = atoi(argv[4]);
    size_t nonempty = 0, wrapped = 0;
    for (size_t r = 0; r < paths.size(); ++r) {
        nonempty += paths[r].size() > 0;
        wrapped += paths[r].size() > 0 && (int)(int16_t)paths[r].getOffset() != paths[r].getOffset();
    }
    long sum_plain = -1, sum_x = -1;
    if (modes & 1) {
        vec<Bool> bad;
        MarkBads(hb, bases, quals, paths, bad);
        sum_plain = Sum(bad);
        BinaryWriter::writeFile(argv[5], bad);
    }
    if (modes & 2) {
        ReadPathVecX px;
        px.append(paths, hb);
        vec<Bool> bad;
        MarkBads(hb, bases, quals, px, bad);
        sum_x = Sum(bad);
        BinaryWriter::writeFile(argv[6], bad);
    }
    std::cout << "BADS_DRIVER K " << hb.K() << " threads " << omp_get_max_threads() << " reads " << n << " E " << hb.E() << " nonempty " << nonempty << " offsets_wrapped "
              << wrapped << " sum_bad_plain " << sum_plain << " sum_bad_x " << sum_x << std::endl;
    return 0;
}
