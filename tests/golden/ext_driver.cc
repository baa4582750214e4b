// ext_driver.cc -- TEST INFRASTRUCTURE ONLY: runs the reference's own ExtendPathsNew (10X/Extend.cc:14-177) for tests/golden/make_ext_golden.py.
//
//   ext_driver in.snkrd a.hbv a.inv in.paths BACK_EXTEND out.pathsX
//
// in.snkrd is the read file of oracle/ref/ref_driver.cc (tests/refio.py), a.hbv / a.inv the graph as DF writes it, in.paths a feudal
// MasterVec<ReadPath> (tmp.paths of a dump, or what snk_write_paths wrote).  The paths are zipped into a ReadPathVecX on the graph, the
// function is called, and the ReadPathVecX it leaves is written with WriteAll.  The thread count comes from OMP_NUM_THREADS.
// Built by the maker in a scratch directory against the reference's headers and objects; nothing compiled from it is kept.
#include <omp.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "10X/Extend.h"
#include "10X/paths/ReadPathVecX.h"
#include "feudal/BinaryStream.h"
#include "feudal/PQVec.h"
#include "paths/HyperBasevector.h"
#include "paths/long/ReadPath.h"
#include "system/RunTime.h"

int main(int argc, char** argv) {
    RunTime();
    if (argc != 7) {
        std::cerr << "usage: ext_driver in.snkrd a.hbv a.inv in.paths BACK_EXTEND out.pathsX" << std::endl;
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
    vec<int> inv;
    BinaryReader::readFile(argv[3], &inv);
    HyperBasevectorX hb(hbv);
    ReadPathVec paths(argv[4]);
    if (paths.size() != n) { std::cerr << paths.size() << " paths for " << n << " reads" << std::endl; return 2; }
    ReadPathVecX px;
    px.append(paths, hb);
    const bool back = atoi(argv[5]) != 0;
    ExtendPathsNew(hb, inv, bases, quals, px, back);
    // ---- what changed, for the fixture's summary line
    ReadPathVec after;
    px.unzip(after, hb);
    size_t nonempty = 0, changed = 0, longer = 0, shorter = 0, offch = 0, e0 = 0, e1 = 0, maxlen = 0;
    for (size_t r = 0; r < paths.size(); ++r) {
        ReadPath const& a = paths[r];
        ReadPath const& c = after[r];
        nonempty += a.size() > 0;
        e0 += a.size();
        e1 += c.size();
        maxlen = std::max(maxlen, (size_t)c.size());
        bool same = a.size() == c.size() && a.getOffset() == c.getOffset();
        for (size_t j = 0; same && j < a.size(); ++j) same = a[j] == c[j];
        changed += !same;
        longer += c.size() > a.size();
        shorter += c.size() < a.size();
        offch += a.size() && a.getOffset() != c.getOffset();
    }
    std::cout << "EXT_DRIVER K " << hb.K() << " back " << back << " threads " << omp_get_max_threads() << " reads " << paths.size() << " E " << hb.E() << " nonempty " << nonempty
              << " changed " << changed << " longer " << longer << " shorter " << shorter << " offset_changed " << offch << " edges " << e0 << " -> " << e1 << " maxlen " << maxlen
              << std::endl;
    px.WriteAll(std::string(argv[6]));
    return 0;
}
