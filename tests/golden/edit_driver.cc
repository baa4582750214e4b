// edit_driver.cc -- TEST INFRASTRUCTURE ONLY: runs the reference's own graph edit -- hbv.DeleteEdgesParallel(dels) and Cleanup
// (paths/long/large/GapToyTools.cc:1287-1302), the pair every simplification step after DF is made of -- for
// tests/golden/make_edit_golden.py.
//
//   edit_driver a.hbv a.inv in.paths dels.bin THREADS out_dir
//
// a.hbv / a.inv are the graph as DF writes it, in.paths a feudal MasterVec<ReadPath> on it (what snk_write_paths wrote), dels.bin one or
// more lists of edge ids (little endian: "SNKDEL01", u64 n_lists, per list u64 n + n x i32).  The lists are applied one after the
// other: list i + 1 is given in the edge ids that the edit with list i left.  After every edit the driver writes to out_dir
//     a.hbv.<i>, a.inv.<i>   the graph and the involution (BinaryWriter::writeFile)
//     a.paths.<i>            the paths (ReadPathVec::WriteAll)
//     a.pathsX.<i>           the same paths zipped on the graph (ReadPathVecX::WriteAll)
// Built by the maker in a scratch directory against the reference's headers and objects; nothing compiled from it is kept.
#include <omp.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <string>
#include <vector>

#include "10X/paths/ReadPathVecX.h"
#include "Basevector.h"
#include "ParallelVecUtilities.h"
#include "feudal/BinaryStream.h"
#include "paths/HyperBasevector.h"
#include "paths/long/ReadPath.h"
#include "paths/long/large/GapToyTools.h"
#include "system/RunTime.h"

int main(int argc, char** argv) {
    RunTime();
    if (argc != 7) { std::cerr << "usage: edit_driver a.hbv a.inv in.paths dels.bin THREADS out_dir" << std::endl; return 2; }
    unsigned threads = atoi(argv[5]);
    SetThreads(threads, False);
    omp_set_num_threads(threads);
    const std::string out(argv[6]);
    HyperBasevector hbv;
    BinaryReader::readFile(argv[1], &hbv);
    vec<int> inv;
    BinaryReader::readFile(argv[2], &inv);
    ReadPathVec paths(argv[3]);
    FILE* f = fopen(argv[4], "rb");
    char magic[8];
    uint64_t n_lists = 0;
    if (!f || fread(magic, 1, 8, f) != 8 || memcmp(magic, "SNKDEL01", 8) || fread(&n_lists, 8, 1, f) != 1) { std::cerr << "edit_driver: cannot read " << argv[4] << std::endl; return 2; }
    const int E0 = hbv.EdgeObjectCount(), N0 = hbv.N();
    std::cout << "EDIT_DRIVER K " << hbv.K() << " threads " << threads << " reads " << paths.size() << " E " << E0 << " N " << N0;
    for (uint64_t i = 0; i < n_lists; ++i) {
        uint64_t n = 0;
        if (fread(&n, 8, 1, f) != 1) { std::cerr << "edit_driver: short input" << std::endl; return 2; }
        std::vector<int32_t> ids(n);
        if (n && fread(ids.data(), 4, n, f) != n) { std::cerr << "edit_driver: short input" << std::endl; return 2; }
        vec<int> dels;
        for (uint64_t j = 0; j < n; ++j) dels.push_back(ids[j]);
        hbv.DeleteEdgesParallel(dels);
        Cleanup(hbv, inv, paths);
        const String tag = String(out.c_str()) + "/";
        const String no = ToString((int)i);
        BinaryWriter::writeFile(tag + "a.hbv." + no, hbv);
        BinaryWriter::writeFile(tag + "a.inv." + no, inv);
        paths.WriteAll(tag + "a.paths." + no);
        HyperBasevectorX hbx(hbv);
        ReadPathVecX px;
        px.append(paths, hbx);
        px.WriteAll(out + "/a.pathsX." + std::string(no.c_str()));
        size_t placed = 0;
        for (size_t r = 0; r < paths.size(); ++r) placed += paths[r].size() > 0;
        std::cout << " | dels " << n << " -> E " << hbv.EdgeObjectCount() << " N " << hbv.N() << " placed " << placed;
    }
    fclose(f);
    std::cout << std::endl;
    return 0;
}
