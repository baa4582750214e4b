// hops_driver.cc -- TEST INFRASTRUCTURE ONLY: runs the reference's own FindEdgePairs (10X/Closomatic.cc:17-354) for
// tests/golden/make_hops_golden.py.
//
//   hops_driver a.hbx a.inv a.pathsX a.paths.inv in.bc in.bad ONE_GOOD out.hops
//
// a.hbx, a.inv, a.pathsX and a.paths.inv are the files of a.48/ as this library's writers make them (byte-equal to the reference's);
// in.bc is a BINWRITE vec<int> with one barcode per read, in.bad a BINWRITE vec<Bool> with one flag per pair (the container of a.bad).
// The function gets ONE dataset, BAR_10X from read 0, so a read's barcode class is bidc's first two branches (10X/DfTools.cc:110-122).
// The result is written with BinaryWriter::writeFile(vec<pair<int,int>>), the way DF writes a.hops (10X/DF.cc:642-643).  The thread count
// comes from OMP_NUM_THREADS.
// Built by the maker in a scratch directory against the reference's headers and objects; nothing compiled from it is kept.
#include <omp.h>

#include <cstdlib>
#include <iostream>
#include <string>

#include "10X/Closomatic.h"
#include "10X/DfTools.h"
#include "10X/paths/ReadPathVecX.h"
#include "feudal/BinaryStream.h"
#include "paths/HyperBasevector.h"
#include "system/RunTime.h"

int main(int argc, char** argv) {
    RunTime();
    if (argc != 9) {
        std::cerr << "usage: hops_driver a.hbx a.inv a.pathsX a.paths.inv in.bc in.bad ONE_GOOD out.hops" << std::endl;
        return 2;
    }
    HyperBasevectorX hb;
    BinaryReader::readFile(argv[1], &hb);
    vec<int> inv;
    BinaryReader::readFile(argv[2], &inv);
    ReadPathVecX pathsX;
    pathsX.ReadAll(argv[3]);
    vec<int32_t> bc;
    BinaryReader::readFile(argv[5], &bc);
    vec<Bool> bad;
    BinaryReader::readFile(argv[6], &bad);
    if (bc.size() != (size_t)pathsX.size() || bad.size() * 2 != bc.size()) {
        std::cerr << pathsX.size() << " paths, " << bc.size() << " barcodes, " << bad.size() << " pair flags" << std::endl;
        return 2;
    }
    vec<DataSet> datasets(1);
    datasets[0].dt = ReadDataType::BAR_10X;
    datasets[0].start = 0;
    vec<std::pair<int, int>> pairs;
    const double t0 = WallClockTime();
    FindEdgePairs(hb, inv, pathsX, argv[4], bad, pairs, datasets, bc, atoi(argv[7]) != 0);
    const double secs = WallClockTime() - t0;
    BinaryWriter::writeFile(argv[8], pairs);
    std::cout << "HOPS_DRIVER K " << hb.K() << " threads " << omp_get_max_threads() << " reads " << bc.size() << " E " << hb.E() << " one_good " << atoi(argv[7]) << " pairs "
              << pairs.size() << " seconds " << secs << std::endl;
    return 0;
}
