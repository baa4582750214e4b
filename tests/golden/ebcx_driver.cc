// ebcx_driver.cc -- TEST INFRASTRUCTURE ONLY (run by make_ebcx_golden.py, never part of the product or of build()).
//
// Calls the reference's own code on the output directory of an `snref_driver ... dump` run, so that the fixtures under
// tests/golden/ebcx/ hold bytes the reference wrote:
//   a.ebcx     VecIntVec::WriteAll of the edge -> barcode map that computeEdgeToBarcodeX (10X/PathsIndex.cc:297-358, called from StageEBC,
//              10X/runstages/RunStages.cc:31-38) makes of the directory's a.hbv, a.inv and tmp.paths (compressed by the sequential
//              ReadPathVecX::append(paths, hb), 10X/paths/ReadPathVecX.cc:378, as a48x_driver.cc does) and of two raw files the
//              generator wrote beside them: bc.i32 (int32 per read) and bci.i64 (int64 per run of reads + 1)
// Compiled against the reference's headers with the flags of oracle/ref/build_ref.sh and linked with the objects that recipe builds.
// The number of OpenMP threads comes from OMP_NUM_THREADS.
//
// usage: ebcx_driver <dump directory>
#include <omp.h>
#include <stdint.h>
#include <stdio.h>

#include <chrono>
#include <iostream>
#include <string>

#include "10X/PathsIndex.h"
#include "10X/paths/ReadPathVecX.h"
#include "Intvector.h"
#include "Vec.h"
#include "feudal/BinaryStream.h"
#include "paths/HyperBasevector.h"
#include "paths/long/ReadPath.h"
#include "system/RunTime.h"

template <typename T>
static bool read_raw(const std::string& fn, vec<T>& out) {
    FILE* f = fopen(fn.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(bytes / sizeof(T));
    const bool ok = bytes % sizeof(T) == 0 && (bytes == 0 || fread(&out[0], 1, bytes, f) == (size_t)bytes);
    fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    RunTime();
    if (argc < 2) { std::cerr << "usage: ebcx_driver <dump directory>" << std::endl; return 2; }
    const String dir(argv[1]);
    const std::string sdir(argv[1]);
    HyperBasevector hbv;
    BinaryReader::readFile(dir + "/a.hbv", &hbv);
    HyperBasevectorX hb(hbv);
    vec<int> inv;
    BinaryReader::readFile(dir + "/a.inv", &inv);
    ReadPathVecX pathsX;
    {
        ReadPathVec paths(dir + "/tmp.paths");
        pathsX.append(paths, hb);
    }
    vec<int32_t> bc;
    vec<int64_t> bci;
    if (!read_raw(sdir + "/bc.i32", bc) || !read_raw(sdir + "/bci.i64", bci)) { std::cerr << "ebcx_driver: cannot read bc.i32 / bci.i64" << std::endl; return 2; }
    if (bc.size() != (size_t)pathsX.size() || bci.empty() || bci.front() != 0 || bci.back() != (int64_t)bc.size()) {
        std::cerr << "ebcx_driver: bc / bci do not fit the " << pathsX.size() << " reads" << std::endl;
        return 2;
    }
    VecIntVec ebcx;
    const auto t0 = std::chrono::steady_clock::now();
    computeEdgeToBarcodeX(pathsX, hb, bc, inv, bci, ebcx, false);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ebcx.WriteAll(dir + "/a.ebcx");
    uint64_t n_ebc = 0, max_list = 0;
    for (size_t e = 0; e < ebcx.size(); ++e) {
        n_ebc += ebcx[e].size();
        if (ebcx[e].size() > max_list) max_list = ebcx[e].size();
    }
    std::cout << "EBCX_DRIVER threads " << omp_get_max_threads() << " reads " << pathsX.size() << " runs " << bci.size() - 1 << " edges " << hb.E() << " n_ebc " << n_ebc
              << " max_list " << max_list << " computeEdgeToBarcodeX " << ms << " ms" << std::endl;
    return 0;
}
