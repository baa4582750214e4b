// a48x_driver.cc -- TEST INFRASTRUCTURE ONLY (run by make_a48x_golden.py, never part of the product or of build()).
//
// Calls the reference's own code on the output directory of an `snref_driver ... dump` run, so that the fixtures under
// tests/golden/a48x/ hold bytes the reference wrote:
//   a.hbx      BinaryWriter::writeFile(HyperBasevectorX(hbv)) of the directory's a.hbv (10X/DF.cc:573-576)
//   a.pathsX   ReadPathVecX::WriteAll of the compressed form of the directory's tmp.paths, made by InitializePathsXFromPaths
//              (10X/DfTools.cc:24-69, as 10X/DF.cc:579 calls it) or, with mode "append", by the sequential
//              ReadPathVecX::append(paths, hb) (10X/paths/ReadPathVecX.cc:378)
// Compiled against the reference's headers with the flags of oracle/ref/build_ref.sh and linked with the objects that recipe builds.
// The number of OpenMP threads comes from OMP_NUM_THREADS.
//
// usage: a48x_driver <dump directory> [init|append]
#include <omp.h>

#include <iostream>
#include <string>

#include "10X/DfTools.h"
#include "10X/paths/ReadPathVecX.h"
#include "feudal/BinaryStream.h"
#include "paths/HyperBasevector.h"
#include "paths/long/ReadPath.h"
#include "system/RunTime.h"

int main(int argc, char** argv) {
    RunTime();
    if (argc < 2) { std::cerr << "usage: a48x_driver <dump directory> [init|append]" << std::endl; return 2; }
    const String dir(argv[1]);
    const std::string mode = argc > 2 ? argv[2] : "init";
    HyperBasevector hbv;
    BinaryReader::readFile(dir + "/a.hbv", &hbv);
    HyperBasevectorX hb(hbv);
    BinaryWriter::writeFile(dir + "/a.hbx", hb);
    ReadPathVecX pathsX;
    if (mode == "init") {
        InitializePathsXFromPaths(pathsX, hb, dir + "/tmp.paths", 100000000, False);
    } else {
        ReadPathVec paths(dir + "/tmp.paths");
        pathsX.append(paths, hb);
    }
    pathsX.WriteAll(std::string(argv[1]) + "/a.pathsX");
    std::cout << "A48X_DRIVER mode " << (mode == "init" ? "InitializePathsXFromPaths" : "append") << " threads " << omp_get_max_threads() << " reads "
              << pathsX.size() << " edges " << hb.E() << " bytes " << pathsX.storageSize() << std::endl;
    return 0;
}
