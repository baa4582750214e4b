// a48_driver.cc -- TEST INFRASTRUCTURE ONLY (run by make_a48_golden.py, never part of the product or of build()).
//
// Calls the reference's own writers on the output directory of an `snref_driver ... dump` run, so that the fixtures under
// tests/golden/a48/ hold bytes the reference's code wrote:
//   a.paths.inv, a.countsb   writePathsIndex (10X/PathsIndex.cc:23-145) over the directory's tmp.paths and a.inv, as 10X/DF.cc:588 calls it
//   a.dup                    BinaryWriter::writeFile(vec<Bool>) (10X/DF.cc:599-600) of the flags MarkDups left in markdups.txt
// Compiled against the reference's headers with the flags of oracle/ref/build_ref.sh and linked with the objects that recipe builds.
//
// usage: a48_driver <dump directory> [chunks]
#include <chrono>
#include <fstream>
#include <iostream>
#include <string>

#include "10X/PathsIndex.h"
#include "Vec.h"
#include "feudal/BinaryStream.h"
#include "paths/long/ReadPath.h"
#include "system/RunTime.h"

int main(int argc, char** argv) {
    RunTime();
    if (argc < 2) { std::cerr << "usage: a48_driver <dump directory> [chunks]" << std::endl; return 2; }
    const String dir(argv[1]);
    const int chunks = argc > 2 ? atoi(argv[2]) : 15;
    ReadPathVec paths(dir + "/tmp.paths");
    vec<int> inv;
    BinaryReader::readFile(dir + "/a.inv", &inv);
    const auto t0 = std::chrono::steady_clock::now();
    writePathsIndex(paths, inv, dir, "a.paths.inv", "a.countsb", chunks, false);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::ifstream md(std::string(argv[1]) + "/markdups.txt");
    std::string head, bits;
    if (std::getline(md, head) && std::getline(md, bits)) {
        vec<Bool> dup(bits.size());
        for (size_t i = 0; i < bits.size(); ++i) dup[i] = bits[i] == '1';
        BinaryWriter::writeFile(dir + "/a.dup", dup);
    }
    std::cout << "A48_DRIVER reads " << paths.size() << " edges " << inv.size() << " writePathsIndex_ms " << ms << std::endl;
    return 0;
}
