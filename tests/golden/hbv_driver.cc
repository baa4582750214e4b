// hbv_driver.cc -- TEST INFRASTRUCTURE ONLY (run by make_hbv_golden.py, never part of the product or of build()).
//
// Calls the reference's own graph-from-unitigs step on a hand-made unitig set (tests/handunitigs.py), so that the fixtures under
// tests/golden/hbv/ hold what the reference's code made of it:
//   buildHBVFromEdges (paths/long/HBVFromEdges.cc:244-296) over the unitigs IN THE ORDER OF THE INPUT FILE (the generator shuffles them:
//   the reference ranks them itself, :272-277), then
//     fwd.i32, rev.i32        the two translation tables, per unitig of the input file
//     to_left.i32, to_right.i32, lens.u32   per HBV edge: its vertices (hbv.ToLeft / ToRight) and the length of its edge object
//     a.hbv, a.inv            BinaryWriter::writeFile of the graph and of hbv.Involution, as DF writes them (10X/runstages/RunStages.cc:418)
//     edges.bv                BinaryWriter::writeFile of the unitigs as a vec<basevector> sorted by BVComp (HBVFromEdges.cc:106-111): the a13
//                             hand-off file in the form its reader takes (BuildReadQGraph48.cc:1640-1642), written by the reference's writer
// Input file (little endian): "SNKUT001", u32 K, u32 0, u64 U, u64 off[U + 1], u8 base codes [off[U]].
// Compiled against the reference's headers with the flags of oracle/ref/build_ref.sh and linked with the objects that recipe builds.
//
// usage: hbv_driver <input file> <output directory> <threads>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <iostream>
#include <string>
#include <vector>

#include "Basevector.h"
#include "ParallelVecUtilities.h"
#include "Vec.h"
#include "feudal/BinaryStream.h"
#include "paths/HyperBasevector.h"
#include "paths/long/HBVFromEdges.h"
#include "system/RunTime.h"

template <typename T>
static bool write_raw(const std::string& fn, const T* p, size_t n) {
    FILE* f = fopen(fn.c_str(), "wb");
    if (!f) return false;
    const bool ok = n == 0 || fwrite(p, sizeof(T), n, f) == n;
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    RunTime();
    if (argc < 4) { std::cerr << "usage: hbv_driver <input file> <output directory> <threads>" << std::endl; return 2; }
    const std::string out(argv[2]);
    unsigned threads = atoi(argv[3]);
    SetThreads(threads, False);
    FILE* f = fopen(argv[1], "rb");
    char magic[8];
    uint32_t K = 0, zero = 0;
    uint64_t U = 0;
    if (!f || fread(magic, 1, 8, f) != 8 || memcmp(magic, "SNKUT001", 8) || fread(&K, 4, 1, f) != 1 || fread(&zero, 4, 1, f) != 1 || fread(&U, 8, 1, f) != 1) {
        std::cerr << "hbv_driver: cannot read " << argv[1] << std::endl;
        return 2;
    }
    std::vector<uint64_t> off(U + 1);
    if (fread(off.data(), 8, U + 1, f) != U + 1) { std::cerr << "hbv_driver: short input" << std::endl; return 2; }
    std::vector<uint8_t> codes(off[U]);
    if (!codes.empty() && fread(codes.data(), 1, codes.size(), f) != codes.size()) { std::cerr << "hbv_driver: short input" << std::endl; return 2; }
    fclose(f);
    vecbvec edges;
    edges.reserve(U);
    for (uint64_t u = 0; u < U; ++u) {
        bvec b((unsigned)(off[u + 1] - off[u]));
        for (uint64_t j = off[u]; j < off[u + 1]; ++j) b.Set((unsigned)(j - off[u]), codes[j]);
        edges.push_back(b);
    }
    HyperBasevector hbv;
    vec<int> fwd, rev;
    buildHBVFromEdges(edges, K, &hbv, &fwd, &rev);
    vec<int> to_left, to_right, inv;
    hbv.ToLeft(to_left);
    hbv.ToRight(to_right);
    hbv.Involution(inv);
    const int E = hbv.EdgeObjectCount();
    std::vector<uint32_t> lens(E);
    for (int e = 0; e < E; ++e) lens[e] = hbv.EdgeObject(e).size();
    vec<basevector> sorted;
    sorted.reserve(U);
    for (uint64_t u = 0; u < U; ++u) sorted.push_back(edges[u]);
    std::sort(sorted.begin(), sorted.end(), [](basevector const& x, basevector const& y) {          // BVComp
        if (x.size() != y.size()) return x.size() > y.size();
        return x < y;
    });
    bool ok = write_raw(out + "/fwd.i32", &fwd[0], fwd.size()) && write_raw(out + "/rev.i32", &rev[0], rev.size()) &&
              write_raw(out + "/to_left.i32", &to_left[0], to_left.size()) && write_raw(out + "/to_right.i32", &to_right[0], to_right.size()) &&
              write_raw(out + "/lens.u32", lens.data(), lens.size());
    if (!ok) { std::cerr << "hbv_driver: cannot write to " << out << std::endl; return 2; }
    BinaryWriter::writeFile(String(out.c_str()) + "/a.hbv", hbv);
    BinaryWriter::writeFile(String(out.c_str()) + "/a.inv", inv);
    BinaryWriter::writeFile(String(out.c_str()) + "/edges.bv", sorted);
    std::cout << "HBV_DRIVER threads " << threads << " K " << K << " U " << U << " E " << E << " N " << hbv.N() << std::endl;
    return 0;
}
