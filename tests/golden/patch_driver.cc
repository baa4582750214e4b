// patch_driver.cc -- TEST INFRASTRUCTURE ONLY: runs the reference's own StageInsertPatch steps (10X/runstages/RunStages.cc:176-230) for
// tests/golden/make_patch_golden.py.
//
//   patch_driver a.hbv in.paths closures.bin THREADS out_dir
//
// a.hbv is the graph as DF writes it, in.paths a feudal MasterVec<ReadPath> on it (what snk_write_paths wrote), closures.bin the closure
// sequences (little endian: "SNKCL001", u64 n, u64 off[n + 1], u8 base codes [off[n]]).  The driver calls, in the order of
// StageInsertPatch, BuildAll (paths/long/large/GapToyTools4.cc:187-214), buildBigKHBVFromReads_sleek (kmers/BigKPather.cc, coverage 4),
// the to3 / left3 loop (RunStages.cc:207-214) and TranslatePaths (GapToyTools4.cc:220-266, on in.paths).
//
// The reference appends its new edges under a lock (BigKPather.cc:408-416), so its edge numbering depends on thread timing.  To leave
// something two runs agree on, the driver then takes the new graph's unitigs (of every edge and its reverse complement the one that
// getCanonicalForm calls FWD; a palindrome once), sorts them by BVComp (HBVFromEdges.cc:106-111), runs the reference's buildHBVFromEdges
// once more on them and renumbers to3 and the translated paths BY EDGE SEQUENCE.  The sequences of the two graphs must map one to one.
// Written to out_dir:
//     a.hbv, a.inv            the renumbered graph and its involution (BinaryWriter::writeFile)
//     to3_off.u64, to3.i32    per old edge its list of new edge ids; left3.i32
//     reads.i32               per read (edge or -1, offset) of the translated path, as ReadPathVecX::unzip returns it
//     a.pathsX                the translated paths zipped on the renumbered graph (ReadPathVecX::WriteAll)
// Built by the maker in a scratch directory against the reference's headers and objects; nothing compiled from it is kept.
#include <omp.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "10X/paths/ReadPathVecX.h"
#include "Basevector.h"
#include "ParallelVecUtilities.h"
#include "feudal/BinaryStream.h"
#include "kmers/BigKPather.h"
#include "paths/HyperBasevector.h"
#include "paths/long/HBVFromEdges.h"
#include "paths/long/ReadPath.h"
#include "paths/long/large/GapToyTools.h"
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
    if (argc != 6) { std::cerr << "usage: patch_driver a.hbv in.paths closures.bin THREADS out_dir" << std::endl; return 2; }
    unsigned threads = atoi(argv[4]);
    SetThreads(threads, False);
    omp_set_num_threads(threads);
    const std::string out(argv[5]);
    HyperBasevector hbv;
    BinaryReader::readFile(argv[1], &hbv);
    const int K = hbv.K();
    // ---- the closures
    FILE* f = fopen(argv[3], "rb");
    char magic[8];
    uint64_t n = 0;
    if (!f || fread(magic, 1, 8, f) != 8 || memcmp(magic, "SNKCL001", 8) || fread(&n, 8, 1, f) != 1) { std::cerr << "patch_driver: cannot read " << argv[3] << std::endl; return 2; }
    std::vector<uint64_t> off(n + 1);
    if (fread(off.data(), 8, n + 1, f) != n + 1) { std::cerr << "patch_driver: short input" << std::endl; return 2; }
    std::vector<uint8_t> codes(off[n]);
    if (!codes.empty() && fread(codes.data(), 1, codes.size(), f) != codes.size()) { std::cerr << "patch_driver: short input" << std::endl; return 2; }
    fclose(f);
    vec<basevector> closures;
    for (uint64_t i = 0; i < n; ++i) {
        basevector b((unsigned)(off[i + 1] - off[i]));
        for (uint64_t j = off[i]; j < off[i + 1]; ++j) b.Set((unsigned)(j - off[i]), codes[j]);
        closures.push_back(b);
    }
    // ---- StageInsertPatch, RunStages.cc:181-226
    HyperBasevector hb3;
    vec<vec<int>> to3;
    vec<int> left3;
    size_t n_allx = 0;
    {
        ReadPathVec allx_paths;
        vecbasevector allx;
        BuildAll(allx, hbv, closures.size());
        allx.append(closures.begin(), closures.end());
        n_allx = allx.size();
        const int coverage = 4;
        buildBigKHBVFromReads_sleek(K, allx, coverage, &hb3, &allx_paths);
        to3.resize(hbv.E());
        left3.resize(hbv.E());
        for (int i = 0; i < hbv.E(); ++i) {
            for (auto const& p : allx_paths[i]) to3[i].push_back(p);
            left3[i] = allx_paths[i].getFirstSkip();
        }
    }
    HyperBasevectorX hbx3 = HyperBasevectorX(hb3);
    ReadPathVecX pathsX;
    TranslatePaths(pathsX, hbx3, to3, left3, String(argv[2]));
    ReadPathVec after;
    pathsX.unzip(after, hbx3);
    // ---- the graph two runs agree on: the unitigs in BVComp order through buildHBVFromEdges, everything renumbered by sequence
    const int E3 = hb3.EdgeObjectCount();
    vecbvec us;
    for (int e = 0; e < E3; ++e) {
        basevector const& x = hb3.EdgeObject(e);
        if (x.getCanonicalForm() == CanonicalForm::REV) continue;
        basevector b(x.size());                          // base by base into a fresh vector: the unused bits of its last byte are zero
        for (unsigned j = 0; j < x.size(); ++j) b.Set(j, x[j]);
        us.push_back(b);
    }
    std::sort(us.begin(), us.end(), [](basevector const& x, basevector const& y) {          // BVComp
        if (x.size() != y.size()) return x.size() > y.size();
        return x < y;
    });
    HyperBasevector hbc;
    vec<int> fwd, rev;
    buildHBVFromEdges(us, K, &hbc, &fwd, &rev);
    const int EC = hbc.EdgeObjectCount();
    if (EC != E3) { std::cerr << "patch_driver: " << E3 << " edges become " << EC << std::endl; return 3; }
    std::map<std::string, int> by_seq;
    for (int e = 0; e < EC; ++e)
        if (!by_seq.insert(std::make_pair(hbc.EdgeObject(e).ToString(), e)).second) { std::cerr << "patch_driver: two edges with one sequence" << std::endl; return 3; }
    std::vector<int> renum(E3, -1), hit(EC, 0);
    for (int e = 0; e < E3; ++e) {
        auto it = by_seq.find(hb3.EdgeObject(e).ToString());
        if (it == by_seq.end() || hit[it->second]++) { std::cerr << "patch_driver: the edge sequences do not map one to one" << std::endl; return 3; }
        renum[e] = it->second;
    }
    std::vector<uint64_t> to3_off(hbv.E() + 1, 0);
    std::vector<int32_t> to3_ids, l3(hbv.E());
    for (int i = 0; i < hbv.E(); ++i) {
        for (int x : to3[i]) to3_ids.push_back(renum[x]);
        to3_off[i + 1] = to3_ids.size();
        l3[i] = left3[i];
    }
    std::vector<int32_t> reads(2 * after.size());
    ReadPathVec renumbered(after.size());
    size_t placed = 0;
    for (size_t r = 0; r < after.size(); ++r) {
        ReadPath p = after[r];
        if (p.size() > 1) { std::cerr << "patch_driver: a translated path of " << p.size() << " edges" << std::endl; return 3; }
        reads[2 * r] = p.size() ? renum[p[0]] : -1;
        reads[2 * r + 1] = p.size() ? p.getOffset() : 0;
        if (p.size()) { p[0] = renum[p[0]]; ++placed; }
        renumbered[r] = p;
    }
    HyperBasevectorX hbxc(hbc);
    ReadPathVecX outX;
    outX.append(renumbered, hbxc);
    vec<int> inv;
    hbc.Involution(inv);
    bool ok = write_raw(out + "/to3_off.u64", to3_off.data(), to3_off.size()) && write_raw(out + "/to3.i32", to3_ids.data(), to3_ids.size()) &&
              write_raw(out + "/left3.i32", l3.data(), l3.size()) && write_raw(out + "/reads.i32", reads.data(), reads.size());
    if (!ok) { std::cerr << "patch_driver: cannot write to " << out << std::endl; return 2; }
    BinaryWriter::writeFile(String(out.c_str()) + "/a.hbv", hbc);
    BinaryWriter::writeFile(String(out.c_str()) + "/a.inv", inv);
    outX.WriteAll(out + "/a.pathsX");
    std::cout << "PATCH_DRIVER K " << K << " threads " << threads << " old E " << hbv.E() << " closures " << n << " allx " << n_allx << " new E " << EC << " N " << hbc.N()
              << " to3 entries " << to3_ids.size() << " reads " << after.size() << " placed " << placed << std::endl;
    return 0;
}
