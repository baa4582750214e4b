#!/usr/bin/env python3
"""Generate tests/golden/hbv/<case>_k<K>.npz: what the REFERENCE's own graph-from-unitigs step makes of the hand-made unitig sets of
tests/handunitigs.py.

Run by hand where the reference's sources can be read (like make_a48_golden.py; needs oracle/libsnkoracle.so).  hbv_driver.cc (next to this
file) reads a unitig set in SHUFFLED order, calls buildHBVFromEdges (paths/long/HBVFromEdges.cc:244-296) and writes the translation tables,
the vertices and lengths of the edges, a.hbv and a.inv (BinaryWriter::writeFile of the graph and of hbv.Involution) and edges.bv
(BinaryWriter::writeFile of the BVComp-sorted vec<basevector>: the a13 hand-off file, by the reference's writer).  It is built like the
other drivers: in a scratch directory, a COPY of oracle/ref/ run with the recipe's own hooks, then compiled with the recipe's flags and
linked against its libref.a with --gc-sections.  Nothing compiled is kept in the repository.
Every case runs with 1 and with 8 threads; both must give the same bytes.  Before a case is saved, the oracle (sno_hbv_build, sno_write_bv)
must give the reference's graph and file: the GPU tests take their expected values for the cases that are NOT saved from it.

Cases (tests/handunitigs.py; each for K = 48 and K = 60, each asserted to be a unitig set: no k-mer twice, at most 8 ends per (K-1)-mer):
  single_k, single_k1, single_pal_k, single_pal_2k   one unitig: K bases (its two ends overlap by K - 2), K + 1 bases, a palindromic k-mer, a
                                                     palindrome of 2K bases
  circle                       one unitig whose first and last (K-1)-mers are equal
  ring_2, ring_3               a circular string cut into pieces
  hairpin, hairpin_flanks      v + i + rc(v): both strands of one unitig in one component, which is its own mirror image
  bubble                       two unitigs of one length between the same two junctions (parallel edges), a flank on either side
  full_vertex                  four unitigs into one junction and four out of it: 8 ends, the reference's limit
  palindromes                  four palindromic unitigs: rank 0, the last rank, one isolated, one on a junction that ordinary unitigs share;
                               an ordinary unitig that begins with a palindromic k-mer
  chain_2, _4, _5, _1023, _1024, _1025   one component of N nodes per strand: both sides of hbv_big = 4 and = 1024
  forest_255, _256, _257       unitigs of one length whose first k-mers differ only at base 0 (isolated) or only at base K - 1 (these share
                               their first (K-1)-mer: components of four), a few of length +-1, three palindromes
  long                         one unitig of 70 000 bases, every length from K to K + 16
  mixed_seed1 .. 4             a random multigraph of about 180 unitigs: one large component among small ones
Saved (handunitigs.SAVED): every case up to chain_5, chain_1025, forest_257, long, mixed_seed1.  For the others the run is the proof that
oracle and reference agree; one line per case and K either way.  A fixture holds K, the unitigs (lengths and 2-bit codes, BVComp order),
the order they were given to the reference in, fwd / rev (per BVComp rank), to_left / to_right / edge_lens (per HBV edge), n_vertices,
a.hbv, a.inv, edges.bv and ref_summary (the driver's line).

usage: python tests/golden/make_hbv_golden.py [--work DIR] [case ...]
"""
from __future__ import annotations

import shutil
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import handunitigs as hu  # noqa: E402
import make_a48_golden  # noqa: E402

GOLD = Path(__file__).resolve().parent
OPT = make_a48_golden.OPT
FILES = ("fwd.i32", "rev.i32", "to_left.i32", "to_right.i32", "lens.u32", "a.hbv", "a.inv", "edges.bv")


def build_driver(work: Path) -> Path:
    """The reference objects are built once (make_a48_golden.build_driver) and shared with the other drivers."""
    import os
    make_a48_golden.build_driver(work)
    refwork = work / "refwork"
    exe = work / "hbv_driver"
    src = GOLD / "hbv_driver.cc"
    if not exe.exists() or exe.stat().st_mtime < src.stat().st_mtime:
        cxx = os.environ.get("CXX", "g++")
        flags = ["-std=c++11", "-fpermissive", "-fopenmp", "-fno-strict-aliasing", "-w", OPT, "-DNDEBUG", "-ffunction-sections", "-fdata-sections",
                 f"-I{refwork / 'overlay'}"]
        obj = work / "hbv_driver.o"
        subprocess.run([cxx, *flags, "-c", str(src), "-o", str(obj)], check=True)
        subprocess.run([cxx, "-fopenmp", "-Wl,--gc-sections", "-o", str(exe), str(obj), str(refwork / "obj" / "LinkTimestamp.o"), str(refwork / "libref.a"),
                        "-lz", "-lpthread"], check=True)
    return exe


def run_driver(exe: Path, c, perm, td: Path) -> tuple[dict, str]:
    off, bases = hu.reordered(c, perm)
    with open(td / "in.unitigs", "wb") as f:
        f.write(b"SNKUT001" + struct.pack("<IIQ", c.K, 0, len(perm)) + off.astype("<u8").tobytes() + bases.tobytes())
    got = {}
    for threads in (1, 8):
        out = td / f"out{threads}"
        out.mkdir()
        r = subprocess.run([str(exe), str(td / "in.unitigs"), str(out), str(threads)], check=True, capture_output=True, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("HBV_DRIVER")][-1]
        got[threads] = ({f: (out / f).read_bytes() for f in FILES}, line)
    for f in FILES:
        assert got[1][0][f] == got[8][0][f], f"{c.name} K={c.K}: {f} differs between 1 and 8 threads"
    return got[1][0], got[1][1] + " | same bytes with 8 threads"


def one_case(exe: Path, name: str, K: int, work: Path) -> None:
    c = hu.case(name, K)
    hu.check_facts(c)
    perm = hu.orders(c)["shuffled"]
    with tempfile.TemporaryDirectory(dir=work) as td:
        td = Path(td)
        files, line = run_driver(exe, c, perm, td)
        i32 = lambda f: np.frombuffer(files[f], "<i4")
        fwd, rev = np.zeros(len(perm), np.int32), np.zeros(len(perm), np.int32)
        fwd[perm], rev[perm] = i32("fwd.i32"), i32("rev.i32")              # the input's unitig i is rank perm[i]
        n_vertices = int(line.split(" N ")[1].split()[0])
        ref = hu.graph_from_xlat(c, fwd, rev, i32("to_left.i32"), i32("to_right.i32"), n_vertices)
        edge_lens = np.frombuffer(files["lens.u32"], "<u4")
        assert np.array_equal(edge_lens, np.diff(c.off.astype(np.int64))[ref["src"]])
        diff = hu.same_graph(hu.oracle_hbv(c), ref)
        assert diff is None, f"{name} K={K}: sno_hbv_build differs from the reference in {diff}"
        assert hu.oracle_bv(c, td / "oracle.bv") == files["edges.bv"], f"{name} K={K}: sno_write_bv differs from the reference's edges.bv"
    f = c.facts
    assert (f["n_edges"], f["n_vertices"]) == (ref["n_edges"], ref["n_vertices"])
    fact_line = (f"{name} K={K}: U {f['U']} E {ref['n_edges']} N {ref['n_vertices']} components {len(f['components'])} (largest {max(f['components'])}) "
                 f"palindromes {f['palindromes']} largest vertex {f['max_ends']} self-loops {f['self_loops']} parallel pairs {f['parallel_pairs']}")
    if name not in hu.SAVED:
        print(fact_line + " | oracle == reference, 1 and 8 threads; not saved")
        return
    out = hu.golden_path(name, K)
    tmp = out.with_suffix(".tmp.npz")
    u8 = lambda f: np.frombuffer(files[f], np.uint8)
    np.savez_compressed(tmp, K=np.int32(K), order=perm.astype(np.int32), unitig_lens=np.diff(c.off.astype(np.int64)).astype(np.uint32), unitig_codes2=hu.pack2(c.bases),
                        fwd=fwd, rev=rev, to_left=ref["v_left"], to_right=ref["v_right"], edge_lens=edge_lens, n_vertices=np.int32(n_vertices),
                        a_hbv=u8("a.hbv"), a_inv=u8("a.inv"), edges_bv=u8("edges.bv"), ref_summary=np.frombuffer(line.encode(), dtype=np.uint8))
    limit = max(p.stat().st_size for p in (GOLD / "a48").glob("*.npz"))
    if tmp.stat().st_size > limit:
        size = tmp.stat().st_size
        tmp.unlink()
        raise AssertionError(f"{name} K={K}: {size} B, larger than the largest fixture under tests/golden/a48/ ({limit} B)")
    tmp.replace(out)
    print(fact_line + f" | oracle == reference, 1 and 8 threads -> {out.name} ({out.stat().st_size / 1024:.0f} KiB)")


def main(argv: list[str]) -> None:
    work, names = None, []
    it = iter(argv)
    for a in it:
        if a == "--work":
            work = Path(next(it)).resolve()
        else:
            names.append(a)
    keep = work is not None
    work = work or Path(tempfile.mkdtemp(prefix="snk_hbv."))
    work.mkdir(parents=True, exist_ok=True)
    try:
        exe = build_driver(work)
        (GOLD / "hbv").mkdir(exist_ok=True)
        for name in names or list(hu.CASES):
            for K in hu.KS:
                one_case(exe, name, K, work)
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:])
