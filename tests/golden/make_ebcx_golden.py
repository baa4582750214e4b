#!/usr/bin/env python3
"""Generate tests/golden/ebcx/<case>.npz: the bytes of a.ebcx as the REFERENCE's own code writes them.

Run by hand where the reference's sources can be read (like make_a48x_golden.py; needs oracle/_ref/snref_driver and libsnk.so).
ebcx_driver.cc (next to this file) reads a dump directory's a.hbv, a.inv and tmp.paths and the raw files bc.i32 and bci.i64 written here,
calls computeEdgeToBarcodeX (10X/PathsIndex.cc:297-358) as StageEBC does (10X/runstages/RunStages.cc:31-38) and writes the VecIntVec with
WriteAll.  It is built like the other two drivers: in a scratch directory, a COPY of oracle/ref/ run with the recipe's own hooks, then
compiled with the recipe's flags and linked against its libref.a with --gc-sections.  Nothing compiled is kept in the repository.
Every case runs with 1 and with 8 OpenMP threads; both must give the same bytes.  Before a case is saved, the restatement of
tests/ebcxref.py must give the reference's lists.

Cases:
  the five K=48 golden cases   the dumped tmp.paths reordered by a stable argsort of the case's raw bc (sparse ids; -1 = the adversarial
                               case's non-10x reads, 0 = no barcode), bci = the runs of equal bc
  ebcx_probe                   on the adversarial case's graph, hand-made paths, bc and bci (probe_runs): what the kernels' edges need
  ebcx_probe_ends_empty        the same without the two runs that visit edge 0 and edge E - 1: both stay empty
Each fixture holds tmp.paths, bc, bci, a.ebcx and ref_summary (the driver's line: sizes and the reference's own time on this host).

usage: python tests/golden/make_ebcx_golden.py [--work DIR] [case ...]
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import a48ref  # noqa: E402
import a48xref  # noqa: E402
import ebcxref  # noqa: E402
import make_a48_golden  # noqa: E402
import make_a48x_golden  # noqa: E402
import make_golden  # noqa: E402

GOLD = Path(__file__).resolve().parent
OPT = make_a48_golden.OPT


def build_driver(work: Path) -> Path:
    """The reference objects are built once (make_a48_golden.build_driver) and shared with the other drivers."""
    make_a48_golden.build_driver(work)
    refwork = work / "refwork"
    exe = work / "ebcx_driver"
    src = GOLD / "ebcx_driver.cc"
    if not exe.exists() or exe.stat().st_mtime < src.stat().st_mtime:
        cxx = os.environ.get("CXX", "g++")
        flags = ["-std=c++11", "-fpermissive", "-fopenmp", "-fno-strict-aliasing", "-w", OPT, "-DNDEBUG", "-ffunction-sections", "-fdata-sections",
                 f"-I{refwork / 'overlay'}"]
        obj = work / "ebcx_driver.o"
        subprocess.run([cxx, *flags, "-c", str(src), "-o", str(obj)], check=True)
        subprocess.run([cxx, "-fopenmp", "-Wl,--gc-sections", "-o", str(exe), str(obj), str(refwork / "obj" / "LinkTimestamp.o"), str(refwork / "libref.a"),
                        "-lz", "-lpthread"], check=True)
    return exe


def run_driver(exe: Path, out: Path) -> tuple[bytes, str]:
    got = {}
    for threads in (1, 8):
        r = subprocess.run([str(exe), str(out)], check=True, capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(threads)))
        line = [l for l in r.stdout.splitlines() if l.startswith("EBCX_DRIVER")][-1]
        got[threads] = ((out / "a.ebcx").read_bytes(), line)
    assert got[1][0] == got[8][0], "1 and 8 threads give different bytes: a finding for DESIGN.md"
    return got[1][0], got[1][1] + " | same bytes with 8 threads: " + got[8][1].split(" computeEdgeToBarcodeX ")[1]


def probe_runs(g: a48xref.Graph, inv: np.ndarray, ends: bool):
    """-> (runs, facts): runs = [(bc, [path, ...]), ...] in file order, a path = list of edge ids; an entry (None, []) is an empty run.
    Every property the case is for is asserted here or in check_probe."""
    E = g.E
    far = {0, int(inv[0]), E - 1, int(inv[E - 1])}                       # only the two runs of `ends` may touch these
    cyc = make_a48x_golden.find_cycle(g)
    assert not far & set(cyc) and not far & {int(inv[e]) for e in cyc}, "the shortest cycle passes edge 0 or E - 1"
    round255 = [cyc[j % len(cyc)] for j in range(255)]
    free = [e for e in range(E) if e not in far and int(inv[e]) not in far]
    busy = set(cyc) | {int(inv[e]) for e in cyc}
    a = next(e for e in free if inv[e] != e and e not in busy)
    s = next(e for e in free if inv[e] == e)                             # (StopIteration: the graph has no self-inverse edge)
    x = next(e for e in free if inv[e] != e and e not in busy and e not in (a, int(inv[a])))
    big = 2**31 - 1
    runs = [(0, [[a], [], [x]])]                                         # a leading run without a barcode
    if ends:
        runs.append((5, [[0]]))                                          # edge 0: the only visit of a run
    runs += [(7, [[], [a], []]), (-1, [[a], [s], []]), (None, []), (9, [[s]])]          # empty paths; bc = -1 and an empty run in the middle
    runs += [(1000 + i, [[a]]) for i in range(300)]                      # 300 one-read runs on a: lists longer than a 256-thread tile
    runs.append((2000, [[a]] * 700))                                     # 1400 equal keys, one barcode
    runs.append((3000, [round255, []]))
    runs.append((3001, [[s], [s]]))                                      # the self-inverse edge, a second run
    runs.append((3003, [[x], [int(inv[x])]]))                            # both strands from one run
    if ends:
        runs.append((big - 1, [[E - 1]]))
    runs.append((big, [[x], [a]]))
    return runs, dict(a=a, s=s, x=x, cyc=cyc)


def flatten(runs):
    bc, paths, bci = [], [], [0]
    for i, (b, ps) in enumerate(runs):
        if b is None:
            assert 0 < i < len(runs) - 1 and runs[i + 1][0] is not None and runs[i + 1][0] > 0          # an empty run: in the middle, and the reference reads the NEXT run's bc for it
        bc += [b] * len(ps)
        paths += ps
        bci.append(len(paths))
    ne = np.array([len(p) for p in paths], np.uint32)
    return np.array(bc, np.int32), np.array(bci, np.int64), ne, np.array([e for p in paths for e in p], np.int32)


def check_probe(runs, facts, off, bcs, inv, E, ends):
    a, s, x = facts["a"], facts["s"], facts["x"]
    lst = lambda e: bcs[int(off[e]):int(off[e + 1])].tolist()
    assert runs[0][0] == 0 and any(b == -1 for b, _ in runs[1:-1]) and any(b is None for b, _ in runs[1:-1])
    want_a = [7] + list(range(1000, 1300)) + [2000, 2**31 - 1]
    assert lst(a) == want_a and lst(int(inv[a])) == want_a and len(want_a) > 256
    assert lst(s) == [9, 3001] and inv[s] == s
    assert lst(x) == [3003, 2**31 - 1] and lst(int(inv[x])) == lst(x)
    assert all(lst(e) == [3000] and lst(int(inv[e])) == [3000] for e in facts["cyc"])
    assert sum(len(p) == 255 for _, ps in runs for p in ps) == 1 and sum(len(ps) == 700 for _, ps in runs) == 1
    assert any(b is not None and b > 0 and any(len(p) == 0 for p in ps) for b, ps in runs)
    if ends:
        assert lst(0) == [5] and lst(int(inv[0])) == [5] and lst(E - 1) == [2**31 - 2] and lst(int(inv[E - 1])) == [2**31 - 2]
    else:
        assert lst(0) == [] and lst(E - 1) == []
    assert int(bcs.max()) == 2**31 - 1


def save(name: str, files: dict, line: str) -> None:
    out = GOLD / "ebcx" / f"{name}.npz"
    tmp = out.with_suffix(".tmp.npz")
    np.savez_compressed(tmp, **files, ref_summary=np.frombuffer(line.encode(), dtype=np.uint8))
    limit = max(p.stat().st_size for p in (GOLD / "a48").glob("*.npz"))
    if tmp.stat().st_size > limit:
        size = tmp.stat().st_size
        tmp.unlink()
        raise AssertionError(f"{name}: {size} B, larger than the largest fixture under tests/golden/a48/ ({limit} B)")
    tmp.replace(out)
    print(f"{name}: {line} -> {out.name} ({out.stat().st_size / 1024:.0f} KiB)")


def main(argv: list[str]) -> None:
    from supernova_amd import graphio
    work, names = None, []
    it = iter(argv)
    for a in it:
        if a == "--work":
            work = Path(next(it)).resolve()
        else:
            names.append(a)
    keep = work is not None
    work = work or Path(tempfile.mkdtemp(prefix="snk_ebcx."))
    work.mkdir(parents=True, exist_ok=True)
    try:
        exe = build_driver(work)
        (GOLD / "ebcx").mkdir(exist_ok=True)
        for name in names or list(ebcxref.CASES):
            with tempfile.TemporaryDirectory(dir=work) as td:
                td = Path(td)
                probe = name in ebcxref.PROBES
                case = make_golden.CASES["adversarial" if probe else name]()
                out = make_a48x_golden.dump(case, td)
                inv = a48ref.parse_inv((out / "a.inv").read_bytes())
                if probe:
                    ends = name == "ebcx_probe"
                    g = a48xref.parse_hbv((out / "a.hbv").read_bytes())
                    runs, facts = probe_runs(g, inv, ends)
                    bc, bci, ne, edges = flatten(runs)
                    offset = np.zeros(len(ne), np.int32)
                else:
                    p_off, p_ne, p_edges = a48xref.parse_paths((out / "tmp.paths").read_bytes())
                    raw = np.asarray(case["bc"], dtype=np.int32)
                    assert len(raw) == len(p_ne)
                    order = np.argsort(raw, kind="stable")
                    start = np.concatenate([[0], np.cumsum(p_ne.astype(np.int64))])
                    bc, offset, ne = raw[order], p_off[order], p_ne[order]
                    edges = np.concatenate([p_edges[start[r]:start[r + 1]] for r in order]) if len(order) else p_edges
                    bci = ebcxref.runs_of(bc)
                graphio.write_paths(out / "tmp.paths", offset, ne, edges)
                bc.astype("<i4").tofile(out / "bc.i32")
                bci.astype("<i8").tofile(out / "bci.i64")
                ebcx, line = run_driver(exe, out)
                off, bcs = ebcxref.parse_ebcx(ebcx)
                x_off, x_bcs = ebcxref.edge_barcodes(ne, edges, bc, inv)
                assert np.array_equal(off, x_off) and np.array_equal(bcs, x_bcs), f"{name}: the restatement differs from the reference"
                assert ebcxref.ebcx_bytes(off, bcs) == ebcx
                if probe:
                    check_probe(runs, facts, off, bcs, inv, len(inv), ends)
                save(name, {"tmp_paths": np.frombuffer((out / "tmp.paths").read_bytes(), dtype=np.uint8), "bc": bc, "bci": bci,
                            "a_ebcx": np.frombuffer(ebcx, dtype=np.uint8)}, line)
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:])
