#!/usr/bin/env python3
"""Generate tests/golden/a48x/<case>.npz: the bytes of a.hbx and a.pathsX as the REFERENCE's own code writes them.

Run by hand where the reference's sources can be read (like make_a48_golden.py; needs oracle/_ref/snref_driver and, for the probe
case, libsnk.so).  a48x_driver.cc (next to this file) reads a dump directory's a.hbv, writes HyperBasevectorX(hbv) as a.hbx
(10X/DF.cc:573-576), makes the ReadPathVecX of its tmp.paths and writes a.pathsX.  It is built like a48_driver: in a scratch directory, a
COPY of oracle/ref/ run with the recipe's own hooks (SNK_REF_EXTRA, SNK_REF_WORK), then compiled with the recipe's flags and linked
against its libref.a with --gc-sections.  Nothing compiled is kept in the repository.

The ReadPathVecX is made by InitializePathsXFromPaths (10X/DfTools.cc:24-69), as DF.cc:579 calls it; should that not link, by the
sequential append(paths, hb) (10X/paths/ReadPathVecX.cc:378).  ref_summary records which one ran.  Every case runs with 1 and with 8
OpenMP threads, and with both functions where both link: all must give the same bytes (the one-thread bytes are stored).

Cases:
  the five K=48 golden cases   a.hbx, a.pathsX
  long_unitig                  error-free pairs over one random 40 kb genome at 30x (a48xref.long_unitig_reads): offsets above 32767.
                               The reads are made again by the tests; the fixture holds their digest and all eight files of a.48/
  probe_paths                  on the adversarial case's graph, a hand-made tmp.paths (written with snk_write_paths): empty paths, a path
                               of exactly 255 edges round a cycle, one-edge paths with offsets -40000, -1, 32767, 32768, a path with a
                               step between two edges that are not adjacent in its middle and one with such a step at its end; 23
                               reads.  Holds tmp.paths and a.pathsX

usage: python tests/golden/make_a48x_golden.py [--work DIR] [case ...]
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

import a48xref  # noqa: E402
import make_a48_golden  # noqa: E402
import make_golden  # noqa: E402
import refio  # noqa: E402

GOLD = Path(__file__).resolve().parent
OPT = make_a48_golden.OPT


def build_driver(work: Path) -> tuple[Path, Path]:
    """-> (a48_driver, a48x_driver); the reference objects are built once (make_a48_golden.build_driver) and shared."""
    a48 = make_a48_golden.build_driver(work)
    refwork = work / "refwork"
    exe = work / "a48x_driver"
    src = GOLD / "a48x_driver.cc"
    if not exe.exists() or exe.stat().st_mtime < src.stat().st_mtime:
        cxx = os.environ.get("CXX", "g++")
        flags = ["-std=c++11", "-fpermissive", "-fopenmp", "-fno-strict-aliasing", "-w", OPT, "-DNDEBUG", "-ffunction-sections", "-fdata-sections",
                 f"-I{refwork / 'overlay'}"]
        obj = work / "a48x_driver.o"
        subprocess.run([cxx, *flags, "-c", str(src), "-o", str(obj)], check=True)
        subprocess.run([cxx, "-fopenmp", "-Wl,--gc-sections", "-o", str(exe), str(obj), str(refwork / "obj" / "LinkTimestamp.o"), str(refwork / "libref.a"),
                        "-lz", "-lpthread"], check=True)
    return a48, exe


def run_driver(exe: Path, out: Path) -> tuple[bytes, bytes, str]:
    """The driver with both functions and both thread counts -> (a.hbx, a.pathsX, summary); all runs must agree."""
    got = {}
    for mode in ("init", "append"):
        for threads in (1, 8):
            r = subprocess.run([str(exe), str(out), mode], check=True, capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(threads)))
            line = [l for l in r.stdout.splitlines() if l.startswith("A48X_DRIVER")][-1]
            got[mode, threads] = ((out / "a.hbx").read_bytes(), (out / "a.pathsX").read_bytes(), line)
    base = got["init", 1]
    for k, v in got.items():
        assert v[0] == base[0] and v[1] == base[1], f"{k} differs from ('init', 1): a finding for DESIGN.md"
    return base[0], base[1], base[2] + " | same bytes with 8 threads and from append(paths, hb)"


def dump(case: dict, td: Path) -> Path:
    refio.write_snkrd(td / "in.snkrd", case["lens"], case["ascii"], case["quals"], case["bc"], case["ign_bc_below"])
    refio.run_ref(td / "in.snkrd", td / "out")
    return td / "out"


def save(name: str, files: dict, line: str, **more) -> None:
    out = GOLD / "a48x" / f"{name}.npz"
    tmp = out.with_suffix(".tmp.npz")
    np.savez_compressed(tmp, **{f.replace(".", "_"): np.frombuffer(b, dtype=np.uint8) for f, b in files.items()},
                        ref_summary=np.frombuffer(line.encode(), dtype=np.uint8), **more)
    limit = max(p.stat().st_size for p in (GOLD / "a48").glob("*.npz"))
    if tmp.stat().st_size > limit:                      # nothing too large is left in the fixture directory
        size = tmp.stat().st_size
        tmp.unlink()
        raise AssertionError(f"{name}: {size} B, larger than the largest fixture under tests/golden/a48/ ({limit} B)")
    tmp.replace(out)
    print(f"{name}: {line} -> {out.name} ({out.stat().st_size / 1024:.0f} KiB; " + ", ".join(f"{f} {len(b)} B" for f, b in files.items()) + ")")


def find_cycle(g: a48xref.Graph) -> list[int]:
    """The shortest closed walk of the graph: edges e0 .. ek with every step adjacent and ek -> e0 adjacent (breadth first from every edge)."""
    adj = lambda e: [int(x) for x in g.from_e[g.from_off[g.v_right[e]]:g.from_off[g.v_right[e] + 1]]]
    best = None
    for e0 in range(g.E):
        prev, frontier, last = {e0: None}, [e0], None
        while frontier and last is None:
            nxt = []
            for e in frontier:
                for e2 in adj(e):
                    if e2 == e0:
                        last = e
                        break
                    if e2 not in prev:
                        prev[e2] = e
                        nxt.append(e2)
                if last is not None:
                    break
            frontier = nxt
        if last is not None:
            walk = [last]
            while prev[walk[-1]] is not None:
                walk.append(prev[walk[-1]])
            if best is None or len(walk) < len(best):
                best = walk[::-1]
            if len(best) == 1:
                break
    assert best is not None, "the graph has no cycle"
    return best


def probe_paths(g: a48xref.Graph):
    """-> (offset i32[23], n_edges u32[23], edges i32[])"""
    cyc = find_cycle(g)
    round255 = [cyc[j % len(cyc)] for j in range(255)]
    adj = lambda e: [int(x) for x in g.from_e[g.from_off[g.v_right[e]]:g.from_off[g.v_right[e] + 1]]]
    a = next(e for e in range(g.E) if adj(e) and adj(adj(e)[-1]))               # a -> b -> c adjacent
    b = adj(a)[-1]
    c = adj(b)[-1]
    x = next(e for e in range(g.E) if g.v_left[e] != g.v_right[b] and adj(e))   # b -> x is no step of the graph
    y = adj(x)[-1]
    z = next(e for e in range(g.E) if g.v_left[e] != g.v_right[c])
    paths = [(0, []), (7, [a]), (-40000, [a]), (-1, [b]), (32767, [c]), (32768, [x]), (0, []), (0, []), (12, round255), (3, [a, b, x, y]),
             (-5, [a, b, c, z]), (0, []), (100, [a, b, c]), (0, [])]
    while len(paths) < 23:
        paths.append((len(paths), [a, b] if len(paths) % 2 else []))
    off = np.array([p[0] for p in paths], np.int32)
    ne = np.array([len(p[1]) for p in paths], np.uint32)
    return off, ne, np.array([e for p in paths for e in p[1]], np.int32)


def main(argv: list[str]) -> None:
    work, names = None, []
    it = iter(argv)
    for a in it:
        if a == "--work":
            work = Path(next(it)).resolve()
        else:
            names.append(a)
    keep = work is not None
    work = work or Path(tempfile.mkdtemp(prefix="snk_a48x."))
    work.mkdir(parents=True, exist_ok=True)
    try:
        a48, exe = build_driver(work)
        (GOLD / "a48x").mkdir(exist_ok=True)
        for name in names or list(make_golden.CASES) + list(a48xref.EXTRA):
            with tempfile.TemporaryDirectory(dir=work) as td:
                td = Path(td)
                if name == "long_unitig":
                    from supernova_amd import synth
                    codes, quals, lens, bc = a48xref.long_unitig_reads()
                    out = dump(dict(lens=lens, ascii=synth.codes_to_ascii(codes), quals=quals, bc=bc, ign_bc_below=0), td)
                    subprocess.run([str(a48), str(out)], check=True, capture_output=True)
                    hbx, px, line = run_driver(exe, out)
                    files = {f: (out / f).read_bytes() for f in a48xref.FILES if f not in ("a.hbx", "a.pathsX")}
                    p_off, p_ne, _ = a48xref.parse_paths(files["tmp.paths"])
                    assert int((p_off[p_ne > 0] > 32767).sum()) >= 1, "no offset above 32767: the case does not do what it is for"
                    line += f" | offsets above 32767: {int((p_off[p_ne > 0] > 32767).sum())}"
                    save(name, {"a.hbx": hbx, "a.pathsX": px, **files}, line, reads_digest=np.frombuffer(a48xref.reads_digest(codes, quals, lens, bc), dtype=np.uint8))
                elif name == "probe_paths":
                    from supernova_amd import graphio
                    out = dump(make_golden.CASES["adversarial"](), td)
                    off, ne, edges = probe_paths(a48xref.parse_hbv((out / "a.hbv").read_bytes()))
                    graphio.write_paths(out / "tmp.paths", off, ne, edges)
                    hbx, px, line = run_driver(exe, out)
                    save(name, {"tmp.paths": (out / "tmp.paths").read_bytes(), "a.pathsX": px}, line)
                else:
                    out = dump(make_golden.CASES[name](), td)
                    hbx, px, line = run_driver(exe, out)
                    save(name, {"a.hbx": hbx, "a.pathsX": px}, line)
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:])
