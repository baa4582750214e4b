#!/usr/bin/env python3
"""Generate tests/golden/a48/<case>.npz: the bytes of the files the REFERENCE leaves in a.48/ beside a.hbv and a.inv.

Run by hand where the reference's sources can be read (like make_golden.py; needs oracle/_ref/snref_driver).  Per K=48 golden case:
  tmp.paths     what pathReads writes (BuildReadQGraph48.cc:1441-1469) -- 10X/DF.cc:584 renames it to a.paths; left behind by the
                `snref_driver ... dump` run
  a.paths.inv   writePathsIndex (10X/PathsIndex.cc:23-145, called at DF.cc:588) over that tmp.paths and a.inv
  a.countsb     the same call
  a.dup         BinaryWriter::writeFile(vec<Bool>) (DF.cc:599-600) of the flags MarkDups left in the dump
The last three are written by a48_driver.cc (next to this file), which calls the reference's functions.  The driver is built in a
scratch directory, never into the repository: a COPY of oracle/ref/ is run there with the recipe's own hooks (SNK_REF_EXTRA adds
10X/PathsIndex to the closure, SNK_REF_WORK keeps the objects and the patched-header overlay), then the driver is compiled with the
recipe's flags and linked against its libref.a with --gc-sections.

usage: python tests/golden/make_a48_golden.py [--work DIR] [--big N] [case ...]
  --work DIR   scratch directory (kept; a libref.a already there is reused), default: a temporary one
  --big N      also time writePathsIndex on N synthetic reads with 0.6 % errors (nothing is stored; the log line is the result)
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

import refio  # noqa: E402
import make_golden  # noqa: E402

GOLD = Path(__file__).resolve().parent
FILES = ("tmp.paths", "a.paths.inv", "a.countsb", "a.dup")
OPT = os.environ.get("SNK_REF_OPT", "-O1")


def build_driver(work: Path) -> Path:
    refwork = work / "refwork"
    if not (refwork / "libref.a").exists():
        shutil.copytree(ROOT / "oracle" / "ref", work / "oracle" / "ref", dirs_exist_ok=True)
        env = dict(os.environ, SNK_REF_EXTRA="10X/PathsIndex", SNK_REF_WORK=str(refwork), SNK_REF_OPT=OPT)
        subprocess.run(["bash", str(work / "oracle" / "ref" / "build_ref.sh")], check=True, env=env)
    exe = work / "a48_driver"
    src = GOLD / "a48_driver.cc"
    if not exe.exists() or exe.stat().st_mtime < src.stat().st_mtime:
        cxx = os.environ.get("CXX", "g++")
        flags = ["-std=c++11", "-fpermissive", "-fopenmp", "-fno-strict-aliasing", "-w", OPT, "-DNDEBUG", "-ffunction-sections", "-fdata-sections",
                 f"-I{refwork / 'overlay'}"]
        obj = work / "a48_driver.o"
        subprocess.run([cxx, *flags, "-c", str(src), "-o", str(obj)], check=True)
        subprocess.run([cxx, "-fopenmp", "-Wl,--gc-sections", "-o", str(exe), str(obj), str(refwork / "obj" / "LinkTimestamp.o"), str(refwork / "libref.a"),
                        "-lz", "-lpthread"], check=True)
    return exe


def run_case(exe: Path, case: dict, td: Path) -> tuple[dict, str]:
    refio.write_snkrd(td / "in.snkrd", case["lens"], case["ascii"], case["quals"], case["bc"], case["ign_bc_below"])
    refio.run_ref(td / "in.snkrd", td / "out")
    r = subprocess.run([str(exe), str(td / "out")], check=True, capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("A48_DRIVER")][-1]
    return {f: np.frombuffer((td / "out" / f).read_bytes(), dtype=np.uint8) for f in FILES}, line


def main(argv: list[str]) -> None:
    work, big, names = None, 0, []
    it = iter(argv)
    for a in it:
        if a == "--work":
            work = Path(next(it)).resolve()
        elif a == "--big":
            big = int(next(it))
        else:
            names.append(a)
    keep = work is not None
    work = work or Path(tempfile.mkdtemp(prefix="snk_a48."))
    work.mkdir(parents=True, exist_ok=True)
    try:
        exe = build_driver(work)
        (GOLD / "a48").mkdir(exist_ok=True)
        for name in names or ([] if big else list(make_golden.CASES)):
            with tempfile.TemporaryDirectory(dir=work) as td:
                files, line = run_case(exe, make_golden.CASES[name](), Path(td))
            out = GOLD / "a48" / f"{name}.npz"
            np.savez_compressed(out, **{f.replace(".", "_"): b for f, b in files.items()}, ref_summary=np.frombuffer(line.encode(), dtype=np.uint8))
            print(f"{name}: {line} -> {out.name} ({out.stat().st_size / 1024:.0f} KiB; " + ", ".join(f"{f} {len(b)} B" for f, b in files.items()) + ")")
        if big:
            from supernova_amd import synth
            sp = synth.synth_params(big, seed=0x5EED0C0D, sub_ppm=6000)
            rows, quals, bc = synth.synth_host(sp)
            case = dict(lens=np.full(big, sp.read_len, np.uint16), ascii=synth.codes_to_ascii(synth.unpack_rows(rows, sp.read_len)), quals=quals, bc=bc,
                        ign_bc_below=0)
            with tempfile.TemporaryDirectory(dir=work) as td:
                _, line = run_case(exe, case, Path(td))
            print(f"synth {big} reads, sub_ppm 6000: {line}")
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:])
