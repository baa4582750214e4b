#!/usr/bin/env python3
"""Generate tests/golden/edit/<case>.npz: what the REFERENCE's DeleteEdgesParallel + Cleanup (paths/long/large/GapToyTools.cc:1287-1302)
make of the cases of tests/editref.py.

Run by hand where the reference's sources can be read (like make_patch_golden.py: make_hops_golden.build_driver makes libref.a, the
patched-header overlay and the objects the earlier drivers need).  On top of it one more object -- paths/long/large/GapToyTools -- and
edit_driver.cc (next to this file) are compiled there and linked; nothing compiled is kept.

Every case runs with 1 and with 8 OpenMP threads and both must give the same files.  Before a case is saved the Python restatement
(tests/editref.py) must reproduce every one of them: a.hbv, a.inv, the paths and the a.pathsX bytes after every edit of the case.

A fixture holds what identifies the input it was made from (the generator makes the input again from its seed), dels, per edit the
reference's a.hbv / a.inv bytes, the paths and the a.pathsX bytes, the driver's summary line -- and, from the restatement alone (the rule
is inline in StageTrim and cannot be called), the read support and the hanging-end selection on the case's input.

`fuzz` (or fuzz_<seed>) makes the fuzz_<seed> family: the edit step of the pinned seeds patchgen.PINNED of tests/patchgen.py, on the graph
that gap-patch insertion left (tests/golden/patch/fuzz_<seed>.npz holds that graph as the reference made it).  Such a fixture holds
results only -- no dels: in_digest covers them -- and is never made unpinned; it is written without a time of day, so a second run gives
the same bytes.

usage: python tests/golden/make_edit_golden.py [--work DIR] [case ...]
"""
from __future__ import annotations

import os
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

import a48xref  # noqa: E402
import editref  # noqa: E402
import make_a48_golden  # noqa: E402
import make_ext_golden  # noqa: E402
import make_hops_golden  # noqa: E402
from make_patch_golden import fuzz_limit, save_fixed  # noqa: E402

GOLD = Path(__file__).resolve().parent
EXTRA = ("paths/long/large/GapToyTools",)
FILES = ("a.hbv", "a.inv", "a.paths", "a.pathsX")


def build_driver(work: Path) -> Path:
    make_hops_golden.build_driver(work)
    refwork = work / "refwork"
    ov = refwork / "overlay"
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++11", "-fpermissive", "-fopenmp", "-fno-strict-aliasing", "-w", make_a48_golden.OPT, "-DNDEBUG", "-ffunction-sections", "-fdata-sections", f"-I{ov}",
             "-D_GLIBCXX_ALIGN_H=1"]
    objs = [work / ("ext_" + rel.replace("/", "_") + ".o") for rel in make_ext_golden.EXTRA]
    for rel in EXTRA:
        obj = work / ("edit_" + rel.replace("/", "_") + ".o")
        objs.append(obj)
        if not obj.exists():
            subprocess.run([cxx, *flags, "-c", str(ov / (rel + ".cc")), "-o", str(obj)], check=True)
    exe, src = work / "edit_driver", GOLD / "edit_driver.cc"
    if not exe.exists() or exe.stat().st_mtime < src.stat().st_mtime:
        obj = work / "edit_driver.o"
        subprocess.run([cxx, *flags, "-c", str(src), "-o", str(obj)], check=True)
        subprocess.run([cxx, "-fopenmp", "-Wl,--gc-sections", "-o", str(exe), str(obj), *map(str, objs), str(refwork / "obj" / "LinkTimestamp.o"), str(refwork / "libref.a"),
                        "-lz", "-lpthread"], check=True)
    return exe


def run_reference(exe: Path, td: Path, c, lists):
    """-> ([{file: bytes} per edit], summary line); 1 and 8 threads must agree"""
    (td / "in.hbv").write_bytes(c.a_hbv)
    (td / "in.inv").write_bytes(c.a_inv)
    (td / "in.paths").write_bytes(make_ext_golden.paths_bytes(c.offset, c.n_edges, c.edges, td))
    (td / "dels.bin").write_bytes(b"SNKDEL01" + struct.pack("<Q", len(lists)) + b"".join(struct.pack("<Q", len(l)) + np.asarray(l, "<i4").tobytes() for l in lists))
    got, line = {}, ""
    for th in (1, 8):
        out = td / f"out{th}"
        out.mkdir()
        r = subprocess.run([str(exe), str(td / "in.hbv"), str(td / "in.inv"), str(td / "in.paths"), str(td / "dels.bin"), str(th), str(out)], check=True, capture_output=True,
                           text=True, env=dict(os.environ, OMP_NUM_THREADS=str(th)))
        got[th] = [{f: (out / f"{f}.{i}").read_bytes() for f in FILES} for i in range(len(lists))]
        if th == 1:
            line = [l for l in r.stdout.splitlines() if l.startswith("EDIT_DRIVER")][-1]
    for i in range(len(lists)):
        for f in FILES:
            assert got[1][i][f] == got[8][i][f], f"{c.key}: 1 and 8 threads differ in {f}.{i}"
    return got[1], line


def pathsx_of(a_hbv: bytes, offset, n_edges, edges) -> bytes:
    idx, data, _ = a48xref.zip_paths(offset, n_edges, edges, a48xref.parse_hbv(a_hbv))
    return a48xref.pathsx_bytes(idx, data, len(n_edges))


def make(exe, work: Path, key: str):
    c = editref.case(key)
    mine = editref.restated(key)
    lists = [c.dels] + ([editref.second_dels(mine[0], c.second)] if c.second else [])
    u8 = lambda b: np.frombuffer(b, np.uint8)
    keep = {}
    if exe is not None:
        with tempfile.TemporaryDirectory(dir=work) as td:
            ref, line = run_reference(exe, Path(td), c, lists)
        for i, (m, r) in enumerate(zip(mine, ref)):          # the restatement must reproduce the reference before anything is kept
            off, ne, ed = a48xref.parse_paths(r["a.paths"])
            assert m.a_hbv == r["a.hbv"], f"{key}: edit {i}: the restatement's a.hbv differs from the reference's"
            assert m.a_inv == r["a.inv"], f"{key}: edit {i}: a.inv differs"
            assert np.array_equal(m.offset, off) and np.array_equal(m.n_edges, ne) and np.array_equal(m.edges, ed), f"{key}: edit {i}: the paths differ"
            assert pathsx_of(m.a_hbv, m.offset, m.n_edges, m.edges) == r["a.pathsX"], f"{key}: edit {i}: a.pathsX differs"
            keep.update({f"a_hbv{i}": u8(r["a.hbv"]), f"a_inv{i}": u8(r["a.inv"]), f"offset{i}": off, f"n_edges{i}": ne, f"edges{i}": ed, f"pathsx{i}": u8(r["a.pathsX"])})
    else:                                                    # no reference at hand: the restatement alone, marked unpinned
        line = "unpinned"
        for i, m in enumerate(mine):
            keep.update({f"a_hbv{i}": u8(m.a_hbv), f"a_inv{i}": u8(m.a_inv), f"offset{i}": m.offset, f"n_edges{i}": m.n_edges, f"edges{i}": m.edges,
                         f"pathsx{i}": u8(pathsx_of(m.a_hbv, m.offset, m.n_edges, m.edges))})
    if key.startswith("none_"):
        assert bytes(keep["a_hbv0"]) == c.a_hbv and bytes(keep["a_inv0"]) == c.a_inv, "no deletion: the graph must come back byte for byte"
    support, hang = editref.hanging_ends(c.a_hbv, c.inv, c.n_edges, c.edges)
    if c.hang_want is not None:
        assert np.array_equal(hang, c.hang_want), f"{key}: the hanging-end rule does not pick the edges the case names"
    out = GOLD / "edit" / f"{key}.npz"
    if key.startswith("fuzz_"):
        assert exe is not None, f"{key}: a fuzz fixture is made by the reference or not at all"
        limit = fuzz_limit(GOLD / "edit")
        save_fixed(out, dict(in_digest=u8(editref.digest(c)), n_steps=np.int64(len(mine)), pinned=np.bool_(True), support=support, hang_dels=hang, ref_summary=u8(line.encode()),
                             **keep))
        assert out.stat().st_size <= limit, f"{out.name}: {out.stat().st_size} B, the largest hand-made fixture has {limit}"
        print(f"{key}: {line} | restatement {[m.counters for m in mine]} -> {out.name} ({out.stat().st_size / 1024:.0f} KiB)")
        return
    np.savez_compressed(out, in_digest=u8(editref.digest(c)), dels=c.dels, n_steps=np.int64(len(mine)), pinned=np.bool_(exe is not None), support=support, hang_dels=hang,
                        ref_summary=u8(line.encode()), **keep)
    assert out.stat().st_size < (1 << 20), f"{out.name} is larger than a committed file may be"
    print(f"{key}: {line} | restatement {[m.counters for m in mine]} -> {out.name} ({out.stat().st_size / 1024:.0f} KiB)")


def main(argv: list[str]) -> None:
    work, names, unpinned = None, [], False
    it = iter(argv)
    for a in it:
        if a == "--work":
            work = Path(next(it)).resolve()
        elif a == "--unpinned":
            unpinned = True
        else:
            names.append(a)
    keep = work is not None
    work = work or Path(tempfile.mkdtemp(prefix="snk_edit."))
    work.mkdir(parents=True, exist_ok=True)
    try:
        exe = None if unpinned else build_driver(work)
        (GOLD / "edit").mkdir(exist_ok=True)
        import patchgen
        fuzz = [patchgen.key_of(s) for s in patchgen.PINNED]
        names = [k for a in names for k in (fuzz if a == "fuzz" else [a])]
        for key in names or editref.ALL + tuple(fuzz):
            make(exe, work, key)
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:])
