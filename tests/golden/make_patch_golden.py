#!/usr/bin/env python3
"""Generate tests/golden/patch/<case>.npz: what the REFERENCE's StageInsertPatch steps (BuildAll, buildBigKHBVFromReads_sleek, the
to3 / left3 loop, TranslatePaths) make of the cases of tests/patchref.py.

Run by hand where the reference's sources can be read (like make_ext_golden.py, whose build_driver makes libref.a, the patched-header
overlay and the three objects the path extension needs).  On top of it two more objects -- kmers/BigKPather and kmers/KmerRecord -- and
patch_driver.cc (next to this file) are compiled there and linked; nothing compiled is kept.

The reference numbers its new edges in the order its threads append them, so the driver renumbers everything by edge sequence onto
the graph that the reference's buildHBVFromEdges makes of the new unitigs in BVComp order (patch_driver.cc).  Every case runs with 1
and with 8 threads and both must give the same files.  Before a case is saved the Python restatement (tests/patchref.py) must
reproduce every one of them.

A fixture holds the patched a.hbv / a.inv bytes, to3 (offsets + ids), left3, per read (edge or -1, offset), the a.pathsX bytes, the
driver's summary line, and what identifies the input it was made from (the generator makes the input again from its seed).
synth_2k_err_ext.npz is the chain case: the a.pathsX bytes the reference's ExtendPathsNew (make_ext_golden's ext_driver, BACK_EXTEND 0)
leaves on that fixture's patched graph and translated paths.

`fuzz` (or fuzz_<seed>) makes the fuzz_<seed> family: the pinned seeds patchgen.PINNED of the seeded generator tests/patchgen.py.  Such a
fixture holds results only -- the same arrays without the closures, and in_digest (patchref.digest) over the whole input --: the input
is made again from the seed, and the digest says when the generator has drifted.  It is written without a time of day, so a second run
gives the same bytes.

usage: python tests/golden/make_patch_golden.py [--work DIR] [case ...]
"""
from __future__ import annotations

import io
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import zipfile
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import handunitigs as hu  # noqa: E402
import make_a48_golden  # noqa: E402
import make_ext_golden  # noqa: E402
import patchref  # noqa: E402

GOLD = Path(__file__).resolve().parent
EXTRA = ("kmers/BigKPather", "kmers/KmerRecord")
FILES = ("a.hbv", "a.inv", "to3_off.u64", "to3.i32", "left3.i32", "reads.i32", "a.pathsX")


def build_driver(work: Path) -> Path:
    make_ext_golden.build_driver(work)
    refwork = work / "refwork"
    ov = refwork / "overlay"
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++11", "-fpermissive", "-fopenmp", "-fno-strict-aliasing", "-w", make_a48_golden.OPT, "-DNDEBUG", "-ffunction-sections", "-fdata-sections", f"-I{ov}",
             "-D_GLIBCXX_ALIGN_H=1"]
    objs = [work / ("ext_" + rel.replace("/", "_") + ".o") for rel in make_ext_golden.EXTRA]
    for rel in EXTRA:
        obj = work / ("patch_" + rel.replace("/", "_") + ".o")
        objs.append(obj)
        if not obj.exists():
            subprocess.run([cxx, *flags, "-c", str(ov / (rel + ".cc")), "-o", str(obj)], check=True)
    exe, src = work / "patch_driver", GOLD / "patch_driver.cc"
    if not exe.exists() or exe.stat().st_mtime < src.stat().st_mtime:
        obj = work / "patch_driver.o"
        subprocess.run([cxx, *flags, "-c", str(src), "-o", str(obj)], check=True)
        subprocess.run([cxx, "-fopenmp", "-Wl,--gc-sections", "-o", str(exe), str(obj), *map(str, objs), str(refwork / "obj" / "LinkTimestamp.o"), str(refwork / "libref.a"),
                        "-lz", "-lpthread"], check=True)
    return exe


def run_reference(exe: Path, td: Path, c):
    """-> ({file: bytes}, summary line); 1 and 8 threads must agree"""
    (td / "in.hbv").write_bytes(c.a_hbv)
    (td / "in.paths").write_bytes(make_ext_golden.paths_bytes(c.offset, c.n_edges, c.edges, td))
    off, cb = patchref.closures_arrays(c.closures)
    (td / "closures.bin").write_bytes(b"SNKCL001" + struct.pack("<Q", len(c.closures)) + off.astype("<u8").tobytes() + cb.tobytes())
    got, line = {}, ""
    for th in (1, 8):
        out = td / f"out{th}"
        out.mkdir()
        r = subprocess.run([str(exe), str(td / "in.hbv"), str(td / "in.paths"), str(td / "closures.bin"), str(th), str(out)], check=True, capture_output=True, text=True,
                           env=dict(os.environ, OMP_NUM_THREADS=str(th)))
        got[th] = {f: (out / f).read_bytes() for f in FILES}
        if th == 1:
            line = [l for l in r.stdout.splitlines() if l.startswith("PATCH_DRIVER")][-1]
    for f in FILES:
        assert got[1][f] == got[8][f], f"{c.key}: 1 and 8 threads differ in {f} after renumbering"
    return got[1], line


def save_fixed(out: Path, arrays: dict) -> None:
    """an .npz that a second run writes again byte for byte: sorted names, no time of day in the archive"""
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[k])
            np.lib.format.write_array(buf, np.ascontiguousarray(a) if a.ndim else a, allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def fuzz_limit(folder: Path) -> int:
    """a fuzz_<seed> fixture stays below the largest hand-made one beside it"""
    return max(p.stat().st_size for p in folder.glob("*.npz") if not p.name.startswith("fuzz_"))


def make(exe: Path, work: Path, key: str):
    c = patchref.case(key)
    with tempfile.TemporaryDirectory(dir=work) as td:
        ref, line = run_reference(exe, Path(td), c)
    to3_off, to3, left3 = np.frombuffer(ref["to3_off.u64"], "<u8"), np.frombuffer(ref["to3.i32"], "<i4"), np.frombuffer(ref["left3.i32"], "<i4")
    reads = np.frombuffer(ref["reads.i32"], "<i4").reshape(-1, 2)
    # the restatement must reproduce the reference before anything is kept
    m = patchref.insert_patch(c.K, c.a_hbv, c.closures, c.offset, c.n_edges, c.edges)
    moff, mids = patchref.flat(m.to3)
    for what, a, b in (("a.hbv", m.a_hbv, ref["a.hbv"]), ("a.inv", m.a_inv, ref["a.inv"]), ("a.pathsX", m.pathsx, ref["a.pathsX"])):
        assert a == b, f"{key}: the restatement's {what} differs from the reference's"
    assert np.array_equal(moff, to3_off) and np.array_equal(mids, to3) and np.array_equal(m.left3, left3), f"{key}: to3 / left3 differ"
    assert np.array_equal(m.edge, reads[:, 0]) and np.array_equal(patchref.a48xref.wrap16(m.offset), reads[:, 1]), f"{key}: translated paths differ"
    if key.startswith("none_"):
        assert ref["a.hbv"] == c.a_hbv and ref["a.inv"] == c.a_inv, "no closures: the graph must come back byte for byte"
    off, cb = patchref.closures_arrays(c.closures)
    u8 = lambda b: np.frombuffer(b, np.uint8)
    out = GOLD / "patch" / f"{key}.npz"
    if key.startswith("fuzz_"):
        save_fixed(out, dict(a_hbv=u8(ref["a.hbv"]), a_inv=u8(ref["a.inv"]), to3_off=to3_off, to3=to3, left3=left3, edge=reads[:, 0].copy(), offset=reads[:, 1].copy(),
                             pathsx=u8(ref["a.pathsX"]), ref_summary=u8(line.encode()), in_digest=u8(patchref.digest(c))))
        assert out.stat().st_size <= fuzz_limit(GOLD / "edit"), f"{out.name}: {out.stat().st_size} B"
        print(f"{key}: {line} | restatement {m.counters} -> {out.name} ({out.stat().st_size / 1024:.0f} KiB)")
        return
    np.savez_compressed(out, a_hbv=u8(ref["a.hbv"]), a_inv=u8(ref["a.inv"]), to3_off=to3_off, to3=to3, left3=left3, edge=reads[:, 0].copy(), offset=reads[:, 1].copy(),
                        pathsx=u8(ref["a.pathsX"]), ref_summary=u8(line.encode()), in_hbv_crc=u8(str(zlib.crc32(c.a_hbv)).encode()), closure_off=off,
                        closure_codes2=hu.pack2(cb), in_paths_crc=u8(str(zlib.crc32(c.offset.tobytes() + c.n_edges.tobytes() + c.edges.tobytes())).encode()))
    print(f"{key}: {line} | restatement {m.counters} -> {out.name} ({out.stat().st_size / 1024:.0f} KiB)")


def make_chain(work: Path):
    """The chain case: the reference's ExtendPathsNew (ext_driver, BACK_EXTEND 0) on the patched graph and the translated paths of
    synth_2k_err, from that case's fixture -> tests/golden/patch/<case>_ext.npz (the a.pathsX bytes it leaves)."""
    import a48xref
    import extref
    import goldens
    key = patchref.SYNTH
    g = patchref.golden(key)
    c = goldens.load(key)
    exe = work / "ext_driver"
    paths = patchref.one_edge_paths(g.edge, g.offset)
    reads = dict(lens=c.lens, ascii=np.frombuffer(b"ACGT", np.uint8)[c.codes], quals=c.quals, codes=c.codes)
    with tempfile.TemporaryDirectory(dir=work) as td:
        td = Path(td)
        in_paths = make_ext_golden.paths_bytes(*paths, td)
        ref, line = make_ext_golden.run_reference(exe, td, reads, g.a_hbv, g.a_inv, in_paths)
    g3 = a48xref.parse_hbv(g.a_hbv)
    mine = make_ext_golden.restate(g3, extref.edge_bases(g3), reads, paths)
    assert mine[0][0] == ref[0], "chain: the restatement of ExtendPathsNew does not reproduce the reference's bytes on the patched graph"
    assert mine[0][1]["n_quality_extended"] + mine[0][1]["n_exact_extended"] >= 1, "chain: no read is extended"
    out = GOLD / "patch" / f"{key}_ext.npz"
    np.savez_compressed(out, pathsx0=np.frombuffer(ref[0], np.uint8), ref_summary=np.frombuffer(line.encode(), np.uint8))
    print(f"{key}_ext: {line} | restatement {mine[0][1]} -> {out.name} ({out.stat().st_size / 1024:.0f} KiB)")


def main(argv: list[str]) -> None:
    work, names = None, []
    it = iter(argv)
    for a in it:
        if a == "--work":
            work = Path(next(it)).resolve()
        else:
            names.append(a)
    keep = work is not None
    work = work or Path(tempfile.mkdtemp(prefix="snk_patch."))
    work.mkdir(parents=True, exist_ok=True)
    try:
        exe = build_driver(work)
        (GOLD / "patch").mkdir(exist_ok=True)
        import patchgen
        fuzz = [patchgen.key_of(s) for s in patchgen.PINNED]
        names = [k for a in names for k in (fuzz if a == "fuzz" else [a])]
        for key in names or patchref.ALL + tuple(fuzz):
            make(exe, work, key)
        if not names or patchref.SYNTH in names:
            make_chain(work)
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:])
