#!/usr/bin/env python3
"""Generate tests/golden/ext/<case>.npz: the a.pathsX bytes the REFERENCE's ExtendPathsNew (10X/Extend.cc:14-177) leaves, with
BACK_EXTEND 0 and 1, for the inputs of tests/extref.py's cases.

Run by hand where the reference's sources can be read (like make_a48_golden.py, whose build_driver makes libref.a and the patched-header
overlay in a scratch directory).  On top of it three more objects -- 10X/Extend, paths/long/large/GapToyTools3 (Validate) and
paths/long/large/GapToyTools4 (ExtendPath) -- and ext_driver.cc (next to this file) are compiled there and linked; nothing compiled is
kept.  Two things those three need with g++ 11:
  -D_GLIBCXX_ALIGN_H=1      std::align otherwise collides with the reference's `class align` (PackAlign.h)
  GapToyTools4.cc           four debug lines (717, 734, 742, 760; none in ExtendPath) end in `<< std::cout;` where `<< std::endl;` is
                            meant and do not compile: edited in flight, in the scratch overlay only
Every run goes with 1 and with 8 OpenMP threads and both must give the same bytes.  Before a case is saved the Python restatement
(tests/extref.py) must reproduce the reference's bytes for both flags, and the property the case is there for is asserted through the
restatement's counters.

Cases: the five K=48 golden cases on the reference's own paths (tmp.paths of tests/golden/a48/, a.hbv / a.inv of tests/golden/<case>.npz:
bytes the reference wrote); `<case>_cut`: the first edge of every path of two or more edges dropped; `<case>_first`: every path cut to
its first edge (flag 0 must give the un-cut case's bytes); hand_k48 / hand_k60: tests/handext.py.  Two limits shape the golden inputs
(extref.golden_input is the one place that applies them):
  - a fixture may not be larger than the largest under tests/golden/a48/, so a case uses its first 10 000 reads (reads are independent
    of each other; only synth_20k_err has more)
  - the reference's input is a ReadPathVecX, whose offsets are int16: a path whose offset lies outside +-32767 (a few reads far down
    synth_20k_err's 33 kb edge) would wrap and send the reference reading outside the read, so such a read goes in without a path
A case without any path of two or more edges (synth_2k_err, synth_6k_clean: one unitig) has no `_cut` / `_first`: they would be the case itself.

A fixture holds in_paths (the input as a feudal paths file), pathsx0 / pathsx1 (the output bytes per flag), ref_summary, and for the
hand-made cases a_hbv / a_inv.

usage: python tests/golden/make_ext_golden.py [--work DIR] [case ...]
"""
from __future__ import annotations

import ctypes as C
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
import extref  # noqa: E402
import goldens  # noqa: E402
import handext  # noqa: E402
import make_a48_golden  # noqa: E402
import refio  # noqa: E402

GOLD = Path(__file__).resolve().parent
EXTRA = ("10X/Extend", "paths/long/large/GapToyTools3", "paths/long/large/GapToyTools4")
ENDL_LINES = (717, 734, 742, 760)
HAND = {"hand_k48": 48, "hand_k60": 60}
PER_CASE = ("n_quality_extended", "n_ambiguous", "n_cut_to_first", "n_exact_extended")      # each at 1 or more in some golden case


def build_driver(work: Path) -> Path:
    make_a48_golden.build_driver(work)
    refwork = work / "refwork"
    ov = refwork / "overlay"
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++11", "-fpermissive", "-fopenmp", "-fno-strict-aliasing", "-w", make_a48_golden.OPT, "-DNDEBUG", "-ffunction-sections", "-fdata-sections", f"-I{ov}"]
    # the in-flight edit, in the overlay only
    g4 = ov / "paths/long/large/GapToyTools4.cc"
    if g4.is_symlink():
        lines = g4.read_text().split("\n")
        for n in ENDL_LINES:
            assert lines[n - 1].rstrip().endswith("<< std::cout;"), (n, lines[n - 1])
            lines[n - 1] = lines[n - 1].replace("<< std::cout;", "<< std::endl;")
        os.chmod(g4.parent, 0o755)
        g4.unlink()
        g4.write_text("\n".join(lines))
    objs = []
    for rel in EXTRA:
        obj = work / ("ext_" + rel.replace("/", "_") + ".o")
        objs.append(obj)
        if not obj.exists():
            subprocess.run([cxx, *flags, "-D_GLIBCXX_ALIGN_H=1", "-c", str(ov / (rel + ".cc")), "-o", str(obj)], check=True)
    exe, src = work / "ext_driver", GOLD / "ext_driver.cc"
    if not exe.exists() or exe.stat().st_mtime < src.stat().st_mtime:
        obj = work / "ext_driver.o"
        subprocess.run([cxx, *flags, "-D_GLIBCXX_ALIGN_H=1", "-c", str(src), "-o", str(obj)], check=True)
        subprocess.run([cxx, "-fopenmp", "-Wl,--gc-sections", "-o", str(exe), str(obj), *map(str, objs), str(refwork / "obj" / "LinkTimestamp.o"), str(refwork / "libref.a"),
                        "-lz", "-lpthread"], check=True)
    return exe


def paths_bytes(offset, n_edges, edges, td: Path) -> bytes:
    """the feudal paths file of these paths (snk_write_paths: byte for byte what pathReads writes)"""
    from supernova_amd import lib as _lib
    offset, n_edges, edges = np.ascontiguousarray(offset, np.int32), np.ascontiguousarray(n_edges, np.uint32), np.ascontiguousarray(edges, np.int32)
    err = C.create_string_buffer(512)
    rc = _lib.load().snk_write_paths(str(td / "w.paths").encode(), len(n_edges), offset.ctypes.data, n_edges.ctypes.data, None, edges.ctypes.data, err, 512)
    assert rc == 0, err.value
    return (td / "w.paths").read_bytes()


def run_reference(exe: Path, td: Path, reads: dict, a_hbv: bytes, a_inv: bytes, in_paths: bytes):
    """-> ({flag: a.pathsX bytes}, summary line of flag 0 | flag 1)"""
    refio.write_snkrd(td / "in.snkrd", reads["lens"], reads["ascii"], reads["quals"])
    (td / "a.hbv").write_bytes(a_hbv)
    (td / "a.inv").write_bytes(a_inv)
    (td / "in.paths").write_bytes(in_paths)
    out, lines = {}, []
    for back in (0, 1):
        got = {}
        for th in (1, 8):
            r = subprocess.run([str(exe), str(td / "in.snkrd"), str(td / "a.hbv"), str(td / "a.inv"), str(td / "in.paths"), str(back), str(td / "out.pathsX")],
                               check=True, capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(th)))
            got[th] = (td / "out.pathsX").read_bytes()
            if th == 1:
                lines.append([l for l in r.stdout.splitlines() if l.startswith("EXT_DRIVER")][-1])
        assert got[1] == got[8], f"BACK_EXTEND {back}: 1 and 8 threads give different bytes"
        out[back] = got[1]
    return out, " | ".join(lines)


def restate(g, eb, reads, paths, per_read=None):
    """the restatement's bytes and counters per flag"""
    out = {}
    for back in (0, 1):
        pr = [] if per_read is not None else None
        o, n, e, cnt = extref.extend(g, reads["codes"], reads["lens"], reads["quals"], *paths, bool(back), eb, pr)
        idx, data, _ = a48xref.zip_paths(o, n, e, g)
        out[back] = (a48xref.pathsx_bytes(idx, data, len(n)), cnt)
        if per_read is not None:
            per_read.append((pr, n))
    return out


def save(name, in_paths, ref, line, extra=None):
    out = GOLD / "ext" / f"{name}.npz"
    u8 = lambda b: np.frombuffer(b, dtype=np.uint8)
    np.savez_compressed(out, in_paths=u8(in_paths), pathsx0=u8(ref[0]), pathsx1=u8(ref[1]), ref_summary=u8(line.encode()), **{k: u8(v) for k, v in (extra or {}).items()})
    limit = max(p.stat().st_size for p in (GOLD / "a48").glob("*.npz"))
    assert out.stat().st_size <= limit, f"{out.name}: {out.stat().st_size} B, the largest fixture under a48/ has {limit}"
    print(f"{name}: {line} -> {out.name} ({out.stat().st_size / 1024:.0f} KiB)")


def golden_cases(exe: Path, work: Path, names):
    seen = dict.fromkeys(PER_CASE, 0)
    for name in names:
        c = goldens.load(name)
        g = a48xref.parse_hbv(c.exp_ahbv)
        eb = extref.edge_bases(g)
        ascii_ = np.frombuffer(b"ACGT", np.uint8)[c.codes]
        p0 = extref.golden_input(a48xref.parse_paths(a48ref.load(name)["tmp.paths"]))
        n = len(p0[1])
        reads = dict(lens=c.lens[:n], ascii=ascii_[:n], quals=c.quals[:n], codes=c.codes[:n])
        base_ref = None
        variants = [("", p0)]
        if (p0[1] >= 2).any():
            variants += [("_cut", extref.cut_first_edge(g, eb, *p0)), ("_first", extref.first_edge_only(*p0))]
        assert set(name + t for t, _ in variants) == set(x for x in extref.ALL if x == name or x in (name + "_cut", name + "_first")), "extref.ALL and the cases made differ"
        for tag, paths in variants:
            with tempfile.TemporaryDirectory(dir=work) as td:
                td = Path(td)
                in_paths = paths_bytes(*paths, td)
                ref, line = run_reference(exe, td, reads, c.exp_ahbv, c.exp_ainv, in_paths)
            mine = restate(g, eb, reads, paths)
            for back in (0, 1):
                assert mine[back][0] == ref[back], f"{name}{tag}: the restatement does not reproduce the reference's bytes (BACK_EXTEND {back})"
            if not tag:
                base_ref = ref
                for k in PER_CASE:
                    seen[k] += mine[0][1][k]
            elif tag == "_cut":
                assert mine[1][1]["n_back_extended"] >= 1 and ref[0] != ref[1], f"{name}_cut: the backward leg does not run"
            else:
                assert ref[0] == base_ref[0], f"{name}_first: leg 2 must not depend on what follows the first edge"
            save(name + tag, in_paths, ref, line + " | restatement " + " ".join(f"{k}={mine[0][1][k]}/{mine[1][1][k]}" for k in extref.COUNTERS))
    if set(names) == set(goldens.CASES):
        assert all(v >= 1 for v in seen.values()), f"a counter no golden case raises: {seen}"


def hand_case(exe: Path, work: Path, name: str):
    from supernova_amd import graphio
    K = HAND[name]
    c = handext.case(K)
    with tempfile.TemporaryDirectory(dir=work) as td:
        td = Path(td)
        graphio.write_hbv(td / "g.hbv", td / "g.inv", K, c.off, c.bases)
        a_hbv, a_inv = (td / "g.hbv").read_bytes(), (td / "g.inv").read_bytes()
        g = a48xref.parse_hbv(a_hbv)
        eb = extref.edge_bases(g)
        codes, quals, lens, paths = handext.arrays(c, handext.edge_index(eb))
        reads = dict(lens=lens, ascii=np.frombuffer(b"ACGT", np.uint8)[codes], quals=quals, codes=codes)
        in_paths = paths_bytes(*paths, td)
        ref, line = run_reference(exe, td, reads, a_hbv, a_inv, in_paths)
    per_read = []
    mine = restate(g, eb, reads, paths, per_read)
    for back in (0, 1):
        assert mine[back][0] == ref[back], f"{name}: the restatement does not reproduce the reference's bytes (BACK_EXTEND {back})"
        hits, n_out = per_read[back]
        for i, r in enumerate(c.reads):
            assert hits[i] == r.hits[back] and n_out[i] == r.n_out[back], (name, r.name, back, sorted(hits[i]), int(n_out[i]))
    assert mine[0][1]["n_too_many"] >= 1
    save(name, in_paths, ref, line, dict(a_hbv=a_hbv, a_inv=a_inv))


def main(argv: list[str]) -> None:
    work, names = None, []
    it = iter(argv)
    for a in it:
        if a == "--work":
            work = Path(next(it)).resolve()
        else:
            names.append(a)
    keep = work is not None
    work = work or Path(tempfile.mkdtemp(prefix="snk_ext."))
    work.mkdir(parents=True, exist_ok=True)
    try:
        exe = build_driver(work)
        (GOLD / "ext").mkdir(exist_ok=True)
        names = names or list(goldens.CASES) + list(HAND)
        golden_cases(exe, work, [n for n in names if n not in HAND])
        for n in names:
            if n in HAND:
                hand_case(exe, work, n)
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:])
