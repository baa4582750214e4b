#!/usr/bin/env python3
"""Generate tests/golden/mow/<case>.npz: what the REFERENCE's own MowLawn (10X/Lawnmower.cc:301-554, the ReadPathVecX overload) leaves,
behind its own MarkDups version 2 (10X/SecretOps.cc:599), for the inputs of tests/mowgen.py's cases.

Run by hand where the reference's sources can be read.  make_bads_golden.build_driver makes libref.a and the patched-header overlay in a
scratch directory; 10X/Lawnmower.cc is compiled there from the overlay and mow_driver.cc (next to this file) is linked with it; nothing
compiled is kept.  The maker writes the reads, a.hbv, a.inv and the paths with the project's own writers; the two files MowLawn opens by
name -- a.paths.inv and the .qualp -- are written by the driver with the reference's own writers.  Every run goes with 1 and with 8
OpenMP threads and both must give the same bytes.  One run has an empty `tests` list (dels, the way StageTrim calls it), one names every
edge in `tests`, which takes the one-thread branch and prints (e1, e2, qss1, qss2) of every candidate that passed the read limit; the
two must agree on dels.  Before a case is saved both forms of the Python restatement (tests/mowref.py) must reproduce dels and scored.

Cases: hand_k48 / hand_k60 (tests/handmow.py: every motif's stated outcome is asserted against the reference), wide_k48, fuzz_<seed> for
mowgen.FUZZ_SEEDS (over them every outcome must occur: deleted, refused by the read limit, by qss1, by qss2, a void group, a read the
quality filter excludes), and the five K = 48 golden graphs on their own paths.

A fixture holds dup (the reference's: an INPUT of the call under test), dels, scored, ref_summary, input_digest (mowref.digest) and for
the generated graphs a_hbv.

usage: python tests/golden/make_mow_golden.py [--work DIR] [case ...]
"""
from __future__ import annotations

import os
import re
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

import editref  # noqa: E402
import make_a48_golden  # noqa: E402
import make_bads_golden  # noqa: E402
import make_ext_golden  # noqa: E402
import mowgen  # noqa: E402
import mowref  # noqa: E402
import refio  # noqa: E402

GOLD = Path(__file__).resolve().parent
PRINT4 = re.compile(r"^e1 = (-?\d+), e2 = (-?\d+), qss1 = (-?\d+), qss2 = (-?\d+)$")


def build_driver(work: Path) -> Path:
    make_bads_golden.build_driver(work)
    refwork = work / "refwork"
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++11", "-fpermissive", "-fopenmp", "-fno-strict-aliasing", "-w", make_a48_golden.OPT, "-DNDEBUG", "-ffunction-sections", "-fdata-sections",
             f"-I{refwork / 'overlay'}", "-D_GLIBCXX_ALIGN_H=1"]
    lawn = work / "mow_10X_Lawnmower.o"
    if not lawn.exists():
        subprocess.run([cxx, *flags, "-c", str(refwork / "overlay" / "10X" / "Lawnmower.cc"), "-o", str(lawn)], check=True)
    exe, src = work / "mow_driver", GOLD / "mow_driver.cc"
    if not exe.exists() or exe.stat().st_mtime < src.stat().st_mtime:
        obj = work / "mow_driver.o"
        subprocess.run([cxx, *flags, "-c", str(src), "-o", str(obj)], check=True)
        ext = [str(work / ("ext_" + rel.replace("/", "_") + ".o")) for rel in make_ext_golden.EXTRA]
        subprocess.run([cxx, "-fopenmp", "-Wl,--gc-sections", "-o", str(exe), str(obj), str(lawn), *ext, str(refwork / "obj" / "LinkTimestamp.o"), str(refwork / "libref.a"),
                        "-lz", "-lpthread"], check=True)
    return exe


def run_reference(exe: Path, td: Path, c):
    """-> (dup, dels, scored, summary line)"""
    refio.write_snkrd(td / "in.snkrd", c.lens, np.frombuffer(b"ACGT", np.uint8)[c.codes], c.quals, c.bc)
    (td / "a.hbv").write_bytes(c.a_hbv)
    (td / "a.inv").write_bytes(editref.inv_bytes(c.inv))
    (td / "in.paths").write_bytes(make_ext_golden.paths_bytes(*c.paths, td))
    got, line = {}, None
    for th in (1, 8):
        for all_tests in (0, 1):
            w = td / f"w{th}{all_tests}"
            w.mkdir()
            r = subprocess.run([str(exe), str(td / "in.snkrd"), str(td / "a.hbv"), str(td / "a.inv"), str(td / "in.paths"), str(w), str(all_tests), str(w / "dup"),
                                str(w / "dels")], check=True, capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(th)))
            scored = sorted((tuple(map(int, m.groups())) for m in map(PRINT4.match, r.stdout.splitlines()) if m), key=lambda s: (s[1], s[0]))
            got[(th, all_tests)] = ((w / "dup").read_bytes(), (w / "dels").read_bytes(), scored)
            if th == 1 and all_tests == 1:
                line = [l for l in r.stdout.splitlines() if l.startswith("MOW_DRIVER")][-1]
            shutil.rmtree(w)
    for all_tests in (0, 1):
        assert got[(1, all_tests)] == got[(8, all_tests)], "1 and 8 threads give different output"
    assert got[(1, 0)][:2] == got[(1, 1)][:2], "the run with every edge in `tests` deletes other edges than the run without"
    assert not got[(1, 0)][2], "PRINT4 lines without a tests list"
    dup, dels, scored = got[(1, 1)]
    return (make_bads_golden.bool_vec(dup), np.asarray([int(x) for x in dels.split()], np.int32), np.asarray(scored, np.int32).reshape(-1, 4), line)


def outcomes(c, dup, dels, scored):
    """per stated motif what the reference did: "deleted", "kept", "limit" or "none" """
    from mowref import candidates
    kmers = np.array([len(b) - c.K + 1 for b in c.eb])
    cands = {(e1, e2) for _, e1, e2 in candidates(c.g, kmers)}
    rows = {(int(r[0]), int(r[1])): (int(r[2]), int(r[3])) for r in scored}
    out = {}
    for m in c.motifs:
        k = (c.edge_of[m.e1], c.edge_of[m.e2])
        out[m.name] = ("none", None) if k not in cands else ("limit", None) if k not in rows else ("deleted" if k[1] in set(dels.tolist()) else "kept", rows[k])
    return out


def make_case(exe: Path, work: Path, name: str, seen: dict):
    c = mowgen.inputs(name)
    with tempfile.TemporaryDirectory(dir=work) as td:
        dup, dels, scored, line = run_reference(exe, Path(td), c)
    detail: dict = {}
    d2, s2, cnt = mowref.mow_entries(c.g, c.eb, c.inv, c.codes, c.lens, c.quals, *c.paths, dup, detail)
    assert np.array_equal(d2, dels) and np.array_equal(s2, scored), f"{name}: the restatement from path entries does not reproduce the reference"
    d1, s1 = mowref.mow_literal(c.g, c.eb, c.inv, c.codes, c.lens, c.quals, *c.paths, dup)
    assert np.array_equal(d1, dels) and np.array_equal(s1, scored), f"{name}: the literal restatement does not reproduce the reference"
    if c.motifs is not None:
        for m in c.motifs:
            got, qss = outcomes(c, dup, dels, scored)[m.name]
            if m.outcome is not None:
                assert got == m.outcome, f"{name}: motif {m.name} is stated {m.outcome}, the reference says {got} {qss}"
            if m.qss is not None:
                assert qss == tuple(m.qss), f"{name}: motif {m.name} is stated {m.qss}, the reference says {qss}"
    for r in scored:
        seen["deleted" if r[2] >= 300 and r[3] <= 30 else "qss1" if r[2] < 300 else "qss2"] += 1
    seen["limit"] += cnt["n_too_many_reads"]
    seen["void_group"] += cnt["n_groups_mixed_sign"]
    seen["hq_excluded"] += cnt["n_reads_hq_excluded"]
    seen["dup_pairs"] += int(dup.sum())
    mine = mowgen.dup_of(c)
    line += f" | dup equals MarkDups version 1 as restated: {bool(np.array_equal(mine, dup))} | restatement {cnt}"
    out = GOLD / "mow" / f"{name}.npz"
    u8 = lambda b: np.frombuffer(b, dtype=np.uint8)
    c.dup = dup
    extra = {} if name in mowgen.GOLDEN else {"a_hbv": u8(c.a_hbv)}
    np.savez_compressed(out, dup=dup, dels=dels, scored=scored, ref_summary=u8(line.encode()), input_digest=u8(mowref.digest(c).encode()), **extra)
    limit = max(p.stat().st_size for p in (GOLD / "a48").glob("*.npz"))
    assert out.stat().st_size <= limit, f"{out.name}: {out.stat().st_size} B, the largest fixture under a48/ has {limit}"
    print(f"{name}: {line} -> {out.name} ({out.stat().st_size / 1024:.1f} KiB)")


def main(argv: list[str]) -> None:
    work, names = None, []
    it = iter(argv)
    for a in it:
        if a == "--work":
            work = Path(next(it)).resolve()
        else:
            names.append(a)
    keep = work is not None
    work = work or Path(tempfile.mkdtemp(prefix="snk_mow."))
    work.mkdir(parents=True, exist_ok=True)
    fuzz = [f"fuzz_{s}" for s in mowgen.FUZZ_SEEDS]
    try:
        exe = build_driver(work)
        (GOLD / "mow").mkdir(exist_ok=True)
        names = names or list(mowgen.HAND) + [mowgen.WIDE] + fuzz + list(mowgen.GOLDEN)
        seen = dict.fromkeys(("deleted", "limit", "qss1", "qss2", "void_group", "hq_excluded", "dup_pairs"), 0)
        for n in names:
            if n in fuzz:
                make_case(exe, work, n, seen)
        print("fuzz seeds, outcomes:", seen)
        if set(fuzz) <= set(names):
            assert all(v >= 1 for v in seen.values()), f"an outcome that no fuzz seed gives: {seen}"
        other = dict.fromkeys(seen, 0)
        for n in names:
            if n not in fuzz:
                make_case(exe, work, n, other)
        print("the other cases, outcomes:", other)
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:])
