#!/usr/bin/env python3
"""Generate tests/golden/bads/<case>.npz: the pair flags both overloads of the REFERENCE's MarkBads (10X/SecretOps.cc:22-59, :70-107)
leave for the inputs of tests/badsref.py's cases.

Run by hand where the reference's sources can be read.  make_ext_golden.build_driver makes libref.a (10X/SecretOps is part of its
closure) and the patched-header overlay in a scratch directory; bads_driver.cc (next to this file) is compiled there and linked;
nothing compiled is kept.  Every run goes with 1 and with 8 OpenMP threads and both must give the same bytes.  Before a case is saved
the Python restatement (tests/badsref.py) must reproduce the reference's flags in both modes.

Cases:
  the five K=48 golden cases on the reference's own paths, cut to extref.golden_input, and `<case>_cut`: the first edge of every path of
      two or more edges dropped while the offset stays, so those reads are compared out of place.  Over these, both flag values must
      occur in both modes
  synth_20k_err_far: the pairs of synth_20k_err that golden_input takes out -- an offset outside +-32767 on the 33 kb edge -- so
      n_offsets_wrapped >= 1.  Every such offset lies in (32767, 33 k] and wraps to a NEGATIVE one below minus the read's length, so the
      ReadPathVecX overload skips every position of these reads: its flags equal the ReadPath overload's (no pair is bad in either)
      and what differs is the number of reads with a mismatch inside m, which is asserted.  Flags that differ between the modes
      come from the hand-made long edge (asserted there)
  hand_k48 / hand_k60: tests/handbads.py; every pair's stated flags are asserted against the reference
  handplain_k48 / handplain_k60: the pairs whose paths a ReadPathVecX cannot hold: the ReadPath overload only

A fixture holds bad_plain and bad_x (u8 per pair), ref_summary, input_digest (badsref.digest: reads, paths and graph) and for the
hand-made cases a_hbv.

usage: python tests/golden/make_bads_golden.py [--work DIR] [case ...]
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import a48ref  # noqa: E402
import a48xref  # noqa: E402
import badsref  # noqa: E402
import extref  # noqa: E402
import goldens  # noqa: E402
import handbads  # noqa: E402
import make_a48_golden  # noqa: E402
import make_ext_golden  # noqa: E402
import refio  # noqa: E402

GOLD = Path(__file__).resolve().parent


def build_driver(work: Path) -> Path:
    make_ext_golden.build_driver(work)
    refwork = work / "refwork"
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++11", "-fpermissive", "-fopenmp", "-fno-strict-aliasing", "-w", make_a48_golden.OPT, "-DNDEBUG", "-ffunction-sections", "-fdata-sections",
             f"-I{refwork / 'overlay'}"]
    exe, src = work / "bads_driver", GOLD / "bads_driver.cc"
    if not exe.exists() or exe.stat().st_mtime < src.stat().st_mtime:
        obj = work / "bads_driver.o"
        subprocess.run([cxx, *flags, "-D_GLIBCXX_ALIGN_H=1", "-c", str(src), "-o", str(obj)], check=True)
        subprocess.run([cxx, "-fopenmp", "-Wl,--gc-sections", "-o", str(exe), str(obj), str(refwork / "obj" / "LinkTimestamp.o"), str(refwork / "libref.a"), "-lz", "-lpthread"],
                       check=True)
    return exe


def bool_vec(b: bytes) -> np.ndarray:
    """BinaryWriter::writeFile(vec<Bool>): "BINWRITE", u64 count, one byte each"""
    assert b[:8] == b"BINWRITE"
    n = int(np.frombuffer(b, "<u8", 1, 8)[0])
    assert len(b) == 16 + n
    return np.frombuffer(b, np.uint8, n, 16).copy()


def run_reference(exe: Path, td: Path, c, a_hbv: bytes, modes: int):
    """-> (bad_plain or None, bad_x or None, summary line)"""
    ascii_ = np.frombuffer(b"ACGT", np.uint8)[c.codes]
    refio.write_snkrd(td / "in.snkrd", c.lens, ascii_, c.quals)
    (td / "a.hbv").write_bytes(a_hbv)
    (td / "in.paths").write_bytes(make_ext_golden.paths_bytes(*c.paths, td))
    got, line = {}, None
    for th in (1, 8):
        for p in (td / "bad_plain", td / "bad_x"):
            p.unlink(missing_ok=True)
        r = subprocess.run([str(exe), str(td / "in.snkrd"), str(td / "a.hbv"), str(td / "in.paths"), str(modes), str(td / "bad_plain"), str(td / "bad_x")],
                           check=True, capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(th)))
        got[th] = tuple((td / f).read_bytes() if (td / f).exists() else None for f in ("bad_plain", "bad_x"))
        if th == 1:
            line = [l for l in r.stdout.splitlines() if l.startswith("BADS_DRIVER")][-1]
    assert got[1] == got[8], "1 and 8 threads give different flags"
    return tuple(bool_vec(b) if b is not None else None for b in got[1]) + (line,)


def check_and_save(name, c, ref_plain, ref_x, line, extra=None):
    mine_plain, cnt = badsref.mark_bads(c.g, c.eb, c.codes, c.lens, c.quals, *c.paths, False)
    assert np.array_equal(mine_plain, ref_plain), f"{name}: the restatement does not reproduce the reference's flags (ReadPath)"
    cnt_x = None
    if ref_x is not None:
        mine_x, cnt_x = badsref.mark_bads(c.g, c.eb, c.codes, c.lens, c.quals, *c.paths, True)
        assert np.array_equal(mine_x, ref_x), f"{name}: the restatement does not reproduce the reference's flags (ReadPathVecX)"
    out = GOLD / "bads" / f"{name}.npz"
    u8 = lambda b: np.frombuffer(b, dtype=np.uint8)
    line += f" | restatement plain {cnt} x {cnt_x}"
    np.savez_compressed(out, bad_plain=ref_plain, bad_x=ref_x if ref_x is not None else np.zeros(0, np.uint8), ref_summary=u8(line.encode()),
                        input_digest=u8(badsref.digest(c).encode()), **{k: u8(v) for k, v in (extra or {}).items()})
    limit = max(p.stat().st_size for p in (GOLD / "a48").glob("*.npz"))
    assert out.stat().st_size <= limit, f"{out.name}: {out.stat().st_size} B, the largest fixture under a48/ has {limit}"
    print(f"{name}: {line} -> {out.name} ({out.stat().st_size / 1024:.1f} KiB)")
    return cnt, cnt_x


def golden_cases(exe: Path, work: Path, names):
    seen = {(m, v): 0 for m in ("plain", "x") for v in (0, 1)}
    for name in names:
        gc = goldens.load(name)
        g = a48xref.parse_hbv(gc.exp_ahbv)
        eb = extref.edge_bases(g)
        raw = a48xref.parse_paths(a48ref.load(name)["tmp.paths"])
        p0 = extref.golden_input(raw)
        variants = [(name, np.arange(len(p0[1])), p0), (name + "_cut", np.arange(len(p0[1])), badsref.cut_input(g, eb, *p0))]
        if name + "_far" == badsref.FAR:
            variants.append((badsref.FAR,) + badsref.far_input(raw, len(raw[1])))
        for vname, ids, paths in variants:
            c = SimpleNamespace(g=g, eb=eb, codes=gc.codes[ids], quals=gc.quals[ids], lens=gc.lens[ids], paths=paths)
            with tempfile.TemporaryDirectory(dir=work) as td:
                ref_plain, ref_x, line = run_reference(exe, Path(td), c, gc.exp_ahbv, 3)
            cnt, cnt_x = check_and_save(vname, c, ref_plain, ref_x, line)
            if vname == badsref.FAR:
                assert cnt_x["n_offsets_wrapped"] >= 1 and cnt["n_mismatch_reads"] != cnt_x["n_mismatch_reads"], "synth_20k_err_far: the two modes do not differ"
            else:
                for m, v in (("plain", ref_plain), ("x", ref_x)):
                    seen[(m, 1)] += int(v.sum())
                    seen[(m, 0)] += int(len(v) - v.sum())
    print("golden cases and their _cut variants, pairs per (mode, flag):", seen)
    if set(names) == set(goldens.CASES):
        assert all(v >= 1 for v in seen.values()), f"a flag value that no golden case gives: {seen}"


def hand_case(exe: Path, work: Path, name: str):
    from supernova_amd import graphio
    plain_only = name in badsref.HAND_PLAIN
    K = {**badsref.HAND, **badsref.HAND_PLAIN}[name]
    h = handbads.case(K, plain_only)
    with tempfile.TemporaryDirectory(dir=work) as td:
        td = Path(td)
        graphio.write_hbv(td / "g.hbv", td / "g.inv", K, h.off, h.bases)
        a_hbv = (td / "g.hbv").read_bytes()
        g = a48xref.parse_hbv(a_hbv)
        eb = extref.edge_bases(g)
        codes, quals, lens, paths = handbads.arrays(h, handbads.edge_index(eb))
        c = SimpleNamespace(g=g, eb=eb, codes=codes, quals=quals, lens=lens, paths=paths)
        ref_plain, ref_x, line = run_reference(exe, td, c, a_hbv, 1 if plain_only else 3)
    for i, p in enumerate(h.pairs):
        assert bool(ref_plain[i]) == p.plain, f"{name}: pair {p.name} is stated {p.plain} (ReadPath), the reference says {bool(ref_plain[i])}"
        if not plain_only:
            assert bool(ref_x[i]) == p.x, f"{name}: pair {p.name} is stated {p.x} (ReadPathVecX), the reference says {bool(ref_x[i])}"
    if not plain_only:
        assert not np.array_equal(ref_plain, ref_x), f"{name}: the two modes do not differ"
    check_and_save(name, c, ref_plain, ref_x, line, dict(a_hbv=a_hbv))


def main(argv: list[str]) -> None:
    work, names = None, []
    it = iter(argv)
    for a in it:
        if a == "--work":
            work = Path(next(it)).resolve()
        else:
            names.append(a)
    keep = work is not None
    work = work or Path(tempfile.mkdtemp(prefix="snk_bads."))
    work.mkdir(parents=True, exist_ok=True)
    hands = {**badsref.HAND, **badsref.HAND_PLAIN}
    try:
        exe = build_driver(work)
        (GOLD / "bads").mkdir(exist_ok=True)
        names = names or list(goldens.CASES) + list(hands)
        golden_cases(exe, work, [n for n in names if n not in hands])
        for n in names:
            if n in hands:
                hand_case(exe, work, n)
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:])
