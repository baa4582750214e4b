#!/usr/bin/env python3
"""Generate tests/golden/hops/<case>.npz: the edge pairs, and the a.hops bytes, that the REFERENCE's FindEdgePairs
(10X/Closomatic.cc:17-354) leaves for the inputs of tests/hopsref.py's cases, with ONE_GOOD False and True.

Run by hand where the reference's sources can be read.  make_ext_golden.build_driver makes libref.a and the patched-header overlay in a
scratch directory; 10X/Closomatic is compiled there as one more object, hops_driver.cc (next to this file) is compiled and linked;
nothing compiled is kept.  The driver is fed a.hbx, a.pathsX and a.paths.inv written by this library's own writers (byte-equal to the
reference's), and one BAR_10X dataset.  Every run goes with 1 and with 8 OpenMP threads and both must give the same bytes.  Before a
case is saved the Python restatement (tests/hopsref.py) must reproduce the reference's pairs for both flags.

Cases:
  the five K=48 golden cases on the reference's own paths, cut to extref.golden_input, bad = the bad_x of tests/golden/bads/
  gapped: the synthetic genome with holes of 50-250 bases cut out of the coverage (every pair with a read that touches a hole is
      dropped), so that the graph breaks into dead-ended contigs that pairs of several barcodes span; graph and paths are the reference's
      own (oracle/ref), bad the restatement's MarkBads (tests/badsref.py) in ReadPathVecX mode
  hand_k48 / hand_k60: tests/handhops.py; every item's stated outcome is asserted against the reference
Over the golden and generated cases, and again over the hand-made ones, every part must give a pair that no other part gives, and the two
flag settings must differ somewhere.

A fixture holds pairs / pairs_one_good, hops / hops_one_good (the file bytes), counts / counts_one_good (hopsref.COUNTERS, from the
restatement), only (pairs each part alone gave), ref_summary (with the reference's wall time), input_digest, and for the generated and
hand-made cases their input.

usage: python tests/golden/make_hops_golden.py [--work DIR] [case ...]
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

import a48xref  # noqa: E402
import extref  # noqa: E402
import goldens  # noqa: E402
import hopsref  # noqa: E402
import make_a48_golden  # noqa: E402
import make_ext_golden  # noqa: E402

GOLD = Path(__file__).resolve().parent


def build_driver(work: Path) -> Path:
    make_ext_golden.build_driver(work)
    refwork = work / "refwork"
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++11", "-fpermissive", "-fopenmp", "-fno-strict-aliasing", "-w", make_a48_golden.OPT, "-DNDEBUG", "-ffunction-sections", "-fdata-sections",
             f"-I{refwork / 'overlay'}", "-D_GLIBCXX_ALIGN_H=1"]
    clo = work / "hops_10X_Closomatic.o"
    if not clo.exists():
        subprocess.run([cxx, *flags, "-c", str(refwork / "overlay" / "10X" / "Closomatic.cc"), "-o", str(clo)], check=True)
    exe, src = work / "hops_driver", GOLD / "hops_driver.cc"
    if not exe.exists() or exe.stat().st_mtime < src.stat().st_mtime:
        obj = work / "hops_driver.o"
        subprocess.run([cxx, *flags, "-c", str(src), "-o", str(obj)], check=True)
        subprocess.run([cxx, "-fopenmp", "-Wl,--gc-sections", "-o", str(exe), str(obj), str(clo), str(refwork / "obj" / "LinkTimestamp.o"), str(refwork / "libref.a"),
                        "-lz", "-lpthread"], check=True)
    return exe


def pair_vec(b: bytes) -> np.ndarray:
    """BinaryWriter::writeFile(vec<pair<int,int>>) as the reference wrote it -> i32[n, 2].  The layout is read off the file: the magic,
    a u64 count, and what is left must be two ints per pair."""
    assert b[:8] == b"BINWRITE"
    n = int(np.frombuffer(b, "<u8", 1, 8)[0])
    assert len(b) == 16 + 8 * n, f"a.hops of {n} pairs has {len(b)} bytes"
    return np.frombuffer(b, "<i4", 2 * n, 16).reshape(-1, 2).copy()


def run_reference(exe: Path, td: Path, c):
    """-> ({one_good: a.hops bytes}, summary line)"""
    from supernova_amd import graphio
    off, bases = graphio.unitigs_to_arrays(c.unitigs)
    graphio.write_hbx(td / "a.hbx", c.K, off, bases)
    assert (td / "a.hbx").read_bytes() == a48xref.hbx_bytes(c.g), "a.hbx of the unitigs is not the graph of a.hbv"
    (td / "a.inv").write_bytes(c.a_inv)
    index, data, _ = a48xref.zip_paths(*c.paths, c.g)
    graphio.write_pathsx(td / "a.pathsX", index, data, len(c.paths[1]))
    pidx = hopsref.paths_index(c.paths[1], c.paths[2], c.g.E)
    ioff = np.concatenate([[0], np.cumsum([len(x) for x in pidx])]).astype(np.uint64)
    ids = (np.concatenate(pidx) if len(pidx) else np.zeros(0)).astype(np.uint64)
    graphio.write_paths_index(td / "a.paths.inv", None, ioff, ids, np.zeros(c.g.E, np.int32))
    bc = np.ascontiguousarray(c.bc, dtype="<i4")
    (td / "in.bc").write_bytes(b"BINWRITE" + np.uint64(len(bc)).tobytes() + bc.tobytes())
    graphio.write_bad(td / "in.bad", c.bad)
    out, lines = {}, []
    for og in (0, 1):
        got = {}
        for th in (1, 8):
            (td / "out.hops").unlink(missing_ok=True)
            r = subprocess.run([str(exe), *(str(td / f) for f in ("a.hbx", "a.inv", "a.pathsX", "a.paths.inv", "in.bc", "in.bad")), str(og), str(td / "out.hops")],
                               check=True, capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(th)))
            got[th] = (td / "out.hops").read_bytes()
            if th == 1:
                lines.append([l for l in r.stdout.splitlines() if l.startswith("HOPS_DRIVER")][-1])
        assert got[1] == got[8], f"ONE_GOOD {og}: 1 and 8 threads give different bytes"
        out[og] = got[1]
    return out, " | ".join(lines)


def check_and_save(name, c, ref, line, extra=None):
    """-> the restatement's info per flag"""
    infos = {}
    for og in (0, 1):
        want = pair_vec(ref[og])
        mine, infos[og] = hopsref.find_edge_pairs(c.g, c.km, c.inv, c.paths[1], c.paths[2], c.bc, c.bad, bool(og))
        assert np.array_equal(mine, want), f"{name}: the restatement does not reproduce the reference's pairs (ONE_GOOD {og}): {len(mine)} against {len(want)}"
        assert hopsref.hops_bytes(mine) == ref[og], f"{name}: the bytes of a.hops are not magic, count, two ints per pair"
    out = GOLD / "hops" / f"{name}.npz"
    u8 = lambda b: np.frombuffer(b, dtype=np.uint8)
    counts = lambda og: np.array([infos[og][k] for k in hopsref.COUNTERS], np.int64)
    only = np.array([len(hopsref.only_part(infos[0], k)) for k in range(3)], np.int64)
    np.savez_compressed(out, pairs=pair_vec(ref[0]), pairs_one_good=pair_vec(ref[1]), hops=u8(ref[0]), hops_one_good=u8(ref[1]), counts=counts(0), counts_one_good=counts(1),
                        only=only, ref_summary=u8(line.encode()), input_digest=u8(hopsref.digest(c).encode()), **(extra or {}))
    limit = max(p.stat().st_size for p in (GOLD / "a48").glob("*.npz"))
    assert out.stat().st_size <= limit, f"{out.name}: {out.stat().st_size} B, the largest fixture under a48/ has {limit}"
    print(f"{name}: {line} | restatement {dict(zip(hopsref.COUNTERS, counts(0).tolist()))} only {only.tolist()} -> {out.name} ({out.stat().st_size / 1024:.1f} KiB)")
    return infos


def gapped_input(work: Path):
    """reads of the synthetic genome without the pairs that touch a coverage hole, pathed by the reference"""
    import badsref
    import refio
    rng = np.random.default_rng(20261020)
    G, n_pairs, L, insert = 24000, 9000, 150, 420
    genome = rng.integers(0, 4, G, dtype=np.uint8)
    holes, at = [], 1500
    while at < G - 1500:
        w = int(rng.integers(50, 251))
        holes.append((at, at + w))
        at += w + int(rng.integers(1200, 2600))
    comp = lambda s: (3 - s)[::-1]
    reads, bcs = [], []
    for _ in range(n_pairs):
        a = int(rng.integers(0, G - insert))
        frag = genome[a:a + insert] if rng.random() < 0.5 else comp(genome[a:a + insert])
        spans = [(a, a + L), (a + insert - L, a + insert)]
        if any(s < h1 and h0 < e for s, e in spans for h0, h1 in holes):
            continue
        reads += [frag[:L], comp(frag)[:L]]
        b = int(rng.integers(1, 41))                 # 40 barcodes: a gap is spanned by pairs of several
        bcs += [b, b]
    order = np.argsort(np.array(bcs[::2]), kind="stable")          # barcoded reads come sorted by barcode
    codes = np.stack(reads).reshape(-1, 2, L)[order].reshape(-1, L)
    bc = np.array(bcs, np.int32).reshape(-1, 2)[order].reshape(-1)
    n = len(codes)
    quals = np.full((n, L), 35, np.uint8)
    lens = np.full(n, L, np.uint16)
    ascii_ = np.frombuffer(b"ACGT", np.uint8)[codes]
    with tempfile.TemporaryDirectory(dir=work) as td:
        td = Path(td)
        refio.write_snkrd(td / "in.snkrd", lens, ascii_, quals, bc, 0)
        if not refio.REF_DRIVER.exists():
            refio.REF_DRIVER = work / "oracle" / "_ref" / "snref_driver"          # (make_a48_golden.build_driver built it there)
        refio.run_ref(td / "in.snkrd", td / "out")
        a_hbv, a_inv, tmp_paths = ((td / "out" / f).read_bytes() for f in ("a.hbv", "a.inv", "tmp.paths"))
        unitigs = (td / "out" / "unitigs.txt").read_text().split() if (td / "out" / "unitigs.txt").exists() else None
    c = SimpleNamespace(name="gapped", a_hbv=a_hbv, a_inv=a_inv, g=a48xref.parse_hbv(a_hbv), bc=bc)
    c.eb = extref.edge_bases(c.g)
    c.unitigs = unitigs or unitigs_of(c.eb, c.g.K)
    c.paths = a48xref.parse_paths(tmp_paths)
    c.bad, _ = badsref.mark_bads(c.g, c.eb, codes, lens, quals, *c.paths, True)
    return hopsref._finish(c)


def unitigs_of(eb, K):
    """the canonical unitigs in BVComp order from the edges' bases"""
    s = set()
    for b in eb:
        t = "".join("ACGT"[x] for x in b)
        r = t.translate(str.maketrans("ACGT", "TGCA"))[::-1]
        s.add(min(t, r))
    return sorted(s, key=lambda u: (-len(u), u))


def non_vacuous(label, infos):
    only = [sum(len(hopsref.only_part(i[0], k)) for i in infos) for k in range(3)]
    assert all(v >= 1 for v in only), f"{label}: a part that alone gives no pair: {only}"
    assert any(i[0]["parts"] != i[1]["parts"] for i in infos), f"{label}: ONE_GOOD changes nothing"
    print(f"{label}: pairs only part 1 / 2 / 3 gives: {only}")


def main(argv: list[str]) -> None:
    work, names = None, []
    it = iter(argv)
    for a in it:
        if a == "--work":
            work = Path(next(it)).resolve()
        else:
            names.append(a)
    keep = work is not None
    work = work or Path(tempfile.mkdtemp(prefix="snk_hops."))
    work.mkdir(parents=True, exist_ok=True)
    try:
        exe = build_driver(work)
        (GOLD / "hops").mkdir(exist_ok=True)
        full = not names
        names = names or list(hopsref.ALL)
        gen, hand = [], []
        for name in names:
            extra = None
            if name in hopsref.GOLDEN:
                c = hopsref.golden_input(name)
            elif name == "gapped":
                c = gapped_input(work)
                assert len(c.paths[1]) <= 20000
                u8 = lambda b: np.frombuffer(b, dtype=np.uint8)
                extra = dict(a_hbv=u8(c.a_hbv), a_inv=u8(c.a_inv), unitigs=u8("\n".join(c.unitigs).encode()), path_offset=c.paths[0], path_n_edges=c.paths[1],
                             path_edges=c.paths[2], bc=c.bc, bad=c.bad)
            else:
                import handhops
                from supernova_amd import graphio
                K = hopsref.HAND[name]
                h = handhops.case(K)
                with tempfile.TemporaryDirectory(dir=work) as td:
                    graphio.write_hbv(Path(td) / "g.hbv", Path(td) / "g.inv", K, h.off, h.bases)
                    a_hbv, a_inv = (Path(td) / "g.hbv").read_bytes(), (Path(td) / "g.inv").read_bytes()
                c = SimpleNamespace(name=name, a_hbv=a_hbv, a_inv=a_inv, g=a48xref.parse_hbv(a_hbv), unitigs=h.unitigs)
                c.eb = extref.edge_bases(c.g)
                c.paths, c.bc, c.bad = handhops.arrays(h, handhops.edge_index(c.eb))
                hopsref._finish(c)
                u8 = lambda b: np.frombuffer(b, dtype=np.uint8)
                extra = dict(a_hbv=u8(a_hbv), a_inv=u8(a_inv))
            with tempfile.TemporaryDirectory(dir=work) as td:
                ref, line = run_reference(exe, Path(td), c)
            if name in hopsref.HAND:
                import handhops
                handhops.assert_items(handhops.case(hopsref.HAND[name]), handhops.edge_index(c.eb), c.inv, {og: pair_vec(ref[og]) for og in (0, 1)}, "the reference")
            infos = check_and_save(name, c, ref, line, extra)
            (hand if name in hopsref.HAND else gen).append(infos)
        if full:
            non_vacuous("golden and generated cases", gen)
            non_vacuous("hand-made cases", hand)
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:])
