#!/usr/bin/env python3
"""Generate tests/golden/closures/<case>.npz: the closures, and the closures.fastb bytes, that the REFERENCE's CloseGap2 and CloseGap
(10X/Closomatic.cc:480-657 and :356-459) give for the pairs of the matching tests/golden/hops/ fixture (ONE_GOOD=False), run the way
StageFindPatch runs them with STACKSTER=False (10X/runstages/RunStages.cc:334-384).

Run by hand where the reference's sources can be read.  make_hops_golden.build_driver makes libref.a, the patched-header overlay and
10X/Closomatic.o in a scratch directory; five more objects (EXTRA) are compiled there, closures_driver.cc (next to this file) is compiled
and linked; nothing compiled is kept.  The driver is fed the reads, a.hbv, a.inv, the paths as a feudal file, a.paths.inv written by this
library's own writer and the fixture's a.hops.  Every run goes with 1 and with 8 OpenMP threads and both must give the same bytes.  Before
a case is saved the Python restatement (tests/closeref.py) must reproduce the reference's closures and pair_first for both flags.

Cases: the five K=48 golden cases and `gapped`, on the inputs of tests/hopsref.py (checked by its input_digest), the reads of `gapped`
made again from make_hops_golden's seed and checked against the fixture's barcodes; and `tandem` / `tandem_k60` (closeref.tandem_input, K = 48 and 60: tandem repeats
across the gap, a wide stack, a path that visits its edge twice, e1 == inv[e2], a side without rows), made from a seed, with pairs of its
own instead of a hops fixture; `tandem` also runs with max_width = 1 200 (<key>_wide), where the wide stack's consensus has 1000 columns or
more and gives nothing; hand_k48 / hand_k60 (tests/handclose.py): every item's stated closures -- CloseGap2, CloseGap, max_width 1 200 -- are asserted against
the reference by name, its filters against the restatement, and that only the long follower passes the default bod_budget.  Over all cases every counter and every filter of GetOffsets1 must move.

`fuzz` (or fuzz_<seed>) makes the fuzz_<seed> family: the pinned seeds closeref.FUZZ of the seeded generator tests/closegen.py, every one
at max_width 400 and 1 200.  Such a fixture holds results only -- fastb_<f>[_wide], pair_first_<f>[_wide], input_digest, ref_summary --:
the input is made again from the seed, and the digest says when the generator has drifted.

A fixture holds per flag (cg2, cg1) fastb_<f> (the file bytes: the closures are parsed from them), pair_first_<f>, counts_<f>
(closeref.COUNTERS, from the restatement) and filters_<f> (closeref.FILTERS); ref_summary (with the reference's wall time); input_digest (over
the hops fixture's input, the pairs, and the reads that the pairs' edges index with their mates).  No read is stored: those of the golden
cases are in tests/golden/<case>.npz, those of `gapped` come from closeref.gapped_reads.

usage: python tests/golden/make_closures_golden.py [--work DIR] [case ...]
"""
from __future__ import annotations

import io
import os
import re
import shutil
import subprocess
import sys
import tempfile
import zipfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import closeref  # noqa: E402
import goldens  # noqa: E402
import hopsref  # noqa: E402
import make_a48_golden  # noqa: E402
import make_ext_golden  # noqa: E402
import make_hops_golden  # noqa: E402
import refio  # noqa: E402

GOLD = Path(__file__).resolve().parent
EXTRA = ("paths/long/ReadStack", "kmers/KmerRecord", "random/Bernoulli", "PrintAlignment", "PackAlign")


def build_driver(work: Path) -> Path:
    make_hops_golden.build_driver(work)
    refwork = work / "refwork"
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++11", "-fpermissive", "-fopenmp", "-fno-strict-aliasing", "-w", make_a48_golden.OPT, "-DNDEBUG", "-ffunction-sections", "-fdata-sections",
             f"-I{refwork / 'overlay'}", "-D_GLIBCXX_ALIGN_H=1"]
    objs = [work / "hops_10X_Closomatic.o"]
    for rel in EXTRA:
        obj = work / ("clo_" + rel.replace("/", "_") + ".o")
        objs.append(obj)
        if not obj.exists():
            subprocess.run([cxx, *flags, "-c", str(refwork / "overlay" / (rel + ".cc")), "-o", str(obj)], check=True)
    exe, src = work / "closures_driver", GOLD / "closures_driver.cc"
    if not exe.exists() or exe.stat().st_mtime < src.stat().st_mtime:
        obj = work / "closures_driver.o"
        subprocess.run([cxx, *flags, "-c", str(src), "-o", str(obj)], check=True)
        subprocess.run([cxx, "-fopenmp", "-Wl,--gc-sections", "-o", str(exe), str(obj), *map(str, objs), str(refwork / "obj" / "LinkTimestamp.o"), str(refwork / "libref.a"),
                        "-lz", "-lpthread"], check=True)
    return exe


def case_reads(name: str, c):
    """-> (codes, quals, lens) of ALL reads of the case's paths"""
    n = len(c.paths[1])
    if name in closeref.GOLDEN:
        gc = goldens.load(name)
        return gc.codes[:n], gc.quals[:n], np.asarray(gc.lens[:n], np.uint16)
    codes, quals, lens, bc = closeref.gapped_reads()
    assert len(codes) == n and np.array_equal(bc, c.bc), "gapped: the reads made again are not those of the hops fixture"
    return codes, quals, lens


def run_reference(exe: Path, td: Path, c, codes, quals, lens, max_width: int = closeref.MAX_WIDTH):
    """-> ({flag: (fastb bytes, pair_first)}, summary line)"""
    from supernova_amd import graphio
    refio.write_snkrd(td / "in.snkrd", lens, np.frombuffer(b"ACGT", np.uint8)[codes], quals)
    (td / "a.hbv").write_bytes(c.a_hbv)
    (td / "a.inv").write_bytes(c.a_inv)
    (td / "in.paths").write_bytes(make_ext_golden.paths_bytes(*c.paths, td))
    pidx = hopsref.paths_index(c.paths[1], c.paths[2], c.g.E)
    ioff = np.concatenate([[0], np.cumsum([len(x) for x in pidx])]).astype(np.uint64)
    ids = (np.concatenate(pidx) if len(pidx) else np.zeros(0)).astype(np.uint64)
    graphio.write_paths_index(td / "a.paths.inv", None, ioff, ids, np.zeros(c.g.E, np.int32))
    (td / "in.hops").write_bytes(c.hops)
    out, lines = {}, []
    for flag, cg2 in (("cg2", 1), ("cg1", 0)):
        got = {}
        for th in (1, 8):
            for f in ("out.fastb", "out.first"):
                (td / f).unlink(missing_ok=True)
            r = subprocess.run([str(exe), *(str(td / f) for f in ("in.snkrd", "a.hbv", "a.inv", "in.paths", "a.paths.inv", "in.hops")), str(cg2), str(max_width),
                                str(td / "out.fastb"), str(td / "out.first")], check=True, capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(th)))
            got[th] = ((td / "out.fastb").read_bytes(), (td / "out.first").read_bytes())
            if th == 1:
                lines.append([l for l in r.stdout.splitlines() if l.startswith("CLOSURES_DRIVER")][-1])
        assert got[1] == got[8], f"{flag}: 1 and 8 threads give different bytes"
        out[flag] = (got[1][0], np.frombuffer(got[1][1], "<u8").copy())
    return out, " | ".join(lines)


def check_and_save(name, c, ref, line, reads, extra, wide=None):
    """-> {flag: (counters, filters)} of the restatement.  wide: the reference's result at closeref.WIDE columns, saved as <key>_wide"""
    I = closeref.Input(c.K, c.eb, c.inv, *c.paths, reads.codes, reads.quals, reads.lens, reads.ids)
    infos, save = {}, {}
    for flag, width, sfx in [(f, closeref.MAX_WIDTH, "") for f in closeref.FLAGS] + [(f, closeref.WIDE, "_wide") for f in closeref.FLAGS if wide]:
        fastb, first = (wide if sfx else ref)[flag]
        want_off, want_bases = closeref.parse_fastb(fastb)
        off, bases, pf, cnt, why = closeref.close_gaps(I, c.pairs, flag == "cg2", width)
        # every fixture but the hand-made long follower stays inside the default bod_budget: what n_place_host == 0 on the device rests on
        assert (why.get("bod_max", 0) > closeref.BOD_BUDGET) == (name == "hand_k48" and flag == "cg2"), f"{name} {flag}: {why.get('bod_max', 0)} 32-mers on a side"
        assert np.array_equal(pf, first), f"{name} {flag}: the restatement gives other closures per pair: {pf.tolist()} against {first.tolist()}"
        assert np.array_equal(off, want_off) and np.array_equal(bases, want_bases), f"{name} {flag}: the restatement does not reproduce the reference's closures"
        assert closeref.fastb_bytes(off, bases) == fastb, f"{name} {flag}: closures.fastb is not the layout of the unitig hand-off file"
        if sfx:
            assert cnt["n_cons_too_long"] >= 1 and len(want_off) > 1, f"{name} {flag}: at {width} columns no consensus is too long, or nothing closes: {cnt}"
            cnt400 = infos[flag][0]
            infos[flag] = ({**cnt400, "n_cons_too_long": cnt["n_cons_too_long"]}, infos[flag][1])
        else:
            infos[flag] = (cnt, why)
        save.update({f"fastb_{flag}{sfx}": np.frombuffer(fastb, np.uint8), f"pair_first_{flag}{sfx}": first,
                     f"counts_{flag}{sfx}": np.array([cnt[k] for k in closeref.COUNTERS], np.int64), f"filters_{flag}{sfx}": np.array([why[k] for k in closeref.FILTERS], np.int64)})
    out = GOLD / "closures" / f"{name}.npz"
    u8 = lambda b: np.frombuffer(b, dtype=np.uint8)
    np.savez_compressed(out, ref_summary=u8(line.encode()), input_digest=u8(closeref.digest(c, reads).encode()), **save, **extra)
    limit = max(p.stat().st_size for p in (GOLD / "a48").glob("*.npz"))
    assert out.stat().st_size <= limit, f"{out.name}: {out.stat().st_size} B, the largest fixture under a48/ has {limit}"
    print(f"{name}: {line} | restatement " + " | ".join(f"{f} {infos[f][0]} {infos[f][1]}" for f in closeref.FLAGS) + f" -> {out.name} ({out.stat().st_size / 1024:.1f} KiB)")
    return infos


def save_fuzz(exe: Path, work: Path, seed: int) -> None:
    """fuzz_<seed>.npz: the reference on closegen.make_case(seed) at both widths, the restatement asserted against it"""
    import closegen
    c = closegen.make_case(seed)
    assert c is not None, f"seed {seed} is skipped: its unitigs are no valid set"
    r = c.reads
    save, lines = {}, []
    with tempfile.TemporaryDirectory(dir=work) as td:
        for sfx, width in (("", closeref.MAX_WIDTH), ("_wide", closeref.WIDE)):
            ref, line = run_reference(exe, Path(td), c, r.codes, r.quals, r.lens, width)
            lines.append(line)
            for flag in closeref.FLAGS:
                fastb, first = ref[flag]
                off, bases, pf, _, _ = closeref.close_gaps(c.I, c.pairs, flag == "cg2", width)
                assert np.array_equal(pf, first), f"fuzz_{seed} {flag} {width}: the restatement gives other closures per pair: {pf.tolist()} against {first.tolist()}"
                assert closeref.fastb_bytes(off, bases) == fastb, f"fuzz_{seed} {flag} {width}: the restatement does not reproduce the reference's closures"
                save.update({f"fastb_{flag}{sfx}": np.frombuffer(fastb, np.uint8), f"pair_first_{flag}{sfx}": first})
    # the same bytes from every run: no wall time in the summary, no time of day in the archive
    line = re.sub(r" seconds \S+", "", " | ".join(lines))
    u8 = lambda b: np.frombuffer(b, dtype=np.uint8)
    out = GOLD / "closures" / f"fuzz_{seed}.npz"
    save.update(ref_summary=u8(line.encode()), input_digest=u8(closeref.digest(c, r).encode()))
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(save):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(save[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    assert out.stat().st_size <= 64 << 10, f"{out.name}: {out.stat().st_size} B"
    print(f"fuzz_{seed}: {line} -> {out.name} ({out.stat().st_size / 1024:.1f} KiB)")


def main(argv: list[str]) -> None:
    work, names = None, []
    it = iter(argv)
    for a in it:
        if a == "--work":
            work = Path(next(it)).resolve()
        else:
            names.append(a)
    keep = work is not None
    work = work or Path(tempfile.mkdtemp(prefix="snk_closures."))
    work.mkdir(parents=True, exist_ok=True)
    try:
        exe = build_driver(work)
        (GOLD / "closures").mkdir(exist_ok=True)
        full = not names
        all_infos = []
        fuzz = [int(a[5:]) for a in names if a.startswith("fuzz_")] + (list(closeref.FUZZ) if "fuzz" in names or full else [])
        names = [a for a in names if not a.startswith("fuzz")]
        for seed in fuzz:
            save_fuzz(exe, work, seed)
        for name in (names if names or fuzz and not full else list(closeref.ALL)):
            extra = {}
            if name in closeref.TANDEM or name in closeref.HAND:
                a_hbv, a_inv = closeref.made_graph(name)
                c, (codes, quals, lens) = closeref.tandem_case(a_hbv, a_inv, name)
                # (the hand-made graph holds an edge too long to store: closeref.load writes it again)
                extra = dict(a_hbv=np.frombuffer(a_hbv, np.uint8), a_inv=np.frombuffer(a_inv, np.uint8)) if name in closeref.TANDEM else {}
            else:
                c = hopsref.load(name)                 # (its input_digest is checked there)
                codes, quals, lens = case_reads(name, c)
            ids = closeref.needed_reads(c)
            reads = SimpleNamespace(ids=ids, codes=codes[ids], quals=quals[ids], lens=lens[ids])
            with tempfile.TemporaryDirectory(dir=work) as td:
                ref, line = run_reference(exe, Path(td), c, codes, quals, lens)
                wide = run_reference(exe, Path(td), c, codes, quals, lens, closeref.WIDE)[0] if name in closeref.WIDE_CASES else None
            if name in closeref.HAND:
                import handclose
                h = handclose.case(c.K)
                for flag, which, r in (("cg2", "closures", ref), ("cg1", "closures_cg1", ref), ("cg2", "closures_wide", wide)):
                    handclose.assert_items(h, c.edge_of, c.pairs, *closeref.parse_fastb(r[flag][0]), r[flag][1], f"the reference ({flag})", which)
                I = closeref.Input(c.K, c.eb, c.inv, *c.paths, reads.codes, reads.quals, reads.lens, reads.ids)
                for it in h.items:
                    w = {}
                    closeref.close_gap(I, c.edge_of[it.pair[0]], c.edge_of[it.pair[1]], True, closeref.MAX_WIDTH, None, w)
                    assert all(w[f] >= 1 for f in it.fires), f"{name}, item {it.name}: {it.fires} must remove an offset: {w}"
                    assert (w.get("bod_max", 0) > handclose.BOD_BUDGET) == (it.name == "long_follower"), f"{name}, item {it.name}: {w.get('bod_max', 0)} 32-mers"
            all_infos.append(check_and_save(name, c, ref, line, reads, extra, wide))
        if full:
            total = {f: {k: sum(i[f][0][k] for i in all_infos) for k in closeref.COUNTERS} for f in closeref.FLAGS}
            filt = {f: {k: sum(i[f][1][k] for i in all_infos) for k in closeref.FILTERS} for f in closeref.FLAGS}
            print("over all cases:", total, filt)
            assert any(i["cg2"][0] != i["cg1"][0] for i in all_infos), "the two flags differ nowhere"
            for f in closeref.FLAGS:
                assert all(total[f][k] >= 1 for k in ("n_pairs_0", "n_pairs_1", "n_pairs_2", "n_pairs_many", "n_rows", "n_cons_too_long")), f"{f}: a counter that no case moves: {total[f]}"
                assert all(v >= 1 for v in filt[f].values()), f"{f}: a filter of GetOffsets1 that removes nothing anywhere: {filt[f]}"
            assert all(total["cg2"][k] >= 1 for k in ("n_partners_tried", "n_partners_placed", "n_followers")), total["cg2"]
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:])
