#!/usr/bin/env python3
"""Generate tests/golden/handreads/paths/ by running the REFERENCE'S OWN pathReads and MarkDups on the reads of tests/handreads.py.

K=48 only: the reference has no K=60 pather.  Needs oracle/_ref/snref_driver, which build() compiles.  Every case runs in its three read
variants -- clean, noisy, and "paths" (the clean reads at random qualities with a layer of substituted and chimeric reads among them) --
through the driver's mode "dump", with 1 thread and with 8; the two must write the same paths.txt and, where the number of reads is even
(MarkDups takes pairs), the same markdups.txt.  Before anything is saved the unitigs of all three runs have to be the case's stored ones
(tests/golden/handreads/NAME_k48.npz, or the digest in big_hashes.json): the paths are paths over the graph the other handreads tests pin.

A fixture holds, per variant, the reference's output only -- path_off, path_n, path_edges (int32), where written dup, interdup, art_perc
-- and the digest of the reads, which are regenerated from their seed.  handreads.HASHED cases are kept as SHA-256 digests in
paths/big_hashes.json.  The .npz members carry a fixed date, so that a second run reproduces the files byte for byte.  A variant that the
reference refuses is named with its message on stdout and left out (at most two).

Over the whole set the maker then asserts that the fixtures are what they are meant to be: a read of more than 16 edges, a negative
offset, an unplaced read of at least K + 1 bases, a chimera with a shorter path than the clean read its prefix came from, a read with
its first or last base substituted that keeps its parent's path, and a case whose clean reads are pathed differently at random qualities
than at quality 30.

usage: python tests/golden/make_handreads_paths_golden.py [case ...]      (one line per case and variant on stdout:
       profiles/handreads_paths.log; the assertions over the whole set run when no case is named)
"""
from __future__ import annotations

import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))

import handreads as hr  # noqa: E402
import refio  # noqa: E402
from make_handreads_golden import save_npz  # noqa: E402
from supernova_amd import synth  # noqa: E402

K = 48
MAX_REFUSED = 2


def run(r, td, tag):
    """the reference on one read set, 1 thread and 8 -> its dump"""
    out = []
    refio.write_snkrd(td / f"{tag}.snkrd", r.lens, synth.codes_to_ascii(r.codes), r.quals, r.bc, 0)
    for threads in (1, 8):
        refio.run_ref(td / f"{tag}.snkrd", td / f"{tag}_{threads}", threads=threads, mode="dump", K=K)
        out.append(refio.read_ref_dump(td / f"{tag}_{threads}", K=K))
    a, b = out
    for f in hr.PATH_FIELDS:
        assert np.array_equal(a[f], b[f]), f"{r.name} {tag}: 1 thread and 8 threads differ in {f}"
    assert (a["dup"] is not None) == (b["dup"] is not None) == (len(r.lens) % 2 == 0 and len(r.lens) > 0)
    if a["dup"] is not None:
        assert np.array_equal(a["dup"], b["dup"]) and a["interdup"] == b["interdup"] and a["art_perc"] == b["art_perc"], f"{r.name} {tag}: markdups.txt"
    return a


def profile(r, d):
    n = d["path_n"]
    line = (f"reads {len(n)} placed {int((n > 0).sum())} most edges {int(n.max()) if len(n) else 0} negative offsets {int((d['path_off'] < 0).sum())} "
            f"edge entries {len(d['path_edges'])}")
    if d["dup"] is not None:
        line += f" dup pairs {int(d['dup'].sum())}"
    if r.noise == "paths":
        line += " layer " + " ".join(f"{k} {v}" for k, v in r.facts["layer"]["kinds"].items())
    return line


def path_of(d, row):
    at = int(d["path_n"][:row].sum())
    return int(d["path_off"][row]), d["path_edges"][at:at + int(d["path_n"][row])].tolist()


def make(name, hashes, seen, refused):
    g = hr.golden(name, K)
    dumps = {}
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        for noise in hr.VARIANTS:
            v, r = hr.vname(noise), hr.reads(name, K, noise)
            try:
                d = run(r, td, v)
            except RuntimeError as ex:
                refused.append((name, v))
                print(f"{name} {v}: REFUSED by the reference: {str(ex).strip().splitlines()[-1]}", flush=True)
                continue
            unitigs = np.frombuffer("\n".join(d["unitigs"]).encode(), np.uint8)
            assert (hr.sha(unitigs) == g.clean["unitigs"]) if g.hashed else np.array_equal(unitigs, g.clean["unitigs"]), f"{name} {v}: not the case's unitigs"
            assert len(d["path_n"]) == len(r.lens) and int(d["path_n"].sum()) == len(d["path_edges"])
            dumps[noise] = (r, d)
            print(f"{name} {v}: " + profile(r, d), flush=True)
    arrays, digests = {}, {}
    for noise, (r, d) in dumps.items():
        v = hr.vname(noise)
        fields = {f: d[f].astype(np.int32) for f in hr.PATH_FIELDS}
        if d["dup"] is not None:
            fields.update(dup=d["dup"].astype(np.uint8), interdup=np.float64(d["interdup"]), art_perc=np.float64(d["art_perc"]))
        if g.hashed:
            digests[v] = {f: (float(a) if a.ndim == 0 else hr.sha(a)) for f, a in fields.items()}
            digests[v].update(reads_digest=r.digest, n_reads=len(r.lens), n_edge_entries=len(d["path_edges"]))
        else:
            arrays.update({f"{v}_{f}": a for f, a in fields.items()})
            arrays[f"{v}_reads_digest"] = np.frombuffer(r.digest.encode(), np.uint8)
    if g.hashed:
        hashes[f"{name}_k{K}"] = digests
    else:
        out = hr.PATHS_GOLD / f"{name}_k{K}.npz"
        save_npz(out, K=np.int64(K), **arrays)
        size = out.stat().st_size
        assert size <= (hr.GOLD.parent / "synth_20k_err.npz").stat().st_size and size <= 1 << 20, (name, size)
    # ---- what the set is to hold
    for noise, (r, d) in dumps.items():
        n, off = d["path_n"], d["path_off"]
        seen["more than 16 edges"] |= bool((n > 16).any())
        seen["a negative offset"] |= bool(((off < 0) & (n > 0)).any())
        seen["an unplaced read of K + 1 bases"] |= bool(((n == 0) & (r.lens >= K + 1)).any())
    if "paths" in dumps and False in dumps:
        r, d = dumps["paths"]
        for row in np.nonzero(r.kind == hr.KINDS.index("chimera"))[0]:
            seen["a chimera with a shorter path than its prefix's read"] |= bool(d["path_n"][row] < d["path_n"][r.parent[row]])
        for row in np.nonzero((r.kind == hr.KINDS.index("first")) | (r.kind == hr.KINDS.index("last")))[0]:
            if d["path_n"][row] > 0 and not seen["a first or last read with its parent's path"]:
                seen["a first or last read with its parent's path"] |= path_of(d, row) == path_of(d, r.parent[row])
        c = dumps[False][1]
        rows = r.clean_rows
        same = np.array_equal(d["path_off"][rows], c["path_off"]) and np.array_equal(d["path_n"][rows], c["path_n"])
        if same:
            keep = np.repeat(np.isin(np.arange(len(r.lens)), rows), d["path_n"])
            same = np.array_equal(d["path_edges"][keep], c["path_edges"])
        seen["clean reads pathed differently at random qualities"] |= not same


if __name__ == "__main__":
    names = sys.argv[1:] or list(hr.CASES)
    hr.PATHS_GOLD.mkdir(exist_ok=True)
    hp = hr.PATHS_GOLD / "big_hashes.json"
    hashes = json.loads(hp.read_text()) if hp.exists() else {}
    seen = {k: False for k in ("more than 16 edges", "a negative offset", "an unplaced read of K + 1 bases", "a chimera with a shorter path than its prefix's read",
                               "a first or last read with its parent's path", "clean reads pathed differently at random qualities")}
    refused: list = []
    for nm in names:
        make(nm, hashes, seen, refused)
    if hashes:
        hp.write_text(json.dumps(hashes, indent=1, sort_keys=True) + "\n")
    assert len(refused) <= MAX_REFUSED, refused
    if not sys.argv[1:]:
        for k, v in seen.items():
            assert v, f"no case holds {k}"
        print("the set holds: " + "; ".join(seen), flush=True)
