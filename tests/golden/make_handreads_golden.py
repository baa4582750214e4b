#!/usr/bin/env python3
"""Generate tests/golden/handreads/ by running the REFERENCE ITSELF on the reads of tests/handreads.py.

Needs the reference drivers that build() compiles into oracle/_ref/ (snref_driver for K=48, snref_driver60 for K=60, which has no barcode
rule).  Every case runs at both K, clean and with the noise layer, with 1 thread and with 8; the two thread counts must agree.  Before
anything is saved the reference has to confirm what the generator promises: it keeps exactly the reachable k-mers of the case, the noisy
run has the clean run's keys, pruned contexts and unitigs (only counts differ), and the unitigs hold every retained k-mer once.

A fixture holds the reference's output only -- good lengths, keys, counts, pruned contexts, the spectrum, the unitigs -- and the digest of
the reads, which are regenerated from their seed.  The K=60 driver writes no spectrum: the histogram of its counts is stored, after the
K=48 runs have shown that the spectrum file is that histogram.  handreads.HASHED cases are kept as SHA-256 digests in big_hashes.json.
The .npz members carry a fixed date, so that a second run reproduces the files byte for byte.

usage: python tests/golden/make_handreads_golden.py [case ...]      (one line per case and K on stdout: profiles/handreads.log)
"""
from __future__ import annotations

import io
import json
import sys
import tempfile
import zipfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import handreads as hr  # noqa: E402
import refio  # noqa: E402
from supernova_amd import synth  # noqa: E402


def save_npz(path, **arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def run(r, K, td, tag):
    """the reference on one read set, 1 thread and 8 -> the normalised result"""
    out = []
    refio.write_snkrd(td / f"{tag}.snkrd", r.lens, synth.codes_to_ascii(r.codes), r.quals, r.bc, 0)
    for threads in (1, 8):
        refio.run_ref(td / f"{tag}.snkrd", td / f"{tag}_{threads}", threads=threads, mode="graph", K=K)
        d = refio.read_ref_dump(td / f"{tag}_{threads}", K=K)
        counts = d["kmers"]["count"]
        own = np.bincount(counts).astype(np.int64) if len(counts) else np.zeros(0, np.int64)
        if K == 48:
            hist = np.asarray(d["hist"]["vals"] if d["hist"] else [], np.int64)
            nz = np.nonzero(hist)[0]
            assert np.array_equal(hist[:(nz[-1] + 1 if len(nz) else 0)], own), "the spectrum file is not the histogram of the counts"
        out.append(hr.normalised(K, d["goodlens"], d["kmers"]["k"], counts, d["kmers"]["ctx"], own, d["unitigs"]))
    for f in hr.FIELDS:
        assert np.array_equal(out[0][f], out[1][f]), f"{r.name} K={K} {tag}: 1 thread and 8 threads differ in {f}"
    return out[0]


def make(name, K, hashes):
    clean_r, noisy_r = hr.reads(name, K, False), hr.reads(name, K, True)
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        clean, noisy = run(clean_r, K, td, "clean"), run(noisy_r, K, td, "noisy")
    reachable = hr._canon_set(hr.unitig_set(name, K), K) - set(clean_r.facts["unreachable"])
    kept = hr.key_strings(clean["keys"], K)
    assert len(kept) == len(set(kept)) and set(kept) == reachable, f"{name} K={K}: the reference keeps {len(kept)} k-mers, the case has {len(reachable)} reachable ones"
    for f in ("keys", "ctx", "unitigs"):
        assert np.array_equal(clean[f], noisy[f]), f"{name} K={K}: the noise layer changes {f}"
    assert np.all(noisy["counts"] >= clean["counts"])
    for r, res in ((clean_r, clean), (noisy_r, noisy)):          # every base has quality 30: a read of at least K bases is good to its end
        assert np.array_equal(res["goodlens"], np.where(r.lens >= K, r.lens, 0))
    unitigs = bytes(clean["unitigs"]).decode().split("\n") if len(clean["unitigs"]) else []
    lens = np.asarray([len(u) for u in unitigs], np.int64)
    assert int((lens - K + 1).sum()) == len(kept)
    circles = sum(u[:K - 1] == u[-(K - 1):] for u in unitigs)
    if name in hr.HASHED:
        hashes[f"{name}_k{K}"] = dict(reads_digest=clean_r.digest, reads_digest_noisy=noisy_r.digest, n_kmers=len(kept), unitig_lens=[int(x) for x in lens],
                                      clean={f: hr.sha(clean[f]) for f in hr.FIELDS}, noisy={f: hr.sha(noisy[f]) for f in hr.FIELDS})
        size = 0
    else:
        out = hr.GOLD / f"{name}_k{K}.npz"
        save_npz(out, K=np.int64(K), reads_digest=np.frombuffer(clean_r.digest.encode(), np.uint8), reads_digest_noisy=np.frombuffer(noisy_r.digest.encode(), np.uint8),
                 **{f: clean[f] for f in hr.FIELDS}, goodlens_noisy=noisy["goodlens"], counts_noisy=noisy["counts"], hist_noisy=noisy["hist"], unitig_lens=lens)
        size = out.stat().st_size
        assert size <= (hr.GOLD.parent / "synth_20k_err.npz").stat().st_size and size <= 1 << 20, (name, K, size)
    print(f"{name} K={K}: reads {clean_r.facts['n_reads']} (+{noisy_r.facts['noise']['n_noise_reads']} noise, {noisy_r.facts['noise']['n_noise_kmers']} noise k-mers) "
          f"retained {len(kept)} unitigs {len(unitigs)} circles {circles} unreachable {len(clean_r.facts['unreachable'])}"
          + (f" -> {size} bytes" if size else " -> big_hashes.json"), flush=True)


if __name__ == "__main__":
    names = sys.argv[1:] or list(hr.CASES)
    hr.GOLD.mkdir(exist_ok=True)
    hp = hr.GOLD / "big_hashes.json"
    hashes = json.loads(hp.read_text()) if hp.exists() else {}
    for nm in names:
        for K in hr.KS:
            make(nm, K, hashes)
    if hashes:
        hp.write_text(json.dumps(hashes, indent=1, sort_keys=True) + "\n")
