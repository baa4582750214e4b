"""Load golden cases (tests/golden/*.npz, produced by the reference via make_golden.py)."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from supernova_amd import synth

GOLD = Path(__file__).resolve().parent / "golden"
CASES = ["synth_2k_err", "synth_6k_clean", "synth_20k_err", "adversarial", "synth_4k_dups"]


class Case:
    def __init__(self, name: str):
        z = np.load(GOLD / f"{name}.npz")
        self.name = name
        self.lens = z["lens"]
        self.rows = z["rows"]
        self.quals = z["quals"]
        self.bc = z["bc"]
        self.ign_bc_below = int(z["ign_bc_below"])
        self.read_len = self.quals.shape[1]
        self.codes = synth.unpack_rows(self.rows, self.read_len)
        self.exp_goodlens = z["exp_goodlens"]
        self.exp_keys = z["exp_keys"]          # [n,3] u32
        self.exp_counts = z["exp_counts"]
        self.exp_ctx = z["exp_ctx"]
        self.exp_unitigs = bytes(z["exp_unitigs"]).decode().split("\n") if len(z["exp_unitigs"]) else []
        self.exp_hbv = bytes(z["exp_hbv"]).decode()
        self.exp_hist = z["exp_hist"]
        # f1: read paths of pathReads (offset, HBV edge ids per read); f2: a.hbv / a.inv file bytes
        self.exp_path_off = z["exp_path_off"]
        self.exp_path_n = z["exp_path_n"]
        self.exp_path_edges = z["exp_path_edges"]
        self.exp_ahbv = bytes(z["exp_ahbv"])
        self.exp_ainv = bytes(z["exp_ainv"])
        # f4: MarkDups over those paths -- flag per pair, inter-barcode rate, the logged artifactual-duplicate percentage
        self.exp_dup = z["exp_dup"]
        self.exp_interdup = float(z["exp_interdup"])
        self.exp_art_perc = float(z["exp_art_perc"])


_cache: dict[str, Case] = {}


def load(name: str) -> Case:
    if name not in _cache:
        _cache[name] = Case(name)
    return _cache[name]


class Case60:
    """K=60 expectations of a base case, dumped from the reference's BuildReadQGraph60 (no barcode rule)."""

    def __init__(self, name: str):
        z = np.load(GOLD / f"{name}_k60.npz")
        self.base = load(name)
        self.exp_goodlens = z["exp_goodlens"]
        self.exp_keys = z["exp_keys"]          # [n,4] u32
        self.exp_counts = z["exp_counts"]
        self.exp_ctx = z["exp_ctx"]
        self.exp_unitigs = bytes(z["exp_unitigs"]).decode().split("\n") if len(z["exp_unitigs"]) else []
        self.exp_hbv = bytes(z["exp_hbv"]).decode()
        self.exp_ahbv = bytes(z["exp_ahbv"])
        self.exp_ainv = bytes(z["exp_ainv"])


K60_CASES = ["adversarial", "synth_20k_err"]


class HotCase:
    """hot_kmers / hot_kmers_k60: the reference's results for the saturating read set of tests/hotgen.py, in a lean layout -- no reads
    (generated, and checked against the stored digest), no paths, the spectrum sparse.  Not in CASES: it has no a48 files."""

    def __init__(self, K: int):
        import hotgen
        z = np.load(GOLD / ("hot_kmers.npz" if K == 48 else "hot_kmers_k60.npz"))
        self.K = K
        self.codes, self.quals, self.lens, self.bc = hotgen.reads(expect_digest=bytes(z["reads_digest"]))
        self.read_len = hotgen.L
        self.rows = synth.pack_rows(self.codes)
        self.exp_goodlens_digest = bytes(z["exp_goodlens_digest"])
        self.exp_keys = z["exp_keys"]          # [n, 3 or 4] u32
        self.exp_counts = z["exp_counts"]
        self.exp_ctx = z["exp_ctx"]
        self.exp_unitigs = bytes(z["exp_unitigs"]).decode().split("\n") if len(z["exp_unitigs"]) else []
        self.exp_ahbv = bytes(z["exp_ahbv"])
        self.exp_ainv = bytes(z["exp_ainv"])
        # stats/histogram_kmer_count.json as (length, nonzero bins, their values); the K=60 reference writes none (length 0)
        self.exp_hist_len = int(z["exp_hist_len"])
        self.exp_hist_bins = z["exp_hist_bins"]
        self.exp_hist_vals = z["exp_hist_vals"]
        self.ref_summary = bytes(z["ref_summary"]).decode()


_hot: dict[int, HotCase] = {}


def load_hot(K: int) -> HotCase:
    if K not in _hot:
        _hot[K] = HotCase(K)
    return _hot[K]
