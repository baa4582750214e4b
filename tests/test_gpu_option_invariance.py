"""include/snk.h, "tuning": "Results never depend on any of it."  Every result-neutral option that no other test forces is forced here to
in-range, non-default values, and the table, counts, contexts, spectrum, good lengths and unitigs are compared with the reference's
goldens or the C oracle -- never with a default run alone; the default run only supplies the baselines of the EVIDENCE that the forced
branch really ran (every entry asserts some).  NEUTRAL is the table tests/test_abi.py::test_every_option_is_classified and the fuzz tool
(tests/tools/fuzz_parity.py) read, so this module imports without torch or a GPU.

What the evidence cannot show is said in NEUTRAL's `evidence` strings: where the result carries no trace of the branch (which trim kernel
ran, whether chunks were merged) the assertion is the branch's own precondition, read off the call site."""
import functools

import numpy as np
import pytest

import goldens
import oracle_lib

pytestmark = pytest.mark.gpu

# option -> values: in-range, non-default; legs: the entry points that read it (a test function each); with: options pinned next to it so
# that the branch is reached on an input of fixture size; evidence: what the test asserts to show that it was
NEUTRAL = {
    # ---- bucket-local prune (snk_local.hip)
    "bl_cpw": dict(values=(1, 3, 7), legs=("local", "grouped", "sharded_local"),
                   evidence="a run without split buckets (chunks = buckets) whose bucket count is no multiple of the value: the last workgroup's tail"),
    "bl_index_fused": dict(values=(0,), legs=("local", "grouped", "sharded_local"), evidence="n_boundary > 0 and equal to the default run's: the separate build pass indexed them"),
    "bl_noclassify": dict(values=(1,), legs=("local", "grouped", "sharded_local"), evidence="n_boundary >= the default run's in every case and > in one: misses went pending unclassified"),
    "chunk_merge": dict(values=(0, 16, 256), legs=("local", "grouped", "sharded_local"),
                        evidence="the merge's precondition, more buckets than count regions (4099 buckets, one residency wave of at most 2 workgroups per CU): "
                                 "the result carries no chunk count; at the default 32 waves NO fixture-sized input merges chunks at all"),
    "defer_compact": dict(values=(0,), legs=("local", "grouped", "sharded_local"), evidence="the unsorted-table cases (the option is only read there); sorted ones run too"),
    # ---- list ranking
    "rank_wyllie": dict(values=(1,), legs=("ranking",), evidence="n_fragments * 2 >= 4096: the default run took the sparse ruling set, this one may not"),
    "rank_round_batch0": dict(values=(1, 2), legs=("ranking",), evidence="rank_rounds > the value while the default run reports >= 3: the second batch ran"),
    "split_log2": dict(values=(1, 3, 8), legs=("ranking", "sharded_ranking"), evidence="n_circles >= 6 in every run; ranking stays partitioned when sharded"),
    "rank_round_batch": dict(values=(1, 3), legs=("sharded_ranking",),
                             evidence="join_ranking partitioned and host read-backs at 1 > at 3 > at the default 8 (the sharded result carries no round count)"),
    # ---- sharded exchange
    "exchange_ranges": dict(values=(1, 3, 7, 64), legs=("exchange",), evidence="every rank has at least as many buckets as ranges, so the value is not clamped; cross-rank queries ran"),
    # ---- trim, stages, sizing
    "trim_rowwise": dict(values=(1,), legs=("trim",), evidence="layouts the tiled kernel would have taken (stride a multiple of 4, <= 160, 16-byte aligned); which kernel ran leaves no trace"),
    "pilot_est": dict(values=(0,), legs=("history",), evidence="two read sets of equal size alternate on one context, both orders: what the second call inherits is the first's"),
    "input_fp": dict(values=(0,), legs=("history",), evidence="as pilot_est: without the fingerprint the second read set inherits the first one's sizing history"),
    "tight_tries": dict(values=(1, 4), legs=("sizing",), **{"with": {"count_tight": 1920, "count_screen_ng": 0}}, evidence="last_count_limit == 1920: booked slots"),
    "screen_target": dict(values=(1000, 8000), legs=("sizing",), **{"with": {"count_screen_ng": 2}},
                          evidence="last_count_limit == 960 (the filter is on) and more buckets at 1000 than at 8000"),
    "msp_sigmas_x10": dict(values=(0, 15), legs=("sizing",), evidence="n_overflow > 0 at 0 sigma: the overflow segment carries records"),
    "msp_site_records": dict(values=(3, 200), legs=("sizing",), evidence="n_overflow at 3 > n_overflow at 200 (smaller sigma, smaller slots)"),
    "lean_cold": dict(values=(0,), legs=("sizing",), evidence="fresh contexts: n_overflow < the default fresh context's (5 sigma instead of 1.5)"),
    "hot": dict(values=(0,), legs=("sizing",), **{"with": {"msp_cap_pct": 20, "hot_min": 8, "hot_factor": 1, "hot_class_inst": 300}},
                evidence="n_hot_buckets > 0 with the same thresholds and hot = 1, and 0 with hot = 0"),
    "bucket_fill_pct": dict(values=(20, 90), legs=("scale",), **{"with": {"count_screen_ng": 0}}, evidence="repartitioned == 1 on a fresh context and more buckets at 20 than at 90"),
    "chunk_kmers": dict(values=(60, 600), legs=("scale",), **{"with": {"count_screen_ng": 0}},
                        evidence="200 k reads at 28x (half the coverage retains twice the share), second call on the context, which knows that share: more buckets at 60 than at 600"),
    # ---- memory, HBV
    "arena_vmm": dict(values=(0,), legs=("arena",), evidence="a context created under SNK_TUNING echoes the option; three calls of different size on it"),
    "hbv_strict": dict(values=(1,), legs=("hbv",), **{"with": {"hbv_dev_min": 0}}, evidence="the call succeeds: the device flood did not give up"),
}

def _pairs(leg):
    return [(o, v) for o, s in NEUTRAL.items() if leg in s["legs"] for v in s["values"]]


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


def _pin(tune, name):
    for k, v in NEUTRAL[name].get("with", {}).items():
        tune(k, v)


# ---- expectations: the reference's goldens (K=48: tests/golden/<name>.npz, K=60: <name>_k60.npz)

class _Exp:
    def __init__(self, name, K):
        c = goldens.load(name)
        g = goldens.Case60(name) if K == 60 else c
        self.c, self.K = c, K
        self.keys, self.counts, self.ctx, self.unitigs, self.goodlens = g.exp_keys, g.exp_counts, g.exp_ctx, g.exp_unitigs, g.exp_goodlens
        self.hist = c.exp_hist if K == 48 else None


@functools.lru_cache(maxsize=None)
def _exp(name, K):
    return _Exp(name, K)


def _table(res):
    k, c, x = res.keys(), res.counts(), res.ctx()
    o = np.lexsort((k[:, 3], k[:, 2], k[:, 1], k[:, 0]))
    return k[o], c[o], x[o]


def _check(res, exp, tag):
    assert np.array_equal(res.good_len().astype(np.uint32), exp.goodlens), tag
    k, c, x = _table(res)
    assert k.shape[0] == exp.keys.shape[0], (tag, k.shape, exp.keys.shape)
    w = exp.keys.shape[1]
    assert np.array_equal(k[:, :w], exp.keys) and np.all(k[:, w:] == 0), tag
    assert np.array_equal(np.minimum(c, (1 << 24) - 1), exp.counts), tag
    assert np.array_equal(x, exp.ctx), tag
    if exp.hist is not None:
        spec = res.spectrum()
        nz = np.nonzero(spec)[0]
        assert np.array_equal(spec[: (nz[-1] + 1 if len(nz) else 0)].astype(np.int64), exp.hist), tag
    assert res.unitigs() == exp.unitigs, tag


def _dev(c):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(c.rows.view(np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(c.quals)).to(dev),
            torch.from_numpy(c.bc.astype(np.int32)).to(dev), torch.from_numpy(c.lens.astype(np.uint16).view(np.int16)).to(dev))


def _run(e, exp, n_buckets=0, sorted_table=True):
    from supernova_amd.engine import Params
    c = exp.c
    rows, quals, bc, lens = _dev(c)
    return e.count_graph(rows, c.read_len, quals=quals, bc=bc if exp.K == 48 else None, lens=lens,
                         params=Params(K=exp.K, n_buckets=n_buckets, sorted_table=sorted_table), ign_bc_below=c.ign_bc_below)


# ---- one GPU, bucket-local stage: (golden, K, n_buckets, sorted_table, merged); merged: one residency wave of count workgroups and 4099
# buckets, so that there are more buckets than count regions -- the only shape in which the graph stage merges chunks at all
LOCAL_CASES = [("adversarial", 48, 0, True, False), ("adversarial", 60, 0, True, False), ("synth_20k_err", 48, 0, True, False),
               ("synth_20k_err", 48, 997, False, False), ("adversarial", 48, 4099, False, True), ("synth_20k_err", 48, 4099, False, True)]


@pytest.mark.parametrize("name,value", _pairs("local"))
def test_local_stage_options(engine, tune, name, value):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    tail = strictly_more = False
    for gname, K, nb, sorted_table, merged in LOCAL_CASES:
        exp, tag = _exp(gname, K), (name, value, gname, K, nb, sorted_table, merged)
        tune("count_persist", 1 if merged else 32)
        engine.clear_option(name)
        base = _run(engine, exp, nb, sorted_table)
        base_f = dict(n_boundary=base.n_boundary, n_buckets=base.n_buckets, split=base.buckets_split)
        _check(base, exp, ("default",) + tag)
        engine.set_option(name, value)
        try:
            res = _run(engine, exp, nb, sorted_table)
            _check(res, exp, tag)
        finally:
            engine.clear_option(name)
        if merged:
            assert res.n_buckets > 2 * n_cu, tag               # (768 threads per count workgroup: at most two per CU)
        if name == "bl_cpw":
            tail |= res.buckets_split == 0 and res.n_buckets % value != 0
        elif name == "bl_index_fused":
            assert res.n_boundary > 0 and (nb == 0 or res.n_boundary == base_f["n_boundary"]), tag      # (nb = 0: the context's second call may size its buckets anew)
        elif name == "bl_noclassify":
            assert nb == 0 or res.n_boundary >= base_f["n_boundary"], tag
            strictly_more |= nb != 0 and res.n_boundary > base_f["n_boundary"]
    if name == "bl_cpw" and value > 1:
        assert tail, "no case left a partial last workgroup"
    if name == "bl_noclassify":
        assert strictly_more


# ---- per-group graphs: one grouped run == the oracle on every group's reads alone

@functools.lru_cache(maxsize=None)
def _grouped_case():
    c = goldens.load("synth_20k_err")
    rng = np.random.default_rng(7)
    n = c.rows.shape[0]
    group = (c.bc.astype(np.int64) % 5).astype(np.int32)
    group[rng.random(n) < 0.1] = 8                      # a sparse extra group behind a gap in the ids
    want = {}
    for gid in np.unique(group):
        sel = group == gid
        want[int(gid)] = oracle_lib.OracleResult(c.codes[sel], c.exp_goodlens[sel], None, min_freq=3, min_bc=0, hbv=False)
    return c, group, want


def _check_groups(res, want, tag):
    """A grouped result against the oracle's run on every group's reads alone (want: group id -> OracleResult)."""
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    k, cnt, ctx = res.keys(), res.counts(), res.ctx()
    off, bases = res.unitig_arrays()
    ug = res.unitig_groups()
    assert np.all(np.diff(ug.astype(np.int64)) >= 0)
    total = 0
    for gid, o in want.items():
        m = k[:, 3] == gid
        kk, cc, xx = k[m], cnt[m], ctx[m]
        order = np.lexsort((kk[:, 2], kk[:, 1], kk[:, 0]))
        assert np.array_equal(kk[order][:, :3], o.keys[:, :3]) and np.array_equal(cc[order], o.counts) and np.array_equal(xx[order], o.ctx), tag + (gid,)
        us = sorted((lut[bases[int(off[u]):int(off[u + 1])]].tobytes().decode() for u in np.nonzero(ug == gid)[0]), key=lambda t: (-len(t), t))
        assert us == o.unitigs, tag + (gid,)
        total += int(m.sum())
    assert total == k.shape[0]


@pytest.mark.parametrize("name,value", _pairs("grouped"))
def test_local_stage_options_per_group(engine, tune, name, value):
    import torch
    from supernova_amd.engine import Params
    c, group, want = _grouped_case()
    rows, quals, bc, lens = _dev(c)
    g_dev = torch.from_numpy(group).to(rows.device)
    for nb, merged in ((0, False), (4099, True)):
        tune("count_persist", 1 if merged else 32)
        tune(name, value)
        res = engine.count_graph(rows, c.read_len, quals=quals, bc=None, lens=lens, group=g_dev,
                                 params=Params(K=48, min_freq=3, min_bc=0, grouped=True, sorted_table=False, n_buckets=nb))
        _check_groups(res, want, (name, value, nb))


# ---- list ranking on tens of thousands of fragments with circles (sharded_cases.plasmid_case), against the C oracle

@functools.lru_cache(maxsize=None)
def _plasmids():
    from sharded_cases import plasmid_case
    from supernova_amd import synth
    codes, quals, bc, L = plasmid_case()
    o = oracle_lib.OracleResult(codes, np.full(codes.shape[0], L, np.uint32), bc, hbv=False)
    assert sum(1 for u in o.unitigs if len(u) >= 95 and u[:47] == u[-47:]) >= 6
    return synth.pack_rows(codes), quals, bc, L, o


def _plasmid_run(e):
    import torch
    from supernova_amd.engine import Params
    rows, quals, bc, L, o = _plasmids()
    dev = torch.device("cuda", 0)
    return e.count_graph(torch.from_numpy(rows.view(np.int32).copy()).to(dev), L, quals=torch.from_numpy(quals).to(dev),
                         bc=torch.from_numpy(bc).to(dev), params=Params(K=48))


def _check_oracle(res, o, tag):
    k, c, x = _table(res)
    assert np.array_equal(k, o.keys) and np.array_equal(c, o.counts) and np.array_equal(x, o.ctx), tag
    assert res.unitigs() == o.unitigs, tag


@pytest.mark.parametrize("name,value", _pairs("ranking"))
def test_one_gpu_ranking_options(engine, tune, name, value):
    """Not checked before the GPU run: how many rounds the default ranking of this input reports; the test asserts >= 3 and fails if the
    input is too small to show the second batch."""
    o = _plasmids()[4]
    engine.clear_option(name)
    base = _plasmid_run(engine)
    _check_oracle(base, o, ("default", name))
    assert base.n_fragments * 2 >= 4096 and base.rank_rounds >= 3 and base.n_circles >= 6
    tune(name, value)
    res = _plasmid_run(engine)
    _check_oracle(res, o, (name, value))
    assert res.n_circles >= 6 and res.n_fragments * 2 >= 4096
    if name == "rank_round_batch0":
        assert res.rank_rounds > value, (res.rank_rounds, base.rank_rounds)


def _gather(out):
    keys = np.concatenate([x["keys"] for x in out])
    order = np.lexsort((keys[:, 3], keys[:, 2], keys[:, 1], keys[:, 0]))
    unitigs = sorted((u for x in out for u in x["unitigs"]), key=lambda s: (-len(s), s))
    return keys[order], np.concatenate([x["counts"] for x in out])[order], np.concatenate([x["ctx"] for x in out])[order], unitigs


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("name,value", _pairs("sharded_ranking"))
def test_sharded_ranking_options(snk, tune, name, value, W):
    from sharded_cases import run_ranks
    rows, quals, bc, L, o = _plasmids()
    base = run_ranks(W, rows, L, quals, bc, pairs=True)
    tune(name, value)
    out = run_ranks(W, rows, L, quals, bc, pairs=True)
    assert all(x["options"].get(name) == value for x in out) and not any(name in x["options"] for x in base)
    k, c, x, us = _gather(out)
    assert np.array_equal(k, o.keys) and np.array_equal(c, o.counts) and np.array_equal(x, o.ctx) and us == o.unitigs, (name, value, W)
    assert {r["ranking"] for r in out} == {"partitioned"} and all(r["n_circles"] >= 6 for r in out)
    assert sum(r["n_frags"] for r in out) > 4096
    if name == "rank_round_batch":
        # the sharded result carries no round count: what a smaller batch shows is more read-backs of the same ranking.  Every value forced
        # is held against both of its neighbours in 1 < 3 < 8 (the default), on the same W.
        syncs = {8: [b["host_syncs"] for b in base], value: [r["host_syncs"] for r in out]}
        other = 4 - value
        tune(name, other)
        out2 = run_ranks(W, rows, L, quals, bc, pairs=True)
        assert all(x["options"].get(name) == other for x in out2)
        syncs[other] = [r["host_syncs"] for r in out2]
        print("host_syncs by rank_round_batch, W = %d: %s" % (W, syncs))
        assert all(a > b > c for a, b, c in zip(syncs[1], syncs[3], syncs[8])), syncs


@pytest.mark.parametrize("W", [2, 5])
@pytest.mark.parametrize("name,value", _pairs("sharded_local"))
def test_local_stage_options_on_ranks(snk, tune, name, value, W):
    """The bucket-local stage on a rank of an N-rank job, where a miss of the prune may be another rank's k-mer to answer (bl_noclassify = 1
    lost exactly those: seen first by the fuzz tool at K = 60, W = 5)."""
    from sharded_cases import run_ranks
    tune(name, value)
    for gname, K in (("adversarial", 48), ("adversarial", 60), ("synth_20k_err", 60)):
        exp = _exp(gname, K)
        c = exp.c
        out = run_ranks(W, c.rows, c.read_len, c.quals, c.bc if K == 48 else None, c.lens, K=K, n_buckets=W * 199, ign_bc_below=c.ign_bc_below)
        assert all(r["options"].get(name) == value for r in out) and sum(r["n_queries"] for r in out) > 0
        k, cnt, x, us = _gather(out)
        w = exp.keys.shape[1]
        tag = (name, value, W, gname, K)
        assert k.shape[0] == exp.keys.shape[0] and np.array_equal(k[:, :w], exp.keys) and np.all(k[:, w:] == 0), tag
        assert np.array_equal(np.minimum(cnt, (1 << 24) - 1), exp.counts) and np.array_equal(x, exp.ctx) and us == exp.unitigs, tag


@pytest.mark.parametrize("W", [2, 3, 5])
@pytest.mark.parametrize("value", NEUTRAL["exchange_ranges"]["values"])
def test_exchange_ranges(snk, tune, value, W):
    from sharded_cases import run_ranks
    from test_gpu_sharded import check
    tune("exchange_ranges", value)
    for gname in ("adversarial", "synth_20k_err"):
        c = goldens.load(gname)
        nb = 0 if value < 7 else value * W * 2        # (at fixture size a rank may have fewer buckets than that by itself)
        out = run_ranks(W, c.rows, c.read_len, c.quals, c.bc, c.lens, n_buckets=nb, ign_bc_below=c.ign_bc_below)
        check(out, c)
        assert all(r["options"].get("exchange_ranges") == value and r["n_buckets"] // W >= value for r in out), [r["n_buckets"] for r in out]
        assert sum(r["n_queries"] for r in out) > 0 and {r["ranking"] for r in out} == {"partitioned"}


# ---- bucket and slot sizing at fixture size

@pytest.mark.parametrize("name", [o for o, s in NEUTRAL.items() if "sizing" in s["legs"]])
def test_sizing_options(snk, tune, name):
    """Fresh contexts throughout: what a context learnt from an earlier call (ratio hints, mapped arena) changes the sizing under test."""
    from supernova_amd.engine import Engine
    exps = [_exp("synth_20k_err", 48), _exp("adversarial", 48)] + ([_exp("synth_20k_err", 60)] if name != "screen_target" else [])
    _pin(tune, name)
    seen = {}
    for value in (None,) + NEUTRAL[name]["values"]:
        if value is not None:
            tune(name, value)
        for exp in exps:
            e = Engine(0)
            try:
                assert e.get_option(name) == value
                res = _run(e, exp)
                _check(res, exp, (name, value, exp.c.name, exp.K))
                seen[(value, exp.c.name, exp.K)] = dict(limit=e.last_count_limit(), n_buckets=res.n_buckets, n_overflow=res.n_overflow, n_hot=res.n_hot_buckets)
            finally:
                e.close()
    at = lambda v, f: seen[(v, "synth_20k_err", 48)][f]
    if name == "tight_tries":
        assert all(s["limit"] == 1920 for s in seen.values())
    elif name == "screen_target":
        assert all(s["limit"] == 960 for s in seen.values()) and at(1000, "n_buckets") > at(None, "n_buckets") > at(8000, "n_buckets")
    elif name == "msp_sigmas_x10":
        assert at(0, "n_overflow") > 0 and at(0, "n_overflow") >= at(15, "n_overflow")
    elif name == "msp_site_records":
        assert at(3, "n_overflow") > at(200, "n_overflow"), seen
    elif name == "lean_cold":
        assert at(0, "n_overflow") < at(None, "n_overflow"), seen
    elif name == "hot":
        assert at(None, "n_hot") > 0 and at(0, "n_hot") == 0


@pytest.mark.parametrize("name", [o for o, s in NEUTRAL.items() if "history" in s["legs"]])
def test_sizing_history_options(snk, tune, name):
    """Two read sets of equal size, one error-free and one with errors, alternate on ONE context in both orders: the second call must not
    compute anything from what the first left behind (region sizes from the pilot, the fingerprint that tells the data apart)."""
    import torch
    from supernova_amd import synth
    from supernova_amd.engine import Engine, Params
    dev = torch.device("cuda", 0)
    sets = []
    for seed, error_free in ((0x5EED0A01, True), (0x5EED0A02, False)):
        sp = synth.synth_params(20_000, seed=seed, error_free=error_free)
        rows_h, quals_h, bc_h = synth.synth_host(sp)
        gl = oracle_lib.good_lens(quals_h, 150)
        o = oracle_lib.OracleResult(synth.unpack_rows(rows_h, 150), gl, bc_h, hbv=False)
        sets.append((torch.from_numpy(rows_h.view(np.int32)).to(dev), torch.from_numpy(quals_h).to(dev), torch.from_numpy(bc_h.astype(np.int32)).to(dev), gl, o))
    tune(name, NEUTRAL[name]["values"][0])
    for order in ((0, 1, 0, 1), (1, 0, 1, 1, 0)):
        e = Engine(0)
        try:
            assert e.get_option(name) == 0
            for i in order:
                rows, quals, bc, gl, o = sets[i]
                res = e.count_graph(rows, 150, quals=quals, bc=bc, params=Params(K=48))
                assert np.array_equal(res.good_len().astype(np.uint32), gl)
                _check_oracle(res, o, (name, order, i))
        finally:
            e.close()


def _error_rich(e, n):
    import math
    from supernova_amd import synth
    sp = synth.synth_params(n, seed=0x5EED0E77, sub_ppm=15000, lowq_tail_ppm=200000)
    lam, term, cum = 150 * 15000 / 1e6, math.exp(-150 * 15000 / 1e6), 0.0
    for j in range(4):
        cum += term
        sp.err_cdf[j] = min(0xFFFFFFFF, int(cum * 4294967296.0))
        term *= lam / (j + 1)
    return e.synth(sp)


@pytest.mark.parametrize("name", [o for o, s in NEUTRAL.items() if "scale" in s["legs"]])
def test_adaptive_sizing_options_on_error_rich_reads(snk, tune, name):
    """bucket_fill_pct: the 1.2 M error-rich reads of test_error_rich_reads_are_repartitioned_into_smaller_buckets (not scaled down: whether a
    smaller input still partitions twice was not measured), without the bit filter, whose own bucket target would hide the option.
    chunk_kmers: 200 k reads at 28x, against the C oracle -- on the error-rich reads both values gave the same bucket counts,
    (66847, 66310): they retain too small a share for the option to decide anything, so the claim that those reads exercise it was wrong.
    At 1.2 M reads the C oracle takes minutes, so there the expectation is the device verifier's (snk_dev_check_graph with the reads:
    every count, context and good length recomputed from the input, the graph rules, no violation) plus its digests, which must equal
    those of the verified run with the fixed default bucket size; the 200 k reads get both."""
    import torch
    from supernova_amd import lib
    from supernova_amd.engine import Engine, Params
    from supernova_amd import synth
    n = 1_200_000 if name == "bucket_fill_pct" else 200_000
    e = Engine(0)
    made = []
    oracle = None
    try:
        if name == "bucket_fill_pct":
            rows, quals, bc = _error_rich(e, n)
        else:
            sp = synth.synth_params(n, seed=0x5EED0228, genome_len=n * 150 // 28)
            rows, quals, bc = e.synth(sp)
            rows_h, quals_h, bc_h = synth.synth_host(sp)
            gl = oracle_lib.good_lens(quals_h, 150)
            oracle = (gl, oracle_lib.OracleResult(synth.unpack_rows(rows_h, 150), gl, bc_h, hbv=False))
        reads = lib.SnkDevReads()
        reads.n_reads, reads.rows, reads.row_words, reads.read_len = n, rows.data_ptr(), rows.shape[1], 150
        reads.quals, reads.qstride, reads.bc = quals.data_ptr(), quals.shape[1], bc.data_ptr()

        def verified(eng):
            res = eng.count_graph(rows, 150, quals=quals, bc=bc, params=Params(K=48, sorted_table=False))
            rep = res.check(reads=reads)
            assert rep["violations"] == 0 and rep["levels"] == 3, {k: v for k, v in rep["counters"].items() if v}
            if oracle:
                assert np.array_equal(res.good_len().astype(np.uint32), oracle[0])
                _check_oracle(res, oracle[1], name)
            return res, (rep["table_digest"], rep["unitig_digest"], rep["n_kmers"], rep["n_unitigs"])

        tune("adaptive_buckets", 0)
        r0, want = verified(e)
        assert r0.repartitioned == 0
        tune("adaptive_buckets", 1)
        _pin(tune, name)
        nb = {}
        for value in NEUTRAL[name]["values"]:
            tune(name, value)
            e2 = Engine(0)               # a fresh context: no bucket-size hint from earlier calls
            made.append(e2)
            r1, got1 = verified(e2)
            assert got1 == want and r1.repartitioned == (1 if name == "bucket_fill_pct" else 0), (name, value, r1.repartitioned)
            r2, got2 = verified(e2)      # the second call knows the first one's ratio and retained share
            assert got2 == want and r2.repartitioned == 0, (name, value)
            nb[value] = (r1.n_buckets, r2.n_buckets)
            e2.close()
        lo, hi = NEUTRAL[name]["values"]
        if name == "bucket_fill_pct":
            assert nb[lo][0] > nb[hi][0], nb
        else:
            assert nb[lo][1] > nb[hi][1], nb
    finally:
        for x in made + [e]:
            x.close()
        torch.cuda.empty_cache()


# ---- trim, arena, HBV

@pytest.mark.parametrize("qstride", [152, 160])
def test_rowwise_trim_for_every_layout(engine, tune, qstride):
    import torch
    from supernova_amd.engine import Params
    c = goldens.load("adversarial")
    dev = torch.device("cuda", 0)
    assert qstride % 4 == 0 and qstride <= 160
    tune("trim_rowwise", 1)
    assert engine.get_option("trim_rowwise") == 1
    rng = np.random.default_rng(qstride)
    lens = torch.from_numpy(c.lens.astype(np.uint16).view(np.int16)).to(dev)
    for n in (1, 255, 257, 1000):
        qp = rng.integers(0, 41, (n, qstride), dtype=np.uint8)
        qp[:, :c.read_len] = c.quals[:n]
        qd = torch.from_numpy(qp).to(dev)
        assert qd.data_ptr() % 16 == 0
        for mq, K in ((7, 48), (10, 60), (31, 48)):
            g = engine.trim(qd, c.read_len, K=K, min_qual=mq, lens=lens[:n].contiguous()).cpu().numpy().view(np.uint16)
            assert np.array_equal(g.astype(np.uint32), oracle_lib.good_lens(c.quals[:n], c.lens[:n], K=K, min_qual=mq)), (n, mq, K)
    # ... and inside count_graph, with the fused trim off: padded rows, garbage behind the read
    tune("trim_fused", 0)
    for gname in ("adversarial", "synth_20k_err"):
        exp = _exp(gname, 48)
        c = exp.c
        qp = rng.integers(0, 41, (c.quals.shape[0], qstride), dtype=np.uint8)
        qp[:, :c.read_len] = c.quals
        rows, _, bc, lens_d = _dev(c)
        res = engine.count_graph(rows, c.read_len, quals=torch.from_numpy(qp).to(dev), bc=bc, lens=lens_d, params=Params(K=48), ign_bc_below=c.ign_bc_below)
        assert np.array_equal(res.good_len().astype(np.uint32), oracle_lib.good_lens(c.quals, c.lens))
        _check(res, exp, ("trim_rowwise", gname, qstride))


def test_cached_blocks_instead_of_the_growing_arena(snk, tune):
    from supernova_amd.engine import Engine
    tune("arena_vmm", 0)            # (read when the arena is made: the context has to be born with it)
    e = Engine(0)
    try:
        assert e.get_option("arena_vmm") == 0
        for gname, K in (("synth_2k_err", 48), ("synth_20k_err", 48), ("adversarial", 60), ("synth_6k_clean", 48), ("synth_20k_err", 60), ("synth_2k_err", 48)):
            _check(_run(e, _exp(gname, K)), _exp(gname, K), ("arena_vmm", gname, K))
    finally:
        e.close()


@pytest.mark.parametrize("gname,K", [("adversarial", 48), ("synth_20k_err", 48), ("adversarial", 60)])
def test_strict_device_flood(engine, tune, gname, K):
    from supernova_amd import graphio
    exp = _exp(gname, K)
    g = goldens.Case60(gname) if K == 60 else exp.c

    def flood(res):
        off, bases = res.unitig_arrays()
        h = res.hbv()
        asc = np.frombuffer(b"ACGT", dtype=np.uint8)[bases].tobytes().decode()
        return [asc[int(off[i]):int(off[i + 1])] for i in h["order"]], h

    tune("hbv_dev_min", 1_000_000_000)
    ranked_h, host = flood(_run(engine, exp))
    _pin(tune, "hbv_strict")
    tune("hbv_strict", 1)
    res = _run(engine, exp)
    _check(res, exp, ("hbv_strict", gname, K))
    ranked, h = flood(res)
    assert ranked == ranked_h == exp.unitigs and graphio.hbv_text(ranked, h) == g.exp_hbv
    for k in ("v_left", "v_right", "src", "is_rc", "fwd", "rev"):
        assert np.array_equal(h[k], host[k]), k
    assert h["n_vertices"] == host["n_vertices"] and h["n_edges"] == host["n_edges"]
