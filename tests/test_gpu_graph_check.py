"""snk_dev_check_graph on the device: clean on every golden case and mode, digests equal to the reference's, every planted corruption
found counter for counter as the host restatement (tests/graphcheck_ref.py) finds it, digests additive over sharded ranks, equal across
configurations, and the checked result left as it was."""
import json
import os
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

import goldens
import graphcheck_ref as R
from test_graph_check_host import plants

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MODES = ["default", "unsorted", "global", "long_minimiser", "streamed"]
READS_LEVEL = ("count_mismatch", "ctx_mismatch", "good_len_mismatch", "instances_mismatch")


@pytest.fixture(scope="module")
def engine(snk):
    from supernova_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _inputs(c):
    return dict(rows=_dev(c.rows.view(np.int32)), quals=_dev(c.quals), bc=_dev(c.bc.astype(np.int32)),
                lens=_dev(c.lens.astype(np.uint16).view(np.int16)))


def _run(e, c, mode, K=48):
    from supernova_amd.engine import Params
    d = _inputs(c)
    p = Params(K=K, sorted_table=mode != "unsorted", global_graph=mode == "global", long_minimiser=mode == "long_minimiser")
    if mode == "streamed":
        e.stream_begin(c.read_len, c.rows.shape[0], has_bc=True, params=p)
        h = c.rows.shape[0] // 2
        for lo, hi in ((0, h), (h, c.rows.shape[0])):
            e.stream_append(d["rows"][lo:hi].contiguous(), c.read_len, quals=d["quals"][lo:hi].contiguous(), bc=d["bc"][lo:hi].contiguous(),
                            lens=d["lens"][lo:hi].contiguous(), ign_bc_below=c.ign_bc_below, read_index_base=lo)
        return e.stream_finish(), d
    return e.count_graph(d["rows"], c.read_len, quals=d["quals"], bc=d["bc"], lens=d["lens"], params=p, ign_bc_below=c.ign_bc_below), d


def _reads(d, read_len, n):
    from supernova_amd import lib
    r = lib.SnkDevReads()
    r.n_reads, r.rows, r.row_words, r.read_len = n, d["rows"].data_ptr(), d["rows"].shape[1], read_len
    r.quals, r.qstride, r.lens = d["quals"].data_ptr(), d["quals"].shape[1], d["lens"].data_ptr()
    return r


def _ref_circles(keys, counts, ctx, unitigs, K=48):
    """circles among the reference's unitigs, as the host restatement classifies them"""
    return R.check(keys, counts, ctx, sorted(unitigs, key=lambda s: s[:K]), K, 3)["n_circles"]


def _ref_digests(keys, counts, ctx, unitigs):
    from supernova_amd import graphcheck as G
    return G.digest_table(keys, counts, ctx), G.digest_strings(unitigs)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", goldens.CASES)
def test_clean_on_golden_cases(engine, name, mode):
    c = goldens.load(name)
    res, d = _run(engine, c, mode)
    # the global graph stage leaves its unitigs in another order than by their first K bases: every other rule holds there
    rep = res.check(reads=_reads(d, c.read_len, c.rows.shape[0]), ordered=mode != "global")
    assert rep["violations"] == 0, {k: v for k, v in rep["counters"].items() if v}
    assert rep["levels"] == 3 and rep["n_kmers"] == res.n_kmers
    assert rep["n_circles"] == _ref_circles(c.exp_keys, c.exp_counts, c.exp_ctx, c.exp_unitigs)
    assert (rep["table_digest"], rep["unitig_digest"]) == _ref_digests(c.exp_keys, c.exp_counts, c.exp_ctx, c.exp_unitigs)


@pytest.mark.parametrize("name", goldens.K60_CASES)
def test_clean_at_k60(engine, name):
    c60 = goldens.Case60(name)
    c = c60.base
    from supernova_amd.engine import Params
    d = _inputs(c)
    res = engine.count_graph(d["rows"], c.read_len, quals=d["quals"], lens=d["lens"], params=Params(K=60, min_bc=0))
    rep = res.check(reads=_reads(d, c.read_len, c.rows.shape[0]))
    assert rep["violations"] == 0, rep["counters"]
    assert rep["n_circles"] == _ref_circles(c60.exp_keys, c60.exp_counts, c60.exp_ctx, c60.exp_unitigs, 60)
    assert (rep["table_digest"], rep["unitig_digest"]) == _ref_digests(c60.exp_keys, c60.exp_counts, c60.exp_ctx, c60.exp_unitigs)


@pytest.mark.parametrize("name", ["synth_20k_err", "adversarial", "synth_4k_dups"])
def test_clean_grouped(engine, name):
    from supernova_amd.engine import Params
    c = goldens.load(name)
    d = _inputs(c)
    res = engine.count_graph(d["rows"], c.read_len, quals=d["quals"], lens=d["lens"], group=d["bc"], params=Params(K=48, grouped=True, min_bc=0))
    r = _reads(d, c.read_len, c.rows.shape[0])
    r.group = d["bc"].data_ptr()
    rep = res.check(reads=r)
    assert rep["violations"] == 0, {k: v for k, v in rep["counters"].items() if v}
    assert rep["n_unitigs"] == res.n_unitigs


def _device_copy(e, keys_w, counts, ctx, unitigs, K):
    """golden-form arrays -> device tensors in the result layout"""
    import torch
    from supernova_amd import graphio
    w = np.asarray(keys_w, dtype=np.uint64)
    if w.shape[1] < 4:
        w = np.concatenate([w, np.zeros((len(w), 4 - w.shape[1]), np.uint64)], axis=1)
    lohi = np.stack([(w[:, 2] << np.uint64(32)) | w[:, 3], (w[:, 0] << np.uint64(32)) | w[:, 1]], axis=1)
    off, bases = graphio.unitigs_to_arrays(unitigs)
    return (_dev(lohi), _dev(np.asarray(counts, np.uint32).view(np.int32)), _dev(np.asarray(ctx, np.uint8)), _dev(off.view(np.int64)),
            _dev(bases if len(bases) else np.zeros(1, np.uint8)))


@pytest.mark.parametrize("name", ["synth_20k_err", "adversarial"])
def test_plants_match_the_host_restatement(engine, name):
    c = goldens.load(name)
    cases = plants(c.exp_keys, c.exp_counts, c.exp_ctx, c.exp_unitigs, 48)
    us = sorted(c.exp_unitigs, key=lambda s: s[:48])
    # two more: the tail of the bases zeroed (the round-6 bug), one table row dropped
    tail = "".join(us)
    cut = len(tail) - (len(tail) * 87) // 100
    zeroed, pos = [], 0
    for u in us:
        zeroed.append("".join(ch if pos + i < cut else "A" for i, ch in enumerate(u)))
        pos += len(u)
    cases.append(("zero_tail", c.exp_keys, c.exp_counts, c.exp_ctx, zeroed, "unitig_kmer_missing"))
    keep = np.ones(len(c.exp_keys), bool)
    keep[len(keep) // 2] = False
    cases.append(("drop_row", c.exp_keys[keep], c.exp_counts[keep], c.exp_ctx[keep], us, "unitig_kmer_missing"))
    for plant, keys, counts, ctx, uts, counter in cases:
        host = R.check(keys, counts, ctx, uts, 48, 3)["counters"]
        k, n, x, off, b = _device_copy(engine, keys, counts, ctx, uts, 48)
        rep = engine.check_graph(k, n, x, off, b, K=48, min_freq=3)
        assert rep["counters"][counter] > 0, plant
        graph_level = {kk: v for kk, v in rep["counters"].items() if kk not in READS_LEVEL}
        assert graph_level == {kk: host[kk] for kk in graph_level}, (plant, graph_level, host)


def test_result_stays_valid(engine):
    c = goldens.load("adversarial")
    res, d = _run(engine, c, "default")
    before = res.bv_image()
    rep = res.check(reads=_reads(d, c.read_len, c.rows.shape[0]))
    assert rep["violations"] == 0 and rep["peak_bytes"] > 0
    assert res.bv_image() == before


def test_configurations_share_digests(engine, tune):
    import torch
    from supernova_amd import synth
    from supernova_amd.engine import Params
    tune("plan_mem_mb", 256)
    n = 2_000_000
    sp = synth.synth_params(n, seed=77)
    rows, quals, bc = engine.synth(sp)
    gl = engine.trim(quals, 150)
    del quals
    torch.cuda.synchronize()
    seen = set()
    for p in (Params(), Params(sorted_table=False), Params(global_graph=True), Params(long_minimiser=True)):
        res = engine.count_graph(rows, 150, good_len=gl, bc=bc, params=p)
        assert engine.last_partition_passes() > 1
        rep = res.check(ordered=not p.global_graph)
        assert rep["violations"] == 0, (p, {k: v for k, v in rep["counters"].items() if v})
        seen.add((rep["table_digest"], rep["unitig_digest"], rep["n_circles"]))
    engine.clear_option("plan_mem_mb")          # the same job in one pass
    res = engine.count_graph(rows, 150, good_len=gl, bc=bc, params=Params())
    assert engine.last_partition_passes() == 1
    rep = res.check()
    assert rep["violations"] == 0, {k: v for k, v in rep["counters"].items() if v}
    seen.add((rep["table_digest"], rep["unitig_digest"], rep["n_circles"]))
    assert len(seen) == 1


def test_reads_level_at_2m_reads(engine):
    import torch
    from supernova_amd import lib, synth
    n = 2_000_000
    sp = synth.synth_params(n, seed=91)
    rows, quals, bc = engine.synth(sp)
    res = engine.count_graph(rows, 150, quals=quals, bc=bc)
    r = lib.SnkDevReads()
    r.n_reads, r.rows, r.row_words, r.read_len = n, rows.data_ptr(), rows.shape[1], 150
    r.quals, r.qstride, r.good_len = quals.data_ptr(), quals.shape[1], res.raw.good_len
    rep = res.check(reads=r)
    torch.cuda.synchronize()
    assert rep["levels"] == 3 and rep["violations"] == 0, rep["counters"]
    assert rep["n_instances"] == res.n_instances


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("name", ["synth_20k_err", "adversarial"])
def test_sharded_digests_add_up(snk, W, name):
    import torch
    from supernova_amd.engine import Engine, Params
    from supernova_amd.sharded import ShardedEngine, SimWorld
    c = goldens.load(name)
    world = SimWorld(W)
    n = c.rows.shape[0]
    bounds = [n * r // W for r in range(W + 1)]
    out, errs = [None] * W, []

    def worker(r):
        try:
            torch.cuda.set_device(0)
            e = Engine(0)
            lo, hi = bounds[r], bounds[r + 1]
            d = {k: v[lo:hi].contiguous() for k, v in _inputs(c).items()}
            sh = ShardedEngine(e, world.comm(r))
            res = sh.count_graph(d["rows"], c.read_len, quals=d["quals"], bc=d["bc"], lens=d["lens"], params=Params(K=48),
                                 ign_bc_below=c.ign_bc_below, read_index_base=lo)
            out[r] = res.check()
            e.close()
        except BaseException as ex:  # noqa: BLE001
            errs.append(ex)
            world.barrier_obj.abort()

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(W)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
    M = (1 << 64) - 1
    assert all(o["levels"] == 0 for o in out)
    got = (sum(o["table_digest"] for o in out) & M, sum(o["unitig_digest"] for o in out) & M)
    assert got == _ref_digests(c.exp_keys, c.exp_counts, c.exp_ctx, c.exp_unitigs)


@pytest.mark.parametrize("args", [["2e6"], ["2e6", "48", "1"], ["2e6", "60"]])
def test_check_job_tool(snk, args):
    env = dict(os.environ, SNK_TUNING="plan_mem_mb=256")
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_job.py"), *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    row = json.loads(r.stdout.strip().splitlines()[-1])
    assert row["clean"] and row["violations"] == 0, row


def test_check_job_tool_finds_the_plant(snk):
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_job.py"), "2e6", "--plant"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    row = json.loads(r.stdout.strip().splitlines()[-1])
    assert row["counters"].get("unitig_kmer_missing", 0) > 0 and row["counters"].get("kmer_uncovered", 0) > 0, row


def test_mspedges_check_graph(snk, tmp_path):
    from supernova_amd import dfin, synth
    sp = synth.synth_params(20000, seed=0x5EED0D0F, unbarcoded_ppm=0, pairs_per_bc=100)
    dfin.write_synth_df(tmp_path / "s", sp, qual_jitter=8, threads=2)
    exe = ROOT / "supernova_amd" / "bin" / "snk_mspedges"
    out = tmp_path / "asm_graph.bv"
    r = subprocess.run([str(exe), f"LR={tmp_path / 's.fastb'}", f"OUT={out}", "CHECK=graph"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads((tmp_path / "asm_graph.bv.check.json").read_text())
    assert rep["n_unitigs"] > 0 and not any(rep["counters"].values()), rep
    from supernova_amd import graphcheck as G
    assert int(rep["unitig_digest"], 16) == G.digest_bv(str(out))


def test_grouped_plant_matches_the_host_restatement(engine):
    """One unitig of a per-group run given a group its k-mers do not carry: group_mismatch, on the device as on the host."""
    import torch
    from supernova_amd import graphio
    from supernova_amd.engine import Params
    c = goldens.load("adversarial")
    d = _inputs(c)
    res = engine.count_graph(d["rows"], c.read_len, quals=d["quals"], lens=d["lens"], group=d["bc"], params=Params(K=48, grouped=True, min_bc=0))
    keys, counts, ctx = res.keys(), res.counts(), res.ctx()
    off, bases = res.unitig_arrays()
    ug = res.unitig_groups().copy()
    us = graphio.arrays_to_unitigs(off, bases)
    j = max(range(len(us)), key=lambda i: len(us[i]))
    ug[j] = 0x7FFFFFF0
    host = R.check(keys, counts, ctx, us, 48, 3, unitig_groups=ug, key_groups=keys[:, 3], sorted_table=True, ordered=False)["counters"]
    lohi = res._dl(res.raw.keys, res.n_kmers * 16, np.uint64, (res.n_kmers, 2))
    rep = engine.check_graph(_dev(lohi), _dev(counts.view(np.int32)), _dev(ctx), _dev(off.view(np.int64)), _dev(bases),
                             K=48, min_freq=3, unitig_group=_dev(ug.view(np.int32)), ordered=False)
    assert rep["counters"]["group_mismatch"] == len(us[j]) - 47 and rep["counters"]["unitig_kmer_missing"] == 0
    dev = {k: v for k, v in rep["counters"].items() if k not in READS_LEVEL}
    assert dev == {k: host[k] for k in dev}, (dev, host)
    torch.cuda.synchronize()


def test_df_seam_result_is_clean_and_equals_the_resident_run(engine, tmp_path):
    """The DF-seam entry (snk_dev_ingest_df_count_graph) on a snk_write_df triple, table in bucket order as snk_mspedges keeps it: clean,
    and its digests are those of a resident count_graph on the same reads."""
    from supernova_amd import dfin, synth
    from supernova_amd.engine import Params
    sp = synth.synth_params(30000, seed=0x5EED0D11, unbarcoded_ppm=0, pairs_per_bc=100)
    rows, quals, bc = synth.synth_host(sp)
    dfin.write_df(tmp_path / "s", rows, quals, bc=bc, read_len=150, threads=2)
    f = dfin.DfFiles(tmp_path / "s")
    p = Params(K=48, sorted_table=False)
    res, _st = f.count_graph(engine, p)
    assert res.params is p
    rep = res.check()
    assert rep["violations"] == 0 and rep["levels"] == 1, {k: v for k, v in rep["counters"].items() if v}
    ref = engine.count_graph(_dev(rows.view(np.int32)), 150, quals=_dev(quals), bc=_dev(bc.astype(np.int32)), params=Params(K=48))
    want = ref.check()
    assert want["violations"] == 0
    assert (rep["table_digest"], rep["unitig_digest"], rep["n_kmers"]) == (want["table_digest"], want["unitig_digest"], want["n_kmers"])
    f.close()
