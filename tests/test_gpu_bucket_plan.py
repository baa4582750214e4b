"""The bucket plan of a call -- how many buckets, which count kernel, how many usable table slots -- pinned run by run against
tests/golden/plans/plan_pins.json, which was recorded on the commit before the sizing policy moved into snk_plan (csrc/snk_plan.h).
A run is a case, an option setting and a call number on ONE context: the second call sizes its buckets from the history the first left.
Every run checks its results against the golden (or the C oracle) as well: a plan that matched while results broke would mean nothing.
plan_mem_mb is pinned throughout, so the free memory of a shared device cannot enter a plan.

record_all() is what wrote the pins file (tools use: python -c "import test_gpu_bucket_plan as t; t.record_all(path)")."""
import json
import threading
from pathlib import Path

import numpy as np
import pytest

import goldens
from test_gpu_option_invariance import _check, _check_groups, _dev, _exp, _grouped_case, _run

pytestmark = pytest.mark.gpu

PINS = Path(__file__).resolve().parent / "golden" / "plans" / "plan_pins.json"
PLAN_MEM_MB = 65536
CASES = [("synth_20k_err", 48), ("synth_20k_err", 60), ("adversarial", 48)]
# option settings of the resident runs; screen_target only decides behind the bit filter, so it is pinned once alone and once with the filter on
SETTINGS = [{}, {"chunk_kmers": 20}, {"count_tight": 1984}, {"count_tight": 0}, {"count_screen_ng": 2}, {"target_inst": 1000}, {"screen_target": 1000},
            {"screen_target": 1000, "count_screen_ng": 2}, {"bucket_fill_pct": 25}, {"adaptive_buckets": 0}]


def _sid(setting):
    return ",".join(f"{k}={v}" for k, v in setting.items()) or "default"


def _engine(setting):
    from supernova_amd.engine import Engine
    e = Engine(0)
    e.set_option("plan_mem_mb", PLAN_MEM_MB)
    for k, v in setting.items():
        e.set_option(k, v)
    return e


def _plan(e, res):
    t = e.get_tuning()
    return dict(n_buckets=res.n_buckets, last_count_limit=e.last_count_limit(), last_count_kernel=t["last_count_kernel"],
                last_partition_passes=e.last_partition_passes(), repartitioned=res.repartitioned, n_overflow=res.n_overflow)


def runs_resident(gname, K, setting, n_buckets=0):
    exp = _exp(gname, K)
    e = _engine(setting)
    out = {}
    try:
        for call in (1, 2):
            rid = f"resident/{gname}/K{K}/{_sid(setting)}/nb{n_buckets}/call{call}"
            res = _run(e, exp, n_buckets)
            _check(res, exp, rid)
            out[rid] = _plan(e, res)
    finally:
        e.close()
    return out


def runs_grouped(count_screen):
    import torch
    from supernova_amd.engine import Params
    c, group, want = _grouped_case()
    rows, quals, bc, lens = _dev(c)
    g_dev = torch.from_numpy(group).to(rows.device)
    e = _engine({"count_screen": count_screen})
    out = {}
    try:
        for call in (1, 2):
            rid = f"grouped/synth_20k_err/count_screen={count_screen}/call{call}"
            res = e.count_graph(rows, c.read_len, quals=quals, bc=None, lens=lens, group=g_dev,
                                params=Params(K=48, min_freq=3, min_bc=0, grouped=True, sorted_table=False))
            _check_groups(res, want, (rid,))
            out[rid] = _plan(e, res)
    finally:
        e.close()
    return out


def runs_streamed():
    from supernova_amd.engine import Params
    exp = _exp("synth_20k_err", 48)
    c = exp.c
    rows, quals, bc, lens = _dev(c)
    n = rows.shape[0]
    cut = (n // 3) & ~1
    e = _engine({})
    out = {}
    try:
        for job in (1, 2):
            rid = f"streamed/synth_20k_err/K48/job{job}"
            e.stream_begin(c.read_len, n, has_bc=True, params=Params(K=48))
            for a, b in ((0, cut), (cut, n)):
                e.stream_append(rows[a:b].contiguous(), c.read_len, quals=quals[a:b].contiguous(), bc=bc[a:b].contiguous(), lens=lens[a:b].contiguous(),
                                ign_bc_below=c.ign_bc_below, read_index_base=a)
            res = e.stream_finish()
            assert res.n_reads == n
            _check(res, exp, rid)
            out[rid] = _plan(e, res)
    finally:
        e.close()
    return out


def runs_sharded(W):
    """W in-process ranks, two steps over the same communicators: the second step sizes its buckets from the group's history."""
    import torch
    from supernova_amd.engine import Params
    from supernova_amd.sharded import ShardedEngine, SimWorld
    from test_gpu_sharded import check
    c = goldens.load("synth_20k_err")
    dev = torch.device("cuda", 0)
    world = SimWorld(W)
    n = c.rows.shape[0]
    bounds = [n * r // W for r in range(W + 1)]
    outs, plans, errs = [[None] * W for _ in range(2)], [[None] * W for _ in range(2)], []

    def worker(r):
        try:
            torch.cuda.set_device(0)
            e = _engine({})
            lo, hi = bounds[r], bounds[r + 1]
            rows = torch.from_numpy(c.rows[lo:hi].view(np.int32).copy()).to(dev)
            quals = torch.from_numpy(np.ascontiguousarray(c.quals[lo:hi])).to(dev)
            bc = torch.from_numpy(c.bc[lo:hi].astype(np.int32)).to(dev)
            lens = torch.from_numpy(c.lens[lo:hi].astype(np.uint16).view(np.int16)).to(dev)
            sh = ShardedEngine(e, world.comm(r))
            for step in range(2):
                res = sh.count_graph(rows, c.read_len, quals=quals, bc=bc, lens=lens, params=Params(K=48), ign_bc_below=c.ign_bc_below,
                                     read_index_base=lo, total_reads=n)
                outs[step][r] = dict(keys=res.keys(), counts=res.counts(), ctx=res.ctx(), spectrum=res.spectrum(), n_instances=res.n_instances, unitigs=res.unitigs())
                plans[step][r] = dict(n_buckets=res.n_buckets, last_count_limit=e.last_count_limit(), last_count_kernel=e.get_tuning()["last_count_kernel"],
                                      last_partition_passes=e.last_partition_passes(), repartitioned=int(res.raw.repartitioned))
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
    out = {}
    for step in range(2):
        check(outs[step], c)
        assert all(p == plans[step][0] for p in plans[step]), plans[step]      # the ranks reach identical plans
        out[f"sharded/synth_20k_err/K48/W{W}/step{step + 1}"] = plans[step][0]
    return out


def _pinned(got):
    pins = json.loads(PINS.read_text())
    for rid, plan in got.items():
        print(rid, plan)
        assert rid in pins, rid
        assert plan == pins[rid], (rid, plan, pins[rid])


@pytest.mark.parametrize("setting", SETTINGS, ids=_sid)
@pytest.mark.parametrize("gname,K", CASES)
def test_resident_plan_is_the_pinned_one(snk, gname, K, setting):
    _pinned(runs_resident(gname, K, setting))


def test_forced_bucket_count_plan_is_the_pinned_one(snk):
    _pinned(runs_resident("synth_20k_err", 48, {}, n_buckets=997))


@pytest.mark.parametrize("count_screen", [0, 2])
def test_grouped_plan_is_the_pinned_one(snk, count_screen):
    _pinned(runs_grouped(count_screen))


def test_streamed_plan_is_the_pinned_one(snk):
    _pinned(runs_streamed())


@pytest.mark.parametrize("W", [1, 2])
def test_sharded_plan_is_the_pinned_one(snk, W):
    _pinned(runs_sharded(W))


def record_all(path=PINS):
    got = {}
    for gname, K in CASES:
        for setting in SETTINGS:
            got.update(runs_resident(gname, K, setting))
    got.update(runs_resident("synth_20k_err", 48, {}, n_buckets=997))
    for s in (0, 2):
        got.update(runs_grouped(s))
    got.update(runs_streamed())
    for W in (1, 2):
        got.update(runs_sharded(W))
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(json.dumps(got, indent=1, sort_keys=True) + "\n")
    return got
