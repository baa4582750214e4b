"""Multiplicity at production scale on the device: the 24-bit count saturation on every count path, and MarkDups on duplicate groups
of up to 257 pairs.

The saturating read set (tests/hotgen.py) has one canonical k-mer above 2^24-1 instances and one exactly one below; the expectations are
the reference binary's own (tests/golden/hot_kmers*.npz), to which the C restatement is pinned on the CPU (tests/test_oracle_golden.py).
Every comparison here takes the device's counts RAW -- no min(., 2^24-1) on the device's side -- so a path that does not clamp, clamps at
another value or loses an instance of the k-mer just below the clamp fails.  The grouped run is compared with the C restatement per
group (the reference has no grouped mode).  The large duplicate groups (tests/pathgen.plant_big_groups, tests/golden/dup_groups.npz)
are compared with the reference's paths and flags.

MarkDups is NOT run on the saturating set: its 44 k homopolymer pairs form two duplicate groups, and the device walks a group with
one thread and a quadratic artifact check (snk_dups.hip)."""
import re
import threading

import numpy as np
import pytest

import a48xref
import goldens
import hotgen
import oracle_lib
import pathgen
from test_gpu_graph_check import _device_copy, _reads
from test_gpu_parity import COUNT_VARIANTS
from test_gpu_paths_index import _check_restatement
from test_gpu_pathsx import _same_as_restatement

pytestmark = pytest.mark.gpu
SAT = hotgen.SAT


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


class _Hot:
    """The read set on the device and what the reference made of it, per K."""

    def __init__(self):
        self.c = {K: goldens.load_hot(K) for K in (48, 60)}
        c = self.c[48]
        self.L, self.n = c.read_len, c.codes.shape[0]
        self.rows, self.quals, self.lens, self.bc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
        self.gl = {}
        for K in (48, 60):
            self.gl[K] = oracle_lib.good_lens(c.quals, c.lens, K=K)
            assert hotgen.digest(self.gl[K].astype(np.uint32), [], [], []) == self.c[K].exp_goodlens_digest
        self.n_instances = {K: int(re.search(r"kmer_instances=(\d+)", self.c[K].ref_summary).group(1)) for K in (48, 60)}

    def d(self):
        return dict(rows=self.rows, quals=self.quals, bc=self.bc, lens=self.lens)


@pytest.fixture(scope="module")
def hot(snk):
    return _Hot()


def _key_row(keys, family, K):
    i = np.nonzero((keys == hotgen.homopolymer_key(family, K)).all(axis=1))[0]
    assert len(i) == 1, (family, i)
    return int(i[0])


def _check_table(keys, counts, ctx, unitigs, c):
    kw = c.exp_keys.shape[1]
    assert keys.shape[0] == c.exp_keys.shape[0], (keys.shape, c.exp_keys.shape)
    assert np.array_equal(keys[:, :kw], c.exp_keys) and np.all(keys[:, kw:] == 0)
    i_over, i_under = _key_row(keys, "over", c.K), _key_row(keys, "under", c.K)
    # the two counts this file is about, by name, then every count: raw
    assert int(counts[i_over]) == SAT, ("over", int(counts[i_over]), hotgen.true_count("over", c.K))
    assert int(counts[i_under]) == hotgen.true_count("under", c.K), ("under", int(counts[i_under]))
    assert np.array_equal(counts, c.exp_counts), np.nonzero(counts != c.exp_counts)[0][:5]
    assert np.array_equal(ctx, c.exp_ctx)
    assert unitigs == c.exp_unitigs


def _check(res, hot, K):
    c = hot.c[K]
    assert res.n_reads == hot.n and res.n_instances == hot.n_instances[K]
    assert np.array_equal(res.good_len().astype(np.uint32), hot.gl[K])
    _check_table(res.keys(), res.counts(), res.ctx(), res.unitigs(), c)
    spec = res.spectrum()
    assert len(spec) == SAT + 1 and int(spec[-1]) == 1
    bins = np.nonzero(spec)[0]
    if c.exp_hist_len:          # the reference's own spectrum (K=48); at K=60 it writes none: the histogram of its counts
        assert c.exp_hist_len == SAT + 1
        want_bins, want_vals = c.exp_hist_bins, c.exp_hist_vals
    else:
        want_bins, want_vals = np.unique(c.exp_counts, return_counts=True)
    assert np.array_equal(bins, want_bins) and np.array_equal(spec[bins].astype(np.int64), want_vals.astype(np.int64))


def _run(engine, hot, K=48, **params):
    from supernova_amd.engine import Params
    return engine.count_graph(hot.rows, hot.L, quals=hot.quals, bc=hot.bc if K == 48 else None, lens=hot.lens, params=Params(K=K, **params))


@pytest.mark.parametrize("K", [48, 60])
@pytest.mark.parametrize("stage", ["local", "global"])
def test_default_path_saturates(engine, hot, tune, stage, K):
    """1. The call as it comes: K=48 under the barcode rule (the one-barcode family is dropped whatever its count), K=60 without barcodes
    (it is kept; its unitig is the two-k-mer circle), bucket-local and global graph stage."""
    tune("global_graph", 1 if stage == "global" else 0)
    res = _run(engine, hot, K)
    _check(res, hot, K)
    print(f"[multiplicity] default K={K} {stage}: n_hot_buckets={res.n_hot_buckets} n_overflow={res.n_overflow} n_supermers={res.n_supermers} "
          f"n_buckets={res.n_buckets} buckets_split={res.buckets_split} phases={res.phase_ms}")
    lens = sorted(len(u) for u in res.unitigs())
    assert lens[:2] == [K, K] and (K + 1 in lens) == (K == 60)          # the homopolymers' self-loops; the dinucleotide circle where it is kept


@pytest.mark.parametrize("variant", sorted(COUNT_VARIANTS))
def test_count_variants_saturate(engine, hot, tune, variant):
    """2. The bit filter in front of a 1024-slot table, and the booked slots."""
    env, limit = COUNT_VARIANTS[variant]
    for k, v in env.items():
        tune(k, v)
    res = _run(engine, hot)
    assert engine.last_count_limit() == limit
    _check(res, hot, 48)


def test_whole_hot_bucket_in_one_workgroup(engine, hot, tune):
    """3. hot=0: the homopolymers' minimiser buckets are not expanded; one workgroup counts all 17.9 M instances into one table slot."""
    tune("hot", 0)
    res = _run(engine, hot)
    assert res.n_hot_buckets == 0
    _check(res, hot, 48)


def test_hot_bucket_classes_at_their_cap(engine, hot, tune):
    """4. The hot-bucket expansion forced with classes of 300 instances: 17.9 M instances ask for far more classes than the 2^12 a bucket
    may have, and every instance of a homopolymer k-mer lands in ONE class of one workgroup all the same."""
    tune("hot_min", 8)
    tune("hot_factor", 1)
    tune("hot_class_inst", 300)
    res = _run(engine, hot)
    assert res.n_hot_buckets > 0
    _check(res, hot, 48)


def test_overflow_list_and_noted_hot_buckets(engine, hot, tune):
    """5. A tenth of the slot capacity, buckets noted hot at their first overflowing slot: the homopolymers' supermer records (every k-mer
    of a homopolymer is a supermer of its own: 35 M records behind two minimisers) go through the overflow list."""
    tune("msp_cap_pct", 10)
    tune("msp_hot_factor", 1)
    tune("msp_hot_min", 1)
    res = _run(engine, hot)
    assert res.n_overflow > 0
    _check(res, hot, 48)


def test_dense_partition_saturates(engine, hot, tune):
    """6. The reservation-free partition: no overflow segment."""
    tune("msp_dense", 1)
    res = _run(engine, hot)
    assert res.n_overflow == 0 and res.n_supermers > 0
    _check(res, hot, 48)


def test_bucket_range_passes_saturate(engine, hot, tune):
    """7. Three bucket-range passes over one slot array.  The pass that holds the homopolymers' buckets asks for 30 times the overflow
    list a job of this size is given: the call opens its passes a second time with a list that holds them (SNK_OVF_RETRY, snk_stages.h;
    before, it refused such data)."""
    tune("partition_passes", 3)
    res = _run(engine, hot)
    assert engine.last_partition_passes() == 3
    assert res.n_overflow > 30_000_000
    _check(res, hot, 48)


def test_streamed_slabs_saturate(engine, hot):
    """8. The reads arrive in slabs with a cut inside every family: the count of a k-mer is the sum over the slabs, clamped once.
    A streamed job cannot look at its slabs twice, so its overflow list is sized from the read total it is opened with; 35 M supermers
    behind two minimisers are 25 times the list of a job opened for these 173 k reads.  Such a job is refused with the advice to declare
    a larger total (the total is a bound, not a count), which is what the second job here does: 160 times the reads, a list of 60 M."""
    import torch
    from supernova_amd.engine import Params
    from supernova_amd.lib import SnkError
    sp = hotgen.spans()
    cuts = [0] + [((a + b) // 2) & ~1 for a, b in (sp[f] for f in ("over", "under", "solo", "back"))] + [hot.n]
    assert all(sp[f][0] < x < sp[f][1] for f, x in zip(("over", "under", "solo", "back"), cuts[1:]))

    def job(total):
        engine.stream_begin(hot.L, total, has_bc=True, params=Params(K=48))
        for a, b in zip(cuts[:-1], cuts[1:]):
            r, q, bcs, ln = hot.rows[a:b].clone(), hot.quals[a:b].clone(), hot.bc[a:b].clone(), hot.lens[a:b].clone()
            engine.stream_append(r, hot.L, quals=q, bc=bcs, lens=ln, read_index_base=a)
            torch.cuda.synchronize()
            del r, q, bcs, ln
        return engine.stream_finish()

    with pytest.raises(SnkError, match="larger total"):
        job(hot.n)
    res = job(160 * hot.n)
    assert res.n_overflow > 30_000_000
    _check(res, hot, 48)


@pytest.mark.parametrize("W", [2, 3])
def test_sharded_owner_saturates(snk, hot, W):
    """9. Simulated ranks, each with a slice of the reads (the rank boundaries fall inside the over family, and for three ranks inside the
    under family too): the shares, concatenated and sorted, are the reference's table.  Each homopolymer k-mer is in exactly one share,
    the over k-mer at 2^24-1 although no rank of three holds that many of its instances, the under k-mer at 2^24-2 exactly: the owner
    of the hot minimiser received every record."""
    import torch
    from supernova_amd.engine import Engine, Params
    from supernova_amd.sharded import ShardedEngine, SimWorld
    c = hot.c[48]
    world = SimWorld(W)
    bounds = [hot.n * r // W for r in range(W + 1)]
    out, errs = [None] * W, []

    def worker(r):
        try:
            torch.cuda.set_device(0)
            e = Engine(0)
            lo, hi = bounds[r], bounds[r + 1]
            d = {k: v[lo:hi].contiguous() for k, v in hot.d().items()}
            sh = ShardedEngine(e, world.comm(r))
            res = sh.count_graph(d["rows"], hot.L, quals=d["quals"], bc=d["bc"], lens=d["lens"], params=Params(K=48), read_index_base=lo)
            out[r] = (res.keys(), res.counts(), res.ctx(), res.unitigs(), res.n_instances, int(res.raw.n_hot_buckets))
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
    sp = hotgen.spans()
    assert any(sp["over"][0] < b < sp["over"][1] for b in bounds) and (W == 2 or any(sp["under"][0] < b < sp["under"][1] for b in bounds))
    for fam in ("over", "under"):
        holders = [r for r in range(W) if (out[r][0] == hotgen.homopolymer_key(fam, 48)).all(axis=1).any()]
        assert len(holders) == 1, (fam, holders)
    print(f"[multiplicity] sharded W={W}: instances per rank {[o[4] for o in out]}, hot buckets per rank {[o[5] for o in out]}")
    keys = np.concatenate([o[0] for o in out])
    counts = np.concatenate([o[1] for o in out])
    ctx = np.concatenate([o[2] for o in out])
    order = np.lexsort((keys[:, 3], keys[:, 2], keys[:, 1], keys[:, 0]))
    unitigs = sorted((u for o in out for u in o[3]), key=lambda s: (-len(s), s))
    _check_table(keys[order], counts[order], ctx[order], unitigs, c)


@pytest.fixture(scope="module")
def grouped_oracles(hot):
    """Two groups: the over family with one half of the background, the under and solo families with the other half -- and the C
    restatement on each group's reads alone (frequency rule only), raw counts."""
    c = hot.c[48]
    sp = hotgen.spans()
    group = np.full(hot.n, 7, np.int32)
    group[sp["over"][0]:sp["over"][1]] = 3
    a, b = sp["back"]
    group[a:(a + b) // 2 & ~1] = 3
    return group, {int(g): oracle_lib.OracleResult(c.codes[group == g], hot.gl[48][group == g], None, min_freq=3, min_bc=0, hbv=False)
                   for g in (3, 7)}


def test_grouped_graphs_saturate(engine, hot, grouped_oracles):
    """10. Per-group graphs: each group's table, raw counts, contexts and unitigs equal the restatement's on that group's reads.  (The
    restatement's clamp, snk_oracle.c, is pinned to the reference by the ungrouped fixtures.)"""
    import torch
    from supernova_amd.engine import Params
    group, oracles = grouped_oracles
    res = engine.count_graph(hot.rows, hot.L, quals=hot.quals, bc=None, lens=hot.lens, group=torch.from_numpy(group).to(hot.rows.device),
                             params=Params(K=48, min_freq=3, min_bc=0, grouped=True, sorted_table=False))
    k, cnt, ctx = res.keys(), res.counts(), res.ctx()
    off, bases = res.unitig_arrays()
    ug = res.unitig_groups()
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    total = 0
    for gid, o in oracles.items():
        m = k[:, 3] == gid
        kk, cc, xx = k[m], cnt[m], ctx[m]
        order = np.lexsort((kk[:, 2], kk[:, 1], kk[:, 0]))
        assert np.array_equal(kk[order][:, :3], o.keys[:, :3]), gid
        assert np.array_equal(cc[order], o.counts), (gid, np.nonzero(cc[order] != o.counts)[0][:5])
        assert np.array_equal(xx[order], o.ctx), gid
        us = sorted((lut[bases[int(off[u]):int(off[u + 1])]].tobytes().decode() for u in np.nonzero(ug == gid)[0]), key=lambda t: (-len(t), t))
        assert us == o.unitigs, gid
        total += int(m.sum())
    assert total == k.shape[0]
    assert int(oracles[3].counts.max()) == SAT and int(oracles[7].counts.max()) == SAT - 1          # what the groups are for
    assert int(cnt.max()) == SAT and int(np.sort(cnt)[-2]) == SAT - 1


def test_verifier_compares_counts_under_the_clamp(engine, hot):
    """11. snk_dev_check_graph on the saturating set: the result is clean at graph level and at reads level (every count recounted from
    the reads).  Its contract for counts is min(., 2^24-1) on both sides: the over k-mer at 2^24+4 in a copied table is still clean, the
    under k-mer moved from 2^24-2 to 2^24-1 is exactly one count_mismatch."""
    c = hot.c[48]
    res = _run(engine, hot)
    rep = res.check()
    assert rep["violations"] == 0, {k: v for k, v in rep["counters"].items() if v}
    rep = res.check(reads=_reads(hot.d(), hot.L, hot.n))
    assert rep["levels"] == 3 and rep["violations"] == 0, {k: v for k, v in rep["counters"].items() if v}
    assert rep["n_instances"] == res.n_instances == hot.n_instances[48]
    us = sorted(c.exp_unitigs, key=lambda s: s[:48])
    keys4 = np.concatenate([c.exp_keys, np.zeros((len(c.exp_keys), 1), np.uint32)], axis=1)
    for family, value, want in (("over", SAT + 5, {}), ("under", SAT, {"count_mismatch": 1})):
        counts = c.exp_counts.copy()
        counts[_key_row(keys4, family, 48)] = value
        k, n, x, off, b = _device_copy(engine, c.exp_keys, counts, c.exp_ctx, us, 48)
        rep = engine.check_graph(k, n, x, off, b, K=48, min_freq=3, n_instances=hot.n_instances[48], reads=_reads(hot.d(), hot.L, hot.n))
        assert {kk: v for kk, v in rep["counters"].items() if v} == want, (family, value)


# ---- duplicate groups of 7 to 257 pairs

@pytest.mark.parametrize("pad_seed", [None, 77])
def test_big_duplicate_groups_match_reference(engine, pad_seed):
    """Count, graph, paths, MarkDups, paths index and pathsX on the dup_groups reads (groups of 7, 63, 64, 65, 255, 256 and 257 pairs with
    interleaved runs; a group spans more than one 256-thread block of the flag kernels): the reference's paths, its flag per pair and
    its inter-barcode rate exactly, its logged artifact percentage, the artifact count of the C restatement (pinned to that log on the
    CPU), and the restatements of the index and of the compressed paths.  Once more with the quality rows padded."""
    c = goldens.load("dup_groups")
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc, pad_seed=pad_seed)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl)
    assert np.array_equal(res.keys()[:, :3], c.exp_keys) and np.array_equal(res.counts(), c.exp_counts) and res.unitigs() == c.exp_unitigs
    off, ne, edges, info = res.path_reads(rows, c.read_len, dq, lens=dl, mark_dups=True, bc=dbc, paths_index=True, pathsx=True)
    assert np.array_equal(ne.astype(np.int64), c.exp_path_n) and np.array_equal(edges, c.exp_path_edges) and np.array_equal(off, c.exp_path_off)
    d = info["dups"]
    print(f"[multiplicity] dup_groups pad={pad_seed}: snk_dev_mark_dups {d['ms']:.3f} ms")
    assert np.array_equal(d["dup"], c.exp_dup), np.nonzero(d["dup"] != c.exp_dup)[0][:10]
    assert d["interdup_rate"] == c.exp_interdup
    o_dup, o_art, o_rate, o_nd, o_ni = oracle_lib.mark_dups(c.codes, c.quals, c.lens, c.exp_path_off, c.exp_path_n, c.exp_path_edges, bc=c.bc)
    assert (d["n_dup_reads"], d["n_interdup_reads"], d["n_dup_pairs"], d["n_art_pairs"]) == (o_nd, o_ni, int(o_dup.sum()), int(o_art.sum()))
    assert d["n_placed"] == int((c.exp_path_n > 0).sum())
    assert float(f"{100.0 * d['n_art_pairs'] / len(o_dup):.2g}") == float(f"{c.exp_art_perc:.2g}")
    _check_restatement(ne, edges, info)
    _same_as_restatement(info, off, ne, edges, a48xref.parse_hbv(c.exp_ahbv))
