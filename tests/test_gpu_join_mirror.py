"""The join's list ranking after the mirror walk (snk_rank.hip, snk_rank_lists): one list of each mirror pair is walked a second time and
writes the ranks of both, the "every state ranked" check is a count, and the set-up passes are folded.  rk[] must come out as before,
so every result must: the hand-made read sets of tests/handreads.py against the reference's goldens, under the default ranking, under
plain pointer jumping (rank_wyllie=1) and under splitter spacings of 2, 32 and 4096 states (split_log2 = 1, 5, 12) -- byte-equal with
the golden AND between the legs: good lengths, table, counts, contexts, spectrum, unitigs in order; circle flags and the table's
checksum through the counters the result carries (n_circles, n_fragments, n_kmers, total bases).

Which ranking ran.  The ruling set only runs from 2048 fragments on (2 * n_fragments >= 4096), and a fragment is never shorter than
the run of k-mers that share a minimiser, so more buckets stop making fragments long before that for a set of a few thousand k-mers:
at n_buckets = 4096, 65536 and 2^20 alike tiny_circles gives 123 / 89 fragments (K = 48 / 60), chain_1025 978 / 728, forest_257 333 /
309, turns 68 / 52, mixed_seed1 648 / 606; only circles_5000 (6407 / 5000) and long (4111 / 3057) have enough.  The legs of the small
sets (SMALL) hold the join to the goldens with the general algorithm, and assert that this is what they took.  Their topologies --
circles of 31 / 32 / 33 and 255 / 256 / 257 k-mers, palindromes, strands that turn into their own reverse complement -- go through
the ruling set in test_all_sets_in_one_job, where the seven sets are one job of some ten thousand fragments, held against the C
oracle on the same reads.  Every leg prints and asserts what it took."""
import functools

import numpy as np
import pytest

import handreads as hr
import oracle_lib

pytestmark = pytest.mark.gpu

CASES = ("tiny_circles", "circles_5000", "chain_1025", "forest_257", "turns", "long", "mixed_seed1")
SMALL = ("tiny_circles", "chain_1025", "forest_257", "turns", "mixed_seed1")          # cannot hold 2048 fragments (see above)
N_BUCKETS = 4096          # (more buckets give no more fragments: see above)
LEGS = (("default", None, None), ("rank_wyllie=1", "rank_wyllie", 1), ("split_log2=1", "split_log2", 1), ("split_log2=5", "split_log2", 5),
        ("split_log2=12", "split_log2", 12))


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


def _run(engine, r, K, group=None, **params):
    import torch
    from supernova_amd.engine import Params
    dev = torch.device("cuda", 0)
    kw = dict(group=torch.from_numpy(group).to(dev)) if group is not None else {}
    bc = torch.from_numpy(r.bc.astype(np.int32)).to(dev) if K == 48 and group is None else None
    return engine.count_graph(torch.from_numpy(hr.rows(r).view(np.int32)).to(dev), r.read_len, quals=torch.from_numpy(np.ascontiguousarray(r.quals)).to(dev), bc=bc,
                              lens=torch.from_numpy(r.lens.astype(np.uint16).view(np.int16)).to(dev), params=Params(K=K, **params), **kw)


def _got(res, K):
    return hr.normalised(K, res.good_len(), res.keys(), res.counts(), res.ctx(), res.spectrum(), res.unitigs())


def _evidence(res):
    return dict(n_fragments=int(res.n_fragments), rank_rounds=int(res.rank_rounds), n_circles=int(res.n_circles), n_kmers=int(res.n_kmers),
                n_unitigs=int(res.n_unitigs), total_bases=int(res.unitig_total_bases))


def _legs(engine, tune, run, tag, ruling, size="n_fragments"):
    """run() under every leg -> the default leg's result; asserts that the legs agree byte for byte and that each took the ranking it
    is there for (ruling: the job has the fragments for the ruling set)"""
    first = first_ev = None
    for leg, option, value in LEGS:
        engine.clear_option("rank_wyllie")
        engine.clear_option("split_log2")
        if option:
            tune(option, value)
        res = run()
        got, ev = res[0], res[1]
        print(f"[join_mirror] {tag} {leg}: {ev}")
        assert (ev[size] * 2 >= 4096) == ruling, (tag, leg, ev)          # (the global stage ranks k-mers, not fragments)
        if first is None:
            first, first_ev = got, ev
            continue
        for f in hr.FIELDS:
            assert np.array_equal(first[f], got[f]), (tag, leg, f)
        # the same lists whatever ranks them: fragments, circles closed by the join, table and unitig totals
        assert {k: v for k, v in ev.items() if k != "rank_rounds"} == {k: v for k, v in first_ev.items() if k != "rank_rounds"}, (tag, leg, ev, first_ev)
        if ruling and leg == "rank_wyllie=1" and ev["n_fragments"] >= 1 << 13:
            # pointer jumping over all states reports one round per doubling until nothing changes; the ruling set reports the
            # rounds over its splitter list, issued in batches of rank_round_batch0 = 12: the counts differ where the lists are long
            print(f"[join_mirror] {tag}: rounds default {first_ev['rank_rounds']}, wyllie {ev['rank_rounds']}")
    return first, first_ev


@pytest.mark.parametrize("noise", [False, True], ids=["clean", "noisy"])
@pytest.mark.parametrize("K", hr.KS)
@pytest.mark.parametrize("name", CASES)
def test_case_equals_the_reference_under_every_ranking(engine, tune, name, K, noise):
    r, exp = hr.load(name, K, noise)

    def run():
        res = _run(engine, r, K, n_buckets=N_BUCKETS)
        got = _got(res, K)
        assert hr.differs(exp, got) is None, hr.differs(exp, got)
        assert (res.n_kmers, res.n_unitigs, res.unitig_total_bases) == (exp.n_kmers, len(exp.unitig_lens), int(exp.unitig_lens.sum()))
        return got, _evidence(res)

    _, ev = _legs(engine, tune, run, f"{name} K={K} {'noisy' if noise else 'clean'}", name not in SMALL)
    if name == "tiny_circles" or (name == "circles_5000" and K == 48):
        assert ev["n_circles"] > 0          # circles the join closed (at K=60 every one of the five thousand closes inside a chunk)


@functools.lru_cache(maxsize=None)
def _all_sets(K, noise, names=CASES):
    """the seven sets (or some of them) as one job (their k-mers are disjoint: random strands of at least K bases, the periodic circles
    in tiny_circles only) and what the C oracle makes of it"""
    from types import SimpleNamespace
    rs = [hr.reads(n, K, noise) for n in names]
    r = SimpleNamespace(codes=np.concatenate([x.codes for x in rs]), quals=np.concatenate([x.quals for x in rs]), lens=np.concatenate([x.lens for x in rs]),
                        bc=np.concatenate([x.bc for x in rs]), read_len=hr.L, rows=None)
    gl = oracle_lib.good_lens(r.quals, r.lens, K=K, min_qual=7)
    o = oracle_lib.OracleResult(r.codes, gl, r.bc if K == 48 else None, K=K, hbv=False)
    want = hr.normalised(K, gl, o.keys, o.counts, o.ctx, np.bincount(o.counts) if len(o.counts) else np.zeros(0, np.int64), o.unitigs)
    return r, want


@pytest.mark.parametrize("K", hr.KS)
def test_all_sets_in_one_job(engine, tune, K):
    """Tiny circles, turns, forests and chains among enough fragments for the ruling set, noisy reads; the global graph stage's k-mer
    level ranking (unweighted, the cut at the minimum k-mer left to the general algorithm) on the same job."""
    r, want = _all_sets(K, True)

    def run(**kw):
        res = _run(engine, r, K, **kw)
        got = _got(res, K)
        for f in hr.FIELDS:
            assert np.array_equal(got[f], want[f]), f
        return got, _evidence(res)

    first, ev = _legs(engine, tune, lambda: run(n_buckets=N_BUCKETS), f"all sets K={K}", True)
    assert ev["n_circles"] > 0
    engine.clear_option("rank_wyllie")
    engine.clear_option("split_log2")
    tune("global_graph", 1)
    got, gev = run()
    print(f"[join_mirror] all sets K={K} global graph: {gev}")
    assert gev["n_kmers"] * 2 >= 4096 and gev["n_circles"] > 0          # every circle is the ranking's to close there
    for f in hr.FIELDS:
        assert np.array_equal(first[f], got[f]), f


@pytest.mark.parametrize("K", hr.KS)
def test_global_graph_without_circles(engine, tune, K):
    """The unweighted ranking (w = 1 per k-mer) of the global graph stage.  It leaves circles to the general algorithm, so the ruling
    set's ranks are the result only in a job without any: the four sets that have none, palindromes and turns among 89 k k-mers."""
    r, want = _all_sets(K, True, ("chain_1025", "forest_257", "turns", "long"))
    tune("global_graph", 1)

    def run():
        res = _run(engine, r, K)
        got = _got(res, K)
        for f in hr.FIELDS:
            assert np.array_equal(got[f], want[f]), f
        return got, _evidence(res)

    _, ev = _legs(engine, tune, run, f"global graph K={K}", True, size="n_kmers")
    assert ev["n_circles"] == 0 and ev["n_fragments"] == 0


def test_all_sets_grouped(engine, tune):
    """Per-group graphs (frequency rule only): two groups, each holding whole sets, against the C oracle per group; default ranking and
    pointer jumping give the same arrays."""
    K = 48
    rs = [hr.reads(n, K, False) for n in CASES]
    from types import SimpleNamespace
    r = SimpleNamespace(codes=np.concatenate([x.codes for x in rs]), quals=np.concatenate([x.quals for x in rs]), lens=np.concatenate([x.lens for x in rs]),
                        bc=np.concatenate([x.bc for x in rs]), read_len=hr.L, rows=None)
    group = np.concatenate([np.full(len(x.lens), 3 if i % 2 else 7, np.int32) for i, x in enumerate(rs)])
    gl = oracle_lib.good_lens(r.quals, r.lens, K=K, min_qual=7)
    oracles = {g: oracle_lib.OracleResult(r.codes[group == g], gl[group == g], None, K=K, min_freq=3, min_bc=0, hbv=False) for g in (3, 7)}
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    seen = []
    for leg, option, value in LEGS[:2]:
        if option:
            tune(option, value)
        res = _run(engine, r, K, group=group, min_freq=3, min_bc=0, grouped=True, sorted_table=False, n_buckets=N_BUCKETS)
        ev = _evidence(res)
        print(f"[join_mirror] grouped {leg}: {ev}")
        assert ev["n_fragments"] * 2 >= 4096 and ev["n_circles"] > 0
        k, cnt, ctx = res.keys(), res.counts(), res.ctx()
        off, bases = res.unitig_arrays()
        ug = res.unitig_groups()
        for gid, o in oracles.items():
            m = k[:, 3] == gid
            order = np.lexsort((k[m][:, 2], k[m][:, 1], k[m][:, 0]))
            assert np.array_equal(k[m][order][:, :3], o.keys[:, :3]) and np.array_equal(cnt[m][order], o.counts) and np.array_equal(ctx[m][order], o.ctx), (leg, gid)
            us = sorted((lut[bases[int(off[u]):int(off[u + 1])]].tobytes().decode() for u in np.nonzero(ug == gid)[0]), key=lambda t: (-len(t), t))
            assert us == o.unitigs, (leg, gid)
        # (the unsorted table of a grouped run comes in a different order from call to call: it is compared per group, sorted, above)
        seen.append((off, bases, ug, res.spectrum()))
    for a, b in zip(*seen):
        assert np.array_equal(a, b)


# ---- the spectrum that the prune accumulates (bl_prune_kernel, snk_local.hip): 65536 bins laid out in advance, counts below 128 through
# a workgroup's LDS histogram, larger ones straight into the bins; a count of 65536 or more needs a longer array: snk_spectrum's passes

@pytest.mark.parametrize("n_hot,folded", [(600, True), (1000, False)], ids=["61800", "103000"])
def test_spectrum_beside_and_beyond_the_fixed_bins(engine, n_hot, folded):
    """Reads of 150 A on top of the turns set: the k-mer A^48 occurs 103 times per read.  600 reads put it at 61 800 (inside the fixed
    range, beyond the LDS bins), 1000 reads at 103 000: the array must grow to 103 001 bins, which only the fallback route makes.  The
    spectrum is the histogram of the C oracle's counts, bin count included."""
    from types import SimpleNamespace
    K = 48
    b = hr.reads("turns", K, True)
    hot = np.zeros((n_hot, hr.L), np.uint8)
    r = SimpleNamespace(codes=np.concatenate([b.codes, hot]), quals=np.concatenate([b.quals, np.full((n_hot, hr.L), 30, np.uint8)]),
                        lens=np.concatenate([b.lens, np.full(n_hot, hr.L, np.uint16)]), bc=np.concatenate([b.bc, 1 + np.arange(n_hot, dtype=np.int32) % hr.N_BC]),
                        read_len=hr.L, rows=None)
    gl = oracle_lib.good_lens(r.quals, r.lens, K=K, min_qual=7)
    o = oracle_lib.OracleResult(r.codes, gl, r.bc, K=K, hbv=False)
    assert int(o.counts.max()) == n_hot * (hr.L - K + 1) and (int(o.counts.max()) < 65536) == folded
    for sorted_table in (False, True):          # (the sorted table keeps the two passes over the counts in either case)
        res = _run(engine, r, K, sorted_table=sorted_table)
        spec = np.asarray(res.spectrum()).astype(np.int64)
        assert len(spec) == max(65536, int(o.counts.max()) + 1), (sorted_table, len(spec))
        want = np.bincount(o.counts, minlength=len(spec))
        assert np.array_equal(spec, want), (sorted_table, np.nonzero(spec != want)[0][:8])
        assert res.unitigs() == o.unitigs
        if sorted_table:
            assert np.array_equal(res.keys()[:, :3], o.keys[:, :3]) and np.array_equal(res.counts(), o.counts) and np.array_equal(res.ctx(), o.ctx)
