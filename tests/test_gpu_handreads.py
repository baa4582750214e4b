"""Count, prune and unitig pull on the device, on reads walked over hand-made unitig sets (tests/handreads.py): topologies that no random
genome produces -- circles of one to a thousand k-mers, five thousand circles and nothing else, strands that turn round into their own
reverse complement, palindromes on junctions, a vertex with all eight ends, a chain of 1025 pieces, a forest of one- to six-k-mer unitigs.

Bar: bit-exact, through the C ABI, against what the REFERENCE made of the same reads (tests/golden/handreads/): good lengths, keys,
counts, pruned contexts, spectrum, unitigs.  tests/test_handreads_host.py holds the oracle to the same fixtures.  The metamorphic tests need
no reference; snk_ctx_last_local_graph confirms that a leg was taken."""
import ctypes as C

import numpy as np
import pytest

import handreads as hr

pytestmark = pytest.mark.gpu

ALL = [(n, K) for n in hr.CASES for K in hr.KS]
THREE = ("mixed_seed1", "tiny_circles", "turns")


@pytest.fixture(params=["local", "global"])
def graph_stage(request, tune):
    tune("global_graph", 1 if request.param == "global" else 0)
    return request.param


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


def _run(engine, r, K, codes=None, rev=False, **params):
    """one count-and-graph call on a read set (K=60: without barcodes, as the reference's K=60 build has no barcode rule)"""
    import torch
    from supernova_amd import synth
    from supernova_amd.engine import Params
    dev = torch.device("cuda", 0)
    rows = hr.rows(r) if codes is None else synth.pack_rows(codes)
    quals, lens, bc = r.quals, r.lens, r.bc
    if rev:
        rows, quals, lens, bc = (np.ascontiguousarray(a[::-1]) for a in (rows, quals, lens, bc))
    return engine.count_graph(torch.from_numpy(rows.view(np.int32)).to(dev), r.read_len, quals=torch.from_numpy(np.ascontiguousarray(quals)).to(dev),
                              bc=torch.from_numpy(bc.astype(np.int32)).to(dev) if K == 48 else None,
                              lens=torch.from_numpy(lens.astype(np.uint16).view(np.int16)).to(dev), params=Params(K=K, **params))


def _got(res, K):
    return hr.normalised(K, res.good_len(), res.keys(), res.counts(), res.ctx(), res.spectrum(), res.unitigs())


def _held(res, K, exp):
    got = _got(res, K)
    assert hr.differs(exp, got) is None, hr.differs(exp, got)
    assert (res.n_kmers, res.n_unitigs, res.unitig_total_bases) == (exp.n_kmers, len(exp.unitig_lens), int(exp.unitig_lens.sum()))
    return got


def _legs(engine):
    """-> (fragment-pass attempts, in-chunk circles, big chunks) of the engine's last call"""
    circles, big = C.c_uint64(0), C.c_uint32(0)
    attempts = int(engine.lib.snk_ctx_last_local_graph(engine._ctx, C.byref(circles), C.byref(big)))
    return attempts, int(circles.value), int(big.value)


def _attempts_due(res, circles, pool=4096):
    """The in-chunk circle pool holds bl_pool + F/256 fragment slots for F open paths (none with bl_pool=0); the fragment pass runs a
    second time iff the circles that closed inside a chunk need more."""
    return 2 if circles > (pool + (res.n_fragments - circles) // 256 if pool else 0) else 1


@pytest.mark.parametrize("noise", [False, True], ids=["clean", "noisy"])
@pytest.mark.parametrize("name,K", ALL)
def test_case_equals_the_reference(engine, graph_stage, name, K, noise):
    r, exp = hr.load(name, K, noise)
    res = _run(engine, r, K)
    _held(res, K, exp)
    attempts, circles, big = _legs(engine)
    if graph_stage == "global" or exp.n_kmers == 0:
        assert (attempts, circles, big) == (0, 0, 0)          # the bucket-local stage did not run
    else:
        assert attempts == _attempts_due(res, circles) and (attempts == 1 or name == "circles_5000")


def _palindromic(keys, K):
    return np.array([k == hr.rc(k) for k in hr.key_strings(keys, K)], bool) if len(keys) else np.zeros(0, bool)


def _mirrored(ctx):
    """the context of a k-mer seen from its other strand: successor x <-> predecessor comp(x) (bits 0..3 successors, 4..7 predecessors)"""
    out = np.zeros_like(ctx)
    for x in range(4):
        out |= ((ctx >> x) & 1) << (7 - x)
        out |= ((ctx >> (4 + x)) & 1) << (3 - x)
    return out


@pytest.mark.parametrize("name,K", ALL)
def test_noise_order_and_strand_change_nothing(engine, graph_stage, name, K):
    """Needs no reference.  The noisy reads give the clean reads' table, contexts and unitigs (counts may grow); the reads in reversed
    order give the same result; so do the reads all reverse-complemented -- except that a palindromic k-mer has no canonical strand, so
    its context comes back mirrored (the reference does the same: "c then x" and "comp(x) then c" are different bits of c's context)."""
    clean = hr.reads(name, K, False)
    a = _got(_run(engine, clean, K), K)
    n = _got(_run(engine, hr.reads(name, K, True), K), K)
    for f in ("keys", "ctx", "unitigs"):
        assert np.array_equal(a[f], n[f]), f
    assert np.all(n["counts"] >= a["counts"])
    b = _got(_run(engine, clean, K, rev=True), K)
    assert np.array_equal(b["goodlens"], a["goodlens"][::-1])
    for f in hr.FIELDS[1:]:
        assert np.array_equal(a[f], b[f]), f
    codes = np.zeros_like(clean.codes)
    for i, m in enumerate(clean.lens):
        codes[i, :m] = 3 - clean.codes[i, :m][::-1]
    c = _got(_run(engine, clean, K, codes=codes), K)
    for f in ("goodlens", "keys", "counts", "hist", "unitigs"):
        assert np.array_equal(a[f], c[f]), f
    assert np.array_equal(np.where(_palindromic(a["keys"], K), _mirrored(a["ctx"]), a["ctx"]), c["ctx"])


# every setting of the graph-side options, forced on its own: option -> value, or a field of Params
SETTINGS = [("bl_pool", 0), ("chunk_merge", 0), ("bl_cpw", 1), ("bl_index_fused", 0), ("bl_noclassify", 1), ("rank_wyllie", 1), ("split_log2", 1),
            ("split_log2", 12), ("emit_grid_log2", 0), ("n_buckets", 1), ("n_buckets", 4096), ("count_tight", 256), ("msp_dense", 1), ("long_minimiser", True)]


@pytest.mark.parametrize("option,value", SETTINGS, ids=[f"{o}={int(v)}" for o, v in SETTINGS])
@pytest.mark.parametrize("K", hr.KS)
@pytest.mark.parametrize("name", THREE)
def test_three_cases_under_every_graph_side_setting(engine, tune, name, K, option, value):
    """(bucket-local graph stage: the options are its own and the partition's)"""
    r, exp = hr.load(name, K, True)
    if option in ("n_buckets", "long_minimiser"):
        res = _run(engine, r, K, **{option: value})
    else:
        tune(option, value)
        res = _run(engine, r, K)
    _held(res, K, exp)
    attempts, circles, _ = _legs(engine)
    assert attempts == _attempts_due(res, circles, 0 if option == "bl_pool" else 4096)         # an empty pool: any in-chunk circle forces the exact re-run
    assert attempts == 1 or option == "bl_pool"
    if name == "tiny_circles":
        assert circles > 0                  # (its short circles keep one minimiser all the way round: one bucket, one chunk)


@pytest.mark.parametrize("K", hr.KS)
def test_five_thousand_circles_and_nothing_else(engine, graph_stage, K):
    """Default options.  No open path in the job, so the in-chunk circle pool holds bl_pool + F/256 = 4096 slots or few more; the circles
    that close inside one chunk take a slot each, the others are closed by the join (n_circles counts those; under the global graph stage
    all of them).  At K=60 every circle closes inside a chunk: a circle of at most K - 16 + 1 = 45 k-mers holds the same 16-mers in every
    rotation, so all its k-mers have one minimiser and lie in one bucket -- 5000 circles overflow the pool and the fragment pass runs again
    with the exact number, the leg that only bl_pool=0 forced so far.  At K=48 that holds up to 33 k-mers only: the longer circles are cut
    by the partition, the join closes them, and what is left (3837 on the day this was written) fits the pool: one attempt."""
    r, exp = hr.load("circles_5000", K, False)
    res = _run(engine, r, K)
    _held(res, K, exp)
    attempts, circles, big = _legs(engine)
    print(f"circles_5000 K={K} {graph_stage}: fragment-pass attempts {attempts}, in-chunk circles {circles}, big chunks {big}, fragments {res.n_fragments}, "
          f"n_circles {res.n_circles}")
    assert res.n_circles + circles == 5000
    assert attempts == (0 if graph_stage == "global" else _attempts_due(res, circles))
    if graph_stage == "local" and K == 60:
        assert (attempts, circles, res.n_circles) == (2, 5000, 0)


def _sharded_held(name, K, W):
    """W in-process ranks on the noisy reads of a case, their union held to the reference -> the ranking every rank reports"""
    import sharded_cases
    r, exp = hr.load(name, K, True)
    out = sharded_cases.run_ranks(W, hr.rows(r), r.read_len, r.quals, bc=r.bc if K == 48 else None, lens=r.lens, K=K)
    keys = np.concatenate([o["keys"] for o in out])
    order = np.lexsort(tuple(keys[:, j] for j in (3, 2, 1, 0)))
    nb = max(len(o["spectrum"]) for o in out)
    spec = sum(np.pad(o["spectrum"].astype(np.int64), (0, nb - len(o["spectrum"]))) for o in out)
    unitigs = sorted((u for o in out for u in o["unitigs"]), key=lambda s: (-len(s), s))
    got = hr.normalised(K, exp.fields["goodlens"], keys[order], np.concatenate([o["counts"] for o in out])[order], np.concatenate([o["ctx"] for o in out])[order],
                        spec, unitigs)
    assert hr.differs(exp, got, hr.FIELDS[1:]) is None, hr.differs(exp, got, hr.FIELDS[1:])
    if name == "tiny_circles":
        assert sum(o["n_circles"] for o in out) > 0
    print(f"{name} K={K} W={W}: ranking {[o['ranking'] for o in out]}")
    return [o["ranking"] for o in out]


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("K", hr.KS)
@pytest.mark.parametrize("name", THREE)
def test_sharded_ranks_write_the_references_unitigs_between_them(snk, name, K, W):
    _sharded_held(name, K, W)


# The partitioned ranking where its set-up and its share arithmetic are thin.  split_log2 = 12: no sampled splitter is left in sets this
# small, so chain_1025 has a handful of head splitters for 8 ranks (ranks with an empty share, k0 == k1) and the circles of tiny_circles
# (31/32/33 and 255/256/257 k-mers) hold no splitter at all; split_log2 = 1: every second fragment is a splitter and the circles show as
# splitter cycles.  The ranking each leg takes was recorded on the commit before the one-GPU and the partitioned ranking were given one
# set-up: all sixteen legs, every rank, "partitioned" -- the circles are cut by the fast path on replicated data and the partitioned
# ranking begins again; none falls back to the replicated ranking.  (No other test runs one of these legs: the test above runs W = 2
# and 3 at the default spacing only.)
@pytest.mark.parametrize("split_log2", [1, 12])
@pytest.mark.parametrize("W", [2, 8])
@pytest.mark.parametrize("K", hr.KS)
@pytest.mark.parametrize("name", ["tiny_circles", "chain_1025"])
def test_sharded_ranks_with_thin_and_dense_splitter_sets(snk, tune, name, K, W, split_log2):
    tune("split_log2", split_log2)
    assert _sharded_held(name, K, W) == ["partitioned"] * W
