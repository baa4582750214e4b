"""The one-wave prune of the bucket-local graph stage (bl_prune_kernel, snk_local.hip) after its LDS and registers were cut for residency:
16-bit hash-table entries claimed with a CAS on the word that holds them, a miss list of 128 entries that a batch with more misses goes
through in rounds, the miss and boundary counters from a scan over the wave, the (count, context) words asked for batch by batch.

Tiny jobs against the C oracle on the same reads, in the manner of test_gpu_frag_registers.py (whose read builders these tests use):
table, counts, contexts, unitigs and the spectrum.  One bucket (n_buckets=1) puts the whole job into one chunk; the table stays in
bucket order (sorted_table=False).  Every test asserts the condition it is there for beside the comparison."""
import re
import zlib
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_lib
from handunitigs import rc
from test_gpu_frag_registers import _buckets, _job, _legs, _mix32, _path_reads, _rand, _run, _tiled

pytestmark = pytest.mark.gpu

KS = (48, 60)
SIZES = (1, 63, 64, 65, 128, 129, 192, 255, 256)


def _miss_list_entries():
    """entries of the one-wave variant's miss list, as bl_prune_chunk (snk_local.hip) declares them: the tests that are there for the
    rounds ask that their batches hold more misses than that, whatever the number becomes"""
    src = (Path(__file__).resolve().parent.parent / "supernova_amd" / "csrc" / "snk_local.hip").read_text()
    m = re.search(r"constexpr int ML = ONE \? (\d+) : 8 \* T;", src)
    assert m, "the miss list's declaration moved"
    return int(m.group(1))


ML = _miss_list_entries()


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


def _rng(tag):
    return np.random.default_rng(zlib.crc32(f"prune_residency/{tag}".encode()))


def _oracle(job, K, **kw):
    gl = oracle_lib.good_lens(job.quals, job.lens, K=K, min_qual=7)
    return oracle_lib.OracleResult(job.codes, gl, job.bc if K == 48 else None, K=K, hbv=False, **kw)


def _same(res, o, K, what=""):
    """table, counts, contexts, unitigs and spectrum of a run against the oracle's"""
    k = res.keys()
    order = np.lexsort(tuple(k[:, j] for j in (3, 2, 1, 0)))
    w = 3 if K == 48 else 4
    assert np.array_equal(k[order][:, :w], o.keys[:, :w]) and not k[:, w:].any(), f"{what}: k-mer table differs from the oracle"
    assert np.array_equal(res.counts()[order], o.counts), f"{what}: counts differ"
    assert np.array_equal(res.ctx()[order], o.ctx), f"{what}: contexts differ"
    assert res.unitigs() == o.unitigs, f"{what}: unitigs differ"
    spec = np.asarray(res.spectrum()).astype(np.int64)
    want = np.bincount(o.counts.astype(np.int64), minlength=len(spec))
    assert len(want) == len(spec) and np.array_equal(spec, want), f"{what}: spectrum differs from the histogram of the oracle's counts"


def _check(engine, job, K, **params):
    res = _run(engine, job, K, **params)
    o = _oracle(job, K)
    _same(res, o, K, str(params))
    attempts, _, big = _legs(engine)
    print(f"[prune_residency] K={K} {params}: {res.n_kmers} k-mers in {res.n_buckets} buckets, {res.n_boundary} boundary k-mers, "
          f"{res.n_fragments} fragments, {big} big chunks")
    assert big == 0 and attempts == 1
    return res, o


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", SIZES)
def test_chunk_sizes(engine, N, K):
    """One chunk of N k-mers: the batch edges (63, 64, 65, 128, 129, 192), a last batch of one lane (65, 129), the capacity (256)."""
    reads, copies = _path_reads(_rng(f"size/{N}/{K}"), N, K)
    res, _ = _check(engine, _job(reads, copies), K, n_buckets=1)
    assert res.n_kmers == N and res.n_boundary == 0


def _all_missing_reads(g, n, K):
    """n k-mers X with all eight context bits set and no neighbour retained: the reads b X b' for the four bases b -- X four times, every
    neighbour once (below min_freq)"""
    reads = []
    for _ in range(n):
        x = _rand(g, K)
        reads += [b + x + b2 for b, b2 in zip("ACGT", "GTAC")]
    return reads


def _all_missing(g, n, K):
    return _job(_all_missing_reads(g, n, K), copies=1)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", (64, 65))
def test_full_miss_list(engine, n, K):
    """64 k-mers of one batch with eight misses each: 512 misses, several rounds of the list; 65: the last k-mer's eight in a batch of
    its own.  One bucket: every miss is settled by the classifier (the neighbour's bucket is this one), none is pending -- a round
    that did not run would not show here (the contexts are 0 either way): the two tests below are there for that."""
    assert 8 * 64 > ML
    job = _all_missing(_rng(f"misses/{n}/{K}"), n, K)
    res, o = _check(engine, job, K, n_buckets=1)
    assert res.n_kmers == n
    assert np.all(o.ctx_raw == 0xFF) and not o.ctx.any()
    assert res.n_boundary == 0


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", (64, 65))
def test_full_miss_list_all_pending(engine, tune, n, K):
    """The same job with bl_noclassify: no miss is settled in the chunk, every one of the 512 is left pending for the boundary index
    (which finds none of the neighbours).  A k-mer is a boundary k-mer when one of its misses came out pending: all n are, those whose
    eight misses lie in the second and later rounds of the list included."""
    assert 8 * 64 > ML
    tune("bl_noclassify", 1)
    job = _all_missing(_rng(f"misses/{n}/{K}"), n, K)
    res, o = _check(engine, job, K, n_buckets=1)
    assert res.n_kmers == n and not o.ctx.any()
    assert res.n_boundary == n


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", (64, 65))
def test_full_miss_list_with_boundary(engine, tune, n, K):
    """The same reads over 16 buckets that are not merged, some four k-mers and 32 misses to a chunk (one round): a miss whose minimiser
    lies in another bucket is left pending and answered by the boundary index, the others by the classifier -- both kinds in the same
    batch.  The boundary k-mers are those with a neighbour in another bucket, counted here with the library's bucket function."""
    tune("chunk_merge", 0)
    reads = _all_missing_reads(_rng(f"misses/{n}/{K}"), n, K)
    want = 0
    for j in range(n):
        b = [_buckets(r, K, 16) for r in reads[4 * j:4 * j + 4]]          # (predecessor, X, successor) of each read
        want += any(p != x or s != x for p, x, s in b)
    res, o = _check(engine, _job(reads, copies=1), K, n_buckets=16)
    assert res.n_kmers == n and np.all(o.ctx_raw == 0xFF) and not o.ctx.any()
    assert 0 < want < n and res.n_boundary == want


def _bucket_of_key(key, NB):
    h = _mix32(key ^ 0x5bd1e995) * 0x9E3779B1 & 0xFFFFFFFF
    h ^= h >> 15
    return h * NB >> 32


def _forks_across_two_buckets(g, n, K):
    """n k-mers X of bucket 0 (of 2) whose predecessors are all retained and all lie in bucket 1: X ends in a 16-mer m of very small
    ordering key, which is its minimiser and lies in bucket 0; a predecessor b + X[:-1] has lost m, and X is kept only if the minimiser
    it has instead puts it into bucket 1 for each b.  Reads b + X, three or four b per X -> (reads, predecessors in all)"""
    code = lambda t: int("".join(str("ACGT".index(c)) for c in t), 4)
    while True:
        m = _rand(g, 16)
        key = _mix32(min(code(m), code(rc(m))))
        if key < (1 << 32) // 4000 and _bucket_of_key(key, 2) == 0:
            break
    reads, preds, seen = [], 0, set()
    while len(seen) < n:
        x = _rand(g, K - 16) + m
        bases = "ACGT" if len(seen) % 3 else "ACG"
        if x in seen or any(_buckets(b + x, K, 2) != [1, 0] for b in bases):
            continue
        seen.add(x)
        reads += [b + x for b in bases]
        preds += len(bases)
    return reads, preds


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", (40, 64))
def test_pending_misses_in_later_rounds(engine, tune, n, K):
    """Misses of the second round that must come out pending and be answered "present".  Two buckets, not merged: bucket 0 is one chunk
    of n k-mers X, one batch, each with three or four retained predecessors, all of them in bucket 1 -- some 3.7 n misses in the batch,
    more than the list holds, three or four to a lane so that the rounds' edges need not fall between lanes, and every miss a context bit
    that the oracle has.  A miss that no round took, or that a round settled as absent, is a bit missing from X's context.  Every k-mer of the job has a neighbour in the
    other bucket and none anywhere else: all are boundary k-mers."""
    tune("chunk_merge", 0)
    reads, preds = _forks_across_two_buckets(_rng(f"later_rounds/{n}/{K}"), n, K)
    assert preds > ML and preds <= 256
    res, o = _check(engine, _job(reads), K, n_buckets=2)
    assert res.n_kmers == n + preds and res.n_buckets == 2
    assert int(np.unpackbits(o.ctx).sum()) == 2 * preds          # (every adjacency stands, a bit at either end)
    assert res.n_boundary == n + preds


@pytest.mark.parametrize("K", KS)
def test_full_hash_table(engine, K):
    """256 unrelated k-mers in the 512-slot table (16-bit entries, two to a word: neighbouring slots are claimed through the same
    word; at that fill probing runs over the table's end).  Each has three misses: 192 per batch."""
    g = _rng(f"table/{K}")
    reads = []
    for _ in range(256):
        s = _rand(g, K)
        reads += [s + b for b in "ACG"]
    res, o = _check(engine, _job(reads, copies=1), K, n_buckets=1)
    assert res.n_kmers == 256 and not o.ctx.any()


def test_grouped_chunk(engine):
    """Per-group graphs (64-bit low key words in LDS): a path of 100 k-mers in each of two groups, one chunk of 200; per group
    against the oracle.  K=48 only: the library counts groups at K=48 and nowhere else (the group id rides in the key's fourth word)."""
    K = 48
    g = _rng("grouped")
    parts = [_job(_tiled([_rand(g, 100 + K - 1)], K)) for _ in range(2)]
    job = SimpleNamespace(**{f: np.concatenate([getattr(p, f) for p in parts]) for f in ("codes", "quals", "lens", "bc")})
    group = np.concatenate([np.full(len(p.lens), gid, np.int32) for p, gid in zip(parts, (3, 7))])
    res = _run(engine, job, K, group=group, min_freq=3, min_bc=0, grouped=True, n_buckets=1)
    attempts, _, big = _legs(engine)
    assert (res.n_kmers, big, attempts) == (200, 0, 1)
    gl = oracle_lib.good_lens(job.quals, job.lens, K=K, min_qual=7)
    k, cnt, ctx = res.keys(), res.counts(), res.ctx()
    off, bases = res.unitig_arrays()
    ug = res.unitig_groups()
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    for gid in (3, 7):
        o = oracle_lib.OracleResult(job.codes[group == gid], gl[group == gid], None, K=K, min_freq=3, min_bc=0, hbv=False)
        m = k[:, 3] == gid
        order = np.lexsort((k[m][:, 2], k[m][:, 1], k[m][:, 0]))
        assert np.array_equal(k[m][order][:, :3], o.keys[:, :3]) and np.array_equal(cnt[m][order], o.counts) and np.array_equal(ctx[m][order], o.ctx), gid
        us = sorted((lut[bases[int(off[u]):int(off[u + 1])]].tobytes().decode() for u in np.nonzero(ug == gid)[0]), key=lambda t: (-len(t), t))
        assert us == o.unitigs, gid


@pytest.mark.parametrize("K", KS)
def test_long_minimiser(engine, K):
    """The 20-base minimiser instantiation: a path of 200 k-mers in one chunk, and eight misses per k-mer in rounds."""
    g = _rng(f"long/{K}")
    reads, copies = _path_reads(g, 200, K)
    res, _ = _check(engine, _job(reads, copies), K, n_buckets=1, long_minimiser=True)
    assert res.n_kmers == 200
    res, o = _check(engine, _all_missing(g, 64, K), K, n_buckets=1, long_minimiser=True)
    assert res.n_kmers == 64 and not o.ctx.any()


@pytest.mark.parametrize("K", KS)
def test_merged_chunk(engine, tune, K):
    """Chunks of several buckets (span above 1): the graph stage merges the buckets b, b + G of a count workgroup only where there are
    more buckets than the G count workgroups -- one residency wave of them (at most two per CU) and 4099 buckets.  A strand of 8000
    k-mers fills one bucket in nine, so some buckets G apart are both occupied: counted here with the library's bucket function.
    chunk_merge at its default and at 0 give the oracle's graph.  (The library reports no count of merged chunks: that pairs which its rule
    merges exist is worked out here, for either number of count workgroups per CU, not read back from it.)"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    NB = 4099
    s = _rand(_rng(f"merged/{K}"), 8000 + K - 1)
    fill = np.bincount(_buckets(s, K, NB), minlength=NB)
    for G in (n_cu, 2 * n_cu):
        pairs = sum(1 for b in range(NB - G) if fill[b] and fill[b + G] and fill[b] + fill[b + G] <= 256)
        print(f"[prune_residency] K={K}: {np.count_nonzero(fill)} of {NB} buckets occupied, {pairs} pairs {G} apart that merge")
        assert pairs > 0
    tune("count_persist", 1)
    job = _job(_tiled([s], K))
    merged, _ = _check(engine, job, K, n_buckets=NB)
    tune("chunk_merge", 0)
    single, _ = _check(engine, job, K, n_buckets=NB)
    assert merged.n_kmers == single.n_kmers == 8000 and merged.n_buckets == NB > 2 * n_cu


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("cpw", (1, 4, 1024))
def test_chunks_per_workgroup(engine, tune, cpw, K):
    """bl_cpw chunks per workgroup, 7 chunks: one workgroup each, a last workgroup of three, all in one workgroup (which then goes
    through chunks of different sizes, empty ones among them, with the same LDS)."""
    tune("chunk_merge", 0)
    tune("bl_cpw", cpw)
    job = _job(_tiled([_rand(_rng(f"cpw/{K}"), 300 + K - 1)], K))
    res, _ = _check(engine, job, K, n_buckets=7)
    assert res.n_kmers == 300 and res.n_buckets % 4 != 0


# ---- empty chunks: the prune (bl_cpw chunks to a workgroup) and the fragment launches walk over them

@pytest.mark.parametrize("K", KS)
def test_runs_of_empty_buckets(engine, K):
    """300 k-mers in 4099 buckets: a few dozen occupied ones with runs of empty ones between them, so the occupied chunks are a small part of
    the chunks and lie far apart."""
    NB = 4099
    s = _rand(_rng(f"empty_runs/{K}"), 300 + K - 1)
    occupied = len(set(_buckets(s, K, NB)))
    res, _ = _check(engine, _job(_tiled([s], K)), K, n_buckets=NB)
    assert res.n_kmers == 300 and res.n_buckets == NB and 1 < occupied < NB // 50


@pytest.mark.parametrize("K", KS)
def test_every_chunk_but_the_last_is_empty(engine, tune, K):
    """Eight buckets, every k-mer in the last: the k-mers of a strand of 2 K - 16 bases all hold the 16-mer in its middle, whose ordering
    key is very small and belongs to bucket 7."""
    tune("chunk_merge", 0)
    g = _rng(f"last_chunk/{K}")
    code = lambda t: int("".join(str("ACGT".index(c)) for c in t), 4)
    while True:
        m = _rand(g, 16)
        key = _mix32(min(code(m), code(rc(m))))
        if key < (1 << 32) // 1000 and _bucket_of_key(key, 8) == 7:
            s = _rand(g, K - 16) + m + _rand(g, K - 16)
            if set(_buckets(s, K, 8)) == {7}:
                break
    res, _ = _check(engine, _job(_tiled([s], K)), K, n_buckets=8)
    assert res.n_kmers == K - 15 and res.n_buckets == 8 and res.n_boundary == 0
