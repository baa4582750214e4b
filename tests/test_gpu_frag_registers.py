"""The fragment kernel of the bucket-local graph stage (bl_frag_kernel, snk_local.hip) with the keys of a chunk in the registers of the
lanes that loaded them: node i of a chunk lies in lane i % 64, register slot i / 64; a place that needs another node's key loads it
again (half links, circles) or takes it from the owning lane by shuffles (head k-mers).  Fragment numbers and base offsets come from a
ballot and a prefix sum over the wave.

Tiny jobs whose chunks have the sizes at which keys change slot and lane, against the C oracle on the same reads: table, counts,
contexts, unitigs.  One bucket (n_buckets=1) puts the whole job into one chunk; the table is left in bucket order (sorted_table=False),
so with one chunk a k-mer's row in the table IS its node number, which is how the tests know the lane and the slot of a node.  Every
test asserts what it is there for (k-mers, fragments, circles closed inside the chunk, no big chunk) beside the comparison."""
import ctypes as C
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_lib
from handunitigs import _CODE, rc

pytestmark = pytest.mark.gpu

L = 150
KS = (48, 60)
SIZES = (1, 63, 64, 65, 128, 255, 256)


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


def _rng(tag):
    return np.random.default_rng(zlib.crc32(f"frag_registers/{tag}".encode()))


def _rand(g, n):
    return "".join("ACGT"[i] for i in g.integers(0, 4, n))


def _canon(s, K):
    return [min(s[p:p + K], rc(s[p:p + K])) for p in range(len(s) - K + 1)]


def _tiled(strands, K):
    """reads of at most L bases over every strand (each of at least K + 1 bases), every window three times in three barcodes: every
    k-mer and every adjacency of a strand stands (3 instances, 3 barcodes), nothing else is in the reads"""
    reads = []
    for s in strands:
        assert len(s) >= K + 1
        starts = sorted(set(range(0, max(1, len(s) - L + 1), (L - K) // 2)) | {max(0, len(s) - L)})
        reads += [s[a:a + L] for a in starts]
    return reads


def _job(reads, copies=3):
    """each read `copies` times, in barcodes 1.., every second read on its other strand"""
    rows = [(rc(s) if i % 2 else s, 1 + (i + c) % 24) for i, s in enumerate(reads) for c in range(copies)]
    n = len(rows)
    codes, quals = np.zeros((n, L), np.uint8), np.zeros((n, L), np.uint8)
    lens, bc = np.zeros(n, np.uint16), np.zeros(n, np.int32)
    for row, (s, b) in enumerate(rows):
        lens[row], bc[row] = len(s), b
        codes[row, :len(s)] = _CODE[np.frombuffer(s.encode(), np.uint8)]
        quals[row, :len(s)] = 30
    return SimpleNamespace(codes=codes, quals=quals, lens=lens, bc=bc)


def _legs(engine):
    """-> (fragment-pass attempts, circles closed inside a chunk, big chunks) of the engine's last call"""
    circles, big = C.c_uint64(0), C.c_uint32(0)
    attempts = int(engine.lib.snk_ctx_last_local_graph(engine._ctx, C.byref(circles), C.byref(big)))
    return attempts, int(circles.value), int(big.value)


def _key_strings(keys, K):
    keys = np.asarray(keys, np.uint32)
    j = np.arange(K)
    b = (keys[:, j // 16] >> (2 * (15 - j % 16)).astype(np.uint32)) & 3
    return [row.tobytes().decode() for row in np.frombuffer(b"ACGT", np.uint8)[b]]


def _run(engine, job, K, group=None, **params):
    import torch
    from supernova_amd import synth
    from supernova_amd.engine import Params
    dev = torch.device("cuda", 0)
    kw = dict(group=torch.from_numpy(group).to(dev)) if group is not None else {}
    bc = torch.from_numpy(job.bc).to(dev) if K == 48 and group is None else None          # (the K=60 reference has no barcode rule)
    return engine.count_graph(torch.from_numpy(synth.pack_rows(job.codes).view(np.int32)).to(dev), L, quals=torch.from_numpy(job.quals).to(dev), bc=bc,
                              lens=torch.from_numpy(job.lens.view(np.int16)).to(dev), params=Params(K=K, sorted_table=False, **params), **kw)


def _held(engine, job, K, n_kmers, n_fragments, circles=0, **params):
    """one chunk-sized job against the C oracle -> the k-mers of the table in its own (bucket) order, as strings"""
    res = _run(engine, job, K, **params)
    gl = oracle_lib.good_lens(job.quals, job.lens, K=K, min_qual=7)
    o = oracle_lib.OracleResult(job.codes, gl, job.bc if K == 48 else None, K=K, hbv=False)
    k = res.keys()
    order = np.lexsort(tuple(k[:, j] for j in (3, 2, 1, 0)))
    w = 3 if K == 48 else 4
    assert np.array_equal(k[order][:, :w], o.keys[:, :w]) and not k[:, w:].any(), "k-mer table differs from the oracle"
    assert np.array_equal(res.counts()[order], o.counts), "counts differ"
    assert np.array_equal(res.ctx()[order], o.ctx), "contexts differ"
    assert res.unitigs() == o.unitigs, "unitigs differ"
    attempts, in_chunk, big = _legs(engine)
    print(f"[frag_registers] K={K} {params}: {res.n_kmers} k-mers, {res.n_fragments} fragments, {in_chunk} circles in chunks, {res.n_unitigs} unitigs")
    assert (res.n_kmers, res.n_fragments, in_chunk, big, attempts) == (n_kmers, n_fragments, circles, 0, 1)
    return _key_strings(k, K)


def _path_reads(g, N, K):
    """reads that retain exactly the N k-mers of one random strand"""
    if N == 1:          # one k-mer followed by three different bases: it stands, its three successors (one instance each) do not
        s = _rand(g, K)
        return [s + b for b in "ACG"], 1
    return _tiled([_rand(g, N + K - 1)], K), 3


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", SIZES)
def test_one_path_fills_the_chunk(engine, N, K):
    """A single path of N k-mers in one chunk: one fragment, N - 1 links; 256 k-mers are the chunk's capacity and the most jumping
    rounds; the nodes fill lanes 0 .. (N - 1) % 64 of slot (N - 1) / 64 last."""
    reads, copies = _path_reads(_rng(f"path/{N}/{K}"), N, K)
    _held(engine, _job(reads, copies), K, N, 1, n_buckets=1)


@pytest.mark.parametrize("K", KS)
def test_every_node_is_a_head(engine, K):
    """256 k-mers, 256 fragments of one k-mer: 85 forks of a k-mer with two successors and one with three.  A successor's only
    predecessor has two ways on, so no link is mutual: every node is a terminal on both sides and the head of its own fragment."""
    g = _rng(f"heads/{K}")
    reads = []
    for f in range(85):
        s = _rand(g, K)
        reads += [s + b for b in ("ACG" if f == 0 else "AC")]
    _held(engine, _job(reads), K, 256, 256, n_buckets=1)


def _circle(g, n, K, taken):
    """a circular string of n bases with n k-mers of its own -> the string that holds them and the adjacency that closes the circle"""
    for _ in range(1000):
        c = _rand(g, n)
        s = (c * (2 + (K + n) // n))[:n + K]
        ks = set(_canon(s, K))
        if len(ks) == n and not any(k == rc(k) for k in ks) and len(set(s[p:p + K] for p in range(n)) | set(rc(s[p:p + K]) for p in range(n))) == 2 * n and not (ks & taken):
            taken |= ks
            return s
    raise AssertionError("no free circle")


@pytest.mark.parametrize("K", KS)
def test_circles_inside_one_chunk(engine, K):
    """Five smooth circles of 40 k-mers in one chunk: each is cut at its minimum k-mer by the lane that holds that k-mer, which walks the
    circle over the other lanes' keys.  At least one of the five minima lies in a lane other than lane 0."""
    g, taken = _rng(f"circles/{K}"), set()
    circles = [_circle(g, 40, K, taken) for _ in range(5)]
    reads = []
    for s in circles:          # (a read goes round the circle as far as its length allows: the closing adjacency is in every read)
        reads.append((s[:40] * 8)[:L])
    table = _held(engine, _job(reads), K, 200, 5, circles=5, n_buckets=1)          # (a circle closed inside a chunk is a fragment)
    row = {k: i for i, k in enumerate(table)}
    lanes = [row[min(_canon(s, K)[:40])] % 64 for s in circles]
    print(f"[frag_registers] K={K}: the circles' minima lie in lanes {lanes}")
    assert any(lanes)


@pytest.mark.parametrize("K", KS)
def test_palindrome_next_to_a_link(engine, K):
    """A palindromic k-mer in the middle of a strand: it takes no link (it is a unitig of its own), the k-mers on either side of it are
    linked to their other neighbours.  The flag rides in a bit of the node's neighbour word."""
    g = _rng(f"palindrome/{K}")
    x = _rand(g, K // 2)
    s = _rand(g, 70) + x + rc(x) + _rand(g, 70)
    n = len(set(_canon(s, K)))
    assert n == len(s) - K + 1 and sum(k == rc(k) for k in _canon(s, K)) == 1
    res_frags = 3          # the strand in front of the palindrome, the palindrome, the strand behind it
    _held(engine, _job(_tiled([s], K)), K, n, res_frags, n_buckets=1)


# ---- two chunks: the bucket of a k-mer, as snk_common.h has it (minimum over the 16-mers of the mixed canonical code, mixed again)

def _mix32(x):
    x ^= x >> 16; x = x * 0x7feb352d & 0xFFFFFFFF
    x ^= x >> 15; x = x * 0x846ca68b & 0xFFFFFFFF
    return x ^ (x >> 16)


def _buckets(s, K, NB):
    """the bucket of every k-mer of the strand s"""
    code = lambda m: int("".join(str("ACGT".index(c)) for c in m), 4)
    keys = [_mix32(min(code(s[p:p + 16]), code(rc(s[p:p + 16])))) for p in range(len(s) - 15)]
    out = []
    for p in range(len(s) - K + 1):
        h = _mix32(min(keys[p:p + K - 15]) ^ 0x5bd1e995) * 0x9E3779B1 & 0xFFFFFFFF
        h ^= h >> 15
        out.append(h * NB >> 32)
    return out


@pytest.mark.parametrize("K", KS)
def test_half_link_from_the_fourth_slot(engine, tune, K):
    """Two buckets, not merged: a strand of some 440 k-mers is cut into two chunks of 193 to 256 k-mers wherever its minimiser changes
    bucket, and every cut leaves two fragment ends whose half links are computed from the end node's key.  Some of those end nodes are
    nodes 192.. of their chunk: the fourth register slot of their lane.  The strand is the first of a seeded series whose chunks have
    that size; which rows the table gives the end nodes is only known after the run, and asserted then."""
    tune("chunk_merge", 0)
    g = _rng(f"halflink/{K}")
    for _ in range(200):
        s = _rand(g, 440 + K - 1)
        ks = _canon(s, K)
        b = _buckets(s, K, 2)
        if len(set(ks)) == 440 and 193 <= sum(b) <= 247:
            break
    else:
        raise AssertionError("no strand with two chunks of that size")
    cuts = sum(b[i] != b[i + 1] for i in range(439))
    table = _held(engine, _job(_tiled([s], K)), K, 440, cuts + 1, n_buckets=2)
    row = {k: i for i, k in enumerate(table)}
    rows = [np.array(sorted(row[k] for k, x in zip(ks, b) if x == which)) for which in (0, 1)]
    for r in rows:          # the chunk of a bucket is a run of rows: the port above puts the k-mers where the library does
        assert len(r) and r[-1] - r[0] + 1 == len(r)
    ends = [int(row[ks[i + d]] - rows[b[i + d]][0]) for i in range(439) if b[i] != b[i + 1] for d in (0, 1)]
    print(f"[frag_registers] K={K}: chunks of {[len(r) for r in rows]} k-mers, {cuts} cuts, end nodes with a half link {sorted(ends)}")
    assert max(ends) >= 192


def test_grouped_chunk(engine):
    """Per-group graphs (the group rides in the low key word, 64 bits wide in LDS before, in registers now): a path of 80 k-mers and a
    circle of 40 in each of two groups, the same circle in both -- one bucket, so one chunk of 240 nodes holds both groups; per group
    against the oracle."""
    K = 48
    g, taken = _rng("grouped"), set()
    circle = _circle(g, 40, K, taken)
    parts = [_job(_tiled([_rand(g, 80 + K - 1)], K) + [(circle[:40] * 8)[:L]]) for _ in range(2)]
    job = SimpleNamespace(**{f: np.concatenate([getattr(p, f) for p in parts]) for f in ("codes", "quals", "lens", "bc")})
    group = np.concatenate([np.full(len(p.lens), gid, np.int32) for p, gid in zip(parts, (3, 7))])
    res = _run(engine, job, K, group=group, min_freq=3, min_bc=0, grouped=True, n_buckets=1)
    attempts, in_chunk, big = _legs(engine)
    print(f"[frag_registers] grouped: {res.n_kmers} k-mers, {res.n_fragments} fragments, {in_chunk} circles in chunks")
    assert (res.n_kmers, res.n_fragments, in_chunk, big, attempts) == (240, 4, 2, 0, 1)
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
