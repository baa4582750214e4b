"""What the four entry points that take reads refuse, and that a refusal leaves the context usable.

snk_dev_count_graph, snk_dev_stream_begin / _append, snk_shard_step and snk_shard_stream_begin / _append share one read intake
(csrc/snk_stages.h: snk_intake_*).  Every row of REFUSALS is a bad input given to one of them; the error code and the message are a
RECORD of what the library answered before the intake was shared (the table was filled by running this file against that build),
not a design -- callers match some of these texts, so they stay byte for byte, the round-2 prefix "snk_shard_hist:" that a caller of
snk_shard_step sees included.  After every refusal the same context runs a good job to the unitigs a fresh context gives.

include/snk.h promises nothing about *out after a refusal (snk_dev_count_graph clears it behind its checks, snk_shard_step writes it
at the end), so nothing is asserted about it.

Already covered elsewhere and not repeated here: the zero-read resident call on one GPU and the streamed job with an empty slab
(test_gpu_parity.py: test_empty_and_degenerate_inputs, the streamed-slabs test), the sharded streamed job with an empty slab
(test_gpu_sharded.py: test_sharded_streamed_slabs_equal_the_resident_step).  The zero-read resident call of snk_shard_step is here.

64 reads of 100 bases over a 180-base sequence, K = 48, one in-process rank."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, L, K = 64, 100, 48
ARG, UNSUPPORTED = -1, -6          # SNK_E_ARG, SNK_E_UNSUPPORTED (include/snk.h)


@pytest.fixture(scope="module")
def data(snk):
    import torch
    from supernova_amd import synth
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0x1A7A4E)
    genome = rng.integers(0, 4, 180, dtype=np.uint8)
    codes = np.stack([genome[s:s + L] for s in (np.arange(N) * 5) % (len(genome) - L + 1)])
    rows = synth.pack_rows(codes).view(np.int32)                      # [N, 7]: 112 bases a row
    return dict(rows=torch.from_numpy(rows.copy()).to(dev),
                narrow=torch.from_numpy(rows[:, :6].copy()).to(dev),   # 96 bases a row: fewer than read_len
                quals=torch.from_numpy(np.full((N, L), 30, dtype=np.uint8)).to(dev),
                bc=torch.from_numpy(np.arange(1, N + 1, dtype=np.int32)).to(dev))


def reads(d, rows="rows", read_len=L, quals=True, bc=True, n=N):
    from supernova_amd.engine import dev_reads
    return dev_reads(d[rows][:n], read_len, d["quals"][:n] if quals else None, None, None, d["bc"][:n] if bc else None)


# ---- the four entry points; a case is (params fields, job fields, reads fields)
def resident(e, d, P, job, rd):
    return e.count_graph_reads(reads(d, **rd), P)


def streamed(e, d, P, job, rd):
    e.stream_begin(job.get("read_len", L), job.get("ub", N), job.get("has_bc", True), P)
    e.stream_append_reads(reads(d, **rd))
    return e.stream_finish()


def _rank(e):
    from supernova_amd.sharded import ShardedEngine, SimWorld
    w = SimWorld(1)                  # (a step that fails aborts its communicator: every step gets its own)
    return w, ShardedEngine(e, w.comm(0))


def shard(e, d, P, job, rd):
    w, sh = _rank(e)
    try:
        res = sh.count_graph_reads(reads(d, **rd), P, total_reads=N)
        return res.unitigs()
    finally:
        sh.close()


def shard_streamed(e, d, P, job, rd):
    from supernova_amd import lib as _lib
    from supernova_amd.sharded import ShardedResult
    w, sh = _rank(e)
    try:
        p = P.to_c()
        e._call(e.lib.snk_shard_stream_begin, sh.comm, C.byref(p), job.get("read_len", L), job.get("ub", N), N, 1 if job.get("has_bc", True) else 0)
        r = reads(d, **rd)
        e._call(e.lib.snk_shard_stream_append, C.byref(r))
        raw = _lib.SnkShardResult()
        e._call(e.lib.snk_shard_stream_finish, sh.comm, 0, C.byref(raw))
        return ShardedResult(e, P.K, raw).unitigs()
    finally:
        sh.close()


ENTRY = dict(resident=resident, streamed=streamed, shard=shard, shard_streamed=shard_streamed)

K47 = "K=47 is not supported (48 or 60)"
BC9 = "min_bc=9: the device barcode rule tells up to eight distinct barcodes apart (min_bc <= 8)"
# (entry point, params, job, reads, code, message)
REFUSALS = [
    ("resident", dict(K=47), {}, {}, UNSUPPORTED, K47),
    ("streamed", dict(K=47), {}, {}, UNSUPPORTED, K47),
    ("shard", dict(K=47), {}, {}, UNSUPPORTED, K47),
    ("shard_streamed", dict(K=47), {}, {}, UNSUPPORTED, K47),
    ("resident", dict(min_bc=9), {}, {}, UNSUPPORTED, BC9),
    ("streamed", dict(min_bc=9), {}, {}, UNSUPPORTED, BC9),
    ("shard", dict(min_bc=9), {}, {}, UNSUPPORTED, BC9),
    ("shard_streamed", dict(min_bc=9), {}, {}, UNSUPPORTED, BC9),
    # read_len = 257
    ("resident", {}, {}, dict(read_len=257), ARG, "snk_dev_count_graph: bad rows/read_len (read_len <= 256)"),
    ("streamed", {}, dict(read_len=257), dict(read_len=257), ARG, "snk_dev_stream_begin: read_len 1..256 and an upper bound of the job's reads are needed"),
    ("shard", {}, {}, dict(read_len=257), ARG, "snk_shard_hist: bad reads"),
    ("shard_streamed", {}, dict(read_len=257), dict(read_len=257), ARG, "snk_shard_stream_begin: read_len 1..256 and an upper bound of this rank's reads are needed"),
    # row_words * 16 < read_len
    ("resident", {}, {}, dict(rows="narrow"), ARG, "snk_dev_count_graph: bad rows/read_len (read_len <= 256)"),
    ("streamed", {}, {}, dict(rows="narrow"), ARG, "snk_dev_stream_append: bad rows / read_len (the job's is 100)"),
    ("shard", {}, {}, dict(rows="narrow"), ARG, "snk_shard_hist: bad reads"),
    ("shard_streamed", {}, {}, dict(rows="narrow"), ARG, "snk_shard_stream_append: bad rows / read_len (the step's is 100)"),
    # neither quals nor good_len
    ("resident", {}, {}, dict(quals=False), ARG, "snk_dev_count_graph: need quals or good_len"),
    ("streamed", {}, {}, dict(quals=False), ARG, "snk_dev_stream_append: need quals or good_len"),
    ("shard", {}, {}, dict(quals=False), ARG, "snk_shard_hist: bad reads"),
    ("shard_streamed", {}, {}, dict(quals=False), ARG, "snk_shard_stream_append: need quals or good_len"),
    # the streamed forms: a slab with another read_len, barcodes in a job opened without them, one read more than the bound
    ("streamed", {}, {}, dict(read_len=99), ARG, "snk_dev_stream_append: bad rows / read_len (the job's is 100)"),
    ("shard_streamed", {}, {}, dict(read_len=99), ARG, "snk_shard_stream_append: bad rows / read_len (the step's is 100)"),
    ("streamed", {}, dict(has_bc=False), {}, ARG, "snk_dev_stream_append: every slab carries barcodes, or none does"),
    ("shard_streamed", {}, dict(has_bc=False), {}, ARG, "snk_shard_stream_append: every slab carries barcodes, or none does"),
    ("streamed", {}, dict(ub=N - 1), {}, ARG, "snk_dev_stream_append: more reads than the job's upper bound (0 + 64 > 63)"),
    ("shard_streamed", {}, dict(ub=N - 1), {}, ARG, "snk_shard_stream_append: more reads than the rank's upper bound (0 + 64 > 63)"),
]


def good(entry, e, d):
    from supernova_amd.engine import Params
    out = ENTRY[entry](e, d, Params(K=K), {}, {})
    return sorted(out if isinstance(out, list) else out.unitigs())


@pytest.fixture(scope="module")
def expected(data):
    """The good job on a fresh context, through every entry point: one unitig set, not an empty one."""
    from supernova_amd.engine import Engine
    outs = {}
    for entry in ENTRY:
        e = Engine(0)
        outs[entry] = good(entry, e, data)
        e.close()
    ref = outs["resident"]
    assert ref and all(o == ref for o in outs.values()), {k: len(v) for k, v in outs.items()}
    return ref


@pytest.mark.parametrize("entry,params,job,rd,code,msg", REFUSALS, ids=[f"{r[0]}-{i}" for i, r in enumerate(REFUSALS)])
def test_refusal_and_the_context_afterwards(data, expected, entry, params, job, rd, code, msg):
    from supernova_amd.engine import Engine, Params
    from supernova_amd.lib import SnkError
    e = Engine(0)
    try:
        with pytest.raises(SnkError) as ei:
            ENTRY[entry](e, data, Params(**dict(dict(K=K), **params)), job, rd)
        got = (ei.value.code, str(ei.value).split(": ", 1)[1])
        print("refusal:", entry, params, job, rd, "->", got)
        assert got == (code, msg)
        assert good(entry, e, data) == expected
    finally:
        e.close()


def test_sharded_step_without_reads(data):
    """snk_shard_step on a rank that holds no reads (a one-rank job: nothing at all): an empty table and no unitigs, as on one GPU."""
    from supernova_amd.engine import Engine, Params
    from supernova_amd.sharded import ShardedEngine, SimWorld
    e = Engine(0)
    sh = ShardedEngine(e, SimWorld(1).comm(0))
    try:
        res = sh.count_graph_reads(reads(data, n=0), Params(K=K))
        assert res.n_instances == 0 and res.n_kmers == 0 and res.n_unitigs == 0
        assert res.keys().shape[0] == 0 and res.unitigs() == []
    finally:
        sh.close()
        e.close()
