"""FASTH ingest on the device (snk_dev_ingest_fasth, snk_dev_ingest_count_graph) on the files an operator may bring and the library's own
synthetic writer never makes: ragged reads, N / lowercase bases, CRLF, a missing final newline, gzip members cut in the middle of a line,
empty members, every kind of barcode field; reads longer than read_len; lanes that only fit by growing the arrays or by a second pass.

Expected values never come from the library: arrays from the pure-Python restatement of the reference's reader (tests/fasthgen.Expected over
supernova_amd.martian.read_fasth, pinned to the reference's vectors in tests/test_martian.py), count + graph from the C oracle on those arrays."""
import os
import re

import numpy as np
import pytest

import fasthgen
import oracle_lib
import pathgen

pytestmark = pytest.mark.gpu

SNK_E_ARG, SNK_E_UNSUPPORTED = -1, -6
DEFAULT_BATCH_PAIRS = 65536          # include/snk.h: batch_pairs = 0


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


def _arrays(engine, dr):
    n = dr.n_reads
    dl = lambda ptr, shape, dt: (lambda a: (engine._download(ptr, a.ctypes.data, a.nbytes), a)[1])(np.empty(shape, dtype=dt))
    if n == 0:
        return (np.zeros((0, int(dr.raw.row_words)), np.uint32), np.zeros((0, int(dr.raw.qstride)), np.uint8), np.zeros(0, np.uint16), np.zeros(0, np.int32))
    return (dl(dr.raw.rows, (n, int(dr.raw.row_words)), np.uint32), dl(dr.raw.quals, (n, int(dr.raw.qstride)), np.uint8),
            dl(dr.raw.lens, (n,), np.uint16), dl(dr.raw.bc, (n,), np.int32))


def _check_arrays(engine, dr, exp):
    from supernova_amd import synth
    assert dr.n_reads == exp.n and int(dr.raw.qstride) == exp.qstride and int(dr.raw.row_words) == exp.rows.shape[1]
    rows, quals, lens, bc = _arrays(engine, dr)
    assert np.array_equal(lens, exp.lens)
    assert np.array_equal(bc, exp.bc)
    inside = np.arange(exp.qstride)[None, :] < exp.lens[:, None].astype(np.int64)
    assert np.array_equal(quals[inside], exp.quals[inside])                  # quals[:, :len]
    assert not quals[~inside].any()                                           # zero from the read's OWN length out to qstride
    codes = synth.unpack_rows(rows, 16 * rows.shape[1]) if exp.n else np.zeros((0, exp.qstride), np.uint8)
    assert not codes[~inside].any()                                           # packed codes at or beyond a read's length are 0
    assert np.array_equal(rows, exp.rows)


def _oracle(exp, K):
    gl = oracle_lib.good_lens(exp.quals[:, :exp.read_len], exp.lens, K=K)
    return oracle_lib.OracleResult(exp.codes, gl, exp.bc, K=K, hbv=False), gl


def _check_result(res, o, gl, in_order):
    assert res.n_reads == len(gl)
    got_gl = res.good_len().astype(np.uint32)
    if in_order:
        assert np.array_equal(got_gl, gl)
    assert sorted(got_gl.tolist()) == sorted(gl.tolist())                     # (a streamed job numbers its reads in arrival order)
    assert np.array_equal(res.keys(), o.keys.reshape(-1, 4))
    assert np.array_equal(np.minimum(res.counts(), (1 << 24) - 1), o.counts)
    assert np.array_equal(res.ctx(), o.ctx)
    spec = res.spectrum()
    assert np.array_equal(spec.astype(np.int64), np.bincount(np.minimum(o.counts, len(spec) - 1), minlength=len(spec)))      # last bin = overflow
    assert res.unitigs() == o.unitigs


# ---------------------------------------------------------------------------------------------------------------- 1. ragged lane, resident
_odd_cache = {}


def _odd_lane(tmp_path_factory, read_len):
    if read_len not in _odd_cache:
        rng = np.random.default_rng(0xFA57 + read_len)
        wl, seqs = fasthgen.odd_whitelist(rng)
        sizes = (1, 1500, 700, 0, 400)
        paths = fasthgen.odd_layout(tmp_path_factory.mktemp(f"odd{read_len}"), fasthgen.odd_records(rng, sum(sizes), read_len, seqs), sizes)
        exp = fasthgen.Expected(paths, wl, read_len)
        assert exp.n == 2 * sum(sizes) and len(set(exp.bc.tolist())) > 10 and (exp.bc == 0).sum() > exp.n // 5 and int(exp.bc.max()) > len(seqs)
        assert 8 in exp.bc and 4 not in exp.bc                  # the duplicated whitelist line: the later index wins
        _odd_cache[read_len] = (paths, wl, sizes, exp, fasthgen.text_size(paths))
    return _odd_cache[read_len]


@pytest.mark.parametrize("threads,batch_pairs", [(1, 1), (3, 37), (0, 0)])
@pytest.mark.parametrize("read_len", [144, 150, 250])
def test_ragged_lane_resident(engine, tmp_path_factory, read_len, threads, batch_pairs):
    """144: stride == read_len; 150: ten pad bytes per row; 250: sixteen words per row.  One pair per batch, batches that cut files at odd
    places, and the defaults."""
    from supernova_amd import ingest
    paths, wl, sizes, exp, text = _odd_lane(tmp_path_factory, read_len)
    dr = ingest.ingest_fasth(engine, paths, read_len, wl, threads=threads, batch_pairs=batch_pairs)
    try:
        _check_arrays(engine, dr, exp)
        bp = batch_pairs or DEFAULT_BATCH_PAIRS
        assert dr.stats["n_reads"] == exp.n and dr.stats["text_bytes"] == text and dr.stats["max_len"] == int(exp.lens.max()) == read_len
        assert dr.stats["n_batches"] >= sum(-(-m // bp) for m in sizes) and dr.stats["n_files"] == len(paths)
    finally:
        dr.close()


# ---------------------------------------------------------------------------------------------------------------- 2. ragged lane, counted
@pytest.fixture(scope="module")
def genome_lane(tmp_path_factory):
    rng = np.random.default_rng(0x6E0)
    wl, seqs = fasthgen.odd_whitelist(rng)
    g, spots = pathgen.genome(rng, 20_000)
    sizes = (1, 1500, 900, 0, 599)
    codes, quals, lens, bc = pathgen.pairs(rng, g, sum(sizes), 150, 0.004, 30, spots=spots, ragged=0.3)
    paths = fasthgen.odd_layout(tmp_path_factory.mktemp("genome"), fasthgen.records_of_reads(codes, quals, lens, bc, seqs), sizes, tag="gen")
    exp = fasthgen.Expected(paths, wl, 150)
    assert exp.n == 2 * sum(sizes) and np.array_equal(exp.lens, lens) and np.array_equal(exp.codes, codes)
    return paths, wl, exp


@pytest.fixture(scope="module")
def genome_oracle(genome_lane):
    cache = {}

    def get(K):
        if K not in cache:
            cache[K] = _oracle(genome_lane[2], K)
            assert len(cache[K][0].unitigs) > 0 and len(cache[K][0].counts) > 10_000      # something survives min_freq
        return cache[K]
    return get


def test_ragged_lane_counted_resident(engine, genome_lane, genome_oracle):
    from supernova_amd import ingest
    from supernova_amd.engine import Params
    paths, wl, exp = genome_lane
    o, gl = genome_oracle(48)
    dr = ingest.ingest_fasth(engine, paths, 150, wl, threads=2, batch_pairs=257)
    try:
        _check_arrays(engine, dr, exp)
        _check_result(engine.count_graph_reads(dr.dev_reads(), Params(K=48)), o, gl, in_order=True)
    finally:
        dr.close()


@pytest.mark.parametrize("K", [48, 60])
def test_ragged_lane_counted_streamed(engine, genome_lane, genome_oracle, K):
    from supernova_amd import ingest
    from supernova_amd.engine import Params
    paths, wl, exp = genome_lane
    o, gl = genome_oracle(K)
    res, st = ingest.ingest_count_graph(engine, paths, 150, wl, params=Params(K=K), threads=2, batch_pairs=257, total_reads_hint=exp.n)
    assert st["n_reads"] == exp.n and st["text_bytes"] == fasthgen.text_size(paths) and st["max_len"] == int(exp.lens.max())
    _check_result(res, o, gl, in_order=False)


# ---------------------------------------------------------------------------------------------------------------- 3. the over-long read
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _bases(rng, length):
    return _ACGT[rng.integers(0, 4, length)].tobytes().decode("ascii")


def _plain_records(rng, n_pairs, lo, hi, seqs, qual=None):
    """Random reads of lo..hi bases; qual: one quality for every base (binned qualities: such text deflates far better), None = random."""
    recs = []
    for q in range(n_pairs):
        ls = [int(rng.integers(lo, hi + 1)) for _ in range(2)]
        qs = [rng.integers(2, 42, l) if qual is None else np.full(l, qual) for l in ls]
        recs.append(fasthgen.record(_bases(rng, ls[0]), qs[0], _bases(rng, ls[1]), qs[1], seqs[q % len(seqs)] + "-1"))
    return recs


def _with_read(rec, mate, length, rng):
    r = list(rec)
    r[2 * mate] = _bases(rng, length)
    r[2 * mate + 1] = rng.integers(2, 42, length).astype(np.uint8)
    return tuple(r)


@pytest.fixture(scope="module")
def good_lane(tmp_path_factory):
    rng = np.random.default_rng(77)
    wl, seqs = fasthgen.odd_whitelist(rng)
    d = tmp_path_factory.mktemp("good")
    paths = [fasthgen.write_fasth(d / f"good{i}.fasth.gz", _plain_records(rng, 23, 60, 150, seqs)) for i in range(2)]
    return paths, wl, seqs, {rl: fasthgen.Expected(paths, wl, rl) for rl in (150, 160)}


def _lane_with(tmp_path, seqs, length, where, seed):
    """Three files of 21 pairs with reads of 100..150 bases, and one read of `length` bases."""
    rng = np.random.default_rng(seed)
    files = [_plain_records(rng, 21, 100, 150, seqs) for _ in range(3)]
    fi, q, mate = {"first": (0, 0, 0), "last": (2, 20, 1), "middle_r2": (1, 10, 1)}[where]
    files[fi][q] = _with_read(files[fi][q], mate, length, rng)
    return [fasthgen.write_fasth(tmp_path / f"l{i}.fasth.gz", recs) for i, recs in enumerate(files)]


def _good_after(engine, good_lane, read_len):
    from supernova_amd import ingest
    paths, wl, _, exps = good_lane
    dr = ingest.ingest_fasth(engine, paths, read_len, wl, threads=2, batch_pairs=8)
    try:
        _check_arrays(engine, dr, exps[read_len])
    finally:
        dr.close()


@pytest.mark.parametrize("where", ["first", "last", "middle_r2"])
@pytest.mark.parametrize("read_len,length", [(150, 151), (150, 160), (150, 161), (160, 161)])
def test_over_long_read_is_refused(engine, good_lane, tmp_path, read_len, length, where):
    """A read longer than read_len is refused by both entry points -- inside the 16-byte row stride (151, 160 at read_len 150) as well as
    beyond it (161) -- and the engine goes on to ingest a good lane: the stream, the page-locked batches and the context were released."""
    from supernova_amd import ingest
    from supernova_amd.engine import Params
    from supernova_amd.lib import SnkError
    _, wl, seqs, _ = good_lane
    paths = _lane_with(tmp_path, seqs, length, where, seed=length * 7 + len(where))
    for call in (lambda: ingest.ingest_fasth(engine, paths, read_len, wl, threads=2, batch_pairs=8),
                 lambda: ingest.ingest_count_graph(engine, paths, read_len, wl, params=Params(K=48), threads=2, batch_pairs=8, total_reads_hint=126)):
        with pytest.raises(SnkError) as ei:
            call()
        assert ei.value.code == SNK_E_UNSUPPORTED, str(ei.value)
        assert re.search(rf"\b{length}\b", str(ei.value)) and re.search(rf"read_len = {read_len}\b", str(ei.value)), str(ei.value)
        _good_after(engine, good_lane, read_len)


@pytest.mark.parametrize("where", ["first", "last", "middle_r2"])
@pytest.mark.parametrize("read_len", [150, 160])
def test_read_of_read_len_is_accepted(engine, good_lane, tmp_path, read_len, where):
    from supernova_amd import ingest
    from supernova_amd.engine import Params
    _, wl, seqs, _ = good_lane
    paths = _lane_with(tmp_path, seqs, read_len, where, seed=read_len + len(where))
    exp = fasthgen.Expected(paths, wl, read_len)
    assert int(exp.lens.max()) == read_len
    dr = ingest.ingest_fasth(engine, paths, read_len, wl, threads=2, batch_pairs=8)
    try:
        assert dr.stats["max_len"] == read_len
        _check_arrays(engine, dr, exp)
    finally:
        dr.close()
    res, st = ingest.ingest_count_graph(engine, paths, read_len, wl, params=Params(K=48), threads=2, batch_pairs=8, total_reads_hint=exp.n)
    assert st["n_reads"] == exp.n and st["max_len"] == read_len
    o, gl = _oracle(exp, 48)
    _check_result(res, o, gl, in_order=False)


# ---------------------------------------------------------------------------------------------------------------- 4. growth and reorder
def _trace(capfd):
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[snk ingest]")]
    return lines


def _compressible_files(d, over_long=0):
    """Two files of 2 000 copies of one pair (120 and 100 bases) at gzip level 9: a few bytes per read.  over_long: the last record of the
    last file gets an R1 of that many bases."""
    rng = np.random.default_rng(99)
    wl, seqs = fasthgen.odd_whitelist(rng)
    g, _ = pathgen.genome(rng, 600, plants=False)
    a = "".join("ACGT"[i] for i in g[:120])
    b = "".join("ACGT"[3 - i] for i in g[449:349:-1])
    rec = fasthgen.record(a, np.full(120, 30), b, np.full(100, 30), seqs[5] + "-1")
    rec2 = fasthgen.record(a, np.full(120, 30), b, np.full(100, 30), seqs[6] + "-1")          # (two barcodes: the k-mers pass min_bc = 2)
    files = [[rec, rec2] * 1000 for _ in range(2)]
    if over_long:
        files[-1][-1] = _with_read(files[-1][-1], 0, over_long, rng)
    return [fasthgen.write_fasth(d / f"c{i}.fasth.gz", recs, level=9) for i, recs in enumerate(files)], wl


@pytest.fixture(scope="module")
def compressible_lane(tmp_path_factory):
    paths, wl = _compressible_files(tmp_path_factory.mktemp("comp"))
    return paths, wl, fasthgen.Expected(paths, wl, 150)


def test_array_growth_ran(engine, compressible_lane, capfd, monkeypatch):
    from supernova_amd import ingest
    paths, wl, exp = compressible_lane
    bp = 16
    cap0 = sum(os.path.getsize(p) for p in paths) // 70 + 4 * bp            # the first capacity (include/snk.h: a guess from the compressed sizes)
    assert exp.n == 8000 and cap0 * 1.5 ** 2 + 2 * 2 * bp * 2.5 < exp.n, cap0       # two growths (x1.5 + a batch each) cannot hold the lane
    monkeypatch.setenv("SNK_INGEST_TRACE", "1")
    capfd.readouterr()
    dr = ingest.ingest_fasth(engine, paths, 150, wl, threads=1, batch_pairs=bp)
    try:
        lines = _trace(capfd)
        _check_arrays(engine, dr, exp)
        assert dr.stats["n_batches"] >= exp.n // (2 * bp)
        m = re.search(r"arrays grown (\d+) times", lines[-1]) if lines else None
        assert m, lines
        assert int(m.group(1)) >= 3, lines[-1]
    finally:
        dr.close()


def test_over_long_read_after_growth_is_refused(engine, good_lane, tmp_path):
    """The refusal of an over-long read when the resident arrays have already been replaced by larger ones several times: the last record
    of the compressible lane has an R1 of 151 bases.  One decode thread has four batches (threads + threads + 2), so all but four batches
    have been given their place in the arrays -- which two growths cannot hold -- when the refusal arrives."""
    from supernova_amd import ingest
    from supernova_amd.lib import SnkError
    paths, wl = _compressible_files(tmp_path, over_long=151)
    bp, n, pool = 16, 8000, 1 + 1 + 2
    cap0 = sum(os.path.getsize(p) for p in paths) // 70 + 4 * bp
    assert cap0 * 1.5 ** 2 + 2 * 2 * bp * 2.5 < n - pool * 2 * bp, cap0
    with pytest.raises(SnkError) as ei:
        ingest.ingest_fasth(engine, paths, 150, wl, threads=1, batch_pairs=bp)
    assert ei.value.code == SNK_E_UNSUPPORTED, str(ei.value)
    assert re.search(r"\b151\b", str(ei.value)) and re.search(r"read_len = 150\b", str(ei.value)), str(ei.value)
    _good_after(engine, good_lane, 150)


def test_reorder_ran(engine, tmp_path, capfd, monkeypatch):
    """Four files, the first ten times the others, four decode threads: the small files' batches arrive while the first file is still
    being read, so the arrival order is not file-major and the arrays are permuted on the device."""
    from supernova_amd import ingest
    rng = np.random.default_rng(123)
    wl, seqs = fasthgen.odd_whitelist(rng)
    sizes = (3000, 300, 300, 300)
    paths = [fasthgen.write_fasth(tmp_path / f"r{i}.fasth.gz", _plain_records(rng, m, 90, 150, seqs), tag=f"r{i}_") for i, m in enumerate(sizes)]
    exp = fasthgen.Expected(paths, wl, 150)
    monkeypatch.setenv("SNK_INGEST_TRACE", "1")
    capfd.readouterr()
    dr = ingest.ingest_fasth(engine, paths, 150, wl, threads=4, batch_pairs=64)
    try:
        lines = _trace(capfd)
        _check_arrays(engine, dr, exp)
        m = re.search(r"reordered (\d)", lines[-1]) if lines else None
        assert m, lines
        assert m.group(1) == "1", lines[-1]
    finally:
        dr.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the streamed path's own bound
def _derived_bound(paths, read_len, batch_pairs):
    """What the library derives for total_reads_hint = 0 (include/snk.h): compressed bytes / 45 or the trailers' text sizes / (2 read_len + 2)."""
    comp = sum(os.path.getsize(p) for p in paths)
    isize = sum(int.from_bytes(open(p, "rb").read()[-4:], "little") for p in paths)
    return max(comp // 45, isize // (2 * read_len + 2)) + 8 * batch_pairs


@pytest.fixture(scope="module")
def bound_lanes(tmp_path_factory, compressible_lane):
    rng = np.random.default_rng(0xB0)
    wl, seqs = fasthgen.odd_whitelist(rng)
    g, spots = pathgen.genome(rng, 6_000)
    d = tmp_path_factory.mktemp("bound")
    lanes = {}
    # (a) every file is cat of four members: a trailer speaks for the last member only (binned qualities: under 45 bytes per read)
    codes, quals, lens, bc = pathgen.pairs(rng, g, 1600, 150, 0.004, 30, spots=spots)
    quals = np.where(quals >= 13, 37, quals).astype(np.uint8)
    recs = fasthgen.records_of_reads(codes, quals, lens, bc, seqs)
    paths = []
    for i in range(2):
        part = recs[i * 800:(i + 1) * 800]
        t = len(fasthgen.text_of(part))
        paths.append(fasthgen.write_fasth(d / f"a{i}.fasth.gz", part, level=9, cuts=(t // 2 + 1, t * 3 // 4 + 3, t * 15 // 16 + 5), tag=f"a{i}_"))
    lanes["four_members"] = (paths, wl, fasthgen.Expected(paths, wl, 150))
    # (b) reads of 20..40 bases at read_len 150: far less text per read than 2 read_len + 2
    paths = [fasthgen.write_fasth(d / f"b{i}.fasth.gz", _plain_records(rng, 1500, 20, 40, seqs, qual=37), level=9, tag=f"b{i}_") for i in range(2)]
    lanes["short_reads"] = (paths, wl, fasthgen.Expected(paths, wl, 150))
    # (c) the compressible lane
    lanes["compressible"] = compressible_lane
    return lanes


@pytest.mark.parametrize("lane", ["four_members", "short_reads", "compressible"])
def test_streamed_default_bound(engine, bound_lanes, lane, capfd, monkeypatch):
    """total_reads_hint = 0 is the library's guess.  Where the guess is too small the job is run again with the count of the first pass
    (the trace says so), and the result is the oracle's either way; with the true count as the hint there is one pass.  Batches of 16
    pairs on repeat-rich lanes (four_members, compressible) are also what a streamed job's overflow list has to take from hundreds of
    small launches: every launch used to start at overflow sub-list 0 and overran it at a sixty-fourth of the list's size."""
    from supernova_amd import ingest
    from supernova_amd.engine import Params
    from supernova_amd.lib import SnkError
    paths, wl, exp = bound_lanes[lane]
    bp = 16
    o, gl = _oracle(exp, 48)
    if lane != "short_reads":
        assert len(o.counts) > 100 and len(o.unitigs) > 0
    too_small = _derived_bound(paths, 150, bp) < exp.n
    assert too_small                                           # (the lanes are built so that the guess cannot hold them)
    monkeypatch.setenv("SNK_INGEST_TRACE", "1")
    for hint in (exp.n, 0):
        capfd.readouterr()
        res, st = ingest.ingest_count_graph(engine, paths, 150, wl, params=Params(K=48), threads=2, batch_pairs=bp, total_reads_hint=hint)
        restarted = any("restarted" in l for l in _trace(capfd))
        assert restarted == (hint == 0 and too_small)
        assert st["n_reads"] == exp.n and st["text_bytes"] == fasthgen.text_size(paths) and st["max_len"] == int(exp.lens.max())
        _check_result(res, o, gl, in_order=False)
    # a caller's own hint that is too small is refused, as soon as it is crossed, with a message one can act on
    with pytest.raises(SnkError, match="upper bound") as ei:
        ingest.ingest_count_graph(engine, paths, 150, wl, params=Params(K=48), threads=2, batch_pairs=bp, total_reads_hint=exp.n // 3)
    assert ei.value.code == SNK_E_ARG and f"total_reads_hint = {exp.n // 3}" in str(ei.value)
    seen = int(re.search(r"(\d+) reads decoded so far", str(ei.value)).group(1))
    assert exp.n // 3 < seen <= exp.n // 3 + 2 * bp                 # refused at the first batch that crosses it


# ---------------------------------------------------------------------------------------------------------------- 6. zero reads
def test_zero_reads(engine, good_lane, tmp_path):
    from supernova_amd import ingest
    from supernova_amd.engine import Params
    _, wl, _, _ = good_lane
    paths = [fasthgen.write_empty(tmp_path / f"e{i}.fasth.gz") for i in range(3)]
    dr = ingest.ingest_fasth(engine, paths, 150, wl, threads=2, batch_pairs=8)
    try:
        assert dr.n_reads == 0 and dr.stats["text_bytes"] == 0 and dr.stats["max_len"] == 0 and dr.stats["n_batches"] == 0
        res = engine.count_graph_reads(dr.dev_reads(), Params(K=48))
        assert res.n_instances == 0 and res.n_kmers == 0 and res.n_unitigs == 0 and res.keys().shape == (0, 4) and res.unitigs() == []
    finally:
        dr.close()
    for hint in (0, 1000):
        res, st = ingest.ingest_count_graph(engine, paths, 150, wl, params=Params(K=48), threads=2, batch_pairs=8, total_reads_hint=hint)
        assert st["n_reads"] == 0 and res.n_reads == 0
        assert res.n_instances == 0 and res.n_kmers == 0 and res.n_unitigs == 0 and res.keys().shape == (0, 4) and res.unitigs() == []
    _good_after(engine, good_lane, 150)
