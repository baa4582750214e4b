"""Pin the CPU oracle (oracle/snk_oracle.c) against the reference's own outputs and known-answer tests.

Golden vectors: tests/golden/*.npz, dumped from the reference binary (path B, lib/assembly) by
tests/golden/make_golden.py.  Known-answer tests restated from the reference's Rust unit tests.
"""
import numpy as np
import pytest

import goldens
import oracle_lib


@pytest.mark.parametrize("name", goldens.CASES)
def test_oracle_matches_reference(name):
    c = goldens.load(name)
    gl = oracle_lib.good_lens(c.quals, c.lens, K=48, min_qual=7)
    assert np.array_equal(gl, c.exp_goodlens)
    o = oracle_lib.OracleResult(c.codes, gl, c.bc, K=48, min_freq=3, min_bc=2, ign_bc_below=c.ign_bc_below)
    assert o.keys.shape[0] == c.exp_keys.shape[0]
    assert np.array_equal(o.keys[:, :3], c.exp_keys)
    assert np.all(o.keys[:, 3] == 0)
    assert np.array_equal(np.minimum(o.counts, (1 << 24) - 1), c.exp_counts)   # B saturates at 2^24-1 (ReadPather.h:128-129)
    assert np.array_equal(o.ctx, c.exp_ctx)
    assert o.unitigs == c.exp_unitigs
    assert o.hbv_text() == c.exp_hbv
    hist = np.bincount(np.minimum(o.counts, (1 << 24) - 1)) if len(o.counts) else np.zeros(0, np.int64)
    assert np.array_equal(hist, c.exp_hist)       # stats/histogram_kmer_count.json (BuildReadQGraph48.cc:199-216)


def test_qv_trim_read_kat():
    """lib/tada/src/cmd_msp.rs:329-350 test_qv_trim_read (min_qual 10, K=48), expectation formula at :347."""
    quals = np.frombuffer(
        b"FFFFFFFFIFFFFFFFFFFIIIFFBFIFFFFIFBFFIBFIFBBFFIFFIFFFFFFFFFFFBBBBBBBBBB07BB7BB<BBBBBBBBBB", dtype=np.uint8)
    K = 48
    n = len(quals)
    for i in range(n):
        q = quals.copy()
        q[i] = 34
        got = int(oracle_lib.good_lens((q - 33)[None, :], n, K=K, min_qual=10)[0])
        exp = n if i < n - K else (i if i >= K else 0)
        assert got == exp, (i, got, exp)


def test_msp_slices_cover_all_kmers():
    """lib/tada/src/msp/mod.rs:202-220 test_slice: union of k-mers over MSP slices == all k-mers (k=50,p=8)."""
    rng = np.random.default_rng(7)
    k, p = 50, 8
    perm = rng.permutation(1 << (2 * p)).astype(np.uint32)
    for it in range(50):
        seq = rng.integers(0, 4, int(rng.integers(k, 400)), dtype=np.uint8)
        sl = oracle_lib.msp_scan(k, p, seq, perm)
        s = bytes(seq)
        allk = {s[i:i + k] for i in range(len(s) - k + 1)}
        got = set()
        for (_v, mp, st, ln) in sl:
            assert ln >= k and ln <= 2 * k - p
            assert st <= mp and mp + p <= st + ln
            for i in range(st, st + ln - k + 1):
                got.add(s[i:i + k])
        assert got == allk


def test_msp_shard_consistency():
    """lib/tada/src/kmer/mod.rs:1102-1150 check_consistent_shard: a k-mer (either strand) always gets the same value."""
    rng = np.random.default_rng(11)
    k, p = 48, 8
    perm = rng.permutation(1 << (2 * p)).astype(np.uint32)
    seen = {}
    base = rng.integers(0, 4, 300, dtype=np.uint8)
    for it in range(60):
        seq = base.copy()
        for _ in range(3):
            seq[int(rng.integers(0, len(seq)))] = rng.integers(0, 4)
        if it & 1:
            seq = (3 - seq[::-1]).astype(np.uint8)
        s = bytes(seq)
        for (v, _mp, st, ln) in oracle_lib.msp_scan(k, p, seq, perm):
            for i in range(st, st + ln - k + 1):
                km = s[i:i + k]
                rc = bytes(3 - b for b in reversed(km))
                key = min(km, rc)
                assert seen.setdefault(key, v) == v


def test_bv_roundtrip(tmp_path):
    """.bv hand-off format round trip (lib/tada/src/sim_tests.rs:142-179; debruijn.rs:895-929)."""
    import ctypes as C
    lib = oracle_lib.load()
    c = goldens.load("adversarial")
    o = oracle_lib.OracleResult(c.codes, c.exp_goodlens, c.bc, ign_bc_below=c.ign_bc_below, hbv=False)
    u = oracle_lib.Unitigs()
    off = np.ascontiguousarray(o.unitig_off, dtype=np.uint64)
    b = np.ascontiguousarray(o.unitig_bases, dtype=np.uint8)
    u.n = len(o.unitigs)
    u.off = off.ctypes.data_as(C.POINTER(C.c_uint64))
    u.bases = b.ctypes.data_as(C.POINTER(C.c_uint8))
    path = str(tmp_path / "x.bv").encode()
    assert lib.sno_write_bv(path, C.byref(u)) == 0
    raw = open(path, "rb").read()
    assert raw[:8] == b"BINWRITE" and int.from_bytes(raw[8:16], "little") == len(o.unitigs)
    v = oracle_lib.Unitigs()
    assert lib.sno_read_bv(path, C.byref(v)) == 0
    assert v.n == u.n
    off2 = np.ctypeslib.as_array(v.off, shape=(v.n + 1,))
    assert np.array_equal(off2, off)
    assert np.array_equal(np.ctypeslib.as_array(v.bases, shape=(int(off[-1]),)), b)
    lib.sno_unitigs_free(C.byref(v))


@pytest.mark.parametrize("name", goldens.K60_CASES)
def test_oracle_k60_matches_reference(name):
    """K=60 pin: the reference's BuildReadQGraph60 (frequency rule only -> oracle run without a barcode vector)."""
    g = goldens.Case60(name)
    c = g.base
    gl = oracle_lib.good_lens(c.quals, c.lens, K=60, min_qual=7)
    assert np.array_equal(gl, g.exp_goodlens)
    o = oracle_lib.OracleResult(c.codes, gl, None, K=60, min_freq=3)
    assert np.array_equal(o.keys, g.exp_keys)
    assert np.array_equal(np.minimum(o.counts, (1 << 24) - 1), g.exp_counts)
    assert np.array_equal(o.ctx, g.exp_ctx)
    assert o.unitigs == g.exp_unitigs
    assert o.hbv_text() == g.exp_hbv


@pytest.mark.parametrize("name", goldens.CASES)
def test_read_paths_match_reference(name):
    """f1: the restatement of pathReads (new aligner) against the read paths the reference binary dumped for the golden cases:
    offset and HBV edge ids of every read, untrimmed reads, N bases as A."""
    c = goldens.load(name)
    off, n, edges = oracle_lib.path_reads(c.codes, c.quals, c.lens, c.exp_unitigs, K=48)
    bad = np.nonzero((n != c.exp_path_n))[0]
    assert len(bad) == 0, (len(bad), bad[:5], n[bad[:5]], c.exp_path_n[bad[:5]])
    assert np.array_equal(edges, c.exp_path_edges)
    assert np.array_equal(off, c.exp_path_off)


def _art_matches_log(n_art, n_pairs, logged):
    """The reference only LOGS the artifactual-duplicate percentage (two significant digits after its fixed/precision
    manipulators): the count is checked through the same rounding."""
    return float(f"{100.0 * n_art / n_pairs:.2g}") == float(f"{logged:.2g}")


@pytest.mark.parametrize("name", goldens.CASES)
def test_mark_dups_matches_reference(name):
    """f4: the restatement of MarkDups against the reference's own MarkDups (10X/SecretOps.cc:413-593) run on the read paths
    it made for the golden cases: the flag of every pair, the inter-barcode rate exactly, the artifact share as logged."""
    c = goldens.load(name)
    dup, art, rate, nd, ni = oracle_lib.mark_dups(c.codes, c.quals, c.lens, c.exp_path_off, c.exp_path_n, c.exp_path_edges, bc=c.bc)
    assert len(dup) == len(c.exp_dup)
    assert np.array_equal(dup, c.exp_dup), np.nonzero(dup != c.exp_dup)[0][:10]
    assert rate == c.exp_interdup
    assert _art_matches_log(int(art.sum()), len(dup), c.exp_art_perc), (int(art.sum()), len(dup), c.exp_art_perc)
    if name == "synth_4k_dups":
        assert dup.sum() > 300 and art.sum() > 100 and 0.0 < rate < 1.0


def test_mark_dups_hand_case():
    """MarkDups by hand (10X/SecretOps.cc:413-593): four pairs of 10-base reads.  Reads 0 and 2 sit on (edge 5, offset 3) and
    their mates start with the same five bases: one duplicate group; read 2's pair has the larger quality sum and survives, so
    pair 0 is flagged; their barcodes differ (inter-barcode rate 1).  Read 4 shares the placement but its mate starts
    differently: no duplicate.  Reads 6 and 7... are not placed.  Then the same with equal qualities: a tie, the earliest read
    survives (pair 1 flagged) and pair 1 is an artifactual duplicate (identical bases and qualities)."""
    n, L = 8, 10
    codes = np.zeros((n, L), dtype=np.uint8)
    codes[1] = [0, 1, 2, 3, 0, 1, 1, 1, 1, 1]
    codes[3] = [0, 1, 2, 3, 0, 2, 2, 2, 2, 2]            # same first five bases as read 1
    codes[5] = [3, 1, 2, 3, 0, 1, 1, 1, 1, 1]            # another head
    quals = np.full((n, L), 5, dtype=np.uint8)
    quals[2] = 7                                          # pair 1: sum 120 against pair 0's 100
    path_off = np.array([3, 0, 3, 0, 3, 0, 0, 0], dtype=np.int32)
    path_n = np.array([1, 0, 1, 0, 1, 0, 0, 0], dtype=np.int32)
    path_edges = np.array([5, 5, 5], dtype=np.int32)
    bc = np.array([7, 7, 9, 9, 7, 7, 0, 0], dtype=np.int32)
    dup, art, rate, nd, ni = oracle_lib.mark_dups(codes, quals, L, path_off, path_n, path_edges, bc=bc)
    assert dup.tolist() == [1, 0, 0, 0] and art.tolist() == [0, 0, 0, 0] and (rate, nd, ni) == (1.0, 1, 1)
    quals[2] = 5                                          # a tie: the earliest read wins, the later identical one is an artifact
    bc[2:4] = 7
    dup, art, rate, nd, ni = oracle_lib.mark_dups(codes, quals, L, path_off, path_n, path_edges, bc=bc)
    assert dup.tolist() == [0, 1, 0, 0] and art.tolist() == [0, 1, 0, 0] and (rate, nd, ni) == (0.0, 1, 0)
    # barcode 0 adopts the next member's barcode without a comparison (:463-466)
    bc[0:2] = 0
    bc[2:4] = 9
    _, _, rate, _, _ = oracle_lib.mark_dups(codes, quals, L, path_off, path_n, path_edges, bc=bc)
    assert rate == 0.0
    # no barcode vector at all, and nothing placed
    dup, art, rate, nd, ni = oracle_lib.mark_dups(codes, quals, L, path_off, np.zeros(n, np.int32), np.zeros(0, np.int32))
    assert dup.sum() == 0 and art.sum() == 0 and (rate, nd, ni) == (0.0, 0, 0)


@pytest.mark.parametrize("name", ["robust_repeats_200k", "robust_err15_200k"])
def test_oracle_matches_reference_digest_off_the_operating_point(name):
    """The C restatement against the REFERENCE's digests (tests/golden/big_hashes.json, made by make_big_hashes.py from
    oracle/_ref/snref_driver) on 200 k reads of the models bench.py's config.robust runs: a repeat-rich genome (interspersed families at
    1-3 % divergence, exact 5-kb duplications, STRs, poly-A) and 1.5 % sequencing errors."""
    import json
    from pathlib import Path
    import bighash
    from supernova_amd import synth
    fix = Path(__file__).resolve().parent / "golden" / "big_hashes.json"
    exp = json.loads(fix.read_text()).get(name)
    if exp is None:
        pytest.skip("no fixture")
    sp = synth.synth_params(exp["n_reads"], seed=exp["seed"], **exp.get("overrides", {}))
    rows, quals, bc = synth.synth_host(sp)
    gl = oracle_lib.good_lens(quals, sp.read_len)
    o = oracle_lib.OracleResult(synth.unpack_rows(rows, sp.read_len), gl, bc, hbv=False)
    hist = np.bincount(np.minimum(o.counts, (1 << 24) - 1)).astype(np.int64)
    dg = bighash.digest(gl.astype(np.uint32), o.keys, np.minimum(o.counts, (1 << 24) - 1), o.ctx, o.unitigs, hist, kw=3)
    bad = [f for f in ("n_reads", "n_kmers", "n_unitigs", "unitig_bases", "goodlens", "keys", "counts", "ctx", "hist", "unitigs") if dg[f] != exp[f]]
    assert not bad, {f: (dg[f], exp[f]) for f in bad}


@pytest.fixture(scope="module", params=[48, 60])
def hot(request):
    """The saturating read set (tests/hotgen.py) through the C restatement, once per K: (fixture, good lengths, oracle result)."""
    K = request.param
    c = goldens.load_hot(K)
    gl = oracle_lib.good_lens(c.quals, c.lens, K=K, min_qual=7)
    return c, gl, oracle_lib.OracleResult(c.codes, gl, c.bc if K == 48 else None, K=K, min_freq=3, min_bc=2)


def test_oracle_saturates_as_the_reference_does(hot):
    """The 24-bit count field (kmers/ReadPather.h:127-131,145) reached by data: one k-mer with 17.9 M (K=48) / 16.8 M (K=60)
    instances, one with exactly 2^24-2 at K=48.  The restatement's RAW counts equal the reference's -- nothing is clamped on the
    oracle's side of the comparison -- and so do keys, contexts, unitigs, the spectrum and the graph."""
    import hotgen
    import a48xref
    c, gl, o = hot
    K = c.K
    assert hotgen.digest(gl.astype(np.uint32), [], [], []) == c.exp_goodlens_digest
    assert np.array_equal(o.keys[:, :c.exp_keys.shape[1]], c.exp_keys) and np.all(o.keys[:, c.exp_keys.shape[1]:] == 0)
    assert np.array_equal(o.counts, c.exp_counts)
    assert np.array_equal(o.ctx, c.exp_ctx)
    assert o.unitigs == c.exp_unitigs
    # the fixture is what it is for: the over family saturated, the under family exact, one entry in the last bin
    for fam in ("over", "under"):
        i = np.nonzero((o.keys == hotgen.homopolymer_key(fam, K)).all(axis=1))[0]
        assert len(i) == 1 and int(c.exp_counts[i[0]]) == min(hotgen.true_count(fam, K), hotgen.SAT), (fam, i)
    assert int((c.exp_counts == hotgen.SAT).sum()) == 1 and int(c.exp_counts.max()) == hotgen.SAT
    # lengths K (the homopolymer's self-loop), K+1 (the dinucleotide circle, where the solo family survives) and the background
    lens = sorted(len(u) for u in c.exp_unitigs)
    assert lens[:2] == [K, K] and (K + 1 in lens) == (K == 60) and lens[-1] > 2000
    hist = np.bincount(o.counts)
    if c.exp_hist_len:          # stats/histogram_kmer_count.json (BuildReadQGraph48.cc:199-216; the K=60 variant writes none)
        assert len(hist) == c.exp_hist_len == hotgen.SAT + 1
        assert np.array_equal(np.nonzero(hist)[0], c.exp_hist_bins) and np.array_equal(hist[c.exp_hist_bins], c.exp_hist_vals)
    assert len(hist) == hotgen.SAT + 1 and hist[-1] == 1
    g = a48xref.parse_hbv(c.exp_ahbv)
    h = o.hbv
    assert (h["n_vertices"], h["n_edges"]) == (g.N, g.E)
    assert np.array_equal(h["v_left"], g.v_left) and np.array_equal(h["v_right"], g.v_right)


def test_hot_hbv_files_match_the_reference_writers(snk, tmp_path, hot):
    """a.hbv / a.inv of the saturating set byte for byte (self-loop edges of the homopolymers, the two-k-mer circle)."""
    from supernova_amd import graphio
    c, _gl, o = hot
    off, bases = graphio.unitigs_to_arrays(o.unitigs)
    graphio.write_hbv(tmp_path / "a.hbv", tmp_path / "a.inv", c.K, off, bases)
    assert (tmp_path / "a.hbv").read_bytes() == c.exp_ahbv and (tmp_path / "a.inv").read_bytes() == c.exp_ainv


def big_group_sizes(codes, path_off, path_n, path_edges):
    """Record count of every duplicate group of MarkDups: placed reads by (first edge, offset, first five bases of the mate)."""
    n = len(path_n)
    start = np.zeros(n + 1, np.int64)
    start[1:] = np.cumsum(path_n)
    placed = np.asarray(path_n) > 0
    first = np.asarray(path_edges)[start[:-1][placed]]
    head = np.zeros(n, np.int64)
    for j in range(5):
        head = head * 4 + codes[np.arange(n) ^ 1, j]
    key = np.stack([first, np.asarray(path_off)[placed], head[placed]], axis=1)
    return np.sort(np.unique(key, axis=0, return_counts=True)[1])


BIG_GROUP_RECORDS = [7, 7, 64, 64, 65, 65, 126, 255, 255, 256, 256, 257, 257]      # both mates' groups; the self-complementary seed: one of 2 x 63


def test_big_duplicate_groups_match_reference():
    """MarkDups on groups of 7 to 257 pairs with interleaved runs (tests/pathgen.plant_big_groups; dup_groups.npz holds the
    reference's own paths and flags): the generator still makes the fixture's reads, the restated pathing and marking reproduce the
    reference, the groups have exactly the planted sizes and none is larger (the device walks a group with one thread, quadratic
    in its size: 257 is a bound by construction), and the plants do what they are for."""
    import pathgen
    c = goldens.load("dup_groups")
    codes, quals, lens, bc, groups = pathgen.big_group_reads()
    assert np.array_equal(codes, c.codes) and np.array_equal(quals, c.quals) and np.array_equal(lens, c.lens) and np.array_equal(bc, c.bc)
    gl = oracle_lib.good_lens(c.quals, c.lens)
    assert np.array_equal(gl, c.exp_goodlens)
    o = oracle_lib.OracleResult(c.codes, gl, c.bc)
    assert np.array_equal(o.keys[:, :3], c.exp_keys) and np.array_equal(o.counts, c.exp_counts) and o.unitigs == c.exp_unitigs
    off, n, edges = oracle_lib.path_reads(c.codes, c.quals, c.lens, o.unitigs)
    assert np.array_equal(n, c.exp_path_n) and np.array_equal(edges, c.exp_path_edges) and np.array_equal(off, c.exp_path_off)
    sizes = big_group_sizes(c.codes, off, n, edges)
    assert sizes[sizes >= 7].tolist() == BIG_GROUP_RECORDS and sizes.max() == 257
    dup, art, rate, nd, ni = oracle_lib.mark_dups(c.codes, c.quals, c.lens, off, n, edges, bc=c.bc)
    assert np.array_equal(dup, c.exp_dup), np.nonzero(dup != c.exp_dup)[0][:10]
    assert rate == c.exp_interdup and 0.0 < rate < 1.0
    assert _art_matches_log(int(art.sum()), len(dup), c.exp_art_perc), (int(art.sum()), len(dup), c.exp_art_perc)
    # what the plants are for, on the reference's flags: one survivor per group -- the first member, or the planted best copy (the last
    # member of groups 3 and 6, a copy in the middle of group 5) -- except where both mates share a group (group 1: the survivor's own
    # mate is a duplicate of it); no artifact at all where the best copy comes first and the tie never fires (group 4)
    surv = [np.nonzero(c.exp_dup[g] == 0)[0].tolist() for g in groups]
    assert [len(g) for g in groups] == [7, 63, 64, 65, 255, 256, 257]
    assert surv[0] == [0] and surv[1] == [] and surv[2] == [0] and surv[3] == [64] and surv[4] == [0] and surv[6] == [256]
    assert len(surv[5]) == 1 and 0 < surv[5][0] < 255
    assert art[groups[4]].sum() == 0 and all(art[g].sum() > len(g) // 2 for i, g in enumerate(groups) if i != 4)
    assert all(0 < art[g].sum() < dup[g].sum() for i, g in enumerate(groups) if i != 4)       # tied but not identical copies are not artifacts
    assert bc[2 * groups[0][0]] == 0 and bc[2 * groups[6][0]] == 0 and len(np.unique(bc[2 * groups[2]])) == 3
