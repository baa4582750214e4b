"""Count, prune and unitig pull on reads walked over hand-made unitig sets (tests/handreads.py), host side: the generator keeps its
promises and still makes the reads the fixtures were made from, and the C oracle -- the judge of the fuzz sweeps and of every GPU test
that has no fixture -- gives what the reference gave on them (tests/golden/handreads/, written by tests/golden/make_handreads_golden.py):
good lengths, keys, counts, pruned contexts, spectrum and unitigs, clean and with the noise layer.  Every comparison is exact.  No GPU."""
import numpy as np
import pytest

import handreads as hr
import oracle_lib

ALL = [(n, K) for n in hr.CASES for K in hr.KS]


@pytest.mark.parametrize("name,K", ALL)
def test_generator_keeps_its_conditions_and_makes_the_fixtures_reads(name, K):
    """(the conditions are asserted inside the generator; the facts say what each case and its noise layer are for)"""
    clean, _ = hr.load(name, K, False)
    noisy, _ = hr.load(name, K, True)
    f, nf = clean.facts, noisy.facts["noise"]
    assert f["n_reads"] == len(clean.lens) == f["n_clean_reads"] and noisy.facts["n_reads"] == f["n_reads"] + nf["n_noise_reads"]
    assert f["n_reachable"] + len(f["unreachable"]) == f["n_case_kmers"]
    assert (f["n_reachable"] == 0) == (name in ("single_k", "single_pal_k")) and (len(f["unreachable"]) > 0) == (
        name in ("single_k", "single_pal_k", "palindromes", "long") or name.startswith("mixed_seed"))
    assert int(clean.lens.max()) <= hr.L and (clean.quals[np.arange(hr.L)[None, :] < clean.lens[:, None]] == 30).all()
    assert clean.bc.min() >= 1 and (noisy.bc == 0).sum() == nf["unbarcoded"] > 0
    assert nf["one_barcode_branch"] == (1 if K == 48 and int(clean.lens.max()) >= K + 40 else 0) and int((noisy.bc == hr.N_BC + 1).sum()) == 4 * nf["one_barcode_branch"]
    if f["n_reachable"]:
        assert nf["substitutions"]["random"] >= 3 and nf["substitutions"]["end"] == 1 and nf["n_noise_kmers"] > 0
    if name in ("circle", "ring_2", "ring_3", "tiny_circles", "circles_5000") or name.startswith("mixed_seed"):
        assert nf["substitutions"]["circle"] == 1
    if name in ("single_pal_2k", "palindromes", "forest_257", "long", "turns", "tiny_circles") or name.startswith("mixed_seed"):
        assert nf["substitutions"]["palindrome"] == 1
    if name in ("circle", "ring_3", "hairpin_flanks", "bubble", "palindromes", "chain_1025", "turns", "tiny_circles", "circles_5000") or name.startswith("mixed_seed"):
        assert nf["substitutions"]["junction"] == 1


def test_the_new_unitig_sets_hold_what_they_are_for():
    for K in hr.KS:
        t = hr.unitig_set("tiny_circles", K)
        periods = sorted(len(u) - (K - 1) for u in t)
        assert periods == sorted([1, 2, 3, 2, 5, 7, K - 1, K, K + 1, 31, 32, 33, 255, 256, 257, 1000]) and all(u[:K - 1] == u[-(K - 1):] for u in t)
        at = next(u for u in t if u.startswith("ATAT"))
        assert all(hr.is_palindrome(at[p:p + K]) for p in range(2))
        c = hr.unitig_set("circles_5000", K)
        assert len(c) == 5000 and {len(u) - (K - 1) for u in c} == set(range(12, 41)) and all(u[:K - 1] == u[-(K - 1):] for u in c)
        u = hr.unitig_set("turns", K)
        assert sorted(len(s) for s in u if hr.is_palindrome(s) and len(s) > K) == [2 * (K - 1), 2 * K, 2 * (K + 1), 4 * K]
        assert sum(hr.is_palindrome(s) and len(s) == K for s in u) == 8         # the middle k-mer of every flanked turn
    assert set(hr.HASHED) < set(hr.CASES) and len(hr.CASES) == 23
    assert sorted(p.name for p in hr.GOLD.glob("*.npz")) == sorted(f"{n}_k{K}.npz" for n, K in ALL if n not in hr.HASHED)


def _oracle(r, K):
    gl = oracle_lib.good_lens(r.quals, r.lens, K=K, min_qual=7)
    o = oracle_lib.OracleResult(r.codes, gl, r.bc if K == 48 else None, K=K, hbv=False)
    return o, hr.normalised(K, gl, o.keys, o.counts, o.ctx, np.bincount(o.counts) if len(o.counts) else np.zeros(0, np.int64), o.unitigs)


@pytest.mark.parametrize("name,K", ALL)
def test_oracle_equals_the_reference(name, K):
    """K=60 runs without barcodes, as the reference's K=60 build has no barcode rule.  The noisy run must have unpruned context bits that
    the prune clears -- the noise layer is what gives the prune something to do on these graphs."""
    clean, exp = hr.load(name, K, False)
    o, got = _oracle(clean, K)
    assert hr.differs(exp, got) is None, hr.differs(exp, got)
    assert len(o.counts) == exp.n_kmers == clean.facts["n_reachable"]
    assert sum(len(u) - K + 1 for u in o.unitigs) == exp.n_kmers
    noisy, nexp = hr.load(name, K, True)
    no, ngot = _oracle(noisy, K)
    assert hr.differs(nexp, ngot) is None, hr.differs(nexp, ngot)
    for f in ("keys", "ctx", "unitigs"):
        assert np.array_equal(got[f], ngot[f]), f
    if clean.facts["n_reachable"]:
        assert (no.ctx_raw & ~no.ctx).any() and not (no.ctx & ~no.ctx_raw).any()


def test_chain_comes_back_as_one_unitig_and_the_long_unitig_whole():
    for K in hr.KS:
        assert len(hr.golden("chain_1025", K).unitig_lens) == 1
        assert 70000 in hr.golden("long", K).unitig_lens
        assert sum(hr.golden("forest_257", K).unitig_lens <= K + 5) > 200
