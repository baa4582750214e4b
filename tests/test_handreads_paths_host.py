"""Read pathing and duplicate marking on reads walked over hand-made unitig sets (tests/handreads.py), host side: the generator still
makes the reads the fixtures were made from -- clean, noisy and the pather's own variant with its layer of substituted and chimeric
reads -- and the C oracle's restatements of pathReads and MarkDups give, on the case's unitigs, what the REFERENCE gave
(tests/golden/handreads/paths/, written by tests/golden/make_handreads_paths_golden.py): every read's offset, edge count and edges, every
pair's duplicate flag, the inter-barcode rate and the logged artifact share.  This is what entitles the K=60 device tests of
tests/test_gpu_handreads_paths.py, for which the reference has no pather, to use the oracle.  Every comparison is exact.  No GPU."""
import numpy as np
import pytest

import handreads as hr
import oracle_lib

K = 48
ALL = [(n, v) for n in hr.CASES for v in hr.VARIANTS]


def test_the_paths_variant_is_what_it_is_for():
    """(its conditions are asserted inside the generator; here: the clean reads are the case's, in their order, at qualities of 8..40, the
    layer lies among them in a barcode of its own, every kind is there, and the count is even)"""
    for name in hr.CASES:
        c, r = hr.reads(name, K, False), hr.reads(name, K, "paths")
        rows, layer = r.clean_rows, r.kind >= 0
        assert np.array_equal(r.codes[rows], c.codes) and np.array_equal(r.lens[rows], c.lens) and np.array_equal(r.bc[rows], c.bc)
        inside = np.arange(hr.L)[None, :] < r.lens[:, None]
        assert not layer[rows].any() and layer.sum() == r.facts["layer"]["n_layer_reads"] == len(r.lens) - len(c.lens)
        q = r.quals[rows][inside[rows]]
        assert q.min() >= 8 and q.max() <= 40 and len(np.unique(q)) > 1
        assert (r.bc[layer] == hr.LAYER_BC).all() and not (c.bc == hr.LAYER_BC).any() and (r.lens[layer] >= K + 1).all() and not r.quals[~inside].any()
        assert np.array_equal(r.kind[r.parent[layer]], np.full(int(layer.sum()), -1)) and (r.lens[r.parent[layer]] >= K + 1).all()
        kinds = r.facts["layer"]["kinds"]
        if (c.lens >= K + 1).any():
            assert len(r.lens) % 2 == 0 and r.quals[layer].max() <= 40 and r.quals[layer][inside[layer]].min() < 7
            assert all(kinds[k] > 0 for k in hr.KINDS if k != "sub2far") and (kinds["sub2far"] > 0) == bool((c.lens >= 2 * K + 10).any())
            assert kinds["chimera"] >= 8 or name == "single_k1"
        else:
            assert name in ("single_k", "single_pal_k") and not layer.any()
    assert sorted(p.name for p in hr.PATHS_GOLD.glob("*.npz")) == sorted(f"{n}_k{K}.npz" for n in hr.CASES if n not in hr.HASHED)


_unitigs: dict = {}


def case_unitigs(name):
    """the reference's unitigs of the case (those of all three variants: the maker asserts it) -- stored, or for the HASHED cases the
    oracle's, held to the stored digest"""
    if name not in _unitigs:
        g = hr.golden(name, K)
        if g.hashed:
            c = hr.reads(name, K, False)
            o = oracle_lib.OracleResult(c.codes, oracle_lib.good_lens(c.quals, c.lens, K=K, min_qual=7), c.bc, K=K, hbv=False)
            assert hr.sha(np.frombuffer("\n".join(o.unitigs).encode(), np.uint8)) == g.clean["unitigs"]
            _unitigs[name] = o.unitigs
        else:
            _unitigs[name] = bytes(g.clean["unitigs"]).decode().split("\n") if len(g.clean["unitigs"]) else []
    return _unitigs[name]


@pytest.mark.parametrize("name,noise", ALL, ids=[f"{n}-{hr.vname(v)}" for n, v in ALL])
def test_oracle_paths_and_dups_equal_the_reference(name, noise):
    r, exp = hr.load_paths(name, noise)
    assert exp.has_dups == (len(r.lens) % 2 == 0)
    off, n, edges = oracle_lib.path_reads(r.codes, r.quals, r.lens, case_unitigs(name), K=K)
    got = dict(path_off=off, path_n=n, path_edges=edges)
    if exp.has_dups:
        dup, art, rate, _, _ = oracle_lib.mark_dups(r.codes, r.quals, r.lens, off, n, edges, bc=r.bc)
        got.update(dup=dup, interdup=rate, n_art=int(art.sum()))
    assert hr.paths_differ(exp, got) is None, hr.paths_differ(exp, got)
