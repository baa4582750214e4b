"""FindEdgePairs on the device against the Python restatement (tests/hopsref.py, pinned to the reference's pairs by test_hops_host.py)
on 200 seeded random cases.  A case: a graph of tests/handunitigs.py building blocks (two lone unitigs, a chain of edges with dead-ended
side edges of 1 .. 140 k-mers leaving and entering every junction -- so stubs, landings and rights fall on either side of 40, 100 and
120; K = 48 and 60 in turn), 48 pairs of reads whose paths are random walks of 1 .. 4 edges over it on either strand (some without a
path), barcodes 0 .. 3, one pair in five flagged bad.  Both flag settings, the index made inside the call, every closure also on the
host leg and at a budget of 2 sequences (where the device hands over the edges whose set needs a third).  Generation is checked on the CPU over the seeds: every part gives pairs and every way part 3 settles an edge occurs, so a
constant answer cannot pass."""
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import a48xref
import extref
import handunitigs as hu
import hopsref

N_CASES, BLOCK, PAIRS = 200, 25, 48


def make_case(seed: int):
    """-> namespace(seed, K, unitigs, g, km, inv, paths, bc, bad, want {one_good: (pairs, info)})"""
    from supernova_amd import graphio
    K = (48, 60)[seed % 2]
    g = hu._Gen(f"hopsfuzz/{seed}", K)
    rng = g.rng
    for _ in range(2):
        g.add(g.rand(K + int(rng.integers(0, 200))))
    n = int(rng.integers(2, 6))
    js = [g.junction() for _ in range(n)]
    side = lambda: int(rng.choice([1, 20, 39, 40, 60, 99, 100, 120, 121, 140])) if rng.random() < 0.6 else int(rng.integers(1, 141))
    arrives = None                       # the base in front of the junction on the chain edge that enters it
    for i in range(n):
        outs, ins = list("ACGT"), [b for b in "ACGT" if b != arrives]
        rng.shuffle(outs)
        rng.shuffle(ins)
        if i + 1 < n:
            s = g.add(js[i].seq + outs.pop() + g.rand(int(rng.integers(1, 70))) + js[i + 1].seq)
            arrives = s[-K]
        for _ in range(int(rng.integers(1, 3))):
            g.add(js[i].seq + outs.pop() + g.rand(side() - 1))
        if rng.random() < 0.6:
            g.add(g.rand(side() - 1) + ins.pop() + js[i].seq)
    us = hu.bvcomp_sorted(sorted({min(s, hu.rc(s)) for s in g.unitigs}))
    try:
        hu.check_valid(us, K)
    except AssertionError:
        return None                      # (two edges into a junction drew the same base: the seed is skipped, and counted)
    off, bases = hu.to_arrays(us)
    with tempfile.TemporaryDirectory() as td:
        graphio.write_hbv(Path(td) / "g.hbv", Path(td) / "g.inv", K, off, bases)
        G = a48xref.parse_hbv((Path(td) / "g.hbv").read_bytes())
        inv = hopsref.involution((Path(td) / "g.inv").read_bytes())
    km = hopsref.kmers_of(G, extref.edge_bases(G))
    if np.diff(G.from_off).max() > 4:
        return None

    def walk():
        if rng.random() < 0.08:
            return []
        e = int(rng.integers(0, G.E))
        w = [e]
        while len(w) < 4 and rng.random() < 0.6:
            v = G.v_right[w[-1]]
            nxt = G.from_e[G.from_off[v]:G.from_off[v + 1]]
            if not len(nxt):
                break
            w.append(int(rng.choice(nxt)))
        return [int(inv[e]) for e in reversed(w)] if rng.random() < 0.5 else w

    popular = [walk() for _ in range(6)]
    pick = lambda: popular[int(rng.integers(0, 6))] if rng.random() < 0.7 else walk()
    paths = [pick() for _ in range(2 * PAIRS)]
    bc = np.repeat(rng.integers(0, 4, PAIRS), 2).astype(np.int32)
    bad = (rng.random(PAIRS) < 0.2).astype(np.uint8)
    pk = (np.zeros(2 * PAIRS, np.int32), np.asarray([len(x) for x in paths], np.uint32), np.asarray([e for x in paths for e in x], np.int32))
    c = SimpleNamespace(seed=seed, K=K, unitigs=us, g=G, km=km, inv=inv, paths=pk, bc=bc, bad=bad)
    c.how = {}
    c.want = {og: hopsref.find_edge_pairs(G, km, inv, pk[1], pk[2], bc, bad, og, c.how if not og else None) for og in (False, True)}
    return c


def test_generation_reaches_every_part(snk):
    """no GPU: over a sample of the seeds every part gives pairs, ONE_GOOD matters, part 3 settles edges in all three ways, and few seeds
    are skipped"""
    parts, how, differ, made = np.zeros(3, np.int64), set(), 0, 0
    for seed in range(0, N_CASES, 5):          # (every case is made again where it runs; this keeps the CPU suite quick)
        c = make_case(seed)
        if c is None:
            continue
        made += 1
        parts += [len(p) for p in c.want[False][1]["parts"]]
        how |= set(c.how.values())
        differ += not np.array_equal(c.want[False][0], c.want[True][0])
    assert made >= 30 and (parts >= 3).all() and how == {"round0", "closure", "not_extended"} and differ >= 3, (made, parts, how, differ)


@pytest.mark.gpu
@pytest.mark.parametrize("block", range(N_CASES // BLOCK))
def test_fuzz_against_the_restatement(snk, block):
    import torch
    from supernova_amd import graphio
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.array(a, dtype=dt))).to(torch.device("cuda", 0))
    made = handed = 0
    try:
        for seed in range(block * BLOCK, (block + 1) * BLOCK):
            c = make_case(seed)
            if c is None:
                continue
            made += 1
            u = graphio.unitigs_to_arrays(c.unitigs)
            d_off, d_bases = dev(u[0].astype(np.int64), np.int64), dev(u[1], np.uint8)
            off, ne, edges = c.paths
            d_in = (dev(off, np.int32), dev(ne.view(np.int32), np.int32), dev(edges if len(edges) else np.zeros(1, np.int32), np.int32)[:len(edges)])
            d_bc, d_bad = dev(c.bc, np.int32), dev(c.bad, np.uint8)
            with graphio.hbv_handle(c.K, *u) as h:
                for og, (want, info) in c.want.items():
                    for ext_host in (False, True):
                        pairs, stats = e.edge_pairs(c.K, h, d_off, d_bases, c.inv, *d_in, d_bc, d_bad, one_good=og, ext_host=ext_host)
                        assert np.array_equal(pairs, want), (seed, og, ext_host, len(pairs), len(want))
                        assert {k: stats[k] for k in hopsref.COUNTERS} == {k: info[k] for k in hopsref.COUNTERS}, (seed, og, ext_host, stats)
                        assert stats["n_ext_host"] == (stats["n_ext_closure"] + stats["n_not_extended"] if ext_host else 0), (seed, stats)
                    pairs, stats = e.edge_pairs(c.K, h, d_off, d_bases, c.inv, *d_in, d_bc, d_bad, one_good=og, ext_budget=2)
                    assert np.array_equal(pairs, want), (seed, og, "budget 2", len(pairs), len(want))
                    assert {k: stats[k] for k in hopsref.COUNTERS} == {k: info[k] for k in hopsref.COUNTERS} and stats["ext_budget"] == 2, (seed, og, stats)
                    handed += stats["n_ext_host"]
    finally:
        e.close()
    assert made >= BLOCK - 5 and handed >= 1, (made, handed)
