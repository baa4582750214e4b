"""MarkBads on the device against the Python restatement (tests/badsref.py, pinned to the reference's flags by test_bads_host.py) on 200
seeded random cases.  A case: a graph of tests/handunitigs.py building blocks (two lone unitigs, a chain of edges with a side branch at
every junction; K = 48 and 60 in turn), 32 pairs of reads walked over it on either strand -- ragged lengths 1 .. 256, 0 - 12
substitutions (two reads in three have at most 3), qualities 0 - 60 -- and their paths, DISPLACED: a shifted offset, the first or last edge dropped, no path at all.  The
ReadPath overload also gets paths with an edge taken out of the middle (not adjacent any more: SNK_BADS_X refuses those, which is
asserted).  Generation is checked on the CPU, per case: both flag values must occur in both modes, so a constant answer cannot pass."""
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import a48xref
import badsref
import extref
import handbads
import handunitigs as hu

N_CASES, BLOCK, PAIRS, L = 200, 25, 32, 256


def make_case(seed: int):
    """-> namespace(K, unitigs, g, eb, codes, quals, lens, paths (adjacent steps only), paths_any (some with a middle edge out), want
    {(x, which): (bad, counters)})"""
    from supernova_amd import graphio
    K = (48, 60)[seed % 2]
    g = hu._Gen(f"badsfuzz/{seed}", K)
    rng = g.rng
    lone = [g.add(g.rand(K + int(rng.integers(60, 400)))) for _ in range(2)]
    n = int(rng.integers(3, 6))
    js = [g.junction() for _ in range(n)]
    chain, side = [g.add(g.rand(int(rng.integers(20, 120))) + js[0].seq)], []
    for i in range(n):
        b = g.rand(1)
        chain.append(g.add(js[i].seq + b + g.rand(int(rng.integers(1, 80))) + (js[i + 1].seq if i + 1 < n else "")))
        side.append(g.add(js[i].seq + handbads._other(b) + g.rand(int(rng.integers(5, 40)))))
    us = hu.bvcomp_sorted(g.unitigs)
    hu.check_valid(us, K)
    off, bases = hu.to_arrays(us)
    with tempfile.TemporaryDirectory() as td:
        graphio.write_hbv(Path(td) / "g.hbv", None, K, off, bases)
        G = a48xref.parse_hbv((Path(td) / "g.hbv").read_bytes())
    eb = extref.edge_bases(G)
    edge_of = handbads.edge_index(eb)

    def walk():
        k = int(rng.integers(0, 4))
        if k == 0:
            w = [lone[int(rng.integers(0, 2))]]
        elif k == 1:
            a = int(rng.integers(0, n))
            w = chain[a:int(rng.integers(a + 1, n + 2))]
        elif k == 2:
            a = int(rng.integers(0, n))
            w = chain[a:int(rng.integers(a + 1, n + 1))]
            w = w + [side[a + len(w) - 1]]
        else:
            w = chain[:]
        return [hu.rc(s) for s in reversed(w)] if rng.random() < 0.5 else w

    codes, quals, lens = np.zeros((2 * PAIRS, L), np.uint8), rng.integers(0, 61, (2 * PAIRS, L)).astype(np.uint8), np.zeros(2 * PAIRS, np.uint16)
    offs, paths, paths_any = [], [], []
    for r in range(2 * PAIRS):
        w = walk()
        m = handbads.cat(K, w)
        nb = int(rng.integers(1, L + 1)) if rng.random() < 0.3 else int(rng.integers(100, 151))
        p = int(rng.integers(-20, max(len(m) - nb // 2, 1)))
        read = rng.integers(0, 4, nb).astype(np.uint8)
        inside = [l for l in range(nb) if 0 <= p + l < len(m)]
        read[inside] = hu._CODE[np.frombuffer(m.encode(), np.uint8)][[p + l for l in inside]]
        for l in rng.integers(0, nb, int(rng.integers(0, 13 if rng.random() < 0.35 else 4))):
            read[l] = (read[l] + 1 + int(rng.integers(0, 3))) % 4
        codes[r, :nb], lens[r] = read, nb
        # ---- the path, displaced
        w_adj = list(w)
        if rng.random() < 0.3:
            p += int(rng.choice([-40, -7, -1, 1, 3, 16, 33]))
        if len(w_adj) >= 2 and rng.random() < 0.25:
            w_adj = w_adj[1:]
        if len(w_adj) >= 2 and rng.random() < 0.15:
            w_adj = w_adj[:-1]
        if rng.random() < 0.1:
            w_adj = []
        w_any = list(w_adj)
        if len(w_any) >= 3 and rng.random() < 0.5:
            del w_any[int(rng.integers(1, len(w_any) - 1))]
        offs.append(p if w_adj else 0)
        paths.append([edge_of[s] for s in w_adj])
        paths_any.append([edge_of[s] for s in w_any])
    pk = lambda ps: (np.asarray(offs, np.int32), np.asarray([len(x) for x in ps], np.uint32), np.asarray([e for x in ps for e in x], np.int32))
    c = SimpleNamespace(seed=seed, K=K, unitigs=us, g=G, eb=eb, codes=codes, quals=quals, lens=lens, paths=pk(paths), paths_any=pk(paths_any))
    c.want = {(False, "any"): badsref.mark_bads(G, eb, codes, lens, quals, *c.paths_any, False), (True, "adj"): badsref.mark_bads(G, eb, codes, lens, quals, *c.paths, True)}
    c.any_is_adjacent = bool(a48xref.all_steps_found(c.paths_any[1], c.paths_any[2], G).all())
    return c


def check_generation(c):
    for key, (bad, cnt) in c.want.items():
        assert 0 < bad.sum() < len(bad), (c.seed, key, int(bad.sum()))


def test_generation_yields_both_flag_values(snk):
    """no GPU: every seed gives at least one pair of each flag value in both modes, and over the seeds every kind of displacement occurs"""
    non_adjacent = unplaced = long_paths = short = 0
    for seed in range(0, N_CASES, 8):          # (every case is checked again where it runs; this keeps the CPU suite quick)
        c = make_case(seed)
        check_generation(c)
        non_adjacent += not c.any_is_adjacent
        unplaced += int((c.paths[1] == 0).sum())
        long_paths += int((c.paths[1] >= 3).sum())
        short += int((c.lens < 48).sum())
    assert min(non_adjacent, unplaced, long_paths, short) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("block", range(N_CASES // BLOCK))
def test_fuzz_against_the_restatement(snk, block):
    import torch
    from supernova_amd import graphio, lib as _lib
    from supernova_amd.engine import Engine
    import pathgen
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.array(a, dtype=dt))).to(torch.device("cuda", 0))
    try:
        for seed in range(block * BLOCK, (block + 1) * BLOCK):
            c = make_case(seed)
            check_generation(c)
            u = graphio.unitigs_to_arrays(c.unitigs)
            d_off, d_bases = dev(u[0].astype(np.int64), np.int64), dev(u[1], np.uint8)
            rows, dq, dl, _ = pathgen.to_device(c.codes, c.quals, c.lens, np.zeros(len(c.lens), np.int32))
            with graphio.hbv_handle(c.K, *u) as h:
                for (x, which), (want, cnt) in c.want.items():
                    off, ne, edges = c.paths if which == "adj" else c.paths_any
                    d_in = (dev(off, np.int32), dev(ne.view(np.int32), np.int32), dev(edges, np.int32))
                    bad, stats = e.mark_bads(c.K, h, d_off, d_bases, rows, L, dq, dl, *d_in, x=x)
                    assert np.array_equal(bad, want), (seed, x, np.nonzero(bad != want)[0][:5])
                    assert {k: stats[k] for k in cnt} == cnt, (seed, x, stats)
                if not c.any_is_adjacent:
                    off, ne, edges = c.paths_any
                    with pytest.raises(_lib.SnkError) as ei:
                        e.mark_bads(c.K, h, d_off, d_bases, rows, L, dq, dl, dev(off, np.int32), dev(ne.view(np.int32), np.int32), dev(edges, np.int32), x=True)
                    assert ei.value.code == -1
    finally:
        e.close()
