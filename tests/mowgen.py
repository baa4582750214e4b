"""Seeded inputs for MowLawn (snk_dev_mow_lawn; 10X/Lawnmower.cc:301-554) -- test infrastructure (tests/golden/make_mow_golden.py,
tests/test_mow_host.py, tests/test_gpu_mow.py, tests/test_gpu_mow_fuzz.py).  numpy and Python only.

    fuzz(seed, K=48)     a graph of bubbles-with-tips (tests/handmow.py's motif: a junction with the two in-edges e1 and e2 and one
                         out-edge) with reads walked over e1.f and e2.f on both strands, with substitutions at seeded qualities, ragged
                         lengths, some pairs that repeat another pair's placement and mate head (duplicates), some reads with many
                         high-quality mismatches (the filter), some e2 with three or more reads (the read limit)
    inputs(name, a_hbv)  the input of a fixture by its name: hand_k48 / hand_k60 / wide_k48 (tests/handmow.py), fuzz_<seed>, or one of
                         the five K = 48 golden graphs on its own paths (extref.golden_input).  a_hbv: the fixture's graph where it
                         holds one (None: it is made again here)
    dup_of(c)            MarkDups as the project restates it (oracle_lib.mark_dups) on the same input
"""
from __future__ import annotations

import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import a48ref
import a48xref
import extref
import handmow

FUZZ_SEEDS = tuple(range(1, 13))          # the seeds pinned to the reference under tests/golden/mow/
GOLDEN = ("synth_2k_err", "synth_6k_clean", "synth_20k_err", "adversarial", "synth_4k_dups")          # = goldens.CASES
HAND = {"hand_k48": 48, "hand_k60": 60}
WIDE = "wide_k48"
_made: dict = {}


def fuzz(seed: int, K: int = 48, n_motifs: int = 24):
    k = ("fuzz", seed, K, n_motifs)
    if k in _made:
        return _made[k]
    M = handmow._Maker(f"mowfuzz{seed}", K)
    rng = np.random.default_rng(0x4D4F57 + seed)
    for i in range(n_motifs):
        snp = bool(rng.integers(0, 3))
        n = int(rng.integers(1, K + 1)) if snp else int(rng.integers(1, 120))
        dl = int(rng.integers(0, 150)) if rng.integers(0, 4) else 0
        e1, e2, f, _ = M.motif(n, dl, tail=int(rng.integers(10, 60)), snp=snp)
        heads = []
        w0 = dl                                                          # the window starts at base dl of e1
        for j in range(int(rng.integers(0, 14))):                        # reads over e1.f
            length = int(rng.integers(40, 151))
            o = int(rng.integers(max(w0 - length + 1, -10), w0 + n))
            rep = bool(heads) and rng.integers(0, 6) == 0                    # the same placement and mate head as an earlier pair
            if rep:
                o, length, head = heads[int(rng.integers(0, len(heads)))]
            nm = int(rng.choice([0, 0, 0, 1, 2, 6]))
            mism = tuple((int(p), int(rng.choice([10, 29, 30, 41]))) for p in rng.choice(length, nm, replace=False))
            quals = tuple((int(p), int(rng.integers(2, 64))) for p in rng.choice(length, 8, replace=False) if p not in {m[0] for m in mism})
            h = M.read([e1, f], o, length, quals=quals, mism=mism, head=head if rep else None, rc=bool(rng.integers(0, 2)), qfill=int(rng.choice([20, 30, 40])))
            heads.append((o, length, h))
        for j in range(int(rng.choice([0, 0, 1, 1, 2, 2, 3, 4]))):      # reads over e2.f
            length = int(rng.integers(40, 151))
            o = int(rng.integers(-30, n))
            M.read([e2, f], o, length, quals=tuple((int(p), int(rng.integers(2, 64))) for p in rng.choice(length, 6, replace=False)),
                   mism=((int(rng.integers(0, length)), 35),) if rng.integers(0, 4) == 0 else (), rc=bool(rng.integers(0, 2)), qfill=int(rng.choice([15, 30, 45])))
        M.state(f"m{i}", e1, e2, None)
    _made[k] = handmow._finish(M, f"fuzz_{seed}")
    return _made[k]


def _from_hand(h, a_hbv):
    from supernova_amd import graphio
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        graphio.write_hbv(td / "g.hbv", td / "g.inv", h.K, h.off, h.bases)
        made, inv = (td / "g.hbv").read_bytes(), a48ref.parse_inv((td / "g.inv").read_bytes())
    assert a_hbv is None or a_hbv == made, f"{h.name}: the fixture's graph is not the one the generator makes now"
    g = a48xref.parse_hbv(made)
    eb = extref.edge_bases(g)
    edge_of = handmow.edge_index(eb)
    codes, quals, lens, paths = handmow.arrays(h, edge_of)
    return SimpleNamespace(K=h.K, g=g, eb=eb, inv=np.asarray(inv, np.int32), a_hbv=made, unitigs=h.unitigs, codes=codes, quals=quals, lens=lens, bc=h.bc, paths=paths,
                           motifs=h.motifs, edge_of=edge_of)


def inputs(name: str, a_hbv: bytes | None = None):
    if name in HAND:
        return _from_hand(handmow.case(HAND[name]), a_hbv)
    if name == WIDE:
        return _from_hand(handmow.wide(48), a_hbv)
    if name.startswith("fuzz_"):
        return _from_hand(fuzz(int(name[5:])), a_hbv)
    assert name in GOLDEN, name
    import goldens
    gc = goldens.load(name)
    g = a48xref.parse_hbv(gc.exp_ahbv)
    paths = extref.golden_input(a48xref.parse_paths(a48ref.load(name)["tmp.paths"]))
    n = len(paths[1])
    return SimpleNamespace(K=g.K, g=g, eb=extref.edge_bases(g), inv=np.asarray(a48ref.parse_inv(bytes(gc.exp_ainv)), np.int32), a_hbv=bytes(gc.exp_ahbv), unitigs=gc.exp_unitigs,
                           codes=gc.codes[:n], quals=gc.quals[:n], lens=gc.lens[:n], bc=np.asarray(gc.bc[:n], np.int32), paths=paths, motifs=None, edge_of=None)


def dup_of(c) -> np.ndarray:
    import oracle_lib
    return oracle_lib.mark_dups(c.codes, c.quals, c.lens, c.paths[0], np.asarray(c.paths[1], np.int64), c.paths[2], bc=c.bc)[0]
