"""Randomised sweep of the path extension (snk_dev_extend_paths: ExtendPathsNew, 10X/Extend.cc:14-177) against its Python restatement
(tests/extref.py, pinned to the reference's own bytes by tests/test_extend_host.py): random genomes with the plants of tests/pathgen.py
(repeats, a tandem run, a palindrome, a long homopolymer, a short-period repeat), ragged read pairs of up to 256 bases with errors, a
device graph of drawn K and filters, the pather's own paths on it.  Per case, without and with SNK_EXT_BACK, over the first MAX_READS
reads: offsets, edge counts, edges and counters == extref.extend.  The call refuses its whole input for one read the reference would
compute from outside a read or an edge (an offset a ReadPathVecX cannot hold, given or made by the backward leg; a read that ends inside
the K-1 bases in front of its path): the reads the restatement refuses (extref.refused_reads) go in without their path, and a device
that refuses any other fails the case.  Test infrastructure, like tests/.
usage: python tests/tools/fuzz_extend.py [n_cases] [seed] [replay_case]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import tempfile
import numpy as np
import torch
import a48xref
import extref
import pathgen
from supernova_amd import graphio, lib as _lib
from supernova_amd.engine import Engine, Params

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 20
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 4321
only = int(sys.argv[3]) if len(sys.argv) > 3 else -1      # replay one case of a sweep
MAX_READS = 3000                                          # the restatement is plain Python
eng = Engine(0)


def draw_case(rng):
    return dict(K=48 if rng.random() < 0.6 else 60, L=int(rng.choice([100, 150, 151, 250, 256])), G=int(rng.choice([3000, 6000, 12000, 40000])),
                cov=float(rng.choice([8, 20, 40])), err=float(rng.choice([0.0, 0.002, 0.01, 0.03])), min_freq=int(rng.choice([1, 2, 3])),
                plants=bool(rng.random() < 0.8))


def run_case(c, codes, quals, lens, bc):
    """-> (mismatch lines, summary)"""
    K, L = c["K"], c["L"]
    rows, dq, dl, _ = pathgen.to_device(codes, quals, lens, bc)
    res = eng.count_graph(rows, L, quals=dq, lens=dl, params=Params(K=K, min_freq=c["min_freq"], min_bc=0))
    us = res.unitigs()
    off, ne, edges, _ = res.path_reads(rows, L, dq, lens=dl)
    u = graphio.unitigs_to_arrays(us)
    with tempfile.TemporaryDirectory() as td:
        graphio.write_hbv(Path(td) / "g.hbv", None, K, *u)
        g = a48xref.parse_hbv((Path(td) / "g.hbv").read_bytes())
    n = min(len(ne), MAX_READS)
    ne64, o = ne[:n].astype(np.int64), off[:n].astype(np.int64)
    eb = extref.edge_bases(g)
    drop = extref.refused_reads(g, codes[:n], lens[:n], quals[:n], o, ne64, edges[:int(ne64.sum())], eb)
    p = (np.where(drop, 0, o).astype(np.int32), np.where(drop, 0, ne64).astype(np.uint32), edges[:int(ne64.sum())][~np.repeat(drop, ne64)].astype(np.int32))
    dev = torch.device("cuda", 0)
    to_dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    bad, seen = [], {}
    with graphio.hbv_handle(K, *u) as h:
        d_u = (to_dev(u[0], np.int64), to_dev(u[1], np.uint8))
        for back in (False, True):
            try:
                want = extref.extend(g, codes[:n], lens[:n], quals[:n], *p, back, eb)
            except extref.Refused as ex:
                bad.append(f"back={back}: the restatement refuses the pather's own paths: {ex}")
                continue
            got = eng.extend_paths(K, h, *d_u, rows[:n], L, dq[:n], dl[:n], to_dev(p[0], np.int32), to_dev(p[1], np.int32), to_dev(p[2], np.int32), back=back)
            same = [np.array_equal(a, b) for a, b in zip(got[:3], want[:3])]
            cnt = {k: got[3][k] for k in want[3]}
            if not all(same) or cnt != want[3]:
                bad.append(f"back={back}: offsets / edge counts / edges {['equal' if x else 'differ' for x in same]}; counters {cnt} vs {want[3]}")
            seen = want[3]
    return bad, f"{len(us)} unitigs, {g.E} edges, {n} reads, {int(drop.sum())} without their path, " + " ".join(f"{k[2:]}={v}" for k, v in seen.items())


rng = np.random.default_rng(seed)
bad_cases = 0
for case in range(n_cases):
    c = draw_case(rng)
    gen, spots = pathgen.genome(rng, c["G"], plants=c["plants"])
    data = pathgen.pairs(rng, gen, max(8, int(c["G"] * c["cov"] / c["L"] / 2)), c["L"], c["err"], 8, spots, spot_frac=0.25)
    if only >= 0 and case != only:
        continue
    tag = f"case {case}: " + " ".join(f"{k}={v}" for k, v in c.items())
    try:
        bad, summary = run_case(c, *data)
    except _lib.SnkError as ex:
        bad, summary = [f"library error: {ex}"], ""
    if bad:
        bad_cases += 1
        print("FAIL " + tag, flush=True)
        for b in bad:
            print("     " + b, flush=True)
    else:
        print(f"ok   {tag} -> {summary}", flush=True)
print(f"{n_cases - bad_cases} of {n_cases} cases bit-exact")
sys.exit(1 if bad_cases else 0)
