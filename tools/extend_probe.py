"""Time of snk_dev_extend_paths (StageExtension: ExtendPathsNew, 10X/Extend.cc:14-177) without and with SNK_EXT_BACK on the bench
workload's reads and graph, next to snk_dev_path_reads of the same run -- the yardstick: both go over every read once -- and the share of
reads that reach the enumeration of ExtendPath (the listed, slow pass).  HIP-event times of the library's own calls, the second of two
calls each (arena warm, like the timed step); the extension's time includes building the graph tables (what dict_ms counts for the
pather, without the dictionary).  The stage refuses an offset outside +-32767 -- its input in the reference is a ReadPathVecX -- so the
reads that lie beyond base 32767 of an edge (the bench genome's unitigs are long) go in without their path, and so do those in front of
a path whose first edge has an in-edge that long (the backward leg would move their offset there); both numbers are reported.

usage: python tools/extend_probe.py [n_reads=1e8]"""
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from supernova_amd import lib as _lib, synth  # noqa: E402
from supernova_amd.engine import Engine, Params, _extend_stats, dev_paths, dev_reads  # noqa: E402


def extend(eng, res, h, r, p, flags):
    """snk_dev_extend_paths on the result's own unitig arrays, the second of two calls -> stats"""
    for _ in range(2):
        x = _lib.SnkDevExtend()
        eng._call(eng.lib.snk_dev_extend_paths, int(res.K), C.byref(r), res.n_unitigs, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(p), flags, C.byref(x))
    return _extend_stats(x)


def run(eng, name, sp):
    rows, quals, bc = eng.synth(sp)
    torch.cuda.synchronize()
    res = eng.count_graph(rows, sp.read_len, quals=quals, bc=bc, params=Params(K=48))
    off, ne, edges, _ = res.path_reads(rows, sp.read_len, quals)
    _, _, _, info = res.path_reads(rows, sp.read_len, quals, download=False)          # (the yardstick: the second call, arena warm)
    n = int(sp.n_reads)
    dev = rows.device
    off_t, ne_t, edges_t = (torch.from_numpy(a.view(np.int32)).to(dev) for a in (off, ne, edges))
    del off, ne, edges
    # The stage refuses an offset a ReadPathVecX cannot hold (the reference would wrap it): reads beyond base 32767 of an edge go in
    # without their path, as a host would pass them.
    far = (ne_t > 0) & ((off_t < -32767) | (off_t > 32767))
    ne64 = ne_t.to(torch.int64)
    edges_t = edges_t[~torch.repeat_interleave(far, ne64)].contiguous()
    zero = torch.zeros((), dtype=torch.int32, device=dev)
    off_t, ne_t = torch.where(far, zero, off_t), torch.where(far, zero, ne_t)
    n_far = int(far.sum())
    del far, ne64
    r = dev_reads(rows, sp.read_len, quals)
    p, start = dev_paths(off_t, ne_t, edges_t)
    h = _lib.SnkHbv()
    ms = C.c_float(0)
    eng._call(eng.lib.snk_dev_hbv, int(res.K), res.n_unitigs, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(ms))
    n_hbv = int(h.n_edges)
    # ... and so does an offset that the backward leg would move there: a path at a negative offset whose first edge has an in-edge of more
    # than 32767 k-mers goes in without its path too (whether or not that in-edge would agree with the read: the call itself refuses what
    # this leaves).  Both flags are timed on the same input.
    U = int(res.n_unitigs)
    arr = lambda q, m: np.ctypeslib.as_array(q, shape=(m,)).copy()
    vl, vr, src = arr(h.v_left, n_hbv), arr(h.v_right, n_hbv), arr(h.src_unitig, n_hbv)
    order = arr(h.bvcomp_order, U) if h.bvcomp_order else np.arange(U)
    u_len = np.diff(res._dl(res.raw.unitig_off, (U + 1) * 8, np.uint64, (U + 1,)).astype(np.int64))
    kmers = u_len[order[src]] - (int(res.K) - 1)
    max_in = np.zeros(int(h.n_vertices), np.int64)
    np.maximum.at(max_in, vr, kmers)
    risky = torch.from_numpy(max_in[vl] > 32767).to(dev)
    first = edges_t[start[:-1].clamp(max=max(int(edges_t.shape[0]) - 1, 0))].to(torch.int64)
    far = (ne_t > 0) & (off_t < 0) & risky[first]
    n_far_back = int(far.sum())
    edges_t = edges_t[~torch.repeat_interleave(far, ne_t.to(torch.int64))].contiguous()
    off_t, ne_t = torch.where(far, zero, off_t), torch.where(far, zero, ne_t)
    del far, first
    p, start = dev_paths(off_t, ne_t, edges_t)
    try:
        torch.cuda.synchronize()
        plain = extend(eng, res, h, r, p, 0)
        back = extend(eng, res, h, r, p, _lib.EXT_BACK)
    finally:
        eng.lib.snk_hbv_free(C.byref(h))
    keys = ("n_back_extended", "n_cut_to_first", "n_quality_extended", "n_ambiguous", "n_too_many", "n_exact_extended", "n_enumerated", "n_edges_total")
    out = {"workload": name, "reads": n, "hbv_edges": n_hbv, "path_entries": int(p.n_edges_total), "reads_beyond_int16_offsets": n_far, "reads_in_front_of_a_long_in_edge": n_far_back,
           "path_reads_ms": round(info["path_ms"], 3), "path_dict_ms": round(info["dict_ms"], 3),
           "extend_ms": round(plain["ms"], 3), "extend_back_ms": round(back["ms"], 3), "enumerated_share": plain["n_enumerated"] / max(n, 1),
           "enumerated_share_back": back["n_enumerated"] / max(n, 1), "counters": {k: plain[k] for k in keys}, "counters_back": {k: back[k] for k in keys}}
    print(json.dumps(out), flush=True)


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    eng = Engine(0)
    run(eng, "bench (0.2 % substitutions)", synth.synth_params(n, seed=0x5EED0001))
    eng.close()


if __name__ == "__main__":
    main()
