"""Time of MowLawn (snk_dev_mow_lawn) and of StageTrim as one call (Engine.stage_trim) on the graph, the read paths and the dup flags of
the bench workload's reads, next to the yardsticks of the same run: snk_dev_hanging_ends, snk_dev_paths_index, snk_dev_mark_bads
(SNK_BADS_X) and snk_dev_delete_edges with MowLawn's selection.  HIP-event times of the library's own calls, the second of two calls
each (arena warm); the phases of snk_dev_mow_lawn are its own stamps (candidates: wall clock of the host's part); stage_trim's total is
the wall clock of the whole method, with the copies it keeps, and the sum of its parts' own times.  One JSON line.

usage: python tools/mow_probe.py [n_reads=1e8]"""
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from supernova_amd import lib as _lib, synth  # noqa: E402
from supernova_amd.engine import Engine, Params, _DevBytes  # noqa: E402


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    K = 48
    eng = Engine(0)
    dev = torch.device("cuda", 0)
    sp = synth.synth_params(n, seed=0x5EED0001)
    rows, quals, bc = eng.synth(sp)
    torch.cuda.synchronize()
    res = eng.count_graph(rows, sp.read_len, quals=quals, bc=bc, params=Params(K=K))
    for _ in range(2):
        _, _, _, info = res.path_reads(rows, sp.read_len, quals, download=False, paths_index=True, mark_bads="x", mark_dups=True, bc=bc)
    pidx_ms, bads_ms, dups_ms = info["pidx"]["ms"], info["bads"]["ms"], info["dups"]["ms"]
    off, ne, edges, info = res.path_reads(rows, sp.read_len, quals, mark_dups=True, bc=bc)
    dup = info["dups"]["dup"]
    uoff, _ = res.unitig_arrays()
    U = len(uoff) - 1
    ub_t = torch.as_tensor(_DevBytes(res.raw.unitig_bases, int(uoff[-1])), device=dev).clone()
    h = _lib.SnkHbv()
    ms = C.c_float(0)
    err = C.create_string_buffer(512)
    rc = eng.lib.snk_dev_hbv(eng._ctx, K, U, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(ms), eng._stream(), err, 512)
    if rc:
        raise _lib.SnkError(rc, err.value.decode(errors="replace"))
    try:
        E = int(h.n_edges)
        inv = np.zeros(max(E, 1), np.int32)
        _lib.call(eng.lib.snk_hbv_involution, C.byref(h), U, inv.ctypes.data)
        inv = inv[:E]
        paths = tuple(torch.from_numpy(a.view(np.int32)).to(dev) for a in (off, ne, edges))
        d_dup = torch.from_numpy(dup).to(dev)
        graph = (K, h, uoff, ub_t, inv)
        reads = (rows, sp.read_len, quals, None)
        out = {"workload": "bench (0.2 % substitutions)", "reads": n, "path_entries": int(len(edges)), "unitigs": U, "hbv_edges": E, "dup_pairs": int(dup.sum()),
               "yardsticks_ms": {"paths_index": round(pidx_ms, 3), "mark_bads_x": round(bads_ms, 3), "mark_dups": round(dups_ms, 3)}}
        for _ in range(2):
            _, hang, hs = eng.hanging_ends(graph, paths)
        out["yardsticks_ms"]["hanging_ends"] = round(hs["ms"], 3)
        for _ in range(2):
            dels, scored, st = eng.mow_lawn(graph, *reads, paths, d_dup)
        out["mow_lawn"] = dict(ms=round(st["ms"], 3), tables_ms=round(st["tables_ms"], 3), phase_ms={k: round(v, 3) for k, v in st["phase_ms"].items()},
                               n_dels=st["n_dels"], n_scored=st["n_scored"], **{k: st[k] for k in _lib.MOW_COUNTERS})
        for _ in range(2):
            r = eng.delete_edges(graph, paths, dels)
        out["yardsticks_ms"]["delete_edges_mow_dels"] = round(r.stats["ms"], 3)
        del r
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr = eng.stage_trim(graph, *reads, bc, paths)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
        s = tr.stats
        assert np.array_equal(tr.mow_dels, dels)
        out["stage_trim"] = dict(wall_ms=round(wall, 1), parts_ms=round(s["dups"]["ms"] + s["mow"]["ms"] + s["first"]["ms"] + s["hang_ms"] + s["ms"], 3),
                                 mark_dups_ms=round(s["dups"]["ms"], 3), mow_ms=round(s["mow"]["ms"], 3), first_delete_ms=round(s["first"]["ms"], 3),
                                 hanging_ends_ms=round(s["hang_ms"], 3), second_delete_ms=round(s["ms"], 3), mow_dels=s["mow_dels"], hang_dels=s["hang_dels"],
                                 n_edges=s["n_edges"], n_unitigs=s["n_unitigs"])
        print(json.dumps(out), flush=True)
    finally:
        eng.lib.snk_hbv_free(C.byref(h))
    eng.close()


if __name__ == "__main__":
    main()
