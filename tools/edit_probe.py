"""Time of the graph edits (snk_dev_hanging_ends, snk_dev_delete_edges) on the graph and the read paths of the bench workload's reads,
next to the two calls of the same run that move the same path entries -- snk_dev_paths_index (a sort of them) and snk_dev_paths_zip --
the yardsticks.  Three edits: the hanging-end selection (StageTrim from line 91 on, 10X/runstages/RunStages.cc), the deletion of that
selection, and the deletion of a seeded, inv-closed 10 % of the edges.  HIP-event times of the library's own calls, the second of two
calls each (arena warm); graph_ms is the wall clock of the host's part inside delete_edges; wall_ms is the whole method, with the copies
it keeps.  One JSON line.

usage: python tools/edit_probe.py [n_reads=1e8]"""
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
        _, _, _, info = res.path_reads(rows, sp.read_len, quals, download=False, paths_index=True, pathsx=True)
    pidx_ms, zip_ms = info["pidx"]["ms"], info["pathsx_stats"]["ms"]
    off, ne, edges, _ = res.path_reads(rows, sp.read_len, quals)
    uoff, _ = res.unitig_arrays()
    U = len(uoff) - 1
    ub_t = torch.as_tensor(_DevBytes(res.raw.unitig_bases, int(uoff[-1])), device=dev).clone()
    h = _lib.SnkHbv()
    ms = C.c_float(0)
    err = C.create_string_buffer(512)
    rc = eng.lib.snk_dev_hbv(eng._ctx, K, U, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(ms), eng._stream(), err, 512)
    if rc:
        raise _lib.SnkError(rc, err.value.decode(errors="replace"))
    del rows, quals, bc
    try:
        E = int(h.n_edges)
        inv = np.zeros(max(E, 1), np.int32)
        _lib.call(eng.lib.snk_hbv_involution, C.byref(h), U, inv.ctypes.data)
        inv = inv[:E]
        paths = tuple(torch.from_numpy(a.view(np.int32)).to(dev) for a in (off, ne, edges))
        graph = (K, h, uoff, ub_t, inv)
        out = {"workload": "bench (0.2 % substitutions)", "reads": n, "path_entries": int(len(edges)), "unitigs": U, "hbv_edges": E,
               "paths_index_ms": round(pidx_ms, 3), "paths_zip_ms": round(zip_ms, 3)}
        for leg in (None, "sort"):
            for _ in range(2):
                support, hang, hs = eng.hanging_ends(graph, paths, leg=leg)
            out[f"hanging_ends_{hs['leg']}_ms"] = round(hs["ms"], 3)
        out.update(hang_dels=int(len(hang)), unsupported=hs["n_unsupported"])
        rng = np.random.default_rng(0xED17)
        low = np.flatnonzero(np.arange(E) <= inv)
        pick = rng.choice(low, max(1, len(low) // 10), replace=False)
        tenth = np.unique(np.concatenate([pick, inv[pick]])).astype(np.int32)
        for name, dels in (("hang", hang), ("tenth", tenth)):
            eng.delete_edges(graph, paths, dels)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = eng.delete_edges(graph, paths, dels)                                             # the second of two calls
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            s = r.stats
            out[f"delete_{name}"] = dict(dels=int(len(dels)), ms=round(s["ms"], 3), paths_ms=round(s["paths_ms"], 3), graph_ms=round(s["graph_ms"], 3), wall_ms=round(wall, 1),
                                         **{k: s[k] for k in ("n_edges", "n_unitigs", "n_runs", "n_absorbed", "max_run", "n_truncated", "n_emptied", "n_collapsed")})
            del r
        print(json.dumps(out), flush=True)
    finally:
        eng.lib.snk_hbv_free(C.byref(h))
    eng.close()


if __name__ == "__main__":
    main()
