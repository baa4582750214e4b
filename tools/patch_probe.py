"""Time of every step of Engine.insert_patch (StageInsertPatch, 10X/runstages/RunStages.cc:176-230) on the graph and the read paths of
the bench workload's reads, next to snk_dev_count_graph of the same run -- the yardstick: the patch step counts the graph's own k-mers
once more.  The closures are generated: bridges from the end of one unitig over a random gap of 0-60 bases to the start of another.
HIP-event times of the library's own calls (count_ms: the count stage's own total on the pieces); wall_ms is the whole method, with
the copies it keeps.  One JSON line.

usage: python tools/patch_probe.py [n_reads=1e7] [n_closures=1000]"""
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
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    n_cl = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    K = 48
    eng = Engine(0)
    dev = torch.device("cuda", 0)
    sp = synth.synth_params(n, seed=0x5EED0001)
    rows, quals, bc = eng.synth(sp)
    torch.cuda.synchronize()
    eng.count_graph(rows, sp.read_len, quals=quals, bc=bc, params=Params(K=K))
    res = eng.count_graph(rows, sp.read_len, quals=quals, bc=bc, params=Params(K=K))             # (the yardstick: the second call, arena warm)
    count_total_ms = res.phase_ms["total"]
    off, ne, edges, _ = res.path_reads(rows, sp.read_len, quals)
    uoff, ubases = res.unitig_arrays()
    U = len(uoff) - 1
    ub_t = torch.as_tensor(_DevBytes(res.raw.unitig_bases, int(uoff[-1])), device=dev).clone()
    h = _lib.SnkHbv()
    ms = C.c_float(0)
    err = C.create_string_buffer(512)
    rc = eng.lib.snk_dev_hbv(eng._ctx, K, U, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(ms), eng._stream(), err, 512)
    if rc:
        raise _lib.SnkError(rc, err.value.decode(errors="replace"))
    rng = np.random.default_rng(0xC105)
    seqs = []
    for _ in range(n_cl):
        a, b = (int(x) for x in rng.integers(0, U, 2))
        gap = rng.integers(0, 4, int(rng.integers(0, 61)), dtype=np.uint8)
        seqs.append(np.concatenate([ubases[int(uoff[a + 1]) - K:int(uoff[a + 1])], gap, ubases[int(uoff[b]):int(uoff[b]) + K]]))
    coff = np.zeros(n_cl + 1, np.uint64)
    coff[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    cb = np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)
    paths = tuple(torch.from_numpy(a.view(np.int32)).to(dev) for a in (off, ne, edges))
    try:
        eng.insert_patch((K, h, uoff, ub_t), (coff, cb), paths).close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.insert_patch((K, h, uoff, ub_t), (coff, cb), paths)                            # the second of two calls
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    finally:
        eng.lib.snk_hbv_free(C.byref(h))
    s = out.stats
    print(json.dumps({"workload": "bench (0.2 % substitutions)", "reads": n, "closures": n_cl, "old_unitigs": U, "old_hbv_edges": int(len(out.left3)),
                      "new_unitigs": int(out.unitig_off.shape[0]) - 1, "new_hbv_edges": int(len(out.inv)), "count_graph_of_the_reads_ms": round(count_total_ms, 3),
                      **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in s.items()}, "wall_ms": round(wall, 1)}), flush=True)
    out.close()
    eng.close()


if __name__ == "__main__":
    main()
