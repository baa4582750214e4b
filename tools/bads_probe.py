"""Time of snk_dev_mark_bads (MarkBads, 10X/SecretOps.cc:22-59, :70-107: the first step of StageFindPatch) on the bench workload's
reads and graph, both flags, and of snk_dev_mark_bads_df on the same reads written as reads.fastb / reads.qualp -- next to
snk_dev_mark_dups and snk_dev_path_reads of the same run, the yardsticks: all of them go over every read once.  HIP-event times of the
library's own calls, the second of two calls each (arena warm, like the timed step).  ms of the resident form spans the graph tables and
the checks of the paths (tables_ms: what dict_ms counts for the pather, without the dictionary) and the comparison kernel (kernel_ms,
the number to hold against the pather's pass); the _df form's is the host's clock over the whole call, file reads and decode included.

On the bench graph most reads lie beyond base 32767 of an edge, so with SNK_BADS_X most offsets wrap: a wrapped offset that is
negative puts the whole read in front of m (nothing compared), a positive one compares it where it does not lie (the mismatch path on
almost every word).  n_offsets_wrapped and the share of placed reads with a mismatch are printed for both flags.

usage: python tools/bads_probe.py [n_reads=1e8] [scratch dir for the triple]"""
import ctypes as C
import json
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from supernova_amd import dfin, lib as _lib, synth  # noqa: E402
from supernova_amd.engine import Engine, Params, _bads_stats, dev_paths, dev_reads  # noqa: E402


def twice(call):
    """the second of two calls -> stats"""
    for _ in range(2):
        b = _lib.SnkDevBads()
        call(b)
    return _bads_stats(b)


def run(eng, name, sp, scratch):
    rows, quals, bc = eng.synth(sp)
    torch.cuda.synchronize()
    res = eng.count_graph(rows, sp.read_len, quals=quals, bc=bc, params=Params(K=48))
    off, ne, edges, _ = res.path_reads(rows, sp.read_len, quals)
    _, _, _, info = res.path_reads(rows, sp.read_len, quals, mark_dups=True, bc=bc, download=False)          # (the yardsticks: the second call, arena warm)
    n = int(sp.n_reads)
    dev = rows.device
    off_t, ne_t, edges_t = (torch.from_numpy(a.view(np.int32)).to(dev) for a in (off, ne, edges))
    del off, ne, edges
    r = dev_reads(rows, sp.read_len, quals)
    p, start = dev_paths(off_t, ne_t, edges_t)          # (start: the struct points into it)
    h = _lib.SnkHbv()
    ms = C.c_float(0)
    eng._call(eng.lib.snk_dev_hbv, int(res.K), res.n_unitigs, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(ms))
    graph = (res.n_unitigs, res.raw.unitig_off, res.raw.unitig_bases, C.byref(h), C.byref(p))
    try:
        torch.cuda.synchronize()
        got = {}
        for tag, flags in (("plain", 0), ("x", _lib.BADS_X)):
            got[tag] = twice(lambda b: eng._call(eng.lib.snk_dev_mark_bads, int(res.K), C.byref(r), *graph, flags, C.byref(b)))
        t0 = time.time()
        dfin.write_synth_df(Path(scratch) / "reads", sp)
        write_s = time.time() - t0
        with dfin.DfFiles(Path(scratch) / "reads") as files:
            for tag, flags in (("df_plain", 0), ("df_x", _lib.BADS_X)):
                got[tag] = twice(lambda b: _lib.call(eng.lib.snk_dev_mark_bads_df, eng._ctx, int(res.K), files._h, 0, n, 0, 0, 0, *graph, flags, C.byref(b)))
            file_bytes = files.file_bytes
    finally:
        eng.lib.snk_hbv_free(C.byref(h))
    same = all(got["df_" + t][k] == got[t][k] for t in ("plain", "x") for k in ("n_placed", "n_mismatch_reads", "n_bad_reads", "n_bad_pairs", "n_offsets_wrapped"))
    out = {"workload": name, "reads": n, "path_entries": int(p.n_edges_total),
           "path_reads_ms": round(info["path_ms"], 3), "path_dict_ms": round(info["dict_ms"], 3), "mark_dups_ms": round(info["dups"]["ms"], 3),
           "triple_bytes": file_bytes, "triple_write_s": round(write_s, 1), "df_counters_equal_resident": same}
    for tag, s in got.items():
        out[tag] = {"ms": round(s["ms"], 3), "tables_ms": round(s["tables_ms"], 3), "kernel_ms": round(s["kernel_ms"], 3), "n_slabs": s["n_slabs"],
                    "mismatch_share": round(s["n_mismatch_reads"] / max(s["n_placed"], 1), 5), "n_placed": s["n_placed"], "n_mismatch_reads": s["n_mismatch_reads"],
                    "n_bad_reads": s["n_bad_reads"], "n_bad_pairs": s["n_bad_pairs"], "n_offsets_wrapped": s["n_offsets_wrapped"]}
    k_ms = got["plain"]["kernel_ms"]
    out["note"] = (f"resident kernel {k_ms:.2f} ms against the pather's pass {info['path_ms']:.2f} ms and MarkDups {info['dups']['ms']:.2f} ms; "
                   + ("below the pather's pass" if k_ms < info["path_ms"] else f"NOT below the pather's pass: tables {got['plain']['tables_ms']:.2f} ms are outside it, the rest is the kernel"))
    print(json.dumps(out), flush=True)


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    eng = Engine(0)
    with tempfile.TemporaryDirectory(dir=sys.argv[2] if len(sys.argv) > 2 else None) as td:
        run(eng, "bench (0.2 % substitutions)", synth.synth_params(n, seed=0x5EED0001, unbarcoded_ppm=0), td)          # (the .bci index needs every read barcoded)
    eng.close()


if __name__ == "__main__":
    main()
