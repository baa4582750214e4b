"""Time of snk_dev_paths_zip and snk_dev_paths_unzip next to the pathing, the paths index and MarkDups of the same run, on the bench
workload's reads and graph and on reads with 0.6 % errors (many edges, more steps per path).  HIP-event times of the library's own
calls, the second of two calls each (arena warm, like the timed step).  GB/s = bytes the zip call has to move once -- 16 B per read of
path arrays, 4 B per path entry, the scanned sizes and offsets (1 + 8 B per read written, then read), the output -- over its time.

usage: python tools/pathsx_probe.py [n_reads=1e8] [n_reads_err=2e7]"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from supernova_amd import graphio, synth  # noqa: E402
from supernova_amd.engine import Engine, Params  # noqa: E402


def run(eng, name, sp):
    rows, quals, bc = eng.synth(sp)
    torch.cuda.synchronize()
    res = eng.count_graph(rows, sp.read_len, quals=quals, bc=bc, params=Params(K=48))
    u = graphio.unitigs_to_arrays(res.unitigs())
    with graphio.hbv_handle(48, *u) as h:
        for _ in range(2):
            _, _, _, info = res.path_reads(rows, sp.read_len, quals, mark_dups=True, bc=bc, download=False, paths_index=True, pathsx=True)
            back, unzip_ms = eng.unzip_paths(h, info["pathsx_dev"], download=False)
        assert int(back.n_reads) == int(sp.n_reads) and int(back.n_edges_total) == info["pidx"]["n_entries"]
    p, d, x = info["pidx"], info["dups"], info["pathsx_stats"]
    n, ent = int(sp.n_reads), p["n_entries"]
    moved = 16 * n + 4 * ent + 2 * 9 * n + x["n_bytes"] + 8 * x["n_index"]
    out = {"workload": name, "reads": n, "hbv_edges": p["n_hbv_edges"], "path_entries": ent, "path_ms": round(info["path_ms"], 3),
           "paths_index_ms": round(p["ms"], 3), "mark_dups_ms": round(d["ms"], 3), "zip_ms": round(x["ms"], 3), "unzip_ms": round(unzip_ms, 3),
           "pathsx_bytes": x["n_bytes"], "bytes_per_read": round(x["n_bytes"] / n, 3), "zip_GBps": round(moved / x["ms"] / 1e6, 1) if x["ms"] > 0 else None,
           "empty": x["n_empty"], "steps_not_found": x["n_steps_not_found"], "offsets_wrapped": x["n_offsets_wrapped"]}
    print(json.dumps(out), flush=True)
    del rows, quals, bc
    torch.cuda.empty_cache()


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    n_err = int(float(sys.argv[2])) if len(sys.argv) > 2 else 20_000_000
    eng = Engine(0)
    run(eng, "bench (0.2 % substitutions)", synth.synth_params(n, seed=0x5EED0001))
    run(eng, "0.6 % substitutions", synth.synth_params(n_err, seed=0x5EED0C0D, sub_ppm=6000))
    eng.close()


if __name__ == "__main__":
    main()
