"""Time of snk_dev_paths_index next to snk_dev_mark_dups (the yardstick: one stable radix sort of one record per read) on the bench
workload's reads and graph (what bench.py's config.next_rows runs) and on reads with 0.6 % errors (many edges).  HIP-event times of the
library's own calls, the second of two calls each (arena warm, like the timed step).

usage: python tools/paths_index_probe.py [n_reads=1e8] [n_reads_err=2e7]"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from supernova_amd import synth  # noqa: E402
from supernova_amd.engine import Engine, Params  # noqa: E402


def run(eng, name, sp):
    rows, quals, bc = eng.synth(sp)
    torch.cuda.synchronize()
    res = eng.count_graph(rows, sp.read_len, quals=quals, bc=bc, params=Params(K=48))
    for _ in range(2):
        _, _, _, info = res.path_reads(rows, sp.read_len, quals, mark_dups=True, bc=bc, download=False, paths_index=True)
    p, d = info["pidx"], info["dups"]
    out = {"workload": name, "reads": int(sp.n_reads), "unitigs": res.n_unitigs, "hbv_edges": p["n_hbv_edges"], "key_bits": p["key_bits"],
           "path_entries": p["n_entries"], "empty_edges": p["n_empty_edges"], "path_ms": round(info["path_ms"], 3),
           "mark_dups_ms": round(d["ms"], 3), "paths_index_ms": round(p["ms"], 3), "ratio_index_over_dups": round(p["ms"] / d["ms"], 3) if d["ms"] > 0 else None}
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
