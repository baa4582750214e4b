"""Time of snk_dev_close_gaps (CloseGap2 / CloseGap, 10X/Closomatic.cc:356-657: the third step of StageFindPatch) on the bench workload's
reads and graph, for the pairs that snk_dev_edge_pairs gives in the same run, next to FindEdgePairs, MarkBads and the pathing of that
run -- res.path_reads(..., mark_dups, mark_bads="x", hops=True, closures=..., download=False), the second of two calls per flag (arena
warm, like the timed step).  HIP-event times of the library's own calls.  Printed per size and flag: ms per part (tables_ms: graph tables,
the checks of the paths and the pairs; gather_ms: rows, followers, placement; close_ms: offsets and closures) and the counters.

usage: python tools/closures_probe.py [n_reads ...] (default 2e6 2e7 1e8)"""
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
    for flag, arg in (("cg2", True), ("cg1", "cg1")):
        for _ in range(2):
            _, _, _, info = res.path_reads(rows, sp.read_len, quals, mark_dups=True, bc=bc, mark_bads="x", hops=True, closures=arg, download=False)
        s, hp = info["closures_stats"], info["hops_stats"]
        out = {"workload": name, "reads": int(sp.n_reads), "flag": flag, "hbv_edges": info["pidx"]["n_hbv_edges"], "path_reads_ms": round(info["path_ms"], 3),
               "mark_bads_ms": round(info["bads"]["ms"], 3), "paths_index_ms": round(info["pidx"]["ms"], 3), "hops_ms": round(hp["ms"], 3),
               "closures_ms": round(s["ms"], 3), "tables_ms": round(s["tables_ms"], 3), "gather_ms": round(s["gather_ms"], 3), "close_ms": round(s["close_ms"], 3)}
        out.update({k: s[k] for k in ("n_pairs", "n_closures", "n_bases", "n_pairs_0", "n_pairs_1", "n_pairs_2", "n_pairs_many", "n_rows", "n_partners_tried",
                                      "n_partners_placed", "n_followers", "n_cons_too_long", "n_place_host", "bod_budget", "max_width")})
        print(json.dumps(out), flush=True)


def main():
    sizes = [int(float(a)) for a in sys.argv[1:]] or [2_000_000, 20_000_000, 100_000_000]
    eng = Engine(0)
    for n in sizes:
        run(eng, "bench (0.2 % substitutions)", synth.synth_params(n, seed=0x5EED0001, unbarcoded_ppm=0))
    eng.close()


if __name__ == "__main__":
    main()
