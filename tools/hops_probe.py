"""Time of snk_dev_edge_pairs (FindEdgePairs, 10X/Closomatic.cc:17-354: the second step of StageFindPatch) on the bench workload's reads
and graph, next to the paths index, MarkBads and the pathing of the same run -- one res.path_reads(..., mark_dups, mark_bads="x",
hops=True, download=False) call, the second of two (arena warm, like the timed step).  HIP-event times of the library's own calls.
Printed per size: ms per part (tables_ms: graph tables and the checks of the paths; part12_ms; part3_ms: classify, closures, rights),
the pair counts, the shares of the edges that the K + 1 test, the two-class test and round 0 settle, the residual count and n_ext_host
at the default budget.

The sizes run in ascending order; a size is skipped when the one before it, scaled as if the time grew with the square of the reads,
would take more than a minute (the closure is one lane per residual edge: its time grows with the index entries of such an edge).

usage: python tools/hops_probe.py [n_reads ...] (default 2e6 2e7 1e8)"""
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
        _, _, _, info = res.path_reads(rows, sp.read_len, quals, mark_dups=True, bc=bc, mark_bads="x", hops=True, download=False)
    s = info["hops_stats"]
    E = info["pidx"]["n_hbv_edges"]
    share = lambda a: round(a / max(E, 1), 5)
    out = {"workload": name, "reads": int(sp.n_reads), "hbv_edges": E, "path_entries": info["n_edges_total"],
           "path_reads_ms": round(info["path_ms"], 3), "path_dict_ms": round(info["dict_ms"], 3), "mark_dups_ms": round(info["dups"]["ms"], 3),
           "mark_bads_ms": round(info["bads"]["ms"], 3), "paths_index_ms": round(info["pidx"]["ms"], 3),
           "hops_ms": round(s["ms"], 3), "tables_ms": round(s["tables_ms"], 3), "part12_ms": round(s["part12_ms"], 3), "part3_ms": round(s["part3_ms"], 3),
           "n_pairs": s["n_pairs"], "n_part1": s["n_part1"], "n_part2": s["n_part2"], "n_part3": s["n_part3"], "n_sink_edges": s["n_sink_edges"],
           "settled_by_K_plus_1": share(E - s["n_long_edges"]), "settled_by_two_class": share(s["n_long_edges"] - s["n_two_class"]),
           "settled_by_round0": share(s["n_ext_round0"]), "residual": s["n_ext_closure"] + s["n_not_extended"], "n_ext_closure": s["n_ext_closure"],
           "n_not_extended": s["n_not_extended"], "n_ext_host": s["n_ext_host"], "ext_budget": s["ext_budget"]}
    print(json.dumps(out), flush=True)
    return s["ms"]


def main():
    sizes = [int(float(a)) for a in sys.argv[1:]] or [2_000_000, 20_000_000, 100_000_000]
    eng = Engine(0)
    last = None
    for n in sizes:
        if last is not None and last[1] * (n / last[0]) ** 2 > 60000.0:
            print(json.dumps({"reads": n, "skipped": f"{last[1]:.1f} ms at {last[0]} reads"}), flush=True)
            break
        last = (n, run(eng, "bench (0.2 % substitutions)", synth.synth_params(n, seed=0x5EED0001, unbarcoded_ppm=0)))
    eng.close()


if __name__ == "__main__":
    main()
