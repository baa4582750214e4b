"""Time of snk_dev_edge_barcodes (the edge -> barcode lists, a.ebcx) on both of its sort paths, next to the paths index of the same run, on
the bench workload's reads and graph with the barcodes of the read model.  The reads are put in barcode order first (a stable sort on the
device: mates stay together), as DF has them, so that the edge-bits sort can run; the full-key sort is timed on the same reads with
SNK_EBC_GENERAL_SORT and on the reads in their native order.  HIP-event times of the library's own calls, the second of two calls each
(arena warm, like the timed step).

The two yardsticks: the paths index of the same run moves half the keys and has no distinct step; the reference's own host time is in
each fixture's ref_summary (tests/golden/ebcx/), at fixture size only.

usage: python tools/ebcx_probe.py [n_reads=1e8]"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from supernova_amd import synth  # noqa: E402
from supernova_amd.engine import Engine, Params  # noqa: E402


def timed(res, rows, read_len, quals, bc, mode):
    for _ in range(2):
        _, _, _, info = res.path_reads(rows, read_len, quals, bc=bc, download=False, paths_index=True, ebcx=mode)
    return info


def run(eng, name, sp):
    rows, quals, bc = eng.synth(sp)
    torch.cuda.synchronize()
    res = eng.count_graph(rows, sp.read_len, quals=quals, bc=bc, params=Params(K=48))
    native = timed(res, rows, sp.read_len, quals, bc, True)
    order = torch.argsort(bc, stable=True)
    rows, quals, bc = rows[order].contiguous(), quals[order].contiguous(), bc[order].contiguous()
    del order
    torch.cuda.synchronize()
    res = eng.count_graph(rows, sp.read_len, quals=quals, bc=bc, params=Params(K=48))
    fast = timed(res, rows, sp.read_len, quals, bc, True)
    general = timed(res, rows, sp.read_len, quals, bc, "general")
    f, g, v = fast["ebcx_stats"], general["ebcx_stats"], native["ebcx_stats"]
    assert (f["bc_sorted"], f["general_sort"], g["general_sort"]) == (1, 0, 1), (f, g)
    assert (f["n_keys"], f["n_ebc"], f["max_list"]) == (g["n_keys"], g["n_ebc"], g["max_list"]) == (v["n_keys"], v["n_ebc"], v["max_list"])
    out = {"workload": name, "reads": int(sp.n_reads), "hbv_edges": f["n_hbv_edges"], "path_entries": fast["pidx"]["n_entries"], "key_bits": f["key_bits"],
           "n_keys": f["n_keys"], "n_ebc": f["n_ebc"], "max_list": f["max_list"], "empty_edges": f["n_empty_edges"],
           "ebcx_edge_bits_sort_ms": round(f["ms"], 3), "ebcx_full_key_sort_ms": round(g["ms"], 3), "paths_index_ms": round(fast["pidx"]["ms"], 3),
           "native_order": {"bc_sorted": v["bc_sorted"], "general_sort": v["general_sort"], "ebcx_ms": round(v["ms"], 3),
                            "paths_index_ms": round(native["pidx"]["ms"], 3)}}
    print(json.dumps(out), flush=True)


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    eng = Engine(0)
    run(eng, "bench (0.2 % substitutions), reads in barcode order", synth.synth_params(n, seed=0x5EED0001))
    eng.close()


if __name__ == "__main__":
    main()
