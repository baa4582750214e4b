"""The graph verifier (snk_dev_check_graph) on a synthetic job made on the device the way tools/r6_full_job.py makes it: reads generated
slab by slab, trimmed and kept in compact form (packed rows + good lengths + barcode ids), one count + graph call, then the check --
graph level always, reads level when its 5 B per entry fit next to the job.  Prints one JSON row: the report, the verifier's ms per
level and its peak scratch bytes.
--plant: the check runs on a copy whose last 87 % of unitig bases are overwritten with base 0 (the round-6 bug of DESIGN 4, restaged);
the row must show unitig_kmer_missing and kmer_uncovered.
usage: python tools/check_job.py [reads=1e8] [K=48] [grouped=0] [plan_mem_mb=0] [--plant] [--no-reads]"""
import json
import os
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from supernova_amd import lib as _lib  # noqa: E402
from supernova_amd import synth  # noqa: E402
from supernova_amd.engine import Engine, Params  # noqa: E402


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    plant, no_reads = "--plant" in sys.argv, "--no-reads" in sys.argv
    n = int(float(argv[0])) if argv else 100_000_000
    K = int(argv[1]) if len(argv) > 1 else 48
    grouped = len(argv) > 2 and argv[2] == "1"
    plan_mb = int(argv[3]) if len(argv) > 3 else 0
    e = Engine(0)
    if plan_mb:
        e.set_option("plan_mem_mb", plan_mb)
    dev = torch.device("cuda", 0)
    sp = synth.synth_params(n, seed=0x5EED0C30)
    long_min = int(sp.genome_len) >= 1_500_000_000
    slab = 50_000_000
    rows = torch.empty((n, 10), dtype=torch.int32, device=dev)
    gl = torch.empty((n,), dtype=torch.int16, device=dev)
    bc = torch.empty((n,), dtype=torch.int32, device=dev)
    for first in range(0, n, slab):
        m = min(slab, n - first)
        r, q, b = e.synth(sp, first, m)
        rows[first:first + m] = r
        gl[first:first + m] = e.trim(q, 150, K=K)
        bc[first:first + m] = b
        del r, q, b
    group = None
    if grouped:      # per-barcode graphs: the group of a read is its barcode id
        group = bc.clone()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    params = (Params(K=K, sorted_table=False, grouped=True, min_bc=0) if grouped
              else Params(K=K, sorted_table=False, long_minimiser=long_min))
    t0 = time.perf_counter()
    res = e.count_graph(rows, 150, good_len=gl, bc=None if grouped else bc, params=params, group=group)
    torch.cuda.synchronize()
    job_s = time.perf_counter() - t0
    reads = None
    if not no_reads:
        reads = _lib.SnkDevReads()
        reads.n_reads, reads.rows, reads.row_words, reads.read_len = n, rows.data_ptr(), 10, 150
        reads.good_len = gl.data_ptr()
        if group is not None:
            reads.group = group.data_ptr()
    row = dict(reads=n, K=K, grouped=grouped, plan_mem_mb=plan_mb, n_kmers=res.n_kmers, n_unitigs=res.n_unitigs, n_circles=res.n_circles,
               job_s=round(job_s, 2), passes=e.last_partition_passes(), plant=plant)
    if plant:
        tb = res.unitig_total_bases
        off = torch.empty((res.n_unitigs + 1,), dtype=torch.int64, device=dev)
        bases = torch.empty((tb,), dtype=torch.uint8, device=dev)
        # device-to-device copies of the result's arrays through torch views of its pointers
        src_off = torch.as_tensor(_DevArr(res.raw.unitig_off, res.n_unitigs + 1, "<i8"), device=dev)
        src_b = torch.as_tensor(_DevArr(res.raw.unitig_bases, tb, "|u1"), device=dev)
        off.copy_(src_off)
        bases.copy_(src_b)
        bases[tb - (tb * 87) // 100:] = 0
        torch.cuda.synchronize()
        p = res.params
        flags = (_lib.CHECK_SORTED_TABLE if p.sorted_table else 0) | _lib.CHECK_ORDERED | (_lib.CHECK_GROUPED if p.grouped else 0)
        rep = e.check_graph_ptrs(K, flags, p.min_freq, res.n_kmers, res.raw.keys, res.raw.counts, res.raw.ctx, res.n_unitigs, off.data_ptr(),
                                 bases.data_ptr(), res.raw.unitig_group if p.grouped else None, n_instances=res.n_instances)
    else:
        try:
            rep = res.check(reads=reads)
        except _lib.SnkError as ex:      # the reads level's 5 B per entry did not fit next to the job: the graph level alone
            if ex.code != -4 or reads is None:
                raise
            row["reads_level"] = "out of memory"
            rep = res.check()
    row.update(levels=rep["levels"], violations=rep["violations"], counters={k: v for k, v in rep["counters"].items() if v},
               check_circles=rep["n_circles"], n_palindromes=rep["n_palindromes"], n_bases=rep["n_bases"],
               graph_ms=round(rep["graph_ms"], 1), reads_ms=round(rep["reads_ms"], 1), peak_gb=round(rep["peak_bytes"] / 2**30, 2),
               table_digest=f"{rep['table_digest']:016x}", unitig_digest=f"{rep['unitig_digest']:016x}",
               clean=rep["violations"] == 0)
    print(json.dumps(row), flush=True)
    e.close()


class _DevArr:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 3}


if __name__ == "__main__":
    main()
