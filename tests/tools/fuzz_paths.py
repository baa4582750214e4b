"""Randomised parity sweep of read pathing (f1, snk_dev_path_reads) and duplicate marking (f4, snk_dev_mark_dups) against the C oracle
(oracle/snk_oracle.c): random genomes with the plants of tests/pathgen.py (repeats, a tandem run, a palindrome, a long homopolymer, a
short-period repeat), read pairs of up to 256 bases with planted duplicate groups, a device graph of drawn K / filters / buckets, and a
drawn pathing variant (look-up structure, passes, lanes, dictionary load, fingerprint mask, first list capacities, MarkDups sort).
Per case, the five stages that run after the pather, each on the paths the pather just made:
  1. snk_dev_mark_dups: the dup flag of every pair and the counters == oracle_lib.mark_dups on those paths
  2. snk_dev_paths_index: index, read support and counters == a48ref.paths_index
  3. snk_dev_paths_zip: index, data and counters == a48xref.zip_paths on the graph parsed from the a.hbv the library writes, no step
     outside the graph
  4. snk_dev_paths_unzip of that result: edge counts and edges back exactly, offsets after the int16 wrap
  5. snk_dev_edge_barcodes: == ebcxref.edge_barcodes, again with SNK_EBC_GENERAL_SORT, and (when the case counts with barcodes) again on
     the reads reordered by barcode, the fast sort path
-- after every read's (offset, edges) == oracle_lib.path_reads on the device's unitigs; on small cases also the per-unitig barcode lists
== oracle_lib.unitig_barcodes, uncut and cut.  The restatements are pinned to the reference's own files by test_a48_files.py,
test_a48x_files.py and test_ebcx_files.py.  Test infrastructure, like tests/: it may use the oracle.
usage: python tests/tools/fuzz_paths.py [n_cases] [seed] [replay_case]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import tempfile
import numpy as np
import a48ref
import a48xref
import ebcxref
import handpaths
import oracle_lib
import pathgen
from supernova_amd import graphio, lib as _lib
from supernova_amd.engine import Engine, Params

eng = None                      # the sweep's engine (main); a test that borrows later_stages passes its own
PATH_OPTIONS = ("path_index", "path_two_pass", "path_fast_gs", "path_fused", "path_redo_all", "path_slots_x10", "path_fp_mask",
                "path_edge_cap", "path_redo_cap", "path_ubc_cap", "dups_two_sorts", "unitig_bc_cut")
BC_LISTS_MAX_READS = 20000      # the barcode lists' restatement is plain Python


def draw_case(rng):
    c = dict(K=48 if rng.random() < 0.6 else 60, L=int(rng.choice([100, 150, 151, 250, 256])),
             G=int(rng.choice([3000, 12000, 12000, 40000, 120000, 120000, 250000])), cov=float(rng.choice([8, 20, 40])),
             err=float(rng.choice([0.0, 0.002, 0.01])), nbc=int(rng.choice([3, 40, 200])), dup_frac=float(rng.choice([0.0, 0.03, 0.1])),
             min_freq=int(rng.choice([1, 2, 3, 4])), min_bc=int(rng.choice([0, 1, 2, 2, 3])), nb=int(rng.choice([0, 0, 1, 5, 97])),
             use_bc=bool(rng.random() < 0.8), pad=bool(rng.random() < 0.7))
    if c["min_freq"] == 1 and c["use_bc"] and c["min_bc"] > 0:
        c["min_bc"] = 0         # without the prune a barcode filter leaves contexts that point at dropped k-mers (fuzz_parity.py)
    v = dict(path_index=int(rng.integers(0, 2)), path_two_pass=int(rng.integers(0, 2)), path_fast_gs=int(rng.choice([8, 16])),
             path_fused=int(rng.random() < 0.25), path_redo_all=int(rng.random() < 0.2), path_slots_x10=int(rng.choice([30, 11])),
             dups_two_sorts=int(rng.integers(0, 2)))
    if not v["path_index"] and rng.random() < 0.15:
        v["path_fp_mask"] = int(rng.choice([0xFF, 0x3]))
    for o in ("path_edge_cap", "path_redo_cap", "path_ubc_cap"):
        if rng.random() < 0.1:
            v[o] = int(rng.choice([0, 1, 100]))
    return c, v


def reads_for(rng, c):
    g, spots = pathgen.genome(rng, c["G"])
    n_pairs = max(8, int(c["G"] * c["cov"] / c["L"] / 2))
    codes, quals, lens, bc = pathgen.pairs(rng, g, n_pairs, c["L"], c["err"], c["nbc"], spots, spot_frac=0.25)
    if c["dup_frac"]:
        codes, quals, lens, bc = pathgen.plant_dups(rng, codes, quals, lens, bc, c["dup_frac"], c["nbc"])
    return codes, quals, lens, bc


def later_stages(c, us, off, ne, edges, bc, info, engine=None):
    """The paths index, the zip, its unzip and the edge -> barcode lists of one case against their numpy restatements -> mismatch lines.
    c: the case's K and use_bc; info: of a path_reads call with paths_index, pathsx and ebcx; engine: the sweep's unless given."""
    import torch
    eng = engine or globals()["eng"]
    bad = []
    K, inv = c["K"], info["inv"]
    u = graphio.unitigs_to_arrays(us)
    with tempfile.TemporaryDirectory() as td:
        graphio.write_hbv(Path(td) / "g.hbv", None, K, *u)
        g = a48xref.parse_hbv((Path(td) / "g.hbv").read_bytes())
    # the paths index
    x_off, x_ids, x_counts = a48ref.paths_index(ne, edges, inv)
    p = info["pidx"]
    got = (p["n_entries"], p["n_hbv_edges"], p["n_empty_edges"], p["key_bits"])
    want = (len(edges), len(inv), int((np.diff(x_off.astype(np.int64)) == 0).sum()), int(len(inv) - 1).bit_length() if len(inv) > 1 else 0)
    same = [np.array_equal(a, b) for a, b in zip(info["paths_index"] + (info["countsb"],), (x_off, x_ids, x_counts))]
    if not all(same) or got != want or g.E != len(inv):
        bad.append(f"paths index: offsets / ids / counts {['equal' if x else 'differ' for x in same]}; counters {got} vs {want}; {g.E} edges in a.hbv")
    # the compressed paths, and back
    x_index, x_data, x_stats = a48xref.zip_paths(off, ne, edges, g)
    index, data = info["pathsx"]
    st = info["pathsx_stats"]
    got = {k: st[k] for k in x_stats}
    if not (np.array_equal(index, x_index) and np.array_equal(data, x_data)) or got != x_stats or x_stats["n_steps_not_found"] != 0:
        bad.append(f"pathsX: index {'equal' if np.array_equal(index, x_index) else 'differs'}, data {'equal' if np.array_equal(data, x_data) else 'differ'}"
                   f" ({len(data)} vs {len(x_data)} bytes); counters {got} vs {x_stats}")
    dev = torch.device("cuda", 0)
    with graphio.hbv_handle(K, *u) as h:
        u_off, u_ne, u_edges, _ = eng.unzip_paths(h, torch.from_numpy(index.copy()).to(dev), torch.from_numpy(data.copy()).to(dev), len(ne))
    back = (np.array_equal(u_ne, ne), np.array_equal(u_edges, edges), np.array_equal(u_off, np.where(ne > 0, a48xref.wrap16(off), 0)))
    if not all(back):
        bad.append(f"unzip: edge counts / edges / wrapped offsets {['equal' if x else 'differ' for x in back]}")
    # the edge -> barcode lists: as path_reads ran them, with the full-key sort, and on the reads reordered by barcode
    x_off, x_bcs = ebcxref.edge_barcodes(ne, edges, bc, inv)
    runs = [("path_reads", True, info["ebcx"][0], info["ebcx"][1])]
    gen = handpaths.EbcxCall(eng, ne, edges, bc, inv, flags=_lib.EBC_GENERAL_SORT)
    runs.append(("general sort", gen.rc == 0 and gen.out.general_sort == 1, gen.off, gen.bcs))
    if c["use_bc"]:
        order = np.argsort(bc, kind="stable")
        n_o = ne[order].astype(np.int64)
        start = np.concatenate([[0], np.cumsum(ne.astype(np.int64))])
        at = np.repeat(start[order] - (np.cumsum(n_o) - n_o), n_o) + np.arange(int(n_o.sum()))      # the entries of the reads in their new order
        srt = handpaths.EbcxCall(eng, ne[order], edges[at], bc[order], inv)
        runs.append(("reads by barcode", srt.rc == 0 and srt.out.bc_sorted == 1 and srt.out.general_sort == 0, srt.off, srt.bcs))
    for name, ran, e_off, e_bcs in runs:
        if not ran:
            bad.append(f"edge barcodes ({name}): refused, or not the sort path it was to take")
        elif not (np.array_equal(e_off, x_off) and np.array_equal(e_bcs, x_bcs)):
            bad.append(f"edge barcodes ({name}): offsets {'equal' if np.array_equal(e_off, x_off) else 'differ'}, {len(e_bcs)} vs {len(x_bcs)} barcodes")
    return bad


def run_case(case, c, v, codes, quals, lens, bc):
    """-> list of mismatch descriptions (empty: bit-exact)."""
    K, L = c["K"], c["L"]
    rows, dq, dl, dbc = pathgen.to_device(codes, quals, lens, bc, pad_seed=1000 + case if c["pad"] else None)
    for o in PATH_OPTIONS:
        eng.clear_option(o)
    for o, x in v.items():
        eng.set_option(o, x)
    res = eng.count_graph(rows, L, quals=dq, bc=dbc if c["use_bc"] else None, lens=dl,
                          params=Params(K=K, min_freq=c["min_freq"], min_bc=c["min_bc"], n_buckets=c["nb"]))
    us = res.unitigs()
    small = codes.shape[0] <= BC_LISTS_MAX_READS
    off, ne, edges, info = res.path_reads(rows, L, dq, lens=dl, mark_dups=True, bc=dbc, unitig_bcs=small, paths_index=True, pathsx=True, ebcx=True)
    bad = []
    o_off, o_n, o_edges = oracle_lib.path_reads(codes, quals, lens, us, K=K)
    if not (np.array_equal(ne.astype(np.int64), o_n) and np.array_equal(edges, o_edges) and np.array_equal(off, o_off)):
        diff = np.nonzero((ne.astype(np.int64) != o_n) | (off != o_off))[0]
        bad.append(f"paths: {len(diff)} reads differ in offset / edge count, first {diff[:5].tolist()} lens {lens[diff[:5]].tolist()}"
                   f" n {ne[diff[:5]].tolist()} vs {o_n[diff[:5]].tolist()}; edge lists {'equal' if np.array_equal(edges, o_edges) else 'differ'}")
    d = info["dups"]
    o_dup, o_art, o_rate, o_nd, o_ni = oracle_lib.mark_dups(codes, quals, lens, o_off, o_n, o_edges, bc=bc)
    got = (d["n_dup_reads"], d["n_interdup_reads"], d["n_dup_pairs"], d["n_art_pairs"], d["n_placed"], d["interdup_rate"])
    want = (o_nd, o_ni, int(o_dup.sum()), int(o_art.sum()), int((o_n > 0).sum()), o_rate)
    if not np.array_equal(d["dup"], o_dup) or got != want:
        bad.append(f"dups: {int((d['dup'] != o_dup).sum())} flags differ; counters {got} vs {want}")
    bad += later_stages(c, us, off, ne, edges, bc, info)
    if small:
        uoff, ubases = res.unitig_arrays()
        asc = np.frombuffer(b"ACGT", dtype=np.uint8)[ubases].tobytes().decode()
        dev_us = [asc[int(uoff[i]):int(uoff[i + 1])] for i in range(res.n_unitigs)]
        exp = oracle_lib.unitig_barcodes(codes, lens, bc, dev_us, K=K)
        cut = 2
        eng.set_option("unitig_bc_cut", cut)
        _, _, _, info_cut = res.path_reads(rows, L, dq, lens=dl, bc=dbc, unitig_bcs=True)
        for name, inf, lim in (("uncut", info, None), ("cut", info_cut, cut)):
            boff, bcs = inf["unitig_bcs"]
            lists = [bcs[int(boff[u]):int(boff[u + 1])].tolist() for u in range(len(dev_us))]
            if lists != [x[:lim] for x in exp]:
                bad.append(f"unitig barcode lists ({name}) differ on {sum(a != b[:lim] for a, b in zip(lists, exp))} unitigs")
    return bad, info, res.n_unitigs, int(o_n.max()) if len(o_n) else 0


def main():
    global eng
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 12345
    only = int(sys.argv[3]) if len(sys.argv) > 3 else -1      # replay one case of a sweep
    eng = Engine(0)
    rng = np.random.default_rng(seed)
    bad_cases = 0
    for case in range(n_cases):
        c, v = draw_case(rng)
        data = reads_for(rng, c)
        if only >= 0 and case != only:
            continue
        n = data[0].shape[0]
        vtxt = " ".join(f"{k}={x}" for k, x in v.items())
        tag = f"case {case}: K={c['K']} L={c['L']} G={c['G']} n={n} err={c['err']} nbc={c['nbc']} dups={c['dup_frac']} min_freq={c['min_freq']} " \
              f"min_bc={c['min_bc']} nb={c['nb']} bc={c['use_bc']} pad={c['pad']} | {vtxt}"
        try:
            bad, info, nu, longest = run_case(case, c, v, *data)
        except _lib.SnkError as ex:
            bad, info, nu, longest = [f"library error: {ex}"], {}, -1, -1
        if bad:
            bad_cases += 1
            print("FAIL " + tag, flush=True)
            for b in bad:
                print("     " + b, flush=True)
        else:
            print(f"ok   {tag} -> {nu} unitigs, longest path {longest} edges, {info['n_slow']} slow, retries {info['retries']}, "
                  f"{info['dups']['n_dup_pairs']} dup pairs", flush=True)
    print(f"{n_cases - bad_cases} of {n_cases} cases bit-exact")
    return 1 if bad_cases else 0


if __name__ == "__main__":
    sys.exit(main())
