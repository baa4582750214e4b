"""Inputs and the rank runner shared by the GPU test modules that drive W simulated ranks on one device."""
import threading

import numpy as np


def plasmid_case(seed=5):
    """A 600 kb linear genome + six circular replicons from 150 bp to 20 kb at 30x, error-free, two barcodes per locus:
    thousands of fragments (the sparse-ruling-set ranking runs, not the small-input fallback) with circles that hold splitters
    and circles that hold none."""
    rng = np.random.default_rng(seed)
    L = 150
    reps = [(rng.integers(0, 4, 600_000, dtype=np.uint8), False)] + [(rng.integers(0, 4, n, dtype=np.uint8), True) for n in (150, 400, 1000, 3000, 8000, 20000)]
    rows = []
    for g, circular in reps:
        G = len(g)
        n = max(40, G * 30 // L)
        ext = np.concatenate([g, g[:L]]) if circular else g
        starts = rng.integers(0, G if circular else G - L + 1, n)
        idx = starts[:, None] + np.arange(L)[None, :]
        r = ext[idx]
        flip = rng.random(n) < 0.5
        r[flip] = (3 - r[flip][:, ::-1])
        rows.append(r)
    codes = np.concatenate(rows).astype(np.uint8)
    perm = rng.permutation(codes.shape[0])
    codes = codes[perm]
    if codes.shape[0] & 1:
        codes = codes[:-1]
    n = codes.shape[0]
    quals = np.full((n, L), 30, dtype=np.uint8)
    bc = rng.integers(1, 50, n).astype(np.int32)
    return codes, quals, bc, L


def run_ranks(W, rows, read_len, quals, bc=None, lens=None, K=48, n_buckets=0, ign_bc_below=0, pairs=False):
    """W in-process ranks (a thread, a context and a share of the reads each; contexts are created here, so they read SNK_TUNING) through
    ShardedEngine.count_graph -> per rank a dict of the host arrays and the counters the step reports.  rows / quals / bc / lens: host
    arrays (rows packed, lens uint16 or None); pairs: cut the shares at even read indices."""
    import torch
    from supernova_amd.engine import Engine, Params
    from supernova_amd.sharded import ShardedEngine, SimWorld
    dev = torch.device("cuda", 0)
    world = SimWorld(W)
    n = rows.shape[0]
    bounds = ([(n // 2 * r // W) * 2 for r in range(W)] + [n]) if pairs else [n * r // W for r in range(W + 1)]
    out, errs = [None] * W, []

    def worker(r):
        try:
            torch.cuda.set_device(0)
            e = Engine(0)
            lo, hi = bounds[r], bounds[r + 1]
            res = ShardedEngine(e, world.comm(r)).count_graph(
                torch.from_numpy(rows[lo:hi].view(np.int32).copy()).to(dev), read_len,
                quals=torch.from_numpy(np.ascontiguousarray(quals[lo:hi])).to(dev),
                bc=None if bc is None else torch.from_numpy(bc[lo:hi].astype(np.int32)).to(dev),
                lens=None if lens is None else torch.from_numpy(lens[lo:hi].astype(np.uint16).view(np.int16)).to(dev),
                params=Params(K=K, n_buckets=n_buckets), ign_bc_below=ign_bc_below, read_index_base=lo, total_reads=n)
            out[r] = dict(keys=res.keys(), counts=res.counts(), ctx=res.ctx(), spectrum=res.spectrum(), unitigs=res.unitigs(),
                          n_instances=res.n_instances, n_frags=res.n_frags, n_queries=res.n_queries, ranking=res.join_ranking,
                          n_circles=res.n_circles, host_syncs=res.host_syncs, n_buckets=res.n_buckets, options=dict(
                              (k, e.get_option(k)) for k in e.options() if e.get_option(k) is not None))
            e.close()
        except BaseException as ex:  # noqa: BLE001
            errs.append(ex)
            world.barrier_obj.abort()

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(W)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
    return out
