"""Host-side engine: one process per GPU, device memory and streams through torch, compute in libsnk.

`Engine.count_graph` is the Python face of the C++ entry the reference exposes for this path,
buildReadQGraph48 (lib/assembly/src/paths/long/BuildReadQGraph48.h:24-34): same thresholds
(minQual, minFreq, minBC, ignBcBelow), same outputs (retained k-mer dictionary with pruned contexts,
canonical unitigs), with reads resident in HBM.  No CPU fallback: without libsnk.so or without a
gfx950 device every call raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import lib as _lib
from .graphio import hbv_arrays

PHASES = ("trim", "plan", "partition", "count", "sort", "graph", "-", "total")


# ---- the two input structs of the device stages, from tensors (the one place each is filled)
class DevArray:
    """A device array the library allocated itself, known by pointer and shape only, where the builders take a tensor."""

    def __init__(self, ptr, *shape):
        self._ptr, self.shape = ptr, shape

    def data_ptr(self):
        return self._ptr


def _ptr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a      # (a tensor, or a plain pointer / None)


def dev_reads(rows, read_len, quals=None, lens=None, good_len=None, bc=None, group=None, ign_bc_below=0, read_index_base=0) -> "_lib.SnkDevReads":
    """snk_dev_reads over tensors: rows i32[n, words] (1-D rows: row_words 0), quals u8[n, stride] or None (null, qstride 0); every other
    pointer is null when None.  It checks nothing: the struct only points into the tensors, which the caller keeps alive over the call."""
    r = _lib.SnkDevReads()
    r.n_reads, r.rows, r.row_words, r.read_len = int(rows.shape[0]), rows.data_ptr(), (int(rows.shape[1]) if len(rows.shape) > 1 else 0), int(read_len)
    if quals is not None:
        r.quals, r.qstride = quals.data_ptr(), int(quals.shape[1])
    r.lens, r.good_len, r.bc, r.group = _ptr(lens), _ptr(good_len), _ptr(bc), _ptr(group)
    r.ign_bc_below, r.read_index_base = ign_bc_below, read_index_base
    return r


def dev_paths(offset, n_edges, edges, start=None):
    """snk_dev_paths as a stage's input, over tensors: offset i32[n], n_edges i32[n] (read as u32), edges i32[sum], start i64[n + 1] (None:
    the paths follow each other, start = the exclusive prefix sum of n_edges, made here on n_edges.device).  -> (SnkDevPaths, start): the
    struct points into start, so the caller holds it until the call has returned."""
    n = int(n_edges.shape[0])
    if start is None:
        start = torch.zeros(n + 1, dtype=torch.int64, device=n_edges.device)
        start[1:] = torch.cumsum(n_edges.to(torch.int64) & 0xFFFFFFFF, 0)
    p = _lib.SnkDevPaths()
    p.n_reads, p.n_edges_total = n, int(edges.shape[0])
    p.offset, p.n_edges, p.start, p.edges = offset.data_ptr(), n_edges.data_ptr(), start.data_ptr(), edges.data_ptr()
    return p, start


@dataclass
class Params:
    K: int = 48
    min_qual: int = 7      # lib/tada/mro/_asm_sn.mro:15, 10X/DF.cc:141
    min_freq: int = 3      # mro/_assembler.mro:44, 10X/DF.cc:139
    min_bc: int = 2        # 10X/DF.cc:140
    n_buckets: int = 0
    graph: bool = True
    sorted_table: bool = True     # False: leave the retained table in bucket order (SNK_F_UNSORTED_TABLE)
    global_graph: bool = False    # True: the global graph stage (SNK_F_GLOBAL_GRAPH), a cross-check of the bucket-local one
    grouped: bool = False         # True: per-group graphs (SNK_F_GROUPED); count_graph(group=...) gives the group of every read
    long_minimiser: bool = False  # True: 20-base minimisers (SNK_F_LONG_MINIMISER): genomes of human size; same results

    def to_c(self) -> _lib.SnkParams:
        p = _lib.SnkParams()
        p.K, p.min_qual, p.min_freq, p.min_bc = self.K, self.min_qual, self.min_freq, self.min_bc
        p.n_buckets = self.n_buckets
        p.flags = ((0 if self.graph else 1) | (0 if self.sorted_table else 2) | (4 if self.global_graph else 0)
                   | (8 if self.grouped else 0) | (64 if self.long_minimiser else 0))
        return p


class Result:
    """Device-resident result of one count_graph call (valid until the next call on the same engine)."""

    def __init__(self, engine: "Engine", raw: _lib.SnkDevResult, K: int, params: "Params | None" = None):
        self._e = engine
        self.raw = raw
        self.K = K
        self.params = params
        for f in ("n_reads", "n_instances", "n_supermers", "n_buckets", "n_kmers", "n_unitigs", "unitig_total_bases",
                  "n_circles", "rank_rounds", "buckets_split", "max_slots_used", "scratch_bytes", "n_boundary", "n_overflow",
                  "n_fragments", "repartitioned", "n_hot_buckets"):
            setattr(self, f, int(getattr(raw, f)))
        self.phase_ms = {PHASES[i]: float(raw.phase_ms[i]) for i in range(8) if PHASES[i] != "-"}
        self.kernel_ms = {"partition": float(raw.kernel_ms[1]),
                          "count": float(raw.kernel_ms[2])}
        names = ("local_prune", "-", "fragments", "join", "table")     # local_prune includes the boundary index + resolve
        self.graph_ms = {names[i]: float(raw.graph_ms[i]) for i in range(5) if names[i] != "-"}

    def _dl(self, ptr, nbytes, dtype, shape):
        return self._e._fetch(ptr, nbytes // np.dtype(dtype).itemsize, dtype).reshape(shape)

    def good_len(self) -> np.ndarray:
        return self._e._fetch(self.raw.good_len, self.n_reads, np.uint16)

    def keys(self) -> np.ndarray:
        """[n_kmers, 4] u32 words MSB-first (include/snk.h key convention), ascending."""
        lohi = self._e._fetch(self.raw.keys, self.n_kmers * 2, np.uint64).reshape(self.n_kmers, 2)
        lo, hi = lohi[:, 0], lohi[:, 1]
        w = np.empty((self.n_kmers, 4), dtype=np.uint32)
        w[:, 0] = hi >> np.uint64(32)
        w[:, 1] = hi & np.uint64(0xFFFFFFFF)
        w[:, 2] = lo >> np.uint64(32)
        w[:, 3] = lo & np.uint64(0xFFFFFFFF)
        return w

    def counts(self) -> np.ndarray:
        return self._e._fetch(self.raw.counts, self.n_kmers, np.uint32)

    def ctx(self) -> np.ndarray:
        return self._e._fetch(self.raw.ctx, self.n_kmers, np.uint8)

    def spectrum(self) -> np.ndarray:
        return self._e._fetch(self.raw.spectrum, self.raw.spectrum_bins, np.uint64)

    def unitig_arrays(self):
        return self._e._fetch(self.raw.unitig_off, self.n_unitigs + 1, np.uint64), self._e._fetch(self.raw.unitig_bases, self.unitig_total_bases, np.uint8)

    def unitig_groups(self) -> np.ndarray:
        """Grouped runs: group id of every unitig (same order as unitig_arrays())."""
        return self._e._fetch(self.raw.unitig_group, self.n_unitigs, np.uint32)

    def bv_image_device(self):
        """a13 on the device: (device pointer, bytes) of the .bv hand-off file -- "BINWRITE", count, per unitig u32 length + 2-bit bases in
        BVComp order (snk_dev_bv_image).  Context memory: valid until the engine's next top-level call."""
        ptr, nb = C.c_void_p(0), C.c_uint64(0)
        self._e._call(self._e.lib.snk_dev_bv_image, int(self.K), *self._unitigs(), 1, C.byref(ptr), C.byref(nb))
        return ptr.value, int(nb.value)

    def bv_image(self) -> bytes:
        return self._e._fetch(*self.bv_image_device(), np.uint8).tobytes()

    def _unitigs(self):
        """(n_unitigs, unitig_off, unitig_bases): the unitig arguments of the device stages"""
        return self.n_unitigs, self.raw.unitig_off, self.raw.unitig_bases

    def hbv(self) -> dict:
        """The graph from the device-resident unitigs (buildHBVFromEdges, HBVFromEdges.cc:244-296; snk_dev_hbv):
        vertex ids per HBV edge, fwd/rev translation per unitig, numbered in BVComp order; 'order'[r] = index of the
        rank-r unitig in unitig_arrays().  Must be called before the engine's next count_graph."""
        h, ms = _lib.SnkHbv(), C.c_float(0)
        self._e._call(self._e.lib.snk_dev_hbv, int(self.K), *self._unitigs(), C.byref(h), C.byref(ms))
        try:
            return dict(hbv_arrays(h, self.n_unitigs, order=True), device_ms=float(ms.value))
        finally:
            self._e.lib.snk_hbv_free(C.byref(h))

    def path_reads(self, rows, read_len: int, quals, lens=None, mark_dups=False, bc=None, unitig_bcs=False, download=True, bcs_nocut=False,
                   paths_index=False, pathsx=False, ebcx=False, extend=False, mark_bads=False, hops=False, closures=False):
        """f1: the reads (untrimmed packed rows + quality rows on the device) onto the graph of this result's unitigs --
        pathReads with the new aligner (BuildReadQGraph48.cc:1441-1469).  Returns (offset i32[n], n_edges u32[n], edges i32[sum],
        info) on the host, HBV edge ids as numbered by buildHBVFromEdges.  Must be called before the engine's next count_graph.
        mark_dups: f4, MarkDups over these paths (10X/SecretOps.cc:413-593; bc = raw barcode ids on the device or None) ->
        info['dups'] = dict(dup u8[n/2], interdup_rate, n_dup_pairs, n_dup_reads, n_art_pairs, n_placed, ms).
        unitig_bcs: the rest of f4 -- per unitig (numbering of unitig_arrays()) the sorted distinct barcodes > 0 of the reads with a
        k-mer on it (tada's edge -> barcode sets) -> info['unitig_bcs'] = (off u64[U+1], bcs u32[...]); unitig_bcs="exhaustive" derives them
        the slow, literal way (every k-mer of every barcoded read looked up); bcs_nocut: without the 20 000-entry cut.
        info['retries']: the lists that overflowed and were regrown (snk_dev_paths.retries: 1 redo list, 2 path edges, 4 barcode keys);
        next to it, in both modes: dict_ms, path_ms, bcs_ms, hbv_device_ms, dict_slots, lookup ('index' or 'kmer_dictionary'), n_slow,
        n_edges_total, n_unitig_bcs.  download=False: (None, None, None, info) -- nothing but counters and times comes to the host.
        paths_index: writePathsIndex over these paths (10X/PathsIndex.cc:23-145; snk_dev_paths_index) -> info['paths_index'] = (off u64[E+1],
        ids u64[...]): the reads of HBV edge e are ids[off[e]:off[e+1]], ascending, a read as often as its path holds e; info['countsb'] =
        i32[E] read support, an edge and its reverse complement summed; info['inv'] = the involution; info['pidx'] = counters and time.
        pathsx: the paths as a ReadPathVecX (10X/DF.cc:579; snk_dev_paths_zip) -> info['pathsx'] = (index i64[ceil(n / 10)], data u8[...]):
        per read its edge count, int16 offset, first edge and 2-bit branch ids; info['pathsx_stats'] = sizes, counters and time (download=False:
        info['pathsx_dev'] = the SnkDevPathsx itself, valid until the engine's next count_graph or path_reads).
        ebcx (needs bc): the edge -> barcode lists of computeEdgeToBarcodeX (10X/PathsIndex.cc:297-358; snk_dev_edge_barcodes) ->
        info['ebcx'] = (off u64[E+1], bcs i32[...]): the ascending distinct barcodes > 0 of the reads whose path holds HBV edge e or its
        reverse complement are bcs[off[e]:off[e+1]]; info['ebcx_stats'] = sizes, which sort ran and time; ebcx="general" asks for the full-key
        sort even when bc is sorted (SNK_EBC_GENERAL_SORT).  download=False: the stats only.
        extend (True, or "back" for SNK_EXT_BACK): StageExtension over these paths (10X/DF.cc:676; ExtendPathsNew, 10X/Extend.cc:14-177;
        snk_dev_extend_paths) -> info['extended'] = (offset i32[n], n_edges u32[n], edges i32[sum]), info['extend_stats'] = the counters and
        time; with pathsx also info['extended_pathsx'] = (index, data), the ReadPathVecX of the extended paths, and
        info['extended_pathsx_stats'].  It runs last: every other result is of the paths as pathed.  download=False: the stats only.
        mark_bads (True, or "x" for SNK_BADS_X: offsets as the ReadPathVecX of a stock DF holds them): MarkBads over these paths
        (10X/SecretOps.cc:22-59,70-107; snk_dev_mark_bads) -> info['bads'] = dict(bad u8[n/2], n_bad_pairs, n_bad_reads, n_mismatch_reads,
        n_placed, n_offsets_wrapped, ms): what graphio.write_bad / write_a48 make a.bad of.  download=False: the counters, and
        info['bads_dev'] = the SnkDevBads itself (device memory of the context, valid until the engine's next count_graph or path_reads).
        hops (True, or "one_good" for SNK_HOPS_ONE_GOOD; needs bc, implies paths_index): FindEdgePairs over these paths (10X/Closomatic.cc:17-354;
        snk_dev_edge_pairs), the second step of StageFindPatch, with the flags of mark_bads when that is given and all-false flags
        otherwise -> info['hops'] = i32[n, 2], the pairs ascending: what graphio.write_hops / write_a48 make a.hops of;
        info['hops_stats'] = the counters and times.  download=False: the stats only.
        closures (True, or "cg1" for SNK_CLOSE_CG1; needs hops): CloseGap2 / CloseGap for those pairs (10X/Closomatic.cc:356-657;
        snk_dev_close_gaps), the third step of StageFindPatch with STACKSTER=False -> info['closures'] = (closure_off u64[n + 1], bases u8[],
        pair_first u64[n_pairs + 1]): what graphio.write_closures makes closures.fastb of and Engine.insert_patch takes;
        info['closures_stats'] = the counters and times.  download=False: the stats only."""
        if closures and not hops:
            raise ValueError("path_reads(closures=...) needs hops: the pairs to close")
        if ebcx and bc is None:
            raise ValueError("path_reads(ebcx=...) needs bc: the barcode of every read, on the device")
        if hops and bc is None:
            raise ValueError("path_reads(hops=...) needs bc: the barcode of every read, on the device")
        paths_index = paths_index or bool(hops)
        e, K = self._e, int(self.K)
        h, ms = _lib.SnkHbv(), C.c_float(0)
        e._call(e.lib.snk_dev_hbv, K, *self._unitigs(), C.byref(h), C.byref(ms))
        graph = (*self._unitigs(), C.byref(h))
        stages = {}
        try:
            r = dev_reads(rows, read_len, quals, lens, bc=bc if unitig_bcs else None)
            out = _lib.SnkDevPaths()
            e._call(e.lib.snk_dev_path_reads2, K, C.byref(r), *graph,
                    (0 if not unitig_bcs else 1 | (2 if unitig_bcs == "exhaustive" else 0) | (4 if bcs_nocut else 0)), C.byref(out))
            if mark_dups:
                if bc is not None:
                    r.bc = bc.data_ptr()
                stages.update(e._dups_info(e._dups(r, out), download))
            bd = None
            if mark_bads:
                bd = e._bads(K, r, graph, out, mark_bads == "x")
                stages.update(e._bads_info(bd, download))
            if paths_index or ebcx:
                n_hbv = int(h.n_edges)
                inv = np.zeros(max(n_hbv, 1), dtype=np.int32)
                _lib.call(e.lib.snk_hbv_involution, C.byref(h), self.n_unitigs, inv.ctypes.data)
            if paths_index:
                px = e._pidx(out, n_hbv, inv)
                stages.update(e._pidx_info(px, n_hbv, inv, download))
            if hops:
                bad = torch.zeros(max(int(out.n_reads) // 2, 1), dtype=torch.uint8, device=bc.device) if bd is None else None
                hp = e._hops(K, graph, inv, out, px, bc.data_ptr(), bad.data_ptr() if bd is None else bd.bad, hops == "one_good")
                stages.update(e._hops_info(hp, download))
                if closures:
                    stages.update(e._close_info(e._close(K, graph, inv, r, out, px, hp.n_pairs, hp.pairs, closures == "cg1"), download))
            if ebcx:
                stages.update(e._ebcx_info(e._ebcx(out, bc, n_hbv, inv, ebcx == "general"), n_hbv, download))
            if pathsx:
                stages.update(e._pathsx_info(e._zip(out, graph[3]), download, dev_key="pathsx_dev"))
            if extend:
                xo = e._extend(K, r, graph, out, extend == "back")
                stages.update(e._extend_info(xo, download))
                if pathsx:
                    stages.update(e._pathsx_info(e._zip(xo.paths, graph[3]), download, prefix="extended_"))
        finally:
            e.lib.snk_hbv_free(C.byref(h))
        info = dict(dict_ms=float(out.dict_ms), path_ms=float(out.path_ms), bcs_ms=float(out.bcs_ms), hbv_device_ms=float(ms.value),
                    dict_slots=int(out.dict_slots), lookup=("index" if out.lookup_index else "kmer_dictionary"), n_slow=int(out.n_slow),
                    retries=int(out.retries), n_edges_total=int(out.n_edges_total), n_unitig_bcs=int(out.n_unitig_bcs))
        info.update(stages)
        if not download:          # timings only (bench.py: the results stay on the device)
            return None, None, None, info
        if unitig_bcs and out.unitig_bc_off:
            info["unitig_bcs"] = (e._fetch(out.unitig_bc_off, self.n_unitigs + 1, np.uint64), e._fetch(out.unitig_bcs, out.n_unitig_bcs, np.uint32))
        return (*e._fetch_paths(out), info)

    def check(self, reads: "_lib.SnkDevReads | None" = None, ordered: bool = True) -> dict:
        """snk_dev_check_graph over this result's own arrays (include/snk.h, "the graph verifier"): the reassembly invariants of the
        table and the unitigs, and the digests; with `reads` (the snk_dev_reads the result was made from) the reads level as well.
        The result stays valid."""
        p = self.params or Params(K=self.K)
        flags = ((_lib.CHECK_SORTED_TABLE if p.sorted_table else 0) | (_lib.CHECK_ORDERED if ordered else 0)
                 | (_lib.CHECK_GROUPED if p.grouped else 0))
        r = self.raw
        return self._e.check_graph_ptrs(self.K, flags, p.min_freq, self.n_kmers, r.keys, r.counts, r.ctx, self.n_unitigs, r.unitig_off,
                                        r.unitig_bases, r.unitig_group if p.grouped else None, n_instances=self.n_instances, reads=reads,
                                        min_qual=p.min_qual)

    def unitigs(self) -> list[str]:
        """Canonical unitigs sorted by (length desc, lexicographic) = BVComp, HBVFromEdges.cc:106-111."""
        off, bases = self.unitig_arrays()
        asc = np.frombuffer(b"ACGT", dtype=np.uint8)[bases].tobytes().decode()
        us = [asc[int(off[i]):int(off[i + 1])] for i in range(self.n_unitigs)]
        us.sort(key=lambda s: (-len(s), s))
        return us


class _DevBytes:
    """Device memory of the library seen by torch without a copy (__cuda_array_interface__ over the raw pointer)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


class PatchResult:
    """What Engine.insert_patch leaves: the patched graph and the read paths on it, in tensors and arrays this object owns (they outlive
    the engine's later calls).  h: the lib.SnkHbv of the new unitigs (bvcomp_order maps its unitig numbering to unitig_off /
    unitig_bases), freed by close(); unitig_off i64[U + 1], unitig_bases u8[], offset / n_edges / start / edges: tensors on the device
    as Engine.extend_paths and Engine.zip_paths take them; inv, to3_off, to3, left3: numpy; stats: sizes, counters and times."""

    def __init__(self, engine: "Engine", K: int, h: "_lib.SnkHbv"):
        self._e, self.K, self.h = engine, K, h

    def close(self):
        if self.h is not None:
            self._e.lib.snk_hbv_free(C.byref(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def unitigs_bvcomp(self):
        """-> (off u64[U + 1], bases u8[]) on the host in BVComp order: the numbering of h, what snk_write_hbv / snk_write_hbx take"""
        off = self.unitig_off.cpu().numpy().view(np.uint64)
        bases = self.unitig_bases.cpu().numpy()
        U = len(off) - 1
        order = np.ctypeslib.as_array(self.h.bvcomp_order, shape=(U,)).astype(np.int64) if U and self.h.bvcomp_order else np.arange(U)
        lens = np.diff(off.astype(np.int64))[order]
        noff = np.zeros(U + 1, np.uint64)
        noff[1:] = np.cumsum(lens, dtype=np.uint64)
        idx = np.repeat(off[:-1].astype(np.int64)[order] - noff[:-1].astype(np.int64), lens) + np.arange(int(noff[-1]))
        return noff, np.ascontiguousarray(bases[idx])

    def write(self, path_hbv, path_inv=None, path_hbx=None):
        """a.hbv (+ a.inv, a.hbx) of the patched graph, as DF writes them"""
        off, bases = self.unitigs_bvcomp()
        h = _lib.SnkHbv.from_buffer_copy(self.h)
        h.bvcomp_order = None
        unitigs = (self.K, len(off) - 1, off.ctypes.data, bases.ctypes.data, C.byref(h))
        _lib.call(self._e.lib.snk_write_hbv, str(path_hbv).encode(), str(path_inv).encode() if path_inv else None, *unitigs)
        if path_hbx:
            _lib.call(self._e.lib.snk_write_hbx, str(path_hbx).encode(), *unitigs)


class EditResult:
    """What Engine.delete_edges leaves: the edited graph and the read paths on it, in tensors and arrays this object owns (they outlive the
    engine's later calls).  h: a lib.SnkHbv over the new unitigs (one per pair {e, inv[e]}, numbered by the pair's smaller edge id; bvcomp_order
    None), its arrays held by this object; unitig_off i64[U + 1], unitig_bases u8[], offset / n_edges / start / edges: tensors on the device;
    inv, edge_map, edge_koff: numpy; stats: counters and times.  graph and paths are the tuples Engine.delete_edges, hanging_ends and
    trim_hanging_ends take; h, the unitig tensors and the path tensors go into zip_paths, extend_paths and the paths index as they are."""

    def __init__(self, engine: "Engine", K: int, raw: "_lib.SnkDevEdit", take):
        self._e, self.K = engine, K
        E, N, U, n, tot = int(raw.h.n_edges), int(raw.h.n_vertices), int(raw.n_unitigs), int(raw.paths.n_reads), int(raw.paths.n_edges_total)
        host = lambda p, m, dt: (np.array(np.ctypeslib.as_array(p, shape=(m,)), dtype=dt, copy=True) if m else np.zeros(0, dt))
        self._arrays = dict(v_left=host(raw.h.v_left, E, np.int32), v_right=host(raw.h.v_right, E, np.int32), src_unitig=host(raw.h.src_unitig, E, np.int32),
                            is_rc=host(raw.h.is_rc, E, np.uint8), fwd_xlat=host(raw.h.fwd_xlat, U, np.int32), rev_xlat=host(raw.h.rev_xlat, U, np.int32))
        self.h = _lib.SnkHbv()
        self.h.n_vertices, self.h.n_edges = N, E
        for k, a in self._arrays.items():
            setattr(self.h, k, a.ctypes.data_as(C.POINTER(C.c_uint8 if k == "is_rc" else C.c_int32)))
        self.inv = host(raw.inv, E, np.int32)
        self.edge_map, self.edge_koff = host(raw.edge_map, int(raw.n_old_edges), np.int32), host(raw.edge_koff, int(raw.n_old_edges), np.int32)
        self.unitig_off, self.unitig_bases = take(raw.unitig_off, U + 1, torch.int64), take(raw.unitig_bases, int(raw.unitig_total_bases), torch.uint8)
        self.offset, self.n_edges, self.start, self.edges = take(raw.paths.offset, n, torch.int32), take(raw.paths.n_edges, n, torch.int32), \
            take(raw.paths.start, n + 1, torch.int64), take(raw.paths.edges, tot, torch.int32)
        self.stats = dict(n_deleted=int(raw.n_deleted), n_runs=int(raw.n_runs), n_absorbed=int(raw.n_absorbed), max_run=int(raw.max_run), n_truncated=int(raw.n_truncated),
                          n_emptied=int(raw.n_emptied), n_collapsed=int(raw.n_collapsed), n_edges=E, n_vertices=N, n_unitigs=U, ms=float(raw.ms), graph_ms=float(raw.graph_ms),
                          paths_ms=float(raw.paths.path_ms))

    @property
    def graph(self):
        return (self.K, self.h, self.unitig_off, self.unitig_bases, self.inv)

    @property
    def paths(self):
        return (self.offset, self.n_edges, self.edges, self.start)

    def write(self, path_hbv, path_inv=None, path_hbx=None):
        """a.hbv (+ a.inv, a.hbx) of the edited graph, as the reference writes them"""
        off = self.unitig_off.cpu().numpy().view(np.uint64)
        bases = np.ascontiguousarray(self.unitig_bases.cpu().numpy())
        unitigs = (self.K, len(off) - 1, off.ctypes.data, bases.ctypes.data, C.byref(self.h))
        _lib.call(self._e.lib.snk_write_hbv, str(path_hbv).encode(), str(path_inv).encode() if path_inv else None, *unitigs)
        if path_hbx:
            _lib.call(self._e.lib.snk_write_hbx, str(path_hbx).encode(), *unitigs)


def _graph(h: "_lib.SnkHbv", unitig_off, unitig_bases):
    """(n_unitigs, unitig_off, unitig_bases, byref(h)): the graph arguments of the device stages, from tensors"""
    return int(unitig_off.shape[0]) - 1, unitig_off.data_ptr(), unitig_bases.data_ptr(), C.byref(h)


def _ebcx_stats(eb: "_lib.SnkDevEbcx") -> dict:
    return dict(n_hbv_edges=int(eb.n_hbv_edges), n_ebc=int(eb.n_ebc), n_keys=int(eb.n_keys), n_empty_edges=int(eb.n_empty_edges), max_list=int(eb.max_list),
                bc_sorted=int(eb.bc_sorted), general_sort=int(eb.general_sort), key_bits=int(eb.key_bits), ms=float(eb.ms))


def _extend_stats(x: "_lib.SnkDevExtend") -> dict:
    return dict(n_reads=int(x.paths.n_reads), n_edges_total=int(x.paths.n_edges_total), n_back_extended=int(x.n_back_extended),
                n_cut_to_first=int(x.n_cut_to_first), n_quality_extended=int(x.n_quality_extended), n_ambiguous=int(x.n_ambiguous),
                n_too_many=int(x.n_too_many), n_exact_extended=int(x.n_exact_extended), n_enumerated=int(x.n_enumerated), ms=float(x.ms))


def _bads_stats(b: "_lib.SnkDevBads") -> dict:
    return dict(n_pairs=int(b.n_pairs), n_placed=int(b.n_placed), n_mismatch_reads=int(b.n_mismatch_reads), n_bad_reads=int(b.n_bad_reads),
                n_bad_pairs=int(b.n_bad_pairs), n_offsets_wrapped=int(b.n_offsets_wrapped), n_slabs=int(b.n_slabs), ms=float(b.ms), tables_ms=float(b.tables_ms), kernel_ms=float(b.kernel_ms))


def _hops_stats(hp: "_lib.SnkDevHops") -> dict:
    d = {k: int(getattr(hp, k)) for k in ("n_pairs", "n_part1", "n_part2", "n_part3", "n_sink_edges", "n_long_edges", "n_two_class", "n_ext_round0", "n_ext_closure",
                                          "n_ext_host", "n_not_extended", "ext_budget")}
    d.update({k: float(getattr(hp, k)) for k in ("ms", "tables_ms", "part12_ms", "part3_ms")})
    return d


def _close_stats(cl: "_lib.SnkDevClosures") -> dict:
    d = {k: int(getattr(cl, k)) for k in ("n_closures", "n_bases", "n_pairs", "n_pairs_0", "n_pairs_1", "n_pairs_2", "n_pairs_many", "n_rows", "n_partners_tried",
                                          "n_partners_placed", "n_followers", "n_cons_too_long", "n_place_host", "max_width", "bod_budget")}
    d.update({k: float(getattr(cl, k)) for k in ("ms", "tables_ms", "gather_ms", "close_ms")})
    return d


def _pathsx_stats(zx: "_lib.SnkDevPathsx") -> dict:
    return dict(n_reads=int(zx.n_reads), n_bytes=int(zx.n_bytes), n_index=int(zx.n_index), n_empty=int(zx.n_empty),
                n_steps_not_found=int(zx.n_steps_not_found), n_offsets_wrapped=int(zx.n_offsets_wrapped), ms=float(zx.ms))


import weakref as _weakref

_LIVE = _weakref.WeakSet()      # contexts that are open (tests pin options on all of them: tests/conftest.py `tune`)


def live_engines():
    return [e for e in list(_LIVE) if getattr(e, "_ctx", None)]


class Engine:
    def __init__(self, device: int | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("supernova_amd.Engine needs a gfx950 GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.cuda.current_device() if device is None else device
        h = C.c_void_p()
        _lib.call(self.lib.snk_ctx_create, self.device, C.byref(h))
        self._ctx = h
        _LIVE.add(self)

    def last_count_limit(self) -> int:
        """Usable count-table slots per pass in the last count_graph call (1216, or 1920 with booked slots; snk_ctx_last_count_limit)."""
        return int(self.lib.snk_ctx_last_count_limit(self._ctx))

    def last_partition_passes(self) -> int:
        """Bucket-range passes of the last count_graph call (1 = the one-pass partition; snk_ctx_last_partition_passes)."""
        return int(self.lib.snk_ctx_last_partition_passes(self._ctx))

    # ---- tuning (include/snk.h "tuning"): options live in the context, not in the environment
    def set_option(self, name: str, value: int):
        _lib.call(self.lib.snk_ctx_set_option, self._ctx, name.encode(), int(value))

    def clear_option(self, name: str | None = None):
        """Back to the library's own choice (None: every option)."""
        self.lib.snk_ctx_clear_option(self._ctx, name.encode() if name is not None else None)

    def get_option(self, name: str):
        """-> the pinned value, or None when the library chooses."""
        v = C.c_longlong(0)
        rc = self.lib.snk_ctx_get_option(self._ctx, name.encode(), C.byref(v))
        if rc < 0:
            raise KeyError(name)
        return int(v.value) if rc == 1 else None

    def options(self) -> dict:
        """name -> description of every option the library knows."""
        out, i = {}, 0
        while True:
            n = self.lib.snk_option_name(i)
            if not n:
                return out
            out[n.decode()] = self.lib.snk_option_doc(i).decode()
            i += 1

    def set_tuning(self, **fields):
        """snk_ctx_set_tuning: the documented knobs as one struct (count_kernel=2, target_inst=4000, ...); unnamed fields = the library's choice."""
        t = _lib.SnkTuning()
        self.lib.snk_tuning_default(C.byref(t))
        for k, v in fields.items():
            if not hasattr(t, k) or k.startswith("last_") or k == "reserved":
                raise AttributeError(k)
            setattr(t, k, int(v))
        _lib.call(self.lib.snk_ctx_set_tuning, self._ctx, C.byref(t))

    def get_tuning(self) -> dict:
        """What is pinned (0 = the library chooses) and, in last_*, what the context's last call ran with."""
        t = _lib.SnkTuning()
        self.lib.snk_ctx_get_tuning(self._ctx, C.byref(t))
        return {k: int(getattr(t, k)) for k, _ in _lib.SnkTuning._fields_ if k != "reserved"}

    def reserve(self, n_bytes: int):
        """Map n_bytes of device memory into the context's scratch arena now and keep them mapped between calls (snk_ctx_reserve): a call
        that outgrows the arena otherwise pays the driver ~25-30 ms per new GB inside the call."""
        _lib.call(self.lib.snk_ctx_reserve, self._ctx, int(n_bytes))

    def release_cache(self):
        """Hand the context's cached, unused device memory back (snk_ctx_trim): for callers that change problem size and share the GPU."""
        self.lib.snk_ctx_trim(self._ctx)

    def close(self):
        if getattr(self, "_ctx", None):
            self.lib.snk_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _download(self, dptr, hptr, nbytes):
        _lib.check(self.lib.snk_dev_download(self._ctx, dptr, hptr, nbytes, self._stream()))

    def _call(self, fn, *args):
        """fn(ctx, *args, stream, err, errcap): the shape of nearly every device entry point"""
        _lib.call(fn, self._ctx, *args, self._stream())

    def _fetch(self, ptr, count, dtype) -> np.ndarray:
        """count elements of device memory as a numpy array of its own (no copy is issued for none)"""
        out = np.empty(int(count), dtype=dtype)
        if out.size:
            self._download(ptr, out.ctypes.data, out.nbytes)
        return out

    def _fetch_paths(self, p: "_lib.SnkDevPaths"):
        """-> (offset i32[n], n_edges u32[n], edges i32[sum])"""
        return self._fetch(p.offset, p.n_reads, np.int32), self._fetch(p.n_edges, p.n_reads, np.uint32), self._fetch(p.edges, p.n_edges_total, np.int32)

    def _fetch_pathsx(self, zx: "_lib.SnkDevPathsx"):
        """-> (index i64[], data u8[])"""
        return self._fetch(zx.index, zx.n_index, np.int64), self._fetch(zx.data, zx.n_bytes, np.uint8)

    # ---- the stages after the graph.  The Python face of a stage is builder, core, fetch: dev_reads / dev_paths make the input structs,
    # one core per stage takes ctypes structs (graph = n_unitigs, unitig_off, unitig_bases, byref(h)) and returns the stage's out-struct,
    # and _fetch brings down what the caller asked for.  Result.path_reads runs the same cores over the paths it has just made and adds
    # each stage's *_info to its info dict.
    def _stage(self, fn, out, *args):
        self._call(fn, *args, C.byref(out))
        return out

    def _dups(self, r, p):
        return self._stage(self.lib.snk_dev_mark_dups, _lib.SnkDevDups(), C.byref(r), C.byref(p))

    def _bads(self, K, r, graph, p, x):
        return self._stage(self.lib.snk_dev_mark_bads, _lib.SnkDevBads(), int(K), C.byref(r), *graph, C.byref(p), _lib.BADS_X if x else 0)

    def _hops(self, K, graph, inv, p, px, bc_ptr, bad_ptr, one_good, ext_host=False, ext_budget=0):
        return self._stage(self.lib.snk_dev_edge_pairs, _lib.SnkDevHops(), int(K), *graph, inv.ctypes.data, C.byref(p), C.byref(px) if px is not None else None,
                           bc_ptr, bad_ptr, (_lib.HOPS_ONE_GOOD if one_good else 0) | (_lib.HOPS_EXT_HOST if ext_host else 0), int(ext_budget))

    def _hops_info(self, hp, download):
        d = {"hops_stats": _hops_stats(hp)}
        if download:
            d["hops"] = self._fetch(hp.pairs, 2 * hp.n_pairs, np.int32).reshape(-1, 2)
        return d

    def _close(self, K, graph, inv, r, p, px, n_pairs, pairs_ptr, cg1=False, max_width=0, place_host=False, bod_budget=0):
        return self._stage(self.lib.snk_dev_close_gaps, _lib.SnkDevClosures(), int(K), *graph, inv.ctypes.data, C.byref(r), C.byref(p), C.byref(px) if px is not None else None,
                           int(n_pairs), pairs_ptr, int(max_width), (_lib.CLOSE_CG1 if cg1 else 0) | (_lib.CLOSE_PLACE_HOST if place_host else 0), int(bod_budget))

    def _close_fetch(self, cl):
        """-> (closure_off u64[n + 1], bases u8[], pair_first u64[n_pairs + 1]) on the host"""
        return (self._fetch(cl.closure_off, cl.n_closures + 1, np.uint64), self._fetch(cl.bases, cl.n_bases, np.uint8), self._fetch(cl.pair_first, cl.n_pairs + 1, np.uint64))

    def _close_info(self, cl, download):
        d = {"closures_stats": _close_stats(cl)}
        if download:
            d["closures"] = self._close_fetch(cl)
        return d

    def _pidx(self, p, n_hbv, inv):
        return self._stage(self.lib.snk_dev_paths_index, _lib.SnkDevPidx(), C.byref(p), n_hbv, inv.ctypes.data)

    def _ebcx(self, p, bc, n_hbv, inv, general):
        return self._stage(self.lib.snk_dev_edge_barcodes, _lib.SnkDevEbcx(), C.byref(p), bc.data_ptr(), n_hbv, inv.ctypes.data,
                           _lib.EBC_GENERAL_SORT if general else 0)

    def _zip(self, p, h_ref):
        return self._stage(self.lib.snk_dev_paths_zip, _lib.SnkDevPathsx(), C.byref(p), h_ref)

    def _extend(self, K, r, graph, p, back):
        return self._stage(self.lib.snk_dev_extend_paths, _lib.SnkDevExtend(), int(K), C.byref(r), *graph, C.byref(p), _lib.EXT_BACK if back else 0)

    def _dups_info(self, dd, download):
        d = dict(interdup_rate=float(dd.interdup_rate), n_dup_pairs=int(dd.n_dup_pairs), n_dup_reads=int(dd.n_dup_reads),
                 n_interdup_reads=int(dd.n_interdup_reads), n_art_pairs=int(dd.n_art_pairs), n_placed=int(dd.n_placed), ms=float(dd.ms))
        if download:
            d["dup"] = self._fetch(dd.dup, dd.n_pairs, np.uint8)
        return {"dups": d}

    def _bads_info(self, bd, download):
        got, stats = self._bads_result(bd, download)
        return {"bads": dict(stats, bad=got)} if download else {"bads": stats, "bads_dev": got}

    def _pidx_info(self, px, n_hbv, inv, download):
        d = {"pidx": dict(n_hbv_edges=n_hbv, n_entries=int(px.n_entries), n_empty_edges=int(px.n_empty_edges), key_bits=int(px.key_bits), ms=float(px.ms))}
        if download:
            d.update(paths_index=(self._fetch(px.index_off, n_hbv + 1, np.uint64), self._fetch(px.index_ids, px.n_entries, np.uint64)),
                     countsb=self._fetch(px.counts, n_hbv, np.int32), inv=inv[:n_hbv].copy())
        return d

    def _ebcx_info(self, eb, n_hbv, download):
        d = {"ebcx_stats": _ebcx_stats(eb)}
        if download:
            d["ebcx"] = (self._fetch(eb.ebc_off, n_hbv + 1, np.uint64), self._fetch(eb.ebc, eb.n_ebc, np.int32))
        return d

    def _pathsx_info(self, zx, download, prefix="", dev_key=None):
        d = {prefix + "pathsx_stats": _pathsx_stats(zx)}
        if download:
            d[prefix + "pathsx"] = self._fetch_pathsx(zx)
        elif dev_key:
            d[dev_key] = zx         # (device memory of the context, for Engine.unzip_paths)
        return d

    def _extend_info(self, xo, download):
        d = {"extend_stats": _extend_stats(xo)}
        if download:
            d["extended"] = self._fetch_paths(xo.paths)
        return d

    # ---- compressed read paths (ReadPathVecX) from and to device-resident paths
    def zip_paths(self, h: "_lib.SnkHbv", offset: torch.Tensor, n_edges: torch.Tensor, edges: torch.Tensor, start: torch.Tensor | None = None,
                  download: bool = True):
        """snk_dev_paths_zip over paths held in torch tensors on this engine's device: offset i32[n], n_edges i32[n] (read as u32), edges
        i32[sum], start i64[n + 1] (None: the paths follow each other), on the graph h (graphio.hbv_handle).  -> (index i64[], data u8[],
        stats) on the host, or with download=False (SnkDevPathsx, stats): device memory of the context, valid until its next top-level call."""
        p, start = dev_paths(offset, n_edges, edges, start)
        zx = self._zip(p, C.byref(h))
        stats = _pathsx_stats(zx)
        return (*self._fetch_pathsx(zx), stats) if download else (zx, stats)

    def unzip_paths(self, h: "_lib.SnkHbv", index, data=None, n_reads: int | None = None, download: bool = True):
        """snk_dev_paths_unzip: a ReadPathVecX on the device -- index i64[] and data u8[] as torch tensors with n_reads, or the SnkDevPathsx
        of zip_paths(download=False) -- back into paths on the graph h.  -> (offset i32[n], n_edges u32[n], edges i32[sum], ms) on the
        host; download=False: (SnkDevPaths, ms)."""
        if isinstance(index, _lib.SnkDevPathsx):
            zx = index
        else:
            zx = _lib.SnkDevPathsx()
            zx.n_reads, zx.n_bytes, zx.n_index = int(n_reads), int(data.shape[0]), int(index.shape[0])
            zx.data, zx.index = data.data_ptr(), index.data_ptr()
        out = self._stage(self.lib.snk_dev_paths_unzip, _lib.SnkDevPaths(), C.byref(zx), C.byref(h))
        return (*self._fetch_paths(out), float(out.path_ms)) if download else (out, float(out.path_ms))

    # ---- path extension (StageExtension) over device-resident reads, unitigs and paths
    def extend_paths(self, K: int, h: "_lib.SnkHbv", unitig_off: torch.Tensor, unitig_bases: torch.Tensor, rows: torch.Tensor, read_len: int,
                     quals: torch.Tensor, lens: torch.Tensor | None, offset: torch.Tensor, n_edges: torch.Tensor, edges: torch.Tensor,
                     start: torch.Tensor | None = None, back: bool = False, download: bool = True):
        """snk_dev_extend_paths -- ExtendPathsNew (10X/Extend.cc:14-177) -- over tensors on this engine's device: the unitigs of the graph h
        (graphio.hbv_handle: unitig_off i64[U + 1], unitig_bases u8[], in the order h numbers them), the reads (packed rows i32[n, words],
        quals u8[n, stride], lens i16[n] or None) and their paths (offset i32[n], n_edges i32[n] read as u32, edges i32[sum], start i64[n + 1]
        or None: the paths follow each other).  back: SNK_EXT_BACK.  -> (offset i32[n], n_edges u32[n], edges i32[sum], stats) on the host;
        download=False: (SnkDevExtend, stats), device memory of the context, valid until its next top-level call."""
        p, start = dev_paths(offset, n_edges, edges, start)
        x = self._extend(K, dev_reads(rows, read_len, quals, lens), _graph(h, unitig_off, unitig_bases), p, back)
        stats = _extend_stats(x)
        return (*self._fetch_paths(x.paths), stats) if download else (x, stats)

    # ---- MarkBads (the first step of StageFindPatch) over device-resident unitigs and paths, and reads that are resident or in the stage's files
    def _paths_struct(self, offset, n_edges, edges, start):
        return dev_paths(offset, n_edges, edges, start)

    def _bads_result(self, b: "_lib.SnkDevBads", download: bool):
        return (self._fetch(b.bad, b.n_pairs, np.uint8) if download else b), _bads_stats(b)

    def mark_bads(self, K: int, h: "_lib.SnkHbv", unitig_off: torch.Tensor, unitig_bases: torch.Tensor, rows: torch.Tensor, read_len: int,
                  quals: torch.Tensor, lens: torch.Tensor | None, offset: torch.Tensor, n_edges: torch.Tensor, edges: torch.Tensor,
                  start: torch.Tensor | None = None, x: bool = False, download: bool = True):
        """snk_dev_mark_bads -- MarkBads (10X/SecretOps.cc:70-107; x=True: the ReadPathVecX overload, :22-59, int16 offsets: what a stock DF
        writes as a.bad) -- over tensors on this engine's device, the arguments of extend_paths.  -> (bad u8[n / 2], stats) on the host;
        download=False: (SnkDevBads, stats), device memory of the context, valid until its next top-level call."""
        p, start = dev_paths(offset, n_edges, edges, start)
        return self._bads_result(self._bads(K, dev_reads(rows, read_len, quals, lens), _graph(h, unitig_off, unitig_bases), p, x), download)

    def mark_bads_df(self, K: int, h: "_lib.SnkHbv", unitig_off: torch.Tensor, unitig_bases: torch.Tensor, files, offset: torch.Tensor,
                     n_edges: torch.Tensor, edges: torch.Tensor, start: torch.Tensor | None = None, first: int = 0, n: int | None = None, read_len: int = 0,
                     threads: int = 0, slab_reads: int = 0, x: bool = False, download: bool = True):
        """snk_dev_mark_bads_df: the same over reads [first, first + n) of an opened triple (dfin.DfFiles), decoded again slab by slab -- for
        a job that kept no quality rows.  The paths are those of these reads.  first and slab_reads must be even.  Results as mark_bads."""
        n = int(n_edges.shape[0]) if n is None else int(n)
        p, start = dev_paths(offset, n_edges, edges, start)
        torch.cuda.current_stream(self.device).synchronize()          # (the call works on the ring's own stream: its inputs must be complete)
        b = _lib.SnkDevBads()
        _lib.call(self.lib.snk_dev_mark_bads_df, self._ctx, int(K), files._h, int(first), n, int(read_len), int(threads), int(slab_reads),
                  *_graph(h, unitig_off, unitig_bases), C.byref(p), _lib.BADS_X if x else 0, C.byref(b))
        return self._bads_result(b, download)

    # ---- FindEdgePairs (the second step of StageFindPatch): the edge pairs gap closing tries, a.hops
    def edge_pairs(self, K: int, h: "_lib.SnkHbv", unitig_off: torch.Tensor, unitig_bases: torch.Tensor, inv: np.ndarray, offset: torch.Tensor,
                   n_edges: torch.Tensor, edges: torch.Tensor, bc: torch.Tensor, bad: torch.Tensor, start: torch.Tensor | None = None, pidx=None,
                   one_good: bool = False, ext_host: bool = False, ext_budget: int = 0, download: bool = True):
        """snk_dev_edge_pairs -- FindEdgePairs (10X/Closomatic.cc:17-354) -- over tensors on this engine's device: the unitigs of the graph h
        (graphio.hbv_handle) and its involution inv (numpy i32[E]), the paths as for extend_paths, bc i32[n] and bad u8[n / 2] (mark_bads).
        pidx: a SnkDevPidx of these paths (the context's last paths index), or None: the index is made inside the call.  one_good:
        SNK_HOPS_ONE_GOOD; ext_host / ext_budget: where part 3's closures run (no result depends on either).  -> (pairs i32[n, 2], stats) on
        the host; download=False: (SnkDevHops, stats), device memory of the context, valid until its next top-level call."""
        p, start = dev_paths(offset, n_edges, edges, start)
        inv = np.ascontiguousarray(inv, dtype=np.int32)
        hp = self._hops(K, _graph(h, unitig_off, unitig_bases), inv, p, pidx, bc.data_ptr(), bad.data_ptr(), one_good, ext_host, ext_budget)
        return (self._hops_info(hp, True)["hops"] if download else hp), _hops_stats(hp)

    # ---- CloseGap2 / CloseGap (the third step of StageFindPatch): the closures of the pairs, closures.fastb
    def close_gaps(self, K: int, h: "_lib.SnkHbv", unitig_off: torch.Tensor, unitig_bases: torch.Tensor, inv: np.ndarray, rows: torch.Tensor, read_len: int,
                   quals: torch.Tensor, lens: torch.Tensor | None, offset: torch.Tensor, n_edges: torch.Tensor, edges: torch.Tensor, pairs: torch.Tensor,
                   start: torch.Tensor | None = None, pidx=None, cg1: bool = False, max_width: int = 0, place_host: bool = False, bod_budget: int = 0,
                   download: bool = True):
        """snk_dev_close_gaps -- CloseGap2 (cg1=True: CloseGap; 10X/Closomatic.cc:356-657) -- over tensors on this engine's device: the graph and
        inv as for edge_pairs, the reads as for mark_bads, the paths as for extend_paths, pairs i32[n_pairs, 2] (edge_pairs).  What DF writes
        as closures.fastb with STACKSTER=False.  max_width: 0 = 400.  place_host / bod_budget: where CloseGap2's partner placement runs (no
        result depends on either).  -> (closure_off u64[n + 1], bases u8[], pair_first u64[n_pairs + 1], stats) on the host: the tuple
        goes into insert_patch as its closures as it is; download=False: (SnkDevClosures, stats), device memory of the context, valid until its next
        top-level call."""
        p, start = dev_paths(offset, n_edges, edges, start)
        inv = np.ascontiguousarray(inv, dtype=np.int32)
        n_pairs = int(pairs.shape[0]) if len(pairs.shape) > 1 else int(pairs.shape[0]) // 2
        cl = self._close(K, _graph(h, unitig_off, unitig_bases), inv, dev_reads(rows, read_len, quals, lens), p, pidx, n_pairs, pairs.data_ptr(), cg1, max_width,
                         place_host, bod_budget)
        return (*self._close_fetch(cl), _close_stats(cl)) if download else (cl, _close_stats(cl))

    # ---- gap patches into the graph (StageInsertPatch)
    def insert_patch(self, graph, closures, paths) -> "PatchResult":
        """StageInsertPatch (10X/runstages/RunStages.cc:176-230) on this engine's device: pieces -> count -> merge -> hbv -> to3 / left3 ->
        translate (snk_dev_patch_pieces, snk_dev_count_graph with min_freq 1 and no barcode rule, snk_dev_patch_merge, snk_dev_hbv,
        snk_dev_patch_paths).
          graph     (K, h, unitig_off, unitig_bases): h a lib.SnkHbv of the OLD unitigs (of snk_dev_hbv, or graphio.hbv_handle), unitig_off
                    u64 / i64[U + 1] (numpy or tensor), unitig_bases u8[] (tensor on the device, or numpy), in the order h's bvcomp_order names
          closures  (off u64[n + 1] numpy, base codes u8[]: numpy or tensor on the device), or the longer tuple close_gaps returns: only these two are read
          paths     (offset i32[n], n_edges i32[n] read as u32, edges i32[sum], start i64[n + 1] or None) tensors on the device, on the old graph
        The count in the middle is a top-level call that frees everything the context handed out before, so the engine first copies what
        it was given into tensors of its own and works on those; the caller's tensors are only read.  -> PatchResult: everything in
        tensors / arrays the result owns, ready for extend_paths, zip_paths and the writers."""
        K, h_old, uoff_in, ub_in = graph
        dev = torch.device("cuda", self.device)
        own = lambda a, dt: (a.detach().to(dev, dt, copy=True) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)).contiguous()
        uoff_h = np.ascontiguousarray(uoff_in.detach().cpu().numpy() if isinstance(uoff_in, torch.Tensor) else uoff_in).astype(np.uint64)
        U_old = len(uoff_h) - 1
        ub_old = own(ub_in, torch.uint8)
        uoff_old = torch.from_numpy(uoff_h.view(np.int64)).to(dev)
        coff_h = np.ascontiguousarray(closures[0]).astype(np.uint64)
        n_cl = len(coff_h) - 1
        cb = own(closures[1], torch.uint8)
        p_off, p_n, p_edges = own(paths[0], torch.int32), own(paths[1], torch.int32), own(paths[2], torch.int32)
        n = int(p_n.shape[0])
        ip, p_start = dev_paths(p_off, p_n, p_edges, own(paths[3], torch.int64) if len(paths) > 3 and paths[3] is not None else None)
        # ---- pieces, into tensors of the engine
        plan = _lib.SnkPatchPlan()
        _lib.call(self.lib.snk_patch_plan_sizes, int(K), U_old, uoff_h.ctypes.data, C.byref(h_old), n_cl, coff_h.ctypes.data, C.byref(plan))
        n_pieces, n_lmax = int(plan.n_pieces), int(plan.n_lonely_max)
        rows = torch.empty((n_pieces, 16), dtype=torch.int32, device=dev)
        lens = torch.empty((n_pieces,), dtype=torch.int16, device=dev)
        lonely = torch.empty((max(n_lmax, 1), 2), dtype=torch.int64, device=dev)
        pc = _lib.SnkDevPieces()
        self._call(self.lib.snk_dev_patch_pieces, int(K), U_old, uoff_h.ctypes.data, ub_old.data_ptr(), C.byref(h_old), n_cl, coff_h.ctypes.data, cb.data_ptr(),
                   n_pieces, rows.data_ptr(), lens.data_ptr(), n_lmax, lonely.data_ptr(), C.byref(pc))
        # ---- the graph: the count stage on the pieces, the K-base sequences it leaves out, the ids
        if n_pieces:
            res = self.count_graph(rows, 256, lens=lens, good_len=lens, params=Params(K=int(K), min_freq=1, min_bc=0))
            raw, count_ms = res.raw, res.phase_ms["total"]
        else:
            raw, count_ms = _lib.SnkDevResult(), 0.0
        mu = _lib.SnkDevPatchUnitigs()
        self._call(self.lib.snk_dev_patch_merge, int(K), C.byref(raw), lonely.data_ptr(), int(pc.n_lonely), C.byref(mu))
        U_new, tot_new = int(mu.n_unitigs), int(mu.unitig_total_bases)
        h_new = _lib.SnkHbv()
        hbv_ms = C.c_float(0)
        self._call(self.lib.snk_dev_hbv, int(K), U_new, mu.unitig_off, mu.unitig_bases, C.byref(h_new), C.byref(hbv_ms))
        try:
            px = _lib.SnkDevPatched()
            self._call(self.lib.snk_dev_patch_paths, int(K), U_old, uoff_old.data_ptr(), ub_old.data_ptr(), C.byref(h_old), U_new, mu.unitig_off, mu.unitig_bases,
                       C.byref(h_new), C.byref(ip), C.byref(px))
            # ---- everything into memory the result owns
            def take(ptr, count, dt):
                nbytes = count * torch.empty((), dtype=dt).element_size()
                return torch.as_tensor(_DevBytes(ptr, nbytes), device=dev).clone().view(dt) if count else torch.empty((0,), dtype=dt, device=dev)
            E_old, n_to3, tot = int(px.n_old_edges), int(px.n_to3), int(px.paths.n_edges_total)
            out = PatchResult(self, int(K), h_new)
            out.unitig_off, out.unitig_bases = take(mu.unitig_off, U_new + 1, torch.int64), take(mu.unitig_bases, tot_new, torch.uint8)
            out.offset, out.n_edges, out.start, out.edges = take(px.paths.offset, n, torch.int32), take(px.paths.n_edges, n, torch.int32), \
                take(px.paths.start, n + 1, torch.int64), take(px.paths.edges, tot, torch.int32)
            out.to3_off, out.to3, out.left3 = self._fetch(px.to3_off, E_old + 1, np.uint64), self._fetch(px.to3, n_to3, np.int32), self._fetch(px.left3, E_old, np.int32)
            inv = np.zeros(max(int(h_new.n_edges), 1), np.int32)
            _lib.call(self.lib.snk_hbv_involution, C.byref(h_new), U_new, inv.ctypes.data)
            out.inv = inv[:int(h_new.n_edges)]
            out.stats = dict(n_pieces=n_pieces, n_unitig_pieces=int(plan.n_unitig_pieces), n_junctions=int(plan.n_junctions), n_closure_pieces=int(plan.n_closure_pieces),
                             n_lonely=int(pc.n_lonely), n_added=int(mu.n_added), n_first=int(px.n_first), n_later=int(px.n_later), n_cleared=int(px.n_cleared),
                             n_kmers=int(raw.n_kmers), pieces_ms=float(pc.ms), count_ms=float(count_ms), merge_ms=float(mu.ms), hbv_ms=float(hbv_ms.value),
                             map_ms=float(px.map_ms), translate_ms=float(px.paths.path_ms))
            return out
        except BaseException:
            self.lib.snk_hbv_free(C.byref(h_new))
            raise

    # ---- graph edits: DeleteEdges + Cleanup, and the hanging-end trim of StageTrim
    def _edit_input(self, graph, paths):
        """(K, h, unitig_off, unitig_bases, inv) and (offset, n_edges, edges[, start]) -> the arguments of the two edit calls and what keeps
        them alive; unitig_off / unitig_bases / the paths: tensors on the device or numpy"""
        K, h, uoff, ub, inv = graph
        dev = torch.device("cuda", self.device)
        on = lambda a, dt: (a.detach().to(dev, dt) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)).contiguous()
        uoff = on(uoff.view(np.int64) if isinstance(uoff, np.ndarray) and uoff.dtype == np.uint64 else uoff, torch.int64)
        ub = on(ub, torch.uint8)
        inv = np.ascontiguousarray(inv, dtype=np.int32)
        if len(inv) != int(h.n_edges):
            raise ValueError("inv does not have one entry per edge")
        p_off, p_n, p_edges = on(paths[0], torch.int32), on(paths[1].view(np.int32) if isinstance(paths[1], np.ndarray) else paths[1], torch.int32), on(paths[2], torch.int32)
        ip, start = dev_paths(p_off, p_n, p_edges, on(paths[3], torch.int64) if len(paths) > 3 and paths[3] is not None else None)
        return (int(K), int(uoff.shape[0]) - 1, uoff.data_ptr(), ub.data_ptr(), C.byref(h), inv.ctypes.data, C.byref(ip)), (uoff, ub, inv, p_off, p_n, p_edges, ip, start)

    def delete_edges(self, graph, paths, dels) -> "EditResult":
        """snk_dev_delete_edges -- hbv.DeleteEdgesParallel(dels) + Cleanup (paths/long/large/GapToyTools.cc:1287-1302) -- on this engine's device.
          graph  (K, h, unitig_off, unitig_bases, inv): h a lib.SnkHbv (snk_dev_hbv, graphio.hbv_handle, an EditResult's), the unitigs in the
                 order h names them, inv numpy i32[E]; an EditResult's .graph
          paths  (offset i32[n], n_edges i32[n] read as u32, edges i32[sum], start i64[n + 1] or None); an EditResult's .paths
          dels   edge ids, any order, duplicates allowed, closed under inv
        The caller's arrays are only read.  -> EditResult: everything in tensors / arrays the result owns."""
        args, hold = self._edit_input(graph, paths)
        dels = np.ascontiguousarray(dels, dtype=np.int32).ravel()
        raw = _lib.SnkDevEdit()
        self._call(self.lib.snk_dev_delete_edges, *args, dels.ctypes.data, len(dels), 0, C.byref(raw))
        try:
            dev = torch.device("cuda", self.device)

            def take(ptr, count, dt):
                nbytes = count * torch.empty((), dtype=dt).element_size()
                return torch.as_tensor(_DevBytes(ptr, nbytes), device=dev).clone().view(dt) if count else torch.empty((0,), dtype=dt, device=dev)
            return EditResult(self, args[0], raw, take)
        finally:
            self.lib.snk_dev_edit_free(C.byref(raw))
            del hold

    def hanging_ends(self, graph, paths, max_kmers: int = 200, leg: str | None = None):
        """snk_dev_hanging_ends -- the selection of StageTrim (10X/runstages/RunStages.cc:91-146): the read support of every edge and the
        unsupported hanging ends of at most max_kmers k-mers, with their inverses.  graph / paths as for delete_edges.  leg: None (the call
        chooses by size), "lds" or "sort" (tests).  -> (support i32[E], dels i32[] ascending, stats) on the host."""
        args, hold = self._edit_input(graph, paths)
        flags = {None: 0, "lds": _lib.HANG_LDS, "sort": _lib.HANG_SORT}[leg]
        raw = _lib.SnkDevHanging()
        self._call(self.lib.snk_dev_hanging_ends, *args, int(max_kmers), flags, C.byref(raw))
        try:
            support = self._fetch(raw.support, raw.n_hbv_edges, np.int32)
            dels = np.array(np.ctypeslib.as_array(raw.dels, shape=(int(raw.n_dels),)), dtype=np.int32, copy=True) if raw.n_dels else np.zeros(0, np.int32)
            return support, dels, dict(n_dels=int(raw.n_dels), n_unsupported=int(raw.n_unsupported), n_entries=int(raw.n_entries),
                                       leg={_lib.HANG_LDS: "lds", _lib.HANG_SORT: "sort"}[int(raw.leg)], ms=float(raw.ms))
        finally:
            self.lib.snk_host_free(C.cast(raw.dels, C.c_void_p))
            del hold

    def trim_hanging_ends(self, graph, paths, max_kmers: int = 200) -> "EditResult":
        """StageTrim from line 91 on: hanging_ends, then delete_edges with its selection.  stats gains the selection's."""
        support, dels, hs = self.hanging_ends(graph, paths, max_kmers)
        out = self.delete_edges(graph, paths, dels)
        out.stats.update(hang_dels=len(dels), hang_unsupported=hs["n_unsupported"], hang_leg=hs["leg"], hang_ms=hs["ms"])
        out.support, out.dels = support, dels
        return out

    # ---- MowLawn, and StageTrim as one call
    def mow_lawn(self, graph, rows: torch.Tensor, read_len: int, quals: torch.Tensor, lens: torch.Tensor | None, paths, dup, download: bool = True):
        """snk_dev_mow_lawn -- MowLawn (10X/Lawnmower.cc:301-554, the ReadPathVecX overload StageTrim calls): the weak-branch rule that picks
        StageTrim's first batch of deletions.  graph / paths as for delete_edges (an EditResult's .graph and .paths are taken as they are);
        the reads as for mark_bads (packed rows i32[n, words], quals u8[n, stride], lens i16[n] or None), reads 2q and 2q + 1 mates; dup
        u8[n / 2], a tensor on the device or numpy: what MarkDups gave (path_reads(mark_dups=True), or the "dup" of stage_trim's stats).
        -> (dels i32[] ascending, scored i32[n, 4] = (e1, e2, qss1, qss2) ascending by (e2, e1), stats); download=False leaves scored out
        (None)."""
        args, hold = self._edit_input(graph, paths)
        dev = torch.device("cuda", self.device)
        d_dup = (dup.detach().to(dev, torch.uint8) if isinstance(dup, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dup, dtype=np.uint8)).to(dev)).contiguous()
        if int(d_dup.shape[0]) != int(rows.shape[0]) // 2:
            raise ValueError("dup does not have one entry per pair")
        r = dev_reads(rows, read_len, quals, lens)
        raw = _lib.SnkDevMow()
        self._call(self.lib.snk_dev_mow_lawn, *args[:-1], C.byref(r), args[-1], d_dup.data_ptr() if int(d_dup.shape[0]) else None, 0, C.byref(raw))
        try:
            dels = np.array(np.ctypeslib.as_array(raw.dels, shape=(int(raw.n_dels),)), dtype=np.int32, copy=True) if raw.n_dels else np.zeros(0, np.int32)
            scored = self._fetch(raw.scored, 4 * raw.n_scored, np.int32).reshape(-1, 4) if download else None
            stats = {k: int(getattr(raw, k)) for k in _lib.MOW_COUNTERS}
            stats.update(n_dels=int(raw.n_dels), n_scored=int(raw.n_scored), ms=float(raw.ms), tables_ms=float(raw.tables_ms),
                         phase_ms={k: float(raw.phase_ms[i]) for i, k in enumerate(_lib.MOW_PHASES)})
            return dels, scored, stats
        finally:
            self.lib.snk_host_free(C.cast(raw.dels, C.c_void_p))
            del hold, d_dup

    def stage_trim(self, graph, rows: torch.Tensor, read_len: int, quals: torch.Tensor, lens: torch.Tensor | None, bc: torch.Tensor, paths, max_kmers: int = 200) -> "EditResult":
        """StageTrim (10X/runstages/RunStages.cc:56-156) as one call: MarkDups, mow_lawn, delete_edges with its selection, hanging_ends on
        that result, delete_edges again.  graph / paths as for delete_edges, the reads as for mow_lawn, bc i32[n] the raw barcode ids.
        -> the EditResult of the second edit.  Its stats carry both selections -- mow_dels, mow (the counters and times of mow_lawn),
        first (the first edit's stats), hang_dels, hang_unsupported, hang_leg, hang_ms -- and dups; the result also has .dup (u8 per pair),
        .scored, .mow_dels, .support and .dels (the second round's) as arrays.  The stage's a.pathsX is zip_paths(result.h, *result.paths).
        MarkDups here is the one the library has (the ReadPath form, 10X/SecretOps.cc:413-593); the reference's StageTrim calls version 2
        (:599), which reads the offsets through the ReadPathVecX -- the two agree on every fixture under tests/golden/mow/."""
        args, hold = self._edit_input(graph, paths)
        ip = hold[6]
        dd = self._dups(dev_reads(rows, read_len, quals, lens, bc=bc), ip)
        dup = self._fetch(dd.dup, dd.n_pairs, np.uint8)
        dups = self._dups_info(dd, False)["dups"]
        del hold
        mow_dels, scored, ms = self.mow_lawn(graph, rows, read_len, quals, lens, paths, dup)
        first = self.delete_edges(graph, paths, mow_dels)
        out = self.trim_hanging_ends(first.graph, first.paths, max_kmers)
        out.stats.update(mow_dels=len(mow_dels), mow=ms, first=first.stats, dups=dups)
        out.dup, out.scored, out.mow_dels = dup, scored, mow_dels
        return out

    # ---- synthetic reads straight into HBM
    def synth(self, sp: _lib.SnkSynthParams, first: int = 0, n: int | None = None, qstride: int | None = None):
        n = sp.n_reads - first if n is None else n
        rw = (sp.read_len + 15) // 16
        qs = qstride or ((sp.read_len + 15) // 16 * 16)
        dev = torch.device("cuda", self.device)
        rows = torch.empty((n, rw), dtype=torch.int32, device=dev)
        quals = torch.empty((n, qs), dtype=torch.uint8, device=dev)
        bc = torch.empty((n,), dtype=torch.int32, device=dev)
        _lib.check(self.lib.snk_synth_dev(self._ctx, C.byref(sp), first, n, rows.data_ptr(), rw, quals.data_ptr(), qs,
                                          bc.data_ptr(), self._stream()))
        return rows, quals, bc

    def trim(self, quals: torch.Tensor, read_len: int, K: int = 48, min_qual: int = 7, lens: torch.Tensor | None = None):
        n, qs = quals.shape
        out = torch.empty((n,), dtype=torch.int16, device=quals.device)
        _lib.check(self.lib.snk_dev_trim(self._ctx, quals.data_ptr(), qs, lens.data_ptr() if lens is not None else None,
                                         read_len, n, K, min_qual, out.data_ptr(), self._stream()))
        return out

    def pack_ascii(self, ascii_rows: torch.Tensor, read_len: int):
        n, stride = ascii_rows.shape
        rw = (read_len + 15) // 16
        rows = torch.empty((n, rw), dtype=torch.int32, device=ascii_rows.device)
        _lib.check(self.lib.snk_dev_pack_ascii(self._ctx, ascii_rows.data_ptr(), stride, read_len, n, rows.data_ptr(), rw,
                                               self._stream()))
        return rows

    def count_graph(self, rows: torch.Tensor, read_len: int, quals: torch.Tensor | None = None,
                    bc: torch.Tensor | None = None, lens: torch.Tensor | None = None,
                    good_len: torch.Tensor | None = None, params: Params | None = None, ign_bc_below: int = 0,
                    read_index_base: int = 0, group: torch.Tensor | None = None) -> Result:
        params = params or Params()
        assert rows.is_cuda and rows.dtype == torch.int32 and rows.is_contiguous()
        if lens is not None:
            assert lens.dtype == torch.int16 and lens.is_cuda
        if quals is not None:
            assert quals.dtype == torch.uint8 and quals.is_cuda and quals.is_contiguous()
        if good_len is not None:
            assert good_len.dtype == torch.int16 and good_len.is_cuda
        if bc is not None:
            assert bc.dtype == torch.int32 and bc.is_cuda
        if group is not None:
            assert group.dtype == torch.int32 and group.is_cuda and group.is_contiguous()
        return self.count_graph_reads(dev_reads(rows, read_len, quals, lens, good_len, bc, group, ign_bc_below, read_index_base), params)

    # ---- streamed input: the job's reads arrive slab by slab (snk_dev_stream_begin / _append / _finish)
    def stream_begin(self, read_len: int, total_reads_ub: int, has_bc: bool = True, params: Params | None = None):
        self._stream_params = params or Params()
        p = self._stream_params.to_c()
        self._call(self.lib.snk_dev_stream_begin, C.byref(p), int(read_len), int(total_reads_ub), 1 if has_bc else 0)

    def stream_append(self, rows: torch.Tensor, read_len: int, quals: torch.Tensor | None = None, bc: torch.Tensor | None = None,
                      lens: torch.Tensor | None = None, good_len: torch.Tensor | None = None, ign_bc_below: int = 0, read_index_base: int = 0):
        """One slab (asynchronous: its tensors must stay alive until the engine's stream has passed the call)."""
        assert rows.is_cuda and rows.dtype == torch.int32 and rows.is_contiguous()
        if quals is not None:
            assert quals.dtype == torch.uint8 and quals.is_cuda and quals.is_contiguous()
        self.stream_append_reads(dev_reads(rows, read_len, quals, lens, good_len, bc, None, ign_bc_below, read_index_base))

    def stream_append_reads(self, r: "_lib.SnkDevReads"):
        self._call(self.lib.snk_dev_stream_append, C.byref(r))

    def stream_finish(self) -> Result:
        raw = _lib.SnkDevResult()
        self._call(self.lib.snk_dev_stream_finish, C.byref(raw))
        return Result(self, raw, self._stream_params.K, self._stream_params)

    def count_graph_reads(self, r: "_lib.SnkDevReads", params: Params | None = None) -> Result:
        """The same for reads described by plain device pointers (e.g. the arrays of snk_dev_ingest_fasth)."""
        params = params or Params()
        p = params.to_c()
        raw = _lib.SnkDevResult()
        self._call(self.lib.snk_dev_count_graph, C.byref(r), C.byref(p), C.byref(raw))
        return Result(self, raw, params.K, params)

    # ---- the graph verifier (snk_dev_check_graph)
    def check_graph_ptrs(self, K: int, flags: int, min_freq: int, n_kmers: int, keys, counts, ctx, n_unitigs: int, unitig_off, unitig_bases,
                         unitig_group=None, n_instances: int = 0, reads: "_lib.SnkDevReads | None" = None, min_qual: int = 7) -> dict:
        """snk_dev_check_graph over plain device pointers; the report as a dict (lib.SnkCheckReport.to_dict)."""
        ci = _lib.SnkCheckInput()
        ci.K, ci.flags, ci.min_freq, ci.min_qual, ci.n_instances = K, flags, min_freq, min_qual, n_instances
        ci.n_kmers, ci.keys, ci.counts, ci.ctx = n_kmers, keys, counts, ctx
        ci.n_unitigs, ci.unitig_off, ci.unitig_bases, ci.unitig_group = n_unitigs, unitig_off, unitig_bases, unitig_group
        rep = _lib.SnkCheckReport()
        rep.struct_size = C.sizeof(_lib.SnkCheckReport)
        self._call(self.lib.snk_dev_check_graph, C.byref(ci), C.byref(reads) if reads is not None else None, C.byref(rep))
        return rep.to_dict()

    def check_graph(self, keys: torch.Tensor, counts: torch.Tensor, ctx: torch.Tensor, unitig_off: torch.Tensor, unitig_bases: torch.Tensor,
                    K: int = 48, min_freq: int = 3, unitig_group: torch.Tensor | None = None, sorted_table: bool = True, ordered: bool = True,
                    digest_only: bool = False, n_instances: int = 0, reads: "_lib.SnkDevReads | None" = None, min_qual: int = 7) -> dict:
        """The verifier over device tensors (any producer's arrays, or a corrupted copy): keys [n, 2] int64/uint64 {lo, hi} (or n*16 bytes),
        counts u32/int32 [n], ctx u8 [n], unitig_off [U + 1] 64-bit, unitig_bases u8, unitig_group 32-bit [U] for a grouped run."""
        for t in (keys, counts, ctx, unitig_off, unitig_bases) + ((unitig_group,) if unitig_group is not None else ()):
            assert t.is_cuda and t.is_contiguous()
        n_kmers = keys.numel() * keys.element_size() // 16
        assert counts.numel() == n_kmers and ctx.numel() == n_kmers and counts.element_size() == 4 and ctx.element_size() == 1
        assert unitig_off.element_size() == 8 and unitig_bases.element_size() == 1
        U = unitig_off.numel() - 1
        flags = ((_lib.CHECK_SORTED_TABLE if sorted_table else 0) | (_lib.CHECK_ORDERED if ordered else 0)
                 | (_lib.CHECK_GROUPED if unitig_group is not None else 0) | (_lib.CHECK_DIGEST_ONLY if digest_only else 0))
        return self.check_graph_ptrs(K, flags, min_freq, n_kmers, keys.data_ptr(), counts.data_ptr(), ctx.data_ptr(), max(U, 0),
                                     unitig_off.data_ptr(), unitig_bases.data_ptr(),
                                     unitig_group.data_ptr() if unitig_group is not None else None, n_instances, reads, min_qual)
