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

PHASES = ("trim", "plan", "partition", "count", "sort", "graph", "-", "total")


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
        out = np.empty(shape, dtype=dtype)
        if nbytes:
            self._e._download(ptr, out.ctypes.data, nbytes)
        return out

    def good_len(self) -> np.ndarray:
        return self._dl(self.raw.good_len, self.n_reads * 2, np.uint16, (self.n_reads,))

    def keys(self) -> np.ndarray:
        """[n_kmers, 4] u32 words MSB-first (include/snk.h key convention), ascending."""
        lohi = self._dl(self.raw.keys, self.n_kmers * 16, np.uint64, (self.n_kmers, 2))
        lo, hi = lohi[:, 0], lohi[:, 1]
        w = np.empty((self.n_kmers, 4), dtype=np.uint32)
        w[:, 0] = hi >> np.uint64(32)
        w[:, 1] = hi & np.uint64(0xFFFFFFFF)
        w[:, 2] = lo >> np.uint64(32)
        w[:, 3] = lo & np.uint64(0xFFFFFFFF)
        return w

    def counts(self) -> np.ndarray:
        return self._dl(self.raw.counts, self.n_kmers * 4, np.uint32, (self.n_kmers,))

    def ctx(self) -> np.ndarray:
        return self._dl(self.raw.ctx, self.n_kmers, np.uint8, (self.n_kmers,))

    def spectrum(self) -> np.ndarray:
        nb = int(self.raw.spectrum_bins)
        return self._dl(self.raw.spectrum, nb * 8, np.uint64, (nb,))

    def unitig_arrays(self):
        off = self._dl(self.raw.unitig_off, (self.n_unitigs + 1) * 8, np.uint64, (self.n_unitigs + 1,))
        bases = self._dl(self.raw.unitig_bases, self.unitig_total_bases, np.uint8, (self.unitig_total_bases,))
        return off, bases

    def unitig_groups(self) -> np.ndarray:
        """Grouped runs: group id of every unitig (same order as unitig_arrays())."""
        return self._dl(self.raw.unitig_group, self.n_unitigs * 4, np.uint32, (self.n_unitigs,))

    def bv_image_device(self):
        """a13 on the device: (device pointer, bytes) of the .bv hand-off file -- "BINWRITE", count, per unitig u32 length + 2-bit bases in
        BVComp order (snk_dev_bv_image).  Context memory: valid until the engine's next top-level call."""
        ptr, nb = C.c_void_p(0), C.c_uint64(0)
        err = C.create_string_buffer(512)
        rc = self._e.lib.snk_dev_bv_image(self._e._ctx, int(self.K), self.n_unitigs, self.raw.unitig_off, self.raw.unitig_bases, 1,
                                          C.byref(ptr), C.byref(nb), self._e._stream(), err, 512)
        if rc:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
        return ptr.value, int(nb.value)

    def bv_image(self) -> bytes:
        ptr, nb = self.bv_image_device()
        return self._dl(ptr, nb, np.uint8, (nb,)).tobytes()

    def hbv(self) -> dict:
        """The graph from the device-resident unitigs (buildHBVFromEdges, HBVFromEdges.cc:244-296; snk_dev_hbv):
        vertex ids per HBV edge, fwd/rev translation per unitig, numbered in BVComp order; 'order'[r] = index of the
        rank-r unitig in unitig_arrays().  Must be called before the engine's next count_graph."""
        h = _lib.SnkHbv()
        ms = C.c_float(0)
        err = C.create_string_buffer(512)
        rc = self._e.lib.snk_dev_hbv(self._e._ctx, int(self.K), self.n_unitigs, self.raw.unitig_off, self.raw.unitig_bases,
                                     C.byref(h), C.byref(ms), self._e._stream(), err, 512)
        if rc:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
        ne, nu = h.n_edges, self.n_unitigs
        arr = lambda p, m, dt: (np.array(np.ctypeslib.as_array(p, shape=(m,)), dtype=dt, copy=True) if m else np.zeros(0, dt))      # (one copy: the C arrays are freed below)
        out = dict(n_vertices=h.n_vertices, n_edges=ne, v_left=arr(h.v_left, ne, np.int32), v_right=arr(h.v_right, ne, np.int32),
                   src=arr(h.src_unitig, ne, np.int32), is_rc=arr(h.is_rc, ne, np.uint8), fwd=arr(h.fwd_xlat, nu, np.int32),
                   rev=arr(h.rev_xlat, nu, np.int32), order=arr(h.bvcomp_order, nu, np.int32), device_ms=float(ms.value))
        self._e.lib.snk_hbv_free(C.byref(h))
        return out

    def path_reads(self, rows, read_len: int, quals, lens=None, mark_dups=False, bc=None, unitig_bcs=False, download=True, bcs_nocut=False,
                   paths_index=False, pathsx=False, ebcx=False, extend=False, mark_bads=False):
        """f1: the reads (untrimmed packed rows + quality rows on the device) onto the graph of this result's unitigs --
        pathReads with the new aligner (BuildReadQGraph48.cc:1441-1469).  Returns (offset i32[n], n_edges u32[n], edges i32[sum],
        info) on the host, HBV edge ids as numbered by buildHBVFromEdges.  Must be called before the engine's next count_graph.
        mark_dups: f4, MarkDups over these paths (10X/SecretOps.cc:413-593; bc = raw barcode ids on the device or None) ->
        info['dups'] = dict(dup u8[n/2], interdup_rate, n_dup_pairs, n_dup_reads, n_art_pairs, n_placed, ms).
        unitig_bcs: the rest of f4 -- per unitig (numbering of unitig_arrays()) the sorted distinct barcodes > 0 of the reads with a
        k-mer on it (tada's edge -> barcode sets) -> info['unitig_bcs'] = (off u64[U+1], bcs u32[...]); unitig_bcs="exhaustive" derives them
        the slow, literal way (every k-mer of every barcoded read looked up); bcs_nocut: without the 20 000-entry cut.
        info['retries']: the lists that overflowed and were regrown (snk_dev_paths.retries: 1 redo list, 2 path edges, 4 barcode keys).
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
        info['bads_dev'] = the SnkDevBads itself (device memory of the context, valid until the engine's next count_graph or path_reads)."""
        if ebcx and bc is None:
            raise ValueError("path_reads(ebcx=...) needs bc: the barcode of every read, on the device")
        e = self._e
        h = _lib.SnkHbv()
        ms = C.c_float(0)
        err = C.create_string_buffer(512)
        rc = e.lib.snk_dev_hbv(e._ctx, int(self.K), self.n_unitigs, self.raw.unitig_off, self.raw.unitig_bases, C.byref(h), C.byref(ms),
                               e._stream(), err, 512)
        if rc:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
        try:
            r = _lib.SnkDevReads()
            r.n_reads, r.rows, r.row_words, r.read_len = rows.shape[0], rows.data_ptr(), rows.shape[1], read_len
            r.quals, r.qstride = quals.data_ptr(), quals.shape[1]
            if lens is not None:
                r.lens = lens.data_ptr()
            out = _lib.SnkDevPaths()
            if unitig_bcs and bc is not None:
                r.bc = bc.data_ptr()
            rc = e.lib.snk_dev_path_reads2(e._ctx, int(self.K), C.byref(r), self.n_unitigs, self.raw.unitig_off, self.raw.unitig_bases,
                                           C.byref(h), (0 if not unitig_bcs else 1 | (2 if unitig_bcs == "exhaustive" else 0) | (4 if bcs_nocut else 0)), C.byref(out), e._stream(), err, 512)
            if rc:
                raise _lib.SnkError(rc, err.value.decode(errors="replace"))
            dups = None
            if mark_dups:
                if bc is not None:
                    r.bc = bc.data_ptr()
                dd = _lib.SnkDevDups()
                rc = e.lib.snk_dev_mark_dups(e._ctx, C.byref(r), C.byref(out), C.byref(dd), e._stream(), err, 512)
                if rc:
                    raise _lib.SnkError(rc, err.value.decode(errors="replace"))
                npairs = int(dd.n_pairs)
                dups = dict(dup=self._dl(dd.dup, npairs, np.uint8, (npairs,)) if download else None, interdup_rate=float(dd.interdup_rate),
                            n_dup_pairs=int(dd.n_dup_pairs), n_dup_reads=int(dd.n_dup_reads), n_interdup_reads=int(dd.n_interdup_reads),
                            n_art_pairs=int(dd.n_art_pairs), n_placed=int(dd.n_placed), ms=float(dd.ms))
            bads = None
            if mark_bads:
                bd = _lib.SnkDevBads()
                rc = e.lib.snk_dev_mark_bads(e._ctx, int(self.K), C.byref(r), self.n_unitigs, self.raw.unitig_off, self.raw.unitig_bases, C.byref(h), C.byref(out),
                                             _lib.BADS_X if mark_bads == "x" else 0, C.byref(bd), e._stream(), err, 512)
                if rc:
                    raise _lib.SnkError(rc, err.value.decode(errors="replace"))
                bads = _bads_stats(bd)
                if download:
                    bads["bad"] = self._dl(bd.bad, int(bd.n_pairs), np.uint8, (int(bd.n_pairs),))
            pidx = None
            if paths_index:
                ne_hbv = int(h.n_edges)
                inv = np.zeros(max(ne_hbv, 1), dtype=np.int32)
                rc = e.lib.snk_hbv_involution(C.byref(h), self.n_unitigs, inv.ctypes.data, err, 512)
                px = _lib.SnkDevPidx()
                if not rc:
                    rc = e.lib.snk_dev_paths_index(e._ctx, C.byref(out), ne_hbv, inv.ctypes.data, C.byref(px), e._stream(), err, 512)
                if rc:
                    raise _lib.SnkError(rc, err.value.decode(errors="replace"))
                nent = int(px.n_entries)
                pidx = dict(n_hbv_edges=ne_hbv, n_entries=nent, n_empty_edges=int(px.n_empty_edges), key_bits=int(px.key_bits), ms=float(px.ms))
                if download:
                    pidx_arrays = (self._dl(px.index_off, (ne_hbv + 1) * 8, np.uint64, (ne_hbv + 1,)), self._dl(px.index_ids, nent * 8, np.uint64, (nent,)),
                                   self._dl(px.counts, ne_hbv * 4, np.int32, (ne_hbv,)), inv[:ne_hbv].copy())
            eb_stats = None
            if ebcx:
                ne_hbv = int(h.n_edges)
                inv = np.zeros(max(ne_hbv, 1), dtype=np.int32)
                rc = e.lib.snk_hbv_involution(C.byref(h), self.n_unitigs, inv.ctypes.data, err, 512)
                eb = _lib.SnkDevEbcx()
                if not rc:
                    rc = e.lib.snk_dev_edge_barcodes(e._ctx, C.byref(out), bc.data_ptr(), ne_hbv, inv.ctypes.data,
                                                     _lib.EBC_GENERAL_SORT if ebcx == "general" else 0, C.byref(eb), e._stream(), err, 512)
                if rc:
                    raise _lib.SnkError(rc, err.value.decode(errors="replace"))
                eb_stats = _ebcx_stats(eb)
                if download:
                    eb_arrays = (self._dl(eb.ebc_off, (ne_hbv + 1) * 8, np.uint64, (ne_hbv + 1,)), self._dl(eb.ebc, int(eb.n_ebc) * 4, np.int32, (int(eb.n_ebc),)))
            px_stats = None
            if pathsx:
                zx = _lib.SnkDevPathsx()
                rc = e.lib.snk_dev_paths_zip(e._ctx, C.byref(out), C.byref(h), C.byref(zx), e._stream(), err, 512)
                if rc:
                    raise _lib.SnkError(rc, err.value.decode(errors="replace"))
                px_stats = _pathsx_stats(zx)
                if download:
                    px_arrays = (self._dl(zx.index, int(zx.n_index) * 8, np.int64, (int(zx.n_index),)), self._dl(zx.data, int(zx.n_bytes), np.uint8, (int(zx.n_bytes),)))
            ext_stats = None
            if extend:
                xo = _lib.SnkDevExtend()
                rc = e.lib.snk_dev_extend_paths(e._ctx, int(self.K), C.byref(r), self.n_unitigs, self.raw.unitig_off, self.raw.unitig_bases, C.byref(h),
                                                C.byref(out), _lib.EXT_BACK if extend == "back" else 0, C.byref(xo), e._stream(), err, 512)
                if rc:
                    raise _lib.SnkError(rc, err.value.decode(errors="replace"))
                ext_stats = _extend_stats(xo)
                xp = xo.paths
                if download:
                    xn, xt = int(xp.n_reads), int(xp.n_edges_total)
                    ext_arrays = (self._dl(xp.offset, xn * 4, np.int32, (xn,)), self._dl(xp.n_edges, xn * 4, np.uint32, (xn,)), self._dl(xp.edges, xt * 4, np.int32, (xt,)))
                ext_px_stats = None
                if pathsx:
                    zx2 = _lib.SnkDevPathsx()
                    rc = e.lib.snk_dev_paths_zip(e._ctx, C.byref(xp), C.byref(h), C.byref(zx2), e._stream(), err, 512)
                    if rc:
                        raise _lib.SnkError(rc, err.value.decode(errors="replace"))
                    ext_px_stats = _pathsx_stats(zx2)
                    if download:
                        ext_px_arrays = (self._dl(zx2.index, int(zx2.n_index) * 8, np.int64, (int(zx2.n_index),)),
                                         self._dl(zx2.data, int(zx2.n_bytes), np.uint8, (int(zx2.n_bytes),)))
        finally:
            e.lib.snk_hbv_free(C.byref(h))
        n, tot = int(out.n_reads), int(out.n_edges_total)
        if not download:          # timings only (bench.py: the results stay on the device)
            info = dict(dict_ms=float(out.dict_ms), path_ms=float(out.path_ms), bcs_ms=float(out.bcs_ms), hbv_device_ms=float(ms.value),
                        dict_slots=int(out.dict_slots), n_edges_total=tot, n_unitig_bcs=int(out.n_unitig_bcs), n_slow=int(out.n_slow),
                        lookup=("index" if out.lookup_index else "kmer_dictionary"), retries=int(out.retries))
            if dups is not None:
                info["dups"] = {k: v for k, v in dups.items() if k != "dup"}
            if bads is not None:
                info["bads"], info["bads_dev"] = bads, bd
            if pidx is not None:
                info["pidx"] = pidx
            if px_stats is not None:
                info["pathsx_stats"], info["pathsx_dev"] = px_stats, zx     # (zx: device memory of the context, for Engine.unzip_paths)
            if eb_stats is not None:
                info["ebcx_stats"] = eb_stats
            if ext_stats is not None:
                info["extend_stats"] = ext_stats
                if ext_px_stats is not None:
                    info["extended_pathsx_stats"] = ext_px_stats
            return None, None, None, info
        off = self._dl(out.offset, n * 4, np.int32, (n,))
        ne = self._dl(out.n_edges, n * 4, np.uint32, (n,))
        edges = self._dl(out.edges, tot * 4, np.int32, (tot,))
        info = dict(dict_ms=float(out.dict_ms), path_ms=float(out.path_ms), bcs_ms=float(out.bcs_ms), hbv_device_ms=float(ms.value), dict_slots=int(out.dict_slots), lookup=("index" if out.lookup_index else "kmer_dictionary"),
                    n_slow=int(out.n_slow), retries=int(out.retries))
        if dups is not None:
            info["dups"] = dups
        if bads is not None:
            info["bads"] = bads
        if pidx is not None:
            info["pidx"], info["paths_index"], info["countsb"], info["inv"] = pidx, pidx_arrays[:2], pidx_arrays[2], pidx_arrays[3]
        if px_stats is not None:
            info["pathsx"], info["pathsx_stats"] = px_arrays, px_stats
        if eb_stats is not None:
            info["ebcx"], info["ebcx_stats"] = eb_arrays, eb_stats
        if ext_stats is not None:
            info["extended"], info["extend_stats"] = ext_arrays, ext_stats
            if ext_px_stats is not None:
                info["extended_pathsx"], info["extended_pathsx_stats"] = ext_px_arrays, ext_px_stats
        if unitig_bcs and out.unitig_bc_off:
            nb = int(out.n_unitig_bcs)
            info["unitig_bcs"] = (self._dl(out.unitig_bc_off, (self.n_unitigs + 1) * 8, np.uint64, (self.n_unitigs + 1,)),
                                  self._dl(out.unitig_bcs, nb * 4, np.uint32, (nb,)))
        return off, ne, edges, info

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
        err = C.create_string_buffer(512)
        h = _lib.SnkHbv.from_buffer_copy(self.h)
        h.bvcomp_order = None
        rc = self._e.lib.snk_write_hbv(str(path_hbv).encode(), str(path_inv).encode() if path_inv else None, self.K, len(off) - 1, off.ctypes.data, bases.ctypes.data,
                                       C.byref(h), err, 512)
        if not rc and path_hbx:
            rc = self._e.lib.snk_write_hbx(str(path_hbx).encode(), self.K, len(off) - 1, off.ctypes.data, bases.ctypes.data, C.byref(h), err, 512)
        if rc:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))


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
        err = C.create_string_buffer(512)
        rc = self.lib.snk_ctx_create(self.device, C.byref(h), err, 512)
        if rc != 0:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
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
        err = C.create_string_buffer(512)
        rc = self.lib.snk_ctx_set_option(self._ctx, name.encode(), int(value), err, 512)
        if rc != 0:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))

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
        err = C.create_string_buffer(512)
        rc = self.lib.snk_ctx_set_tuning(self._ctx, C.byref(t), err, 512)
        if rc != 0:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))

    def get_tuning(self) -> dict:
        """What is pinned (0 = the library chooses) and, in last_*, what the context's last call ran with."""
        t = _lib.SnkTuning()
        self.lib.snk_ctx_get_tuning(self._ctx, C.byref(t))
        return {k: int(getattr(t, k)) for k, _ in _lib.SnkTuning._fields_ if k != "reserved"}

    def reserve(self, n_bytes: int):
        """Map n_bytes of device memory into the context's scratch arena now and keep them mapped between calls (snk_ctx_reserve): a call
        that outgrows the arena otherwise pays the driver ~25-30 ms per new GB inside the call."""
        err = C.create_string_buffer(512)
        rc = self.lib.snk_ctx_reserve(self._ctx, int(n_bytes), err, 512)
        if rc != 0:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))

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

    # ---- compressed read paths (ReadPathVecX) from and to device-resident paths
    def zip_paths(self, h: "_lib.SnkHbv", offset: torch.Tensor, n_edges: torch.Tensor, edges: torch.Tensor, start: torch.Tensor | None = None,
                  download: bool = True):
        """snk_dev_paths_zip over paths held in torch tensors on this engine's device: offset i32[n], n_edges i32[n] (read as u32), edges
        i32[sum], start i64[n + 1] (None: the paths follow each other), on the graph h (graphio.hbv_handle).  -> (index i64[], data u8[],
        stats) on the host, or with download=False (SnkDevPathsx, stats): device memory of the context, valid until its next top-level call."""
        n = int(n_edges.shape[0])
        if start is None:
            start = torch.zeros(n + 1, dtype=torch.int64, device=n_edges.device)
            start[1:] = torch.cumsum(n_edges.to(torch.int64) & 0xFFFFFFFF, 0)
        p = _lib.SnkDevPaths()
        p.n_reads, p.n_edges_total = n, int(edges.shape[0])
        p.offset, p.n_edges, p.start, p.edges = offset.data_ptr(), n_edges.data_ptr(), start.data_ptr(), edges.data_ptr()
        zx = _lib.SnkDevPathsx()
        err = C.create_string_buffer(512)
        rc = self.lib.snk_dev_paths_zip(self._ctx, C.byref(p), C.byref(h), C.byref(zx), self._stream(), err, 512)
        if rc:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
        stats = _pathsx_stats(zx)
        if not download:
            return zx, stats
        index = np.empty(int(zx.n_index), np.int64)
        data = np.empty(int(zx.n_bytes), np.uint8)
        if index.size:
            self._download(zx.index, index.ctypes.data, index.nbytes)
        if data.size:
            self._download(zx.data, data.ctypes.data, data.nbytes)
        return index, data, stats

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
        out = _lib.SnkDevPaths()
        err = C.create_string_buffer(512)
        rc = self.lib.snk_dev_paths_unzip(self._ctx, C.byref(zx), C.byref(h), C.byref(out), self._stream(), err, 512)
        if rc:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
        if not download:
            return out, float(out.path_ms)
        n, tot = int(out.n_reads), int(out.n_edges_total)
        off, ne, edges = np.empty(n, np.int32), np.empty(n, np.uint32), np.empty(tot, np.int32)
        for a, ptr in ((off, out.offset), (ne, out.n_edges), (edges, out.edges)):
            if a.size:
                self._download(ptr, a.ctypes.data, a.nbytes)
        return off, ne, edges, float(out.path_ms)

    # ---- path extension (StageExtension) over device-resident reads, unitigs and paths
    def extend_paths(self, K: int, h: "_lib.SnkHbv", unitig_off: torch.Tensor, unitig_bases: torch.Tensor, rows: torch.Tensor, read_len: int,
                     quals: torch.Tensor, lens: torch.Tensor | None, offset: torch.Tensor, n_edges: torch.Tensor, edges: torch.Tensor,
                     start: torch.Tensor | None = None, back: bool = False, download: bool = True):
        """snk_dev_extend_paths -- ExtendPathsNew (10X/Extend.cc:14-177) -- over tensors on this engine's device: the unitigs of the graph h
        (graphio.hbv_handle: unitig_off i64[U + 1], unitig_bases u8[], in the order h numbers them), the reads (packed rows i32[n, words],
        quals u8[n, stride], lens i16[n] or None) and their paths (offset i32[n], n_edges i32[n] read as u32, edges i32[sum], start i64[n + 1]
        or None: the paths follow each other).  back: SNK_EXT_BACK.  -> (offset i32[n], n_edges u32[n], edges i32[sum], stats) on the host;
        download=False: (SnkDevExtend, stats), device memory of the context, valid until its next top-level call."""
        n = int(n_edges.shape[0])
        if start is None:
            start = torch.zeros(n + 1, dtype=torch.int64, device=n_edges.device)
            start[1:] = torch.cumsum(n_edges.to(torch.int64) & 0xFFFFFFFF, 0)
        r = _lib.SnkDevReads()
        r.n_reads, r.rows, r.row_words, r.read_len = int(rows.shape[0]), rows.data_ptr(), (int(rows.shape[1]) if rows.dim() > 1 else 0), int(read_len)
        r.quals, r.qstride = (quals.data_ptr(), int(quals.shape[1])) if quals is not None else (None, 0)
        if lens is not None:
            r.lens = lens.data_ptr()
        p = _lib.SnkDevPaths()
        p.n_reads, p.n_edges_total = n, int(edges.shape[0])
        p.offset, p.n_edges, p.start, p.edges = offset.data_ptr(), n_edges.data_ptr(), start.data_ptr(), edges.data_ptr()
        x = _lib.SnkDevExtend()
        err = C.create_string_buffer(512)
        rc = self.lib.snk_dev_extend_paths(self._ctx, int(K), C.byref(r), int(unitig_off.shape[0]) - 1, unitig_off.data_ptr(), unitig_bases.data_ptr(),
                                           C.byref(h), C.byref(p), _lib.EXT_BACK if back else 0, C.byref(x), self._stream(), err, 512)
        if rc:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
        stats = _extend_stats(x)
        if not download:
            return x, stats
        m, tot = int(x.paths.n_reads), int(x.paths.n_edges_total)
        off, ne, ed = np.empty(m, np.int32), np.empty(m, np.uint32), np.empty(tot, np.int32)
        for a, ptr in ((off, x.paths.offset), (ne, x.paths.n_edges), (ed, x.paths.edges)):
            if a.size:
                self._download(ptr, a.ctypes.data, a.nbytes)
        return off, ne, ed, stats

    # ---- MarkBads (the first step of StageFindPatch) over device-resident unitigs and paths, and reads that are resident or in the stage's files
    def _paths_struct(self, offset, n_edges, edges, start):
        n = int(n_edges.shape[0])
        if start is None:
            start = torch.zeros(n + 1, dtype=torch.int64, device=n_edges.device)
            start[1:] = torch.cumsum(n_edges.to(torch.int64) & 0xFFFFFFFF, 0)
        p = _lib.SnkDevPaths()
        p.n_reads, p.n_edges_total = n, int(edges.shape[0])
        p.offset, p.n_edges, p.start, p.edges = offset.data_ptr(), n_edges.data_ptr(), start.data_ptr(), edges.data_ptr()
        return p, start

    def _bads_result(self, b: "_lib.SnkDevBads", download: bool):
        stats = _bads_stats(b)
        if not download:
            return b, stats
        bad = np.empty(int(b.n_pairs), np.uint8)
        if bad.size:
            self._download(b.bad, bad.ctypes.data, bad.nbytes)
        return bad, stats

    def mark_bads(self, K: int, h: "_lib.SnkHbv", unitig_off: torch.Tensor, unitig_bases: torch.Tensor, rows: torch.Tensor, read_len: int,
                  quals: torch.Tensor, lens: torch.Tensor | None, offset: torch.Tensor, n_edges: torch.Tensor, edges: torch.Tensor,
                  start: torch.Tensor | None = None, x: bool = False, download: bool = True):
        """snk_dev_mark_bads -- MarkBads (10X/SecretOps.cc:70-107; x=True: the ReadPathVecX overload, :22-59, int16 offsets: what a stock DF
        writes as a.bad) -- over tensors on this engine's device, the arguments of extend_paths.  -> (bad u8[n / 2], stats) on the host;
        download=False: (SnkDevBads, stats), device memory of the context, valid until its next top-level call."""
        r = _lib.SnkDevReads()
        r.n_reads, r.rows, r.row_words, r.read_len = int(rows.shape[0]), rows.data_ptr(), (int(rows.shape[1]) if rows.dim() > 1 else 0), int(read_len)
        r.quals, r.qstride = (quals.data_ptr(), int(quals.shape[1])) if quals is not None else (None, 0)
        if lens is not None:
            r.lens = lens.data_ptr()
        p, start = self._paths_struct(offset, n_edges, edges, start)
        b = _lib.SnkDevBads()
        err = C.create_string_buffer(512)
        rc = self.lib.snk_dev_mark_bads(self._ctx, int(K), C.byref(r), int(unitig_off.shape[0]) - 1, unitig_off.data_ptr(), unitig_bases.data_ptr(),
                                        C.byref(h), C.byref(p), _lib.BADS_X if x else 0, C.byref(b), self._stream(), err, 512)
        if rc:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
        return self._bads_result(b, download)

    def mark_bads_df(self, K: int, h: "_lib.SnkHbv", unitig_off: torch.Tensor, unitig_bases: torch.Tensor, files, offset: torch.Tensor,
                     n_edges: torch.Tensor, edges: torch.Tensor, start: torch.Tensor | None = None, first: int = 0, n: int | None = None, read_len: int = 0,
                     threads: int = 0, slab_reads: int = 0, x: bool = False, download: bool = True):
        """snk_dev_mark_bads_df: the same over reads [first, first + n) of an opened triple (dfin.DfFiles), decoded again slab by slab -- for
        a job that kept no quality rows.  The paths are those of these reads.  first and slab_reads must be even.  Results as mark_bads."""
        n = int(n_edges.shape[0]) if n is None else int(n)
        p, start = self._paths_struct(offset, n_edges, edges, start)
        torch.cuda.current_stream(self.device).synchronize()          # (the call works on the ring's own stream: its inputs must be complete)
        b = _lib.SnkDevBads()
        err = C.create_string_buffer(512)
        rc = self.lib.snk_dev_mark_bads_df(self._ctx, int(K), files._h, int(first), n, int(read_len), int(threads), int(slab_reads), int(unitig_off.shape[0]) - 1,
                                           unitig_off.data_ptr(), unitig_bases.data_ptr(), C.byref(h), C.byref(p), _lib.BADS_X if x else 0, C.byref(b), err, 512)
        if rc:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
        return self._bads_result(b, download)

    # ---- gap patches into the graph (StageInsertPatch)
    def insert_patch(self, graph, closures, paths) -> "PatchResult":
        """StageInsertPatch (10X/runstages/RunStages.cc:176-230) on this engine's device: pieces -> count -> merge -> hbv -> to3 / left3 ->
        translate (snk_dev_patch_pieces, snk_dev_count_graph with min_freq 1 and no barcode rule, snk_dev_patch_merge, snk_dev_hbv,
        snk_dev_patch_paths).
          graph     (K, h, unitig_off, unitig_bases): h a lib.SnkHbv of the OLD unitigs (of snk_dev_hbv, or graphio.hbv_handle), unitig_off
                    u64 / i64[U + 1] (numpy or tensor), unitig_bases u8[] (tensor on the device, or numpy), in the order h's bvcomp_order names
          closures  (off u64[n + 1] numpy, base codes u8[]: numpy or tensor on the device)
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
        if len(paths) > 3 and paths[3] is not None:
            p_start = own(paths[3], torch.int64)
        else:
            p_start = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            p_start[1:] = torch.cumsum(p_n.to(torch.int64) & 0xFFFFFFFF, 0)
        err = C.create_string_buffer(512)

        def call(fn, *args):
            rc = fn(*args, self._stream(), err, 512)
            if rc:
                raise _lib.SnkError(rc, err.value.decode(errors="replace"))

        # ---- pieces, into tensors of the engine
        plan = _lib.SnkPatchPlan()
        rc = self.lib.snk_patch_plan_sizes(int(K), U_old, uoff_h.ctypes.data, C.byref(h_old), n_cl, coff_h.ctypes.data, C.byref(plan), err, 512)
        if rc:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
        n_pieces, n_lmax = int(plan.n_pieces), int(plan.n_lonely_max)
        rows = torch.empty((n_pieces, 16), dtype=torch.int32, device=dev)
        lens = torch.empty((n_pieces,), dtype=torch.int16, device=dev)
        lonely = torch.empty((max(n_lmax, 1), 2), dtype=torch.int64, device=dev)
        pc = _lib.SnkDevPieces()
        call(self.lib.snk_dev_patch_pieces, self._ctx, int(K), U_old, uoff_h.ctypes.data, ub_old.data_ptr(), C.byref(h_old), n_cl, coff_h.ctypes.data, cb.data_ptr(),
             n_pieces, rows.data_ptr(), lens.data_ptr(), n_lmax, lonely.data_ptr(), C.byref(pc))
        # ---- the graph: the count stage on the pieces, the K-base sequences it leaves out, the ids
        if n_pieces:
            res = self.count_graph(rows, 256, lens=lens, good_len=lens, params=Params(K=int(K), min_freq=1, min_bc=0))
            raw, count_ms = res.raw, res.phase_ms["total"]
        else:
            raw, count_ms = _lib.SnkDevResult(), 0.0
        mu = _lib.SnkDevPatchUnitigs()
        call(self.lib.snk_dev_patch_merge, self._ctx, int(K), C.byref(raw), lonely.data_ptr(), int(pc.n_lonely), C.byref(mu))
        U_new, tot_new = int(mu.n_unitigs), int(mu.unitig_total_bases)
        h_new = _lib.SnkHbv()
        hbv_ms = C.c_float(0)
        call(self.lib.snk_dev_hbv, self._ctx, int(K), U_new, mu.unitig_off, mu.unitig_bases, C.byref(h_new), C.byref(hbv_ms))
        try:
            ip = _lib.SnkDevPaths()
            ip.n_reads, ip.n_edges_total = n, int(p_edges.shape[0])
            ip.offset, ip.n_edges, ip.start, ip.edges = p_off.data_ptr(), p_n.data_ptr(), p_start.data_ptr(), p_edges.data_ptr()
            px = _lib.SnkDevPatched()
            call(self.lib.snk_dev_patch_paths, self._ctx, int(K), U_old, uoff_old.data_ptr(), ub_old.data_ptr(), C.byref(h_old), U_new, mu.unitig_off, mu.unitig_bases,
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
            out.to3_off = take(px.to3_off, E_old + 1, torch.int64).cpu().numpy().view(np.uint64)
            out.to3, out.left3 = take(px.to3, n_to3, torch.int32).cpu().numpy(), take(px.left3, E_old, torch.int32).cpu().numpy()
            inv = np.zeros(max(int(h_new.n_edges), 1), np.int32)
            rc = self.lib.snk_hbv_involution(C.byref(h_new), U_new, inv.ctypes.data, err, 512)
            if rc:
                raise _lib.SnkError(rc, err.value.decode(errors="replace"))
            out.inv = inv[:int(h_new.n_edges)]
            out.stats = dict(n_pieces=n_pieces, n_unitig_pieces=int(plan.n_unitig_pieces), n_junctions=int(plan.n_junctions), n_closure_pieces=int(plan.n_closure_pieces),
                             n_lonely=int(pc.n_lonely), n_added=int(mu.n_added), n_first=int(px.n_first), n_later=int(px.n_later), n_cleared=int(px.n_cleared),
                             n_kmers=int(raw.n_kmers), pieces_ms=float(pc.ms), count_ms=float(count_ms), merge_ms=float(mu.ms), hbv_ms=float(hbv_ms.value),
                             map_ms=float(px.map_ms), translate_ms=float(px.paths.path_ms))
            return out
        except BaseException:
            self.lib.snk_hbv_free(C.byref(h_new))
            raise

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
        r = _lib.SnkDevReads()
        r.n_reads = rows.shape[0]
        r.rows = rows.data_ptr()
        r.row_words = rows.shape[1]
        r.read_len = read_len
        if lens is not None:
            assert lens.dtype == torch.int16 and lens.is_cuda
            r.lens = lens.data_ptr()
        if quals is not None:
            assert quals.dtype == torch.uint8 and quals.is_cuda and quals.is_contiguous()
            r.quals = quals.data_ptr()
            r.qstride = quals.shape[1]
        if good_len is not None:
            assert good_len.dtype == torch.int16 and good_len.is_cuda
            r.good_len = good_len.data_ptr()
        if bc is not None:
            assert bc.dtype == torch.int32 and bc.is_cuda
            r.bc = bc.data_ptr()
        r.ign_bc_below = ign_bc_below
        r.read_index_base = read_index_base
        if group is not None:
            assert group.dtype == torch.int32 and group.is_cuda and group.is_contiguous()
            r.group = group.data_ptr()
        return self.count_graph_reads(r, params)

    # ---- streamed input: the job's reads arrive slab by slab (snk_dev_stream_begin / _append / _finish)
    def stream_begin(self, read_len: int, total_reads_ub: int, has_bc: bool = True, params: Params | None = None):
        self._stream_params = params or Params()
        p = self._stream_params.to_c()
        err = C.create_string_buffer(512)
        rc = self.lib.snk_dev_stream_begin(self._ctx, C.byref(p), int(read_len), int(total_reads_ub), 1 if has_bc else 0, self._stream(), err, 512)
        if rc != 0:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))

    def stream_append(self, rows: torch.Tensor, read_len: int, quals: torch.Tensor | None = None, bc: torch.Tensor | None = None,
                      lens: torch.Tensor | None = None, good_len: torch.Tensor | None = None, ign_bc_below: int = 0, read_index_base: int = 0):
        """One slab (asynchronous: its tensors must stay alive until the engine's stream has passed the call)."""
        assert rows.is_cuda and rows.dtype == torch.int32 and rows.is_contiguous()
        r = _lib.SnkDevReads()
        r.n_reads, r.rows, r.row_words, r.read_len = rows.shape[0], rows.data_ptr(), rows.shape[1], read_len
        if lens is not None:
            r.lens = lens.data_ptr()
        if quals is not None:
            assert quals.dtype == torch.uint8 and quals.is_cuda and quals.is_contiguous()
            r.quals, r.qstride = quals.data_ptr(), quals.shape[1]
        if good_len is not None:
            r.good_len = good_len.data_ptr()
        if bc is not None:
            r.bc = bc.data_ptr()
        r.ign_bc_below, r.read_index_base = ign_bc_below, read_index_base
        self.stream_append_reads(r)

    def stream_append_reads(self, r: "_lib.SnkDevReads"):
        err = C.create_string_buffer(512)
        rc = self.lib.snk_dev_stream_append(self._ctx, C.byref(r), self._stream(), err, 512)
        if rc != 0:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))

    def stream_finish(self) -> Result:
        raw = _lib.SnkDevResult()
        err = C.create_string_buffer(512)
        rc = self.lib.snk_dev_stream_finish(self._ctx, C.byref(raw), self._stream(), err, 512)
        if rc != 0:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
        return Result(self, raw, self._stream_params.K, self._stream_params)

    def count_graph_reads(self, r: "_lib.SnkDevReads", params: Params | None = None) -> Result:
        """The same for reads described by plain device pointers (e.g. the arrays of snk_dev_ingest_fasth)."""
        params = params or Params()
        p = params.to_c()
        raw = _lib.SnkDevResult()
        err = C.create_string_buffer(512)
        rc = self.lib.snk_dev_count_graph(self._ctx, C.byref(r), C.byref(p), C.byref(raw), self._stream(), err, 512)
        if rc != 0:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
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
        err = C.create_string_buffer(512)
        rc = self.lib.snk_dev_check_graph(self._ctx, C.byref(ci), C.byref(reads) if reads is not None else None, C.byref(rep), self._stream(),
                                          err, 512)
        if rc != 0:
            raise _lib.SnkError(rc, err.value.decode(errors="replace"))
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
