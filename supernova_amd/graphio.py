"""Host-side hand-off formats and the graph-from-unitigs step, through libsnk's C ABI.

  write_bv / read_bv   the `.bv` file tada writes and DF reads through MSPEDGES=
                       (lib/tada/src/debruijn.rs:895-929; BuildReadQGraph48.cc:1640-1642)
  hbv_from_unitigs     buildHBVFromEdges (lib/assembly/src/paths/long/HBVFromEdges.cc:244-296)
  write_hbv            a.hbv / a.inv as DF keeps the graph (paths/HyperBasevector.cc:121-125)
  write_paths, write_paths_index, write_dup, write_a48
                       the rest of a.48/: a.paths, a.paths.inv, a.countsb, a.dup (10X/DF.cc:584-600, 10X/PathsIndex.cc:23-145)
  write_hops / read_hops  a.hops, the edge pairs of FindEdgePairs that StageFindPatch leaves (10X/DF.cc:642-643); write_a48 adds it when the result holds 'hops'
  write_bad            a.bad, the pair flags of MarkBads that StageFindPatch leaves (10X/DF.cc:644); write_a48 adds it when the result holds 'bads'
  write_pathsx / read_pathsx, write_hbx
                       the compressed forms DF goes on working from: a.pathsX (10X/paths/ReadPathVecX.cc:976-996) and a.hbx
                       (paths/HyperBasevector.cc:133-137); write_a48 adds them when the result holds 'pathsx'
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import lib as _lib

_CODE = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def unitigs_to_arrays(unitigs: list[str]):
    """ASCII unitigs -> (off u64[n+1], bases u8 codes)."""
    off = np.zeros(len(unitigs) + 1, dtype=np.uint64)
    if unitigs:
        off[1:] = np.cumsum([len(u) for u in unitigs], dtype=np.uint64)
    bases = _CODE[np.frombuffer("".join(unitigs).encode(), dtype=np.uint8)] if unitigs else np.zeros(0, np.uint8)
    return off, np.ascontiguousarray(bases)


def arrays_to_unitigs(off: np.ndarray, bases: np.ndarray) -> list[str]:
    asc = np.frombuffer(b"ACGT", dtype=np.uint8)[bases].tobytes().decode()
    return [asc[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def write_bv(path: str, off: np.ndarray, bases: np.ndarray) -> None:
    lib = _lib.load()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    _lib.call(lib.snk_write_bv, str(path).encode(), len(off) - 1, off.ctypes.data, bases.ctypes.data)


def read_bv(path: str):
    lib = _lib.load()
    n = C.c_uint64(0)
    po = C.POINTER(C.c_uint64)()
    pb = C.POINTER(C.c_uint8)()
    _lib.call(lib.snk_read_bv, str(path).encode(), C.byref(n), C.byref(po), C.byref(pb))
    off = np.ctypeslib.as_array(po, shape=(n.value + 1,)).copy()
    tot = int(off[-1])
    bases = np.ctypeslib.as_array(pb, shape=(max(tot, 1),))[:tot].copy()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(po)
    libc.free(pb)
    return off, bases


def hbv_arrays(h: "_lib.SnkHbv", n_unitigs: int, order: bool = False) -> dict:
    """A lib.SnkHbv as a dict of numpy copies (the C arrays stay the caller's to free); order: with 'order' = bvcomp_order."""
    ne, nu = h.n_edges, n_unitigs
    arr = lambda p, m, dt: (np.array(np.ctypeslib.as_array(p, shape=(m,)), dtype=dt, copy=True) if m else np.zeros(0, dt))
    out = dict(n_vertices=h.n_vertices, n_edges=ne, v_left=arr(h.v_left, ne, np.int32), v_right=arr(h.v_right, ne, np.int32),
               src=arr(h.src_unitig, ne, np.int32), is_rc=arr(h.is_rc, ne, np.uint8), fwd=arr(h.fwd_xlat, nu, np.int32),
               rev=arr(h.rev_xlat, nu, np.int32))
    if order:
        out["order"] = arr(h.bvcomp_order, nu, np.int32)
    return out


def hbv_from_unitigs(K: int, off: np.ndarray, bases: np.ndarray) -> dict:
    """Unitigs in BVComp order -> HBV description (vertex ids per edge, fwd/rev translation)."""
    with hbv_handle(K, off, bases) as h:
        return hbv_arrays(h, len(off) - 1)


@contextlib.contextmanager
def hbv_handle(K: int, off: np.ndarray, bases: np.ndarray):
    """The snk_hbv of unitigs in BVComp order as the C struct (lib.SnkHbv) the device calls take -- Engine.zip_paths / unzip_paths --
    freed when the block ends."""
    lib = _lib.load()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    h = _lib.SnkHbv()
    _lib.call(lib.snk_hbv_from_unitigs, K, len(off) - 1, off.ctypes.data, bases.ctypes.data, C.byref(h))
    try:
        yield h
    finally:
        lib.snk_hbv_free(C.byref(h))


def write_hbv(path_hbv, path_inv, K: int, off: np.ndarray, bases: np.ndarray) -> np.ndarray:
    """Unitigs in BVComp order -> a.hbv (+ a.inv) as DF writes them; returns the involution."""
    lib = _lib.load()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    nu = len(off) - 1
    with hbv_handle(K, off, bases) as h:
        inv = np.zeros(max(h.n_edges, 1), dtype=np.int32)
        _lib.call(lib.snk_hbv_involution, C.byref(h), nu, inv.ctypes.data)
        _lib.call(lib.snk_write_hbv, str(path_hbv).encode(), str(path_inv).encode() if path_inv else None, K, nu, off.ctypes.data,
                  bases.ctypes.data, C.byref(h))
        return inv[:h.n_edges].copy()


def write_paths(path, offset: np.ndarray, n_edges: np.ndarray, edges: np.ndarray, start: np.ndarray | None = None) -> None:
    """a.paths (the tmp.paths of pathReads, BuildReadQGraph48.cc:1441-1469): per read its offset and HBV edge ids.  start = position of
    every read's first edge in `edges`, None = the paths follow each other."""
    offset = np.ascontiguousarray(offset, dtype=np.int32)
    n_edges = np.ascontiguousarray(n_edges, dtype=np.uint32)
    edges = np.ascontiguousarray(edges, dtype=np.int32)
    assert len(offset) == len(n_edges)
    if start is not None:
        start = np.ascontiguousarray(start, dtype=np.uint64)
        assert len(start) >= len(n_edges)
    _lib.call(_lib.load().snk_write_paths, str(path).encode(), len(n_edges), offset.ctypes.data, n_edges.ctypes.data,
              start.ctypes.data if start is not None else None, edges.ctypes.data)


def write_paths_index(path_inv, path_countsb, off: np.ndarray, ids: np.ndarray, counts: np.ndarray) -> None:
    """a.paths.inv and a.countsb (writePathsIndex, 10X/PathsIndex.cc:23-145) from the index of snk_dev_paths_index: the reads of edge e
    are ids[off[e]:off[e+1]].  Either path may be None."""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    E = len(off) - 1
    assert E >= 0 and len(counts) == E and len(ids) == int(off[-1])
    _lib.call(_lib.load().snk_write_paths_index, str(path_inv).encode() if path_inv else None, str(path_countsb).encode() if path_countsb else None, E,
              off.ctypes.data, ids.ctypes.data, counts.ctypes.data)


def write_dup(path, dup: np.ndarray) -> None:
    """a.dup (vec<Bool> of MarkDups, 10X/DF.cc:599-600): one flag per read pair."""
    dup = np.ascontiguousarray(dup, dtype=np.uint8)
    _lib.call(_lib.load().snk_write_dup, str(path).encode(), len(dup), dup.ctypes.data)


def write_bad(path, bad: np.ndarray) -> None:
    """a.bad (vec<Bool> of MarkBads, 10X/DF.cc:644): one flag per read pair.  BinaryWriter::writeFile(vec<Bool>), the container of a.dup."""
    bad = np.ascontiguousarray(bad, dtype=np.uint8)
    _lib.call(_lib.load().snk_write_dup, str(path).encode(), len(bad), bad.ctypes.data)


def write_hops(path, pairs: np.ndarray) -> None:
    """a.hops (vec<pair<int,int>> of FindEdgePairs, 10X/DF.cc:642-643): pairs i32[n, 2], as snk_dev_edge_pairs gives them."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    _lib.call(_lib.load().snk_write_hops, str(path).encode(), len(pairs), pairs.ctypes.data)


def write_closures(path, off: np.ndarray, bases: np.ndarray) -> None:
    """closures.fastb (vec<basevector> of StageFindPatch, 10X/DF.cc:645): closure_off u64[n + 1] and base codes u8[], as snk_dev_close_gaps
    gives them.  BinaryWriter::writeFile(vec<basevector>) is the layout of the unitig hand-off file: snk_write_bv writes it."""
    write_bv(path, off, bases)


def read_hops(path) -> np.ndarray:
    """a.hops -> pairs i32[n, 2]."""
    lib = _lib.load()
    n = C.c_uint64(0)
    pp = C.POINTER(C.c_int32)()
    _lib.call(lib.snk_read_hops, str(path).encode(), C.byref(n), C.byref(pp))
    try:
        return np.ctypeslib.as_array(pp, shape=(n.value, 2)).copy() if n.value else np.zeros((0, 2), np.int32)
    finally:
        lib.snk_host_free(pp)


def write_pathsx(path, index: np.ndarray, data: np.ndarray, n_reads: int) -> None:
    """a.pathsX (ReadPathVecX::writeBinary, 10X/paths/ReadPathVecX.cc:976-996) from what snk_dev_paths_zip made: index i64[ceil(n_reads / 10)] =
    the byte offset of every 10th read's record, data u8[...] = the records."""
    index = np.ascontiguousarray(index, dtype=np.int64)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    _lib.call(_lib.load().snk_write_pathsx, str(path).encode(), int(n_reads), index.ctypes.data, len(index), data.ctypes.data, len(data))


def read_pathsx(path):
    """a.pathsX -> (index i64[], data u8[], n_reads)."""
    lib = _lib.load()
    n, ni, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    pi = C.POINTER(C.c_int64)()
    pd = C.POINTER(C.c_uint8)()
    _lib.call(lib.snk_read_pathsx, str(path).encode(), C.byref(n), C.byref(ni), C.byref(pi), C.byref(nb), C.byref(pd))
    try:
        index = np.ctypeslib.as_array(pi, shape=(ni.value,)).copy() if ni.value else np.zeros(0, np.int64)
        data = np.ctypeslib.as_array(pd, shape=(nb.value,)).copy() if nb.value else np.zeros(0, np.uint8)
    finally:
        lib.snk_host_free(pi)
        lib.snk_host_free(pd)
    return index, data, int(n.value)


def write_ebcx(path, off: np.ndarray, bcs: np.ndarray) -> None:
    """a.ebcx (VecIntVec::WriteAll of computeEdgeToBarcodeX's result, 10X/PathsIndex.cc:297-358) from the lists of snk_dev_edge_barcodes:
    the barcodes of edge e are bcs[off[e]:off[e+1]].  Not one of the files of a.48/: write_a48 leaves it alone."""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    bcs = np.ascontiguousarray(bcs, dtype=np.int32)
    E = len(off) - 1
    assert E >= 0 and len(bcs) == int(off[-1])
    _lib.call(_lib.load().snk_write_ebcx, str(path).encode(), E, off.ctypes.data, bcs.ctypes.data)


def read_ebcx(path):
    """a.ebcx -> (off u64[E+1], bcs i32[])."""
    lib = _lib.load()
    E = C.c_uint64(0)
    po = C.POINTER(C.c_uint64)()
    pb = C.POINTER(C.c_int32)()
    _lib.call(lib.snk_read_ebcx, str(path).encode(), C.byref(E), C.byref(po), C.byref(pb))
    try:
        off = np.ctypeslib.as_array(po, shape=(E.value + 1,)).copy()
        bcs = np.ctypeslib.as_array(pb, shape=(int(off[-1]),)).copy() if off[-1] else np.zeros(0, np.int32)
    finally:
        lib.snk_host_free(po)
        lib.snk_host_free(pb)
    return off, bcs


def write_hbx(path, K: int, off: np.ndarray, bases: np.ndarray) -> None:
    """Unitigs in BVComp order -> a.hbx, the HyperBasevectorX of the graph a.hbv holds (10X/DF.cc:573-576)."""
    lib = _lib.load()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    with hbv_handle(K, off, bases) as h:
        _lib.call(lib.snk_write_hbx, str(path).encode(), K, len(off) - 1, off.ctypes.data, bases.ctypes.data, C.byref(h))


def write_a48(dir, K: int, off: np.ndarray, bases: np.ndarray, path_offset: np.ndarray, path_n_edges: np.ndarray, path_edges: np.ndarray, info: dict) -> np.ndarray:
    """The six files DF leaves in a.<K>/ after StageBuildGraph (10X/DF.cc:564-601) from one result: a.hbv, a.inv (the unitigs in BVComp
    order: graphio.unitigs_to_arrays(res.unitigs())), a.paths (what res.path_reads returned), a.paths.inv, a.countsb (info['paths_index'],
    info['countsb']: path_reads(..., paths_index=True)) and a.dup (info['dups']['dup']: mark_dups=True).  With info['pathsx']
    (path_reads(..., pathsx=True)) also a.hbx and a.pathsX, the two other files a DF entered at START=patch opens (10X/DF.cc:612-630).
    With info['bads'] (path_reads(..., mark_bads="x"), or dict(bad=...) of Engine.mark_bads) also a.bad, which StageFindPatch leaves
    (10X/DF.cc:644); with info['hops'] (path_reads(..., hops=True), or the pairs of Engine.edge_pairs) also a.hops, the other file of that
    step (10X/DF.cc:642-643).  Returns the involution."""
    from pathlib import Path
    d = Path(dir)
    d.mkdir(parents=True, exist_ok=True)
    for k in ("paths_index", "countsb", "dups"):
        if k not in info:
            raise KeyError(f"write_a48 needs info[{k!r}]: path_reads(..., mark_dups=True, paths_index=True)")
    inv = write_hbv(d / "a.hbv", d / "a.inv", K, off, bases)
    iv = info.get("inv")
    if iv is not None and not np.array_equal(iv, inv):
        raise ValueError("write_a48: the unitigs are not the ones the paths index was made on (involutions differ)")
    write_paths(d / "a.paths", path_offset, path_n_edges, path_edges)
    write_paths_index(d / "a.paths.inv", d / "a.countsb", info["paths_index"][0], info["paths_index"][1], info["countsb"])
    write_dup(d / "a.dup", info["dups"]["dup"])
    if "pathsx" in info:
        write_hbx(d / "a.hbx", K, off, bases)
        write_pathsx(d / "a.pathsX", info["pathsx"][0], info["pathsx"][1], len(path_n_edges))
    if "bads" in info:
        write_bad(d / "a.bad", info["bads"]["bad"])
    if "hops" in info:
        write_hops(d / "a.hops", info["hops"])
    return inv


def hbv_text(unitigs: list[str], h: dict) -> str:
    """Same text layout as oracle/ref/ref_driver.cc's hbv.txt (golden fixtures)."""
    comp = str.maketrans("ACGT", "TGCA")
    lines = [f"N {h['n_vertices']} E {h['n_edges']} U {len(unitigs)}"]
    for e in range(h["n_edges"]):
        s = unitigs[h["src"][e]]
        if h["is_rc"][e]:
            s = s.translate(comp)[::-1]
        lines.append(f"E {e} {h['v_left'][e]} {h['v_right'][e]} {s}")
    for u in range(len(unitigs)):
        lines.append(f"X {u} {h['fwd'][u]} {h['rev'][u]}")
    return "\n".join(lines) + "\n"
