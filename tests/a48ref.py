"""The a.48 fixtures (tests/golden/a48/*.npz: file bytes written by the reference's own code, see make_a48_golden.py), a small parser
of a.paths.inv / a.countsb, and the numpy restatement of writePathsIndex (10X/PathsIndex.cc:23-145) the GPU tests use at sizes
without fixtures -- test_a48_files.py pins the restatement to the reference's files."""
from __future__ import annotations

import struct
from pathlib import Path

import numpy as np

A48 = Path(__file__).resolve().parent / "golden" / "a48"
FILES = ("tmp.paths", "a.paths.inv", "a.countsb", "a.dup")


def load(name: str) -> dict:
    z = np.load(A48 / f"{name}.npz")
    return {f: bytes(z[f.replace(".", "_")]) for f in FILES}


def paths_index(n_edges: np.ndarray, edges: np.ndarray, inv: np.ndarray):
    """-> (off u64[E+1], ids u64[len(edges)], counts i32[E]): the (edge, read id) pairs of the paths sorted (duplicates kept,
    PathsIndex.cc:51-57,90,104-107), cut per edge; counts = entries per edge, e < inv[e]: both get the sum (:122-133)."""
    E = len(inv)
    edges = np.asarray(edges, dtype=np.int64)
    read_of_entry = np.repeat(np.arange(len(n_edges), dtype=np.uint64), np.asarray(n_edges, dtype=np.int64))
    order = np.argsort(edges, kind="stable")
    ids = read_of_entry[order]
    own = np.bincount(edges, minlength=E).astype(np.int64)
    off = np.zeros(E + 1, dtype=np.uint64)
    off[1:] = np.cumsum(own)
    inv = np.asarray(inv, dtype=np.int64)
    counts = np.where(inv == np.arange(E), own, own + own[inv]) if E else own
    assert counts.max(initial=0) < 2**31
    return off, ids, counts.astype(np.int32)


def parse_paths_inv(b: bytes):
    """a.paths.inv (feudal MasterVec<ULongVec>) -> (off u64[E+1] in entries, ids u64)."""
    n32, flags, sz_fixed, sz_x, sz_a, var, fixed = struct.unpack("<IBBBBQQ", b[:24])
    assert flags == 1 and sz_fixed == 0 and sz_x == 16 and sz_a == 8 and fixed == len(b) and (fixed - var) % 8 == 0
    tab = np.frombuffer(b[var:fixed], dtype="<u8")
    assert len(tab) - 1 == n32 and tab[0] == 24 and tab[-1] == var and np.all(np.diff(tab.astype(np.int64)) >= 0) and np.all((tab - 24) % 8 == 0)
    return ((tab - 24) // 8).astype(np.uint64), np.frombuffer(b[24:var], dtype="<u8")


def parse_countsb(b: bytes) -> np.ndarray:
    assert b[:8] == b"BINWRITE" and struct.unpack("<QQ", b[8:24])[0] == 1
    E = struct.unpack("<Q", b[16:24])[0]
    assert len(b) == 24 + 4 * E
    return np.frombuffer(b[24:], dtype="<i4")


def parse_inv(b: bytes) -> np.ndarray:
    assert b[:8] == b"BINWRITE"
    E = struct.unpack("<Q", b[8:16])[0]
    assert len(b) == 16 + 4 * E
    return np.frombuffer(b[16:], dtype="<i4")
