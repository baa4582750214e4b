"""The a.ebcx fixtures (tests/golden/ebcx/*.npz: bytes the reference's own code wrote, see tests/golden/make_ebcx_golden.py), a parser of
that file (feudal MasterVec<SerfVec<int>>, VecIntVec::WriteAll) and a numpy restatement of computeEdgeToBarcodeX
(10X/PathsIndex.cc:297-358) in the form the device computes it: per edge the ascending set of distinct bc > 0 over the reads whose path
holds the edge or its reverse complement.  test_ebcx_files.py pins the restatement to the fixtures; the GPU tests use it at sizes
without fixtures."""
from __future__ import annotations

import struct
from pathlib import Path

import numpy as np

EBCX = Path(__file__).resolve().parent / "golden" / "ebcx"
GOLDEN = ("synth_2k_err", "synth_6k_clean", "synth_20k_err", "adversarial", "synth_4k_dups")      # goldens.CASES, reads reordered by barcode
PROBES = ("ebcx_probe", "ebcx_probe_ends_empty")
CASES = GOLDEN + PROBES
FCB = 24                                         # bytes of a feudal control block


class Fixture:
    """offset / n_edges / edges: the paths of tmp.paths (reads sorted by barcode); bc i32 per read; bci i64: the start of every run;
    ebcx: the bytes of a.ebcx; inv: the involution of the case's graph."""

    def __init__(self, name: str):
        import a48ref
        import a48xref
        import goldens
        z = np.load(EBCX / f"{name}.npz")
        self.name = name
        self.tmp_paths = bytes(z["tmp_paths"])
        self.offset, self.n_edges, self.edges = a48xref.parse_paths(self.tmp_paths)
        self.bc = z["bc"].astype(np.int32)
        self.bci = z["bci"].astype(np.int64)
        self.ebcx = bytes(z["a_ebcx"])
        self.ref_summary = bytes(z["ref_summary"]).decode()
        self.inv = a48ref.parse_inv(goldens.load(name if name in GOLDEN else "adversarial").exp_ainv).astype(np.int32)
        self.E = len(self.inv)
        assert len(self.bc) == len(self.n_edges) and self.bci[0] == 0 and self.bci[-1] == len(self.bc)


_cache: dict[str, Fixture] = {}


def load(name: str) -> Fixture:
    if name not in _cache:
        _cache[name] = Fixture(name)
    return _cache[name]


def edge_barcodes(n_edges, edges, bc, inv):
    """-> (off u64[E+1], bcs i32[]): the barcodes of edge e are bcs[off[e]:off[e+1]], strictly ascending."""
    inv = np.asarray(inv, dtype=np.int64)
    E = len(inv)
    edges = np.asarray(edges, dtype=np.int64)
    b = np.repeat(np.asarray(bc, dtype=np.int64), np.asarray(n_edges, dtype=np.int64))
    keep = b > 0
    e, b = edges[keep], b[keep]
    keys = np.unique(np.concatenate([e, inv[e]]) << 32 | np.concatenate([b, b]))
    off = np.zeros(E + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(keys >> 32, minlength=E))
    return off, (keys & 0xFFFFFFFF).astype(np.int32)


def stats(off: np.ndarray) -> dict:
    n = np.diff(off.astype(np.int64))
    return dict(n_ebc=int(off[-1]), n_empty_edges=int((n == 0).sum()), max_list=int(n.max(initial=0)))


def parse_ebcx(b: bytes):
    """a.ebcx -> (off u64[E+1] in entries, bcs i32[]).  Control block (feudal/FeudalControlBlock.h:157-166): u32 count, u8 flags = 1,
    u8 sizeof fixed = 0, u8 sizeof(SerfVec<int>) = 16, u8 sizeof(int) = 4, u64 offset of the table of E + 1 file offsets, u64 end of it
    (= the file's size: no fixed-length data)."""
    assert len(b) >= FCB + 8, "shorter than a control block and one offset"
    n32, flags, sz_fixed, sz_x, sz_a, var, fixed = struct.unpack("<IBBBBQQ", b[:FCB])
    assert (flags, sz_fixed, sz_x, sz_a) == (1, 0, 16, 4), (flags, sz_fixed, sz_x, sz_a)
    assert fixed == len(b) and FCB <= var <= fixed and (fixed - var) % 8 == 0 and (var - FCB) % 4 == 0
    tab = np.frombuffer(b[var:fixed], dtype="<u8")
    assert len(tab) - 1 == n32 and tab[0] == FCB and tab[-1] == var and np.all(np.diff(tab.astype(np.int64)) >= 0) and np.all((tab - FCB) % 4 == 0)
    return ((tab - FCB) // 4).astype(np.uint64), np.frombuffer(b[FCB:var], dtype="<i4").astype(np.int32)


def ebcx_bytes(off, bcs) -> bytes:
    off = np.asarray(off, dtype=np.uint64)
    var = FCB + 4 * int(off[-1])
    return (struct.pack("<IBBBBQQ", (len(off) - 1) & 0xFFFFFFFF, 1, 0, 16, 4, var, var + 8 * len(off)) + np.asarray(bcs, "<i4").tobytes()
            + (FCB + 4 * off).astype("<u8").tobytes())


def runs_of(bc) -> np.ndarray:
    """bci of reads sorted by barcode: the start of every run of equal bc, and the number of reads."""
    bc = np.asarray(bc)
    if len(bc) == 0:
        return np.zeros(1, np.int64)
    return np.concatenate([[0], np.nonzero(bc[1:] != bc[:-1])[0] + 1, [len(bc)]]).astype(np.int64)


def toy_involution(E: int) -> np.ndarray:
    """Pairs (0, 1), (2, 3), ...; with an odd E the last edge is its own reverse complement."""
    inv = np.arange(E, dtype=np.int32) ^ 1
    if E % 2:
        inv[E - 1] = E - 1
    return inv
