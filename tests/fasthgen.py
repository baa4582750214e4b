"""FASTH files from explicit lists of records, and what the reference reads from them -- test infrastructure.

A record is one read pair: (r1, q1, r2, q2, barcode field, line end), bases and barcode field as str, qualities as raw phred values.
`write_fasth` writes the nine-line text of a list of records (header, R1, Q1, R2, Q2, barcode field, three ignored lines:
lib/tada/src/multifastq.rs:69-127) as gzip: one member, or several cut at ARBITRARY byte offsets of the text (cat a.gz b.gz, where a
line may straddle the seam).  `expected` is the pure-Python restatement of the reference's reader (supernova_amd.martian.read_fasth
with BcIndexer, pinned to the reference's vectors by tests/test_martian.py) brought into the layout of the device arrays: packed rows
with every byte that is not A, C, G or T as code 0 (base_to_bits, lib/tada/src/kmer/mod.rs:311-319 -- lowercase letters included),
quality rows zero-padded to the row stride, lengths, barcode ids."""
from __future__ import annotations

import gzip
from pathlib import Path

import numpy as np


def record(r1: str, q1, r2: str, q2, bcf: str, eol: str = "\n"):
    return (r1, np.asarray(q1, dtype=np.uint8), r2, np.asarray(q2, dtype=np.uint8), bcf, eol)


def text_of(records, final_newline: bool = True, tag: str = "p") -> bytes:
    out = []
    for i, (r1, q1, r2, q2, bcf, eol) in enumerate(records):
        assert len(r1) == len(q1) and len(r2) == len(q2)
        qs = lambda q: (np.asarray(q, dtype=np.uint8) + 33).tobytes().decode("ascii")
        out.append(eol.join([f"@{tag}{i}", r1, qs(q1), r2, qs(q2), bcf, "FFFFFFFF", "ACGTACGT", "FFFFFFFF"]) + eol)
    t = "".join(out)
    if not final_newline and records:
        t = t[:-len(records[-1][5])]
    return t.encode("ascii")


def write_fasth(path, records, level: int = 6, final_newline: bool = True, cuts=(), tag: str = "p") -> str:
    """cuts: byte offsets of the text at which a new gzip member starts (any byte, not a record or line boundary)."""
    t = text_of(records, final_newline, tag)
    edges = [0] + sorted(int(c) for c in cuts) + [len(t)]
    assert all(a < b for a, b in zip(edges, edges[1:])) or len(t) == 0, "cuts must fall strictly inside the text"
    Path(path).write_bytes(b"".join(gzip.compress(t[a:b], level, mtime=0) for a, b in zip(edges, edges[1:])))
    return str(path)


def write_empty(path) -> str:
    """A valid gzip member that holds zero bytes of text."""
    Path(path).write_bytes(gzip.compress(b"", 6, mtime=0))
    return str(path)


def text_size(paths) -> int:
    return sum(len(gzip.open(p, "rb").read()) for p in paths)


def whitelist_lines(whitelist: bytes):
    return whitelist.decode("ascii").splitlines(keepends=True)


_LUT = np.zeros(256, dtype=np.uint8)
for _c, _v in ((b"C", 1), (b"G", 2), (b"T", 3)):
    _LUT[_c[0]] = _v


class Expected:
    """codes u8[n, read_len], rows u32[n, ceil(read_len/16)], quals u8[n, qstride] (zero behind every read's own length), lens u16[n], bc i32[n]."""

    def __init__(self, paths, whitelist: bytes, read_len: int):
        from supernova_amd import synth
        from supernova_amd.martian import BcIndexer, read_fasth
        asc, qa, lens, bc = read_fasth([str(p) for p in paths], BcIndexer(whitelist_lines(whitelist)))
        n = asc.shape[0]
        assert n == 0 or int(lens.max()) <= read_len, "the lane holds a read longer than read_len"
        w = min(asc.shape[1], read_len) if n else 0
        qstride = (read_len + 15) // 16 * 16
        self.codes = np.zeros((n, read_len), dtype=np.uint8)
        self.quals = np.zeros((n, qstride), dtype=np.uint8)
        if n:
            self.codes[:, :w] = _LUT[asc[:, :w]]
            self.quals[:, :w] = qa[:, :w]
            beyond = np.arange(read_len)[None, :] >= lens[:, None]
            assert not self.codes[beyond].any() and not self.quals[:, :read_len][beyond].any()
        self.rows = synth.pack_rows(self.codes) if n else np.zeros((0, (read_len + 15) // 16), dtype=np.uint32)
        self.lens = lens.astype(np.uint16)
        self.bc = bc.astype(np.int32)
        self.n, self.read_len, self.qstride = n, read_len, qstride


# ---------------------------------------------------------------------------------------------------------------------------------
# the odd lane of tests/test_gpu_ingest_ragged.py: five files with everything the library's own synthetic writer never makes

def odd_whitelist(rng, n: int = 40):
    """-> (bytes, sequences): line 7 repeats line 3 (the later index wins, utils.rs:101-118), the last line has no newline."""
    seqs = []
    while len(seqs) < n:
        s = "".join("ACGT"[i] for i in rng.integers(0, 4, 16))
        if s not in seqs:
            seqs.append(s)
    seqs[7] = seqs[3]
    return ("\n".join(seqs)).encode("ascii"), seqs


def odd_field(rng, seqs, kind: int) -> str:
    s = seqs[int(rng.integers(0, len(seqs)))]
    if kind == 0:
        return s + "-1"
    if kind == 1:
        return s + "-2"
    if kind == 2:
        return s                                  # no gem group
    if kind == 3:
        return s + "-1,RAWRAWRAWRAWRAWR"
    if kind == 4:
        return "".join("ACGT"[i] for i in rng.integers(0, 4, 16))[:15] + "N-1"      # off the whitelist
    if kind == 5:
        return "NNNNNNNNNNNNNNNN-1"
    return s + "ACGTAC-1"                         # longer than 16 characters


N_FIELD_KINDS = 7


def odd_layout(directory, records, sizes=(1, 1500, 700, 0, 400), tag: str = "odd"):
    """records -> five files: sizes[i] pairs each; file 2 is two gzip members cut in the middle of a line; file 3 is the empty member;
    the last record of file 4 has no final newline.  Returns the paths."""
    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    assert sum(sizes) == len(records) and sizes[3] == 0
    paths, at = [], 0
    for fi, m in enumerate(sizes):
        recs = records[at:at + m]
        at += m
        p = directory / f"{tag}{fi}.fasth.gz"
        if fi == 3:
            paths.append(write_empty(p))
            continue
        cuts = ()
        if fi == 2:
            t = text_of(recs)
            cut = len(t) // 2
            while t[cut - 1:cut] in (b"\n", b"\r") or t[cut:cut + 1] in (b"\n", b"\r"):      # strictly inside a line
                cut += 1
            cuts = (cut,)
        paths.append(write_fasth(p, recs, final_newline=(fi != 4), cuts=cuts, tag=f"{tag}{fi}_"))
    return paths


def odd_records(rng, n_pairs: int, read_len: int, seqs):
    """Ragged pairs: lengths from {0, 1, 47, 48, 49, read_len - 1, read_len} and uniform ones, the two mates of a pair never alike;
    bases with N, n and lowercase acgt; a third of the records with CRLF; every kind of barcode field."""
    special = [0, 1, 47, 48, 49, read_len - 1, read_len]
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTNnacgt", dtype=np.uint8)
    recs = []
    for q in range(n_pairs):
        ls = []
        for _ in range(2):
            l = special[int(rng.integers(0, len(special)))] if rng.random() < 0.5 else int(rng.integers(0, read_len + 1))
            while ls and l == ls[0]:
                l = int(rng.integers(0, read_len + 1))
            ls.append(l)
        rd = [alphabet[rng.integers(0, len(alphabet), l)].tobytes().decode("ascii") for l in ls]
        qu = [rng.integers(0, 42, l, dtype=np.uint8) for l in ls]
        recs.append(record(rd[0], qu[0], rd[1], qu[1], odd_field(rng, seqs, q % N_FIELD_KINDS), "\r\n" if q % 3 == 0 else "\n"))
    return recs


def records_of_reads(codes, quals, lens, bc, seqs, crlf_every: int = 3):
    """Reads in array form (tests/pathgen.pairs: reads 2q, 2q+1 = one pair, mates share the barcode id; id b > 0 = whitelist line b - 1,
    0 = a sequence off the whitelist) -> records."""
    asc = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    recs = []
    for q in range(codes.shape[0] // 2):
        a, b = 2 * q, 2 * q + 1
        assert bc[a] == bc[b]
        f = (seqs[int(bc[a]) - 1] + ("-1" if q % 2 else "") + (",RAWRAWRAW" if q % 5 == 0 else "")) if bc[a] > 0 else "NNNNNNNNNNNNNNNN-1"
        recs.append(record(asc[a, :int(lens[a])].tobytes().decode("ascii"), quals[a, :int(lens[a])], asc[b, :int(lens[b])].tobytes().decode("ascii"),
                           quals[b, :int(lens[b])], f, "\r\n" if q % crlf_every == 0 else "\n"))
    return recs
