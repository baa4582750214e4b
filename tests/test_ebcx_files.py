"""a.ebcx without a GPU: the numpy restatement of computeEdgeToBarcodeX (tests/ebcxref.py) against the lists the reference's own code
wrote (tests/golden/ebcx/, see make_ebcx_golden.py), and the host writer / reader of the file against those bytes."""
import ctypes as C
import struct

import numpy as np
import pytest

import ebcxref

SNK_E_IO = -5


@pytest.mark.parametrize("name", ebcxref.CASES)
def test_restatement_gives_the_reference_lists(name):
    f = ebcxref.load(name)
    off, bcs = ebcxref.parse_ebcx(f.ebcx)
    assert len(off) == f.E + 1
    x_off, x_bcs = ebcxref.edge_barcodes(f.n_edges, f.edges, f.bc, f.inv)
    assert np.array_equal(off, x_off) and np.array_equal(bcs, x_bcs)
    assert ebcxref.ebcx_bytes(off, bcs) == f.ebcx
    # what the fixture is: reads sorted by barcode, bci = the runs of equal bc (an empty run repeats a start), the lists strictly ascending
    pos = f.bc[f.bc > 0]
    assert np.all(np.diff(pos.astype(np.int64)) >= 0) and np.all(np.diff(f.bci) >= 0)
    for e in range(f.E):
        assert np.all(np.diff(bcs[int(off[e]):int(off[e + 1])].astype(np.int64)) > 0), e
    assert "EBCX_DRIVER" in f.ref_summary and " ms" in f.ref_summary


def test_the_probe_does_what_it_is_for():
    """The properties make_ebcx_golden.py asserted before it saved the probe, read off the fixture again."""
    f, g = ebcxref.load("ebcx_probe"), ebcxref.load("ebcx_probe_ends_empty")
    off, bcs = ebcxref.parse_ebcx(f.ebcx)
    n = np.diff(off.astype(np.int64))
    runs = np.diff(f.bci)
    first = f.bc[np.minimum(f.bci[:-1], len(f.bc) - 1)]
    assert first[0] == 0 and -1 in f.bc[f.bci[1:-2]] and 0 in runs[1:-1] and runs[-1] > 0
    assert n.max() > 256 and 700 in runs and 255 in f.n_edges and int(bcs.max()) == 2**31 - 1
    assert np.any((f.n_edges == 0) & (f.bc > 0))
    self_inv = np.nonzero(f.inv == np.arange(f.E))[0]
    assert any(n[e] == 2 for e in self_inv)
    assert n[0] == 1 and n[f.E - 1] == 1
    g_off, _ = ebcxref.parse_ebcx(g.ebcx)
    assert g_off[1] == g_off[0] and g_off[g.E] == g_off[g.E - 1]


@pytest.mark.parametrize("name", ebcxref.CASES)
def test_writer_gives_the_fixture_bytes_and_the_reader_gives_them_back(snk, tmp_path, name):
    from supernova_amd import graphio
    f = ebcxref.load(name)
    off, bcs = ebcxref.parse_ebcx(f.ebcx)
    graphio.write_ebcx(tmp_path / "a.ebcx", off, bcs)
    assert (tmp_path / "a.ebcx").read_bytes() == f.ebcx
    r_off, r_bcs = graphio.read_ebcx(tmp_path / "a.ebcx")
    assert r_off.dtype == np.uint64 and r_bcs.dtype == np.int32
    assert np.array_equal(r_off, off) and np.array_equal(r_bcs, bcs)


@pytest.mark.parametrize("E", [0, 1, 5])
def test_no_edges_and_all_empty_lists(snk, tmp_path, E):
    from supernova_amd import graphio
    off = np.zeros(E + 1, np.uint64)
    graphio.write_ebcx(tmp_path / "a.ebcx", off, np.zeros(0, np.int32))
    b = (tmp_path / "a.ebcx").read_bytes()
    assert b == ebcxref.ebcx_bytes(off, np.zeros(0, np.int32)) and len(b) == 24 + 8 * (E + 1)
    p_off, p_bcs = ebcxref.parse_ebcx(b)
    assert np.array_equal(p_off, off) and len(p_bcs) == 0
    r_off, r_bcs = graphio.read_ebcx(tmp_path / "a.ebcx")
    assert np.array_equal(r_off, off) and len(r_bcs) == 0


def _refused(snk, path):
    E = C.c_uint64(7)
    po, pb = C.POINTER(C.c_uint64)(), C.POINTER(C.c_int32)()
    err = C.create_string_buffer(512)
    rc = snk.snk_read_ebcx(str(path).encode(), C.byref(E), C.byref(po), C.byref(pb), err, 512)
    assert not po and not pb and E.value == 0
    return rc, err.value


def test_reader_refuses_files_that_do_not_add_up(snk, tmp_path):
    from supernova_amd import graphio
    f = ebcxref.load("adversarial")
    p = tmp_path / "bad.ebcx"
    for cut in (0, 10, 24, len(f.ebcx) - 8, len(f.ebcx) - 1):                 # truncated: inside the control block, the lists, the table
        p.write_bytes(f.ebcx[:cut])
        rc, msg = _refused(snk, p)
        assert rc == SNK_E_IO and b"snk_read_ebcx" in msg, cut
    p.write_bytes(f.ebcx + bytes(8))                                           # ... and longer than its control block says
    assert _refused(snk, p)[0] == SNK_E_IO
    var, fixed = struct.unpack_from("<QQ", f.ebcx, 8)
    E = (fixed - var) // 8 - 1
    assert E == f.E
    tab = np.frombuffer(f.ebcx[var:fixed], "<u8").copy()
    mid = int(np.argmax(np.diff(tab.astype(np.int64)) > 0)) + 1               # the end of the first list that is not empty

    def with_table(t):
        return f.ebcx[:var] + t.astype("<u8").tobytes()

    for what, t in (("decreases", np.concatenate([tab[:mid], [tab[mid - 1] - 4], tab[mid + 1:]]) if tab[mid - 1] > 24 else None),
                    ("leaves the data", np.concatenate([tab[:mid], [var + 4], tab[mid + 1:]])),
                    ("does not start at the data", np.concatenate([[28], tab[1:]])),
                    ("does not end at the table", np.concatenate([tab[:-1], [var - 4]])),
                    ("splits an int", np.concatenate([tab[:mid], [tab[mid] - 2], tab[mid + 1:]]))):
        if t is None:
            continue
        p.write_bytes(with_table(t))
        rc, msg = _refused(snk, p)
        assert rc == SNK_E_IO and b"does not add up" in msg, what
    bad = bytearray(f.ebcx)
    bad[7] = 8                                                                 # sizeof(int) in the control block
    p.write_bytes(bytes(bad))
    assert _refused(snk, p)[0] == SNK_E_IO
    assert _refused(snk, tmp_path / "none.ebcx")[0] == SNK_E_IO
    p.write_bytes(f.ebcx)                                                      # the reader still reads
    off, bcs = graphio.read_ebcx(p)
    assert np.array_equal(off, ebcxref.parse_ebcx(f.ebcx)[0])


def test_writer_refuses_offsets_that_are_no_lists(snk, tmp_path):
    from supernova_amd import lib as _lib
    err = C.create_string_buffer(512)
    bcs = np.arange(1, 5, dtype=np.int32)
    for off in ([1, 2, 4], [0, 3, 2]):
        o = np.array(off, np.uint64)
        assert snk.snk_write_ebcx(str(tmp_path / "x").encode(), 2, o.ctypes.data, bcs.ctypes.data, err, 512) == -1 and b"ebc_off" in err.value
    assert snk.snk_write_ebcx(None, 0, None, None, err, 512) == -1
    assert _lib.EBC_GENERAL_SORT == 1 and C.sizeof(_lib.SnkDevEbcx) == 120
