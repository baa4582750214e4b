"""The Python binding's shared pieces, without a device: the one checked call (lib.call), the two struct builders (engine.dev_reads,
engine.dev_paths), and a scan that keeps every module of the package on them."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def test_the_package_has_one_checked_call_and_one_builder_per_struct():
    """supernova_amd/*.py: the error buffer is made and SnkError is constructed in lib.py alone (lib.call / lib.check); SnkDevReads() and
    SnkDevPaths() are each constructed in one module -- engine.py: dev_reads, and dev_paths for a stage's input next to the two
    out-structs that C fills (path_reads2, unzip)."""
    where = {"buf": set(), "err": set(), "reads": {}, "paths": {}}
    n_files = 0
    for f in sorted((ROOT / "supernova_amd").glob("*.py")):
        text = f.read_text()
        n_files += 1
        if "create_string_buffer(512" in text or re.search(r"create_string_buffer\(\s*(_lib\.)?ERRCAP", text):
            where["buf"].add(f.name)
        if re.search(r"(?<!class )\bSnkError\(", text):
            where["err"].add(f.name)
        for key, name in (("reads", "SnkDevReads()"), ("paths", "SnkDevPaths()")):
            if text.count(name):
                where[key][f.name] = [ln.strip() for ln in text.splitlines() if name in ln]
    assert n_files >= 10
    assert where["buf"] == {"lib.py"} and where["err"] == {"lib.py"}
    assert list(where["reads"]) == ["engine.py"] and len(where["reads"]["engine.py"]) == 1
    assert list(where["paths"]) == ["engine.py"]
    made = where["paths"]["engine.py"]
    assert len(made) == 3 and sum(ln.startswith("p = ") for ln in made) == 1          # the builder's ...
    assert sum("snk_dev_paths_unzip" in ln or ln == "out = _lib.SnkDevPaths()" for ln in made) == 2          # ... and the two C fills


def _raw(snk, fn, *args):
    err = C.create_string_buffer(512)
    return fn(*args, err, 512), err.value.decode(errors="replace")


def test_call_returns_none_or_raises_what_the_raw_call_reports(snk, tmp_path):
    from supernova_amd import lib
    assert lib.ERRCAP == 512
    assert lib.call(snk.snk_option_check, b"path_slots_x10", 30) is None
    rc, text = _raw(snk, snk.snk_option_check, b"no_such_option", 1)
    assert rc != 0 and text
    with pytest.raises(lib.SnkError) as ex:
        lib.call(snk.snk_option_check, b"no_such_option", 1)
    assert ex.value.code == rc and str(ex.value) == f"libsnk error {rc}: {text}"

    missing = str(tmp_path / "none.bv").encode()
    out = lambda: (C.byref(C.c_uint64(0)), C.byref(C.POINTER(C.c_uint64)()), C.byref(C.POINTER(C.c_uint8)()))
    rc, text = _raw(snk, snk.snk_read_bv, missing, *out())
    assert rc != 0 and text
    with pytest.raises(lib.SnkError) as ex:
        lib.call(snk.snk_read_bv, missing, *out())
    assert ex.value.code == rc and str(ex.value) == f"libsnk error {rc}: {text}"


@pytest.mark.parametrize("n_edges", [[], [2], [3, -1, 2]])
def test_dev_paths_points_into_the_tensors_and_reads_n_edges_as_u32(snk, n_edges):
    from supernova_amd.engine import dev_paths
    n = len(n_edges)
    ne = torch.tensor(n_edges, dtype=torch.int32)
    off = torch.arange(n, dtype=torch.int32)
    edges = torch.arange(7, dtype=torch.int32)
    p, start = dev_paths(off, ne, edges)
    assert (p.n_reads, p.n_edges_total) == (n, 7)
    assert (p.offset, p.n_edges, p.edges) == tuple(t.data_ptr() or None for t in (off, ne, edges))
    assert start.dtype == torch.int64 and start.device == ne.device and p.start == start.data_ptr()
    want = [0]
    for v in n_edges:
        want.append(want[-1] + (v & 0xFFFFFFFF))
    assert start.tolist() == want
    if n == 3:
        assert want[2] - want[1] == 4294967295
    given = torch.zeros(n + 1, dtype=torch.int64)
    p2, back = dev_paths(off, ne, edges, given)
    assert back is given and p2.start == given.data_ptr() and given.tolist() == [0] * (n + 1)


def test_dev_reads_fills_what_it_is_given_and_nothing_else(snk):
    from supernova_amd.engine import dev_reads
    rows = torch.zeros((5, 3), dtype=torch.int32)
    r = dev_reads(rows, 40)
    assert (r.n_reads, r.rows, r.row_words, r.read_len) == (5, rows.data_ptr(), 3, 40)
    assert (r.quals, r.qstride, r.lens, r.good_len, r.bc, r.group) == (None, 0, None, None, None, None)
    assert (r.ign_bc_below, r.read_index_base, r.reserved0) == (0, 0, 0)
    flat = dev_reads(rows.view(-1), 40)
    assert (flat.n_reads, flat.row_words) == (15, 0)
    quals = torch.zeros((5, 48), dtype=torch.uint8)
    lens, good, bc, group = (torch.zeros(5, dtype=dt) for dt in (torch.int16, torch.int16, torch.int32, torch.int32))
    r = dev_reads(rows, 40, quals, lens, good, bc, group, ign_bc_below=-7, read_index_base=1 << 40)
    assert (r.quals, r.qstride) == (quals.data_ptr(), 48)
    assert (r.lens, r.good_len, r.bc, r.group) == (lens.data_ptr(), good.data_ptr(), bc.data_ptr(), group.data_ptr())
    assert (r.ign_bc_below, r.read_index_base) == (-7, 1 << 40)
    r = dev_reads(rows, 40, bc=bc)
    assert r.bc == bc.data_ptr() and (r.quals, r.lens, r.good_len, r.group) == (None, None, None, None)
