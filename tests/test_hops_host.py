"""The FindEdgePairs fixtures (tests/golden/hops/: pairs and a.hops bytes the reference's own function wrote,
tests/golden/make_hops_golden.py) against the Python restatement (tests/hopsref.py) that the GPU tests use beside them, the stated
outcomes of the hand-made items (tests/handhops.py), the a.hops writer and reader, and the argument refusals that need no device.
No GPU."""
import ctypes as C
import re
import struct
from pathlib import Path

import numpy as np
import pytest

import goldens
import handhops
import hopsref

ROOT = Path(__file__).resolve().parent.parent
SNK_E_ARG, SNK_E_IO = -1, -5


def test_every_case_has_its_fixture():
    assert sorted(p.stem for p in hopsref.HOPS.glob("*.npz")) == sorted(hopsref.ALL) and hopsref.GOLDEN == tuple(goldens.CASES)
    limit = max(p.stat().st_size for p in (hopsref.HOPS.parent / "a48").glob("*.npz"))
    assert all(p.stat().st_size <= limit for p in hopsref.HOPS.glob("*.npz"))


@pytest.mark.parametrize("name", hopsref.ALL)
def test_restatement_reproduces_the_reference(name):
    """Both flag settings: the restatement's pairs are the reference's, the stored counts are the restatement's, the file's bytes are
    magic, count, two ints per pair, and the pair count is what the reference's driver printed."""
    c = hopsref.load(name)
    for og, want, hops, cnt, line in ((False, c.pairs, c.hops, c.counts, 0), (True, c.pairs_one_good, c.hops_one_good, c.counts_one_good, 1)):
        pairs, info = hopsref.restated(name, og)
        assert np.array_equal(pairs, want), (og, len(pairs), len(want))
        assert {k: info[k] for k in hopsref.COUNTERS} == cnt
        assert info["n_two_class"] == info["n_ext_round0"] + info["n_ext_closure"] + info["n_not_extended"]
        assert hopsref.hops_bytes(want) == hops
        said = c.ref_summary.split(" | ")[line].split()
        said = dict(zip(said[1::2], said[2::2]))
        assert int(said["pairs"]) == len(want) and int(said["one_good"]) == int(og) and int(said["reads"]) == len(c.paths[1]) and float(said["seconds"]) > 0
        assert (np.diff(want[:, 0].astype(np.int64) << 32 | want[:, 1]) > 0).all(), "the pairs ascend"
    assert c.only == tuple(len(hopsref.only_part(hopsref.restated(name, False)[1], k)) for k in range(3))


@pytest.mark.parametrize("names", (hopsref.GOLDEN + hopsref.GENERATED, tuple(hopsref.HAND)))
def test_every_part_gives_a_pair_of_its_own_and_one_good_matters(names):
    """from the counts stored in the fixtures: over the golden and generated cases, and again over the hand-made ones, each part
    contributes a pair no other part does, and the two flag settings differ somewhere"""
    only = np.sum([hopsref.load(n).only for n in names], axis=0)
    assert (only >= 1).all(), only
    assert any(hopsref.load(n).hops != hopsref.load(n).hops_one_good for n in names)
    for k in ("n_ext_round0", "n_ext_closure", "n_not_extended", "n_sink_edges"):
        assert sum(hopsref.load(n).counts[k] for n in names) >= 1, k


def test_the_gapped_case_is_what_it_is_for():
    """dead-ended contigs that pairs of several barcodes span: every edge is a sink, and part 1 pairs them up"""
    c = hopsref.load("gapped")
    assert len(c.paths[1]) <= 20000 and c.counts["n_sink_edges"] >= 4 and c.counts["n_part1"] >= 2 and len(np.unique(c.bc)) >= 10


@pytest.mark.parametrize("K", (48, 60))
def test_hand_made_items_get_their_stated_outcome(K):
    """by name: what an item states for each flag setting is the reference's and the restatement's"""
    name = f"hand_k{K}"
    c, h = hopsref.load(name), handhops.case(K)
    edge_of = handhops.edge_index(c.eb)
    handhops.assert_items(h, edge_of, c.inv, {0: c.pairs, 1: c.pairs_one_good}, "the reference")
    handhops.assert_items(h, edge_of, c.inv, {0: hopsref.restated(name, False)[0], 1: hopsref.restated(name, True)[0]}, "the restatement")
    names = {it.name for it in h.items}
    assert {"sink_stub_120", "sink_stub_121_and_one_good", "sink_end_has_second_in_edge", "sink_end_has_out_edge", "one_class", "all_bc_zero_is_one_class", "e2_is_e1",
            "part2_landing_99", "part2_landing_100", "part2_same_vertex", "part2_e1_seen_by_part1", "part3_start_K", "part3_start_K_plus_1", "part3_round0_99",
            "part3_round0_100", "part3_closure_3_links", "part3_closure_2_links", "part3_closure_loop_with_tail", "part3_overlap_mismatch", "part3_right_39",
            "part3_right_40", "part3_too_easy", "part3_only_bad_pairs", "part3_f_is_inv_e", "part3_palindrome", "part3_edge_twice_on_a_path"} <= names
    assert any(a != b for it in h.items for a, b in it.expect.values()) and any(a for it in h.items for a, _ in it.expect.values())


@pytest.mark.parametrize("K", (48, 60))
def test_hand_made_premises(K):
    """what the items are for, from the graph itself: the stub lengths, the landing lengths, how each part-3 edge was settled"""
    c, h = hopsref.load(f"hand_k{K}"), handhops.case(K)
    edge_of = handhops.edge_index(c.eb)
    by = {it.name: it for it in h.items}
    km = lambda s: int(c.km[edge_of[s]])
    first = lambda name: by[name].pairs[0][0][0]
    stub = lambda name: max(km(s) for s in edge_of if s.startswith(first(name)[-(K - 1):]))
    assert stub("sink_stub_120") == 120 and stub("sink_stub_121_and_one_good") == 121
    assert km(by["part2_landing_100"].pairs[0][1][0]) == 100 and km(by["part2_landing_99"].pairs[0][1][0]) == 99
    assert km(first("part3_start_K")) == K and km(first("part3_start_K_plus_1")) == K + 1
    assert km(handhops.rc(by["part3_right_40"].pairs[0][1][0])) == 40 and km(handhops.rc(by["part3_right_39"].pairs[0][1][0])) == 39
    how: dict = {}
    hopsref.find_edge_pairs(c.g, c.km, c.inv, c.paths[1], c.paths[2], c.bc, c.bad, False, how)
    settled = lambda name: how.get(edge_of[first(name)])
    assert settled("part3_round0_100") == "round0" and settled("part3_round0_99") == "not_extended"
    assert settled("part3_closure_3_links") == "closure" and settled("part3_closure_2_links") == "not_extended"
    assert settled("part3_closure_loop_with_tail") == "closure" and settled("part3_closure_loop_without_tail") == "not_extended"
    assert settled("part3_overlap_match") == "closure" and settled("part3_overlap_mismatch") == "not_extended"
    assert settled("part3_start_K") is None and settled("part3_one_class") is None
    pal = first("part3_palindrome")
    assert pal == handhops.rc(pal) and c.inv[edge_of[pal]] == edge_of[pal]
    loop = by["part3_closure_loop_with_tail"].pairs[2][0][1]
    assert km(loop) == 1 and c.g.v_left[edge_of[loop]] == c.g.v_right[edge_of[loop]]
    twice = by["part3_edge_twice_on_a_path"].pairs[0][0]
    assert twice[1] == twice[2]


# ---- the file

def test_write_and_read_hops(snk, tmp_path):
    """a.hops is BinaryWriter::writeFile(vec<pair<int,int>>): the writer gives every fixture's bytes (the reference's file), the reader
    gives the pairs back, and a file that is not one is refused"""
    from supernova_amd import graphio, lib as _lib
    for name in hopsref.ALL:
        c = hopsref.load(name)
        for pairs, hops in ((c.pairs, c.hops), (c.pairs_one_good, c.hops_one_good)):
            graphio.write_hops(tmp_path / "a.hops", pairs)
            assert (tmp_path / "a.hops").read_bytes() == hops
            back = graphio.read_hops(tmp_path / "a.hops")
            assert back.dtype == np.int32 and back.shape == pairs.shape and np.array_equal(back, pairs)
    graphio.write_hops(tmp_path / "e.hops", np.zeros((0, 2), np.int32))
    assert (tmp_path / "e.hops").read_bytes() == b"BINWRITE" + struct.pack("<Q", 0) and graphio.read_hops(tmp_path / "e.hops").shape == (0, 2)
    (tmp_path / "short.hops").write_bytes(hopsref.load("adversarial").hops[:-4])
    (tmp_path / "magic.hops").write_bytes(b"BINWRITX" + hopsref.load("adversarial").hops[8:])
    for bad in ("short.hops", "magic.hops", "missing.hops"):
        with pytest.raises(_lib.SnkError) as ei:
            graphio.read_hops(tmp_path / bad)
        assert ei.value.code == SNK_E_IO
    err = C.create_string_buffer(256)
    assert snk.snk_write_hops(None, 0, None, err, 256) == SNK_E_ARG and snk.snk_write_hops(str(tmp_path / "x").encode(), 1, None, err, 256) == SNK_E_ARG
    n, p = C.c_uint64(7), C.POINTER(C.c_int32)()
    assert snk.snk_read_hops(None, C.byref(n), C.byref(p), err, 256) == SNK_E_ARG
    assert snk.snk_read_hops(str(tmp_path / "missing.hops").encode(), C.byref(n), C.byref(p), err, 256) == SNK_E_IO and n.value == 0 and not p


def test_write_a48_writes_a_hops_only_when_asked(snk, tmp_path):
    import a48ref
    import a48xref
    from supernova_amd import graphio
    name = "synth_4k_dups"
    gc = goldens.load(name)
    off, ne, edges = a48xref.parse_paths(a48ref.load(name)["tmp.paths"])
    E = a48xref.parse_hbv(gc.exp_ahbv).E
    info = dict(paths_index=(np.zeros(E + 1, np.uint64), np.zeros(0, np.uint64)), countsb=np.zeros(E, np.int32), dups=dict(dup=np.zeros(len(ne) // 2, np.uint8)))
    u = graphio.unitigs_to_arrays(gc.exp_unitigs)
    graphio.write_a48(tmp_path / "without", 48, *u, off, ne, edges, info)
    fx = hopsref.load(name)
    graphio.write_a48(tmp_path / "with", 48, *u, off, ne, edges, dict(info, hops=fx.pairs))
    names = lambda d: sorted(p.name for p in d.iterdir())
    assert names(tmp_path / "without") == ["a.countsb", "a.dup", "a.hbv", "a.inv", "a.paths", "a.paths.inv"], "the file set of a result without 'hops' changed"
    assert names(tmp_path / "with") == sorted(names(tmp_path / "without") + ["a.hops"])
    for f in names(tmp_path / "without"):
        assert (tmp_path / "with" / f).read_bytes() == (tmp_path / "without" / f).read_bytes()
    assert (tmp_path / "with" / "a.hops").read_bytes() == fx.hops and len(fx.pairs) > 0


# ---- the entry point

def test_library_exports_and_header_declares_the_entry_points(snk):
    text = (ROOT / "include" / "snk.h").read_text()
    for sym in ("snk_dev_edge_pairs", "snk_write_hops", "snk_read_hops"):
        assert hasattr(snk, sym), f"libsnk.so does not export {sym}"
        assert re.search(rf"^int {sym}\(", text, re.M), f"include/snk.h does not declare {sym}"
    assert re.search(r"^#define SNK_HOPS_ONE_GOOD 1u", text, re.M) and re.search(r"^#define SNK_HOPS_EXT_HOST 2u", text, re.M) and "typedef struct snk_dev_hops {" in text
    from supernova_amd import lib
    assert (lib.HOPS_ONE_GOOD, lib.HOPS_EXT_HOST) == (1, 2) and {"snk_dev_edge_pairs", "snk_write_hops", "snk_read_hops"} <= set(lib.exported_symbols())
    assert C.sizeof(lib.SnkDevHops) == 152


def test_refusals_that_need_no_device(snk):
    """NULL arguments, unknown flags, an odd read count, a K that is not supported, an inv that is no involution, a paths index of
    another graph: refused before a context is touched (the context pointer is never followed), *out all zero"""
    from supernova_amd import lib as _lib
    c = hopsref.load("hand_k48")
    from supernova_amd import graphio
    u = graphio.unitigs_to_arrays(c.unitigs)
    n, tot = len(c.paths[1]), len(c.paths[2])
    inv = np.ascontiguousarray(c.inv, np.int32)
    fake = C.c_void_p(16)            # stands for device memory and for the context: none of these calls gets as far as using it

    def call(h, K=48, n_reads=n, flags=0, inv=inv, px=None, ctx=fake, bc=fake):
        p = _lib.SnkDevPaths()
        p.n_reads, p.n_edges_total = n_reads, tot
        p.offset = p.n_edges = p.start = p.edges = fake.value
        out = _lib.SnkDevHops()
        C.memset(C.byref(out), 0xAB, C.sizeof(out))
        err = C.create_string_buffer(512)
        rc = snk.snk_dev_edge_pairs(ctx, K, len(u[0]) - 1, fake, fake, C.byref(h), inv.ctypes.data if inv is not None else None, C.byref(p),
                                    C.byref(px) if px is not None else None, bc, fake, flags, 0, C.byref(out), None, err, 512)
        return rc, err.value.decode(), bytes(out) == bytes(C.sizeof(out))

    with graphio.hbv_handle(48, *u) as h:
        not_inv = inv.copy()
        not_inv[[0, 1]] = not_inv[[1, 0]] if inv[0] != 1 else inv[[2, 2]]
        px_e, px_n = _lib.SnkDevPidx(), _lib.SnkDevPidx()
        px_e.n_hbv_edges, px_e.n_entries, px_e.index_off, px_e.index_ids = c.g.E + 1, tot, fake.value, fake.value
        px_n.n_hbv_edges, px_n.n_entries, px_n.index_off, px_n.index_ids = c.g.E, tot + 1, fake.value, fake.value
        for what, kw, code in (("ctx", dict(ctx=None), SNK_E_ARG), ("flags", dict(flags=4), SNK_E_ARG), ("odd", dict(n_reads=n - 1), SNK_E_ARG), ("K", dict(K=32), -6),
                               ("inv NULL", dict(inv=None), SNK_E_ARG), ("inv", dict(inv=not_inv), SNK_E_ARG), ("px edges", dict(px=px_e), SNK_E_ARG),
                               ("px entries", dict(px=px_n), SNK_E_ARG), ("bc NULL", dict(bc=None), SNK_E_ARG)):
            rc, msg, zero = call(h, **kw)
            assert rc == code and msg and zero, (what, rc, msg)
