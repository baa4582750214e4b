"""The MarkBads fixtures (tests/golden/bads/: flags the reference's two overloads of MarkBads wrote, tests/golden/make_bads_golden.py)
against the Python restatement (tests/badsref.py) that the GPU tests use beside them, the stated flags of the hand-made pairs
(tests/handbads.py), the a.bad writer, and the presence of the two entry points in the library and its header.  No GPU."""
import re
import struct
from pathlib import Path

import numpy as np
import pytest

import badsref
import goldens
import handbads

ROOT = Path(__file__).resolve().parent.parent


def test_every_case_has_its_fixture():
    assert sorted(p.stem for p in badsref.BADS.glob("*.npz")) == sorted(badsref.ALL) and badsref.GOLDEN == tuple(goldens.CASES)
    limit = max(p.stat().st_size for p in (badsref.BADS.parent / "a48").glob("*.npz"))
    assert all(p.stat().st_size <= limit for p in badsref.BADS.glob("*.npz"))


@pytest.mark.parametrize("name", badsref.ALL)
def test_restatement_reproduces_the_reference(name):
    """Both overloads: the restatement's flags are the reference's, and Sum(bad) is what its driver printed."""
    c = badsref.load(name)
    bad, cnt = badsref.restated(name, False)
    assert np.array_equal(bad, c.bad_plain), np.nonzero(bad != c.bad_plain)[0][:5]
    said = dict(zip(c.ref_summary.split(" | ")[0].split()[1::2], c.ref_summary.split(" | ")[0].split()[2::2]))
    assert int(said["sum_bad_plain"]) == cnt["n_bad_pairs"] == int(c.bad_plain.sum()) and int(said["nonempty"]) == cnt["n_placed"]
    assert int(said["offsets_wrapped"]) == cnt["n_offsets_wrapped"]
    if c.bad_x is None:
        assert int(said["sum_bad_x"]) == -1
        return
    bad_x, cnt_x = badsref.restated(name, True)
    assert np.array_equal(bad_x, c.bad_x), np.nonzero(bad_x != c.bad_x)[0][:5]
    assert int(said["sum_bad_x"]) == cnt_x["n_bad_pairs"] == int(c.bad_x.sum())


def test_both_flag_values_occur_in_both_modes():
    """over the golden cases and their _cut variants (the hand-made cases aside)"""
    for key in ("bad_plain", "bad_x"):
        v = np.concatenate([getattr(badsref.load(n + t), key) for n in badsref.GOLDEN for t in ("", "_cut")])
        assert 0 < v.sum() < len(v)


def test_the_far_case_is_the_reads_golden_input_takes_out():
    import a48ref
    import a48xref
    import extref
    c = badsref.load(badsref.FAR)
    raw = a48xref.parse_paths(a48ref.load("synth_20k_err")["tmp.paths"])
    kept = extref.golden_input((raw[0], raw[1], raw[2]))
    n = len(kept[1])
    removed = np.nonzero((raw[1][:n] > 0) & (kept[1] == 0))[0]
    far = np.nonzero((c.paths[0] < -32767) | (c.paths[0] > 32767))[0]
    assert len(removed) and set(removed) <= set(c.ids[far]) and len(c.ids) % 2 == 0 and np.array_equal(c.ids[0::2] + 1, c.ids[1::2])
    cnt, cnt_x = badsref.restated(badsref.FAR, False)[1], badsref.restated(badsref.FAR, True)[1]
    assert cnt_x["n_offsets_wrapped"] == len(far) >= 1
    # every wrapped offset lands in front of the read: X mode skips all of it, so the flags agree and the mismatch counts do not
    assert (badsref.a48xref.wrap16(c.paths[0][far]) < -256).all() and cnt["n_mismatch_reads"] > cnt_x["n_mismatch_reads"]


@pytest.mark.parametrize("name", list(badsref.HAND) + list(badsref.HAND_PLAIN))
def test_hand_made_pairs_get_their_stated_flags(name):
    """by name: the flag a pair states for each mode is the reference's and the restatement's"""
    c = badsref.load(name)
    bad = badsref.restated(name, False)[0]
    wrong = [p.name for i, p in enumerate(c.pairs) if bool(bad[i]) != p.plain or bool(c.bad_plain[i]) != p.plain]
    assert not wrong, wrong
    if c.bad_x is not None:
        bad_x = badsref.restated(name, True)[0]
        wrong = [p.name for i, p in enumerate(c.pairs) if bool(bad_x[i]) != p.x or bool(c.bad_x[i]) != p.x]
        assert not wrong, wrong
        assert any(p.plain != p.x for p in c.pairs)


@pytest.mark.parametrize("K", (48, 60))
def test_hand_made_premises(K):
    """what the pairs are for: a badsum of exactly 150 and 151, lengths 0, 1 and 256, the three offsets an int16 cannot hold"""
    c = badsref.load(f"hand_k{K}")
    sums: list = []
    badsref.mark_bads(c.g, c.eb, c.codes, c.lens, c.quals, *c.paths, False, sums)
    by = {p.name: (sums[2 * i], sums[2 * i + 1]) for i, p in enumerate(c.pairs)}
    assert by["sum_150"][0] == 150 and by["sum_151"][0] == 151 and by["split_150_150"] == (150, 150)
    assert by["epos_minus_1"][0] == 150 and by["epos_0"][0] == 151 and by["epos_end"][0] == 150 and by["epos_last"][0] == 151
    for tag in ("fw", "rc"):
        assert by[f"{tag}_150"][0] == 150 and all(by[f"{tag}_edge{j}_{w}"][0] == 151 for j in (1, 2) for w in ("last_overlap", "first_own"))
    assert by["all_mismatch_top_quality"][0] == 256 * handbads.QMAX and by["mate_without_path"][1] is None
    assert {0, 1, 256} <= set(int(x) for x in c.lens)
    assert {65541, 32768, -32769} <= set(int(x) for x in c.paths[0])
    e_rc = {handbads.edge_index(c.eb)[s] for p in c.pairs if p.name.startswith("rc_") for s in p.reads[0].path}
    assert len(e_rc) == 3


@pytest.mark.parametrize("K", (48, 60))
def test_x_mode_refuses_what_a_readpathvecx_cannot_hold(K):
    c = badsref.load(f"handplain_k{K}")
    h = handbads.case(K, plain_only=True)
    for only, code in ((("nonadjacent_later_wins",), "arg"), (("path_256_edges_150",), "unsupported")):
        codes, quals, lens, paths = handbads.arrays(h, handbads.edge_index(c.eb), only=only)
        with pytest.raises(badsref.Refused) as ei:
            badsref.mark_bads(c.g, c.eb, codes, lens, quals, *paths, True)
        assert ei.value.code == code
        assert len(badsref.mark_bads(c.g, c.eb, codes, lens, quals, *paths, False)[0]) == 1
    assert int(c.paths[1].max()) == 256


# ---- the file

def test_write_bad_bytes(snk, tmp_path):
    """a.bad is BinaryWriter::writeFile(vec<Bool>): "BINWRITE", the count as u64, one byte per pair"""
    from supernova_amd import graphio
    c = badsref.load("adversarial_cut")
    graphio.write_bad(tmp_path / "a.bad", c.bad_x)
    assert (tmp_path / "a.bad").read_bytes() == b"BINWRITE" + struct.pack("<Q", len(c.bad_x)) + c.bad_x.tobytes()
    graphio.write_bad(tmp_path / "e.bad", np.zeros(0, np.uint8))
    assert (tmp_path / "e.bad").read_bytes() == b"BINWRITE" + struct.pack("<Q", 0)


def test_write_a48_writes_a_bad_only_when_asked(snk, tmp_path):
    import a48ref
    import a48xref
    from supernova_amd import graphio
    name = "synth_2k_err"
    gc = goldens.load(name)
    files = a48ref.load(name)
    off, ne, edges = a48xref.parse_paths(files["tmp.paths"])
    E = a48xref.parse_hbv(gc.exp_ahbv).E
    info = dict(paths_index=(np.zeros(E + 1, np.uint64), np.zeros(0, np.uint64)), countsb=np.zeros(E, np.int32), dups=dict(dup=np.zeros(len(ne) // 2, np.uint8)))
    u = graphio.unitigs_to_arrays(gc.exp_unitigs)
    graphio.write_a48(tmp_path / "without", 48, *u, off, ne, edges, info)
    bad = badsref.load(name).bad_x
    graphio.write_a48(tmp_path / "with", 48, *u, off, ne, edges, dict(info, bads=dict(bad=bad)))
    names = lambda d: sorted(p.name for p in d.iterdir())
    assert "a.bad" not in names(tmp_path / "without") and names(tmp_path / "with") == sorted(names(tmp_path / "without") + ["a.bad"])
    for f in names(tmp_path / "without"):
        assert (tmp_path / "with" / f).read_bytes() == (tmp_path / "without" / f).read_bytes()
    assert (tmp_path / "with" / "a.bad").read_bytes() == b"BINWRITE" + struct.pack("<Q", len(bad)) + bad.tobytes()


# ---- the entry points

def test_library_exports_and_header_declares_the_entry_points(snk):
    text = (ROOT / "include" / "snk.h").read_text()
    for sym in ("snk_dev_mark_bads", "snk_dev_mark_bads_df"):
        assert hasattr(snk, sym), f"libsnk.so does not export {sym}"
        assert re.search(rf"^int {sym}\(snk_ctx\* ctx, uint32_t K,", text, re.M), f"include/snk.h does not declare {sym}"
    assert re.search(r"^#define SNK_BADS_X 1u", text, re.M) and "typedef struct snk_dev_bads {" in text
    from supernova_amd import lib
    assert lib.BADS_X == 1 and {"snk_dev_mark_bads", "snk_dev_mark_bads_df"} <= set(lib.exported_symbols())
