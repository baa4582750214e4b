"""MowLawn without a GPU: the two forms of the Python restatement (tests/mowref.py) against the fixtures the reference's own MowLawn
left (tests/golden/mow/, see tests/golden/make_mow_golden.py), the stated outcomes of the hand-made motifs (tests/handmow.py), the
reference's dup against MarkDups as the project restates it, and the declaration and binding of snk_dev_mow_lawn."""
import re
from pathlib import Path

import numpy as np
import pytest

import mowgen
import mowref

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(mowgen.HAND) + [mowgen.WIDE] + [f"fuzz_{s}" for s in mowgen.FUZZ_SEEDS] + list(mowgen.GOLDEN)


@pytest.fixture(autouse=True, scope="module")
def _bound(snk):
    """everything here is about snk_dev_mow_lawn: without its binding nothing in this file says anything"""
    from supernova_amd import lib
    assert "snk_dev_mow_lawn" in lib.exported_symbols() and tuple(mowref.COUNTERS) == lib.MOW_COUNTERS


def test_every_case_has_its_fixture():
    assert mowref.names() == sorted(NAMES)
    for n in NAMES:
        s = mowref.load(n).ref_summary
        assert s.startswith("MOW_DRIVER") and " threads 1 " in s, n


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name):
    """both forms give the reference's dels and scored: one visit per path entry, window first, is the same rule"""
    c = mowref.load(name)
    dels, scored, cnt = mowref.restated(name)
    assert np.array_equal(dels, c.dels) and np.array_equal(scored, c.scored)
    d1, s1 = mowref.mow_literal(c.g, c.eb, c.inv, c.codes, c.lens, c.quals, *c.paths, c.dup)
    assert np.array_equal(d1, c.dels) and np.array_equal(s1, c.scored)
    assert cnt["n_candidates"] - cnt["n_too_many_reads"] == len(scored) and cnt["n_deleted_candidates"] * 2 >= len(dels)
    assert cnt["n_entries_in_window"] <= cnt["n_entries_on_candidates"] and cnt["n_records"] + cnt["n_reads_hq_excluded"] <= cnt["n_entries_in_window"]
    assert np.array_equal(np.unique(dels), dels) and all(int(c.inv[e]) in set(dels.tolist()) for e in dels)


@pytest.mark.parametrize("name", list(mowgen.HAND) + [mowgen.WIDE])
def test_stated_outcomes(name):
    """every hand-made motif does what is stated next to it"""
    c = mowref.load(name)
    dels, scored, _ = mowref.restated(name)
    kmers = np.array([len(b) - c.K + 1 for b in c.eb])
    cands = {(e1, e2) for _, e1, e2 in mowref.candidates(c.g, kmers)}
    rows = {(int(r[0]), int(r[1])): (int(r[2]), int(r[3])) for r in scored}
    gone = set(dels.tolist())
    stated = 0
    for m in c.motifs:
        k = (c.edge_of[m.e1], c.edge_of[m.e2])
        got = "none" if k not in cands else "limit" if k not in rows else "deleted" if k[1] in gone else "kept"
        if m.outcome is not None:
            assert got == m.outcome, (m.name, got, rows.get(k))
            stated += 1
        if m.qss is not None:
            assert rows[k] == tuple(m.qss), (m.name, rows[k])
    assert stated >= (20 if name in mowgen.HAND else 1)
    if name in mowgen.HAND:
        assert {m.outcome for m in c.motifs} >= {"deleted", "kept", "limit", "none"}


def test_wide_crosses_the_partitions():
    """one e1 with thousands of entries of which few reach the window, and one group of more than 64 records"""
    c = mowref.load(mowgen.WIDE)
    detail: dict = {}
    _, _, cnt = mowref.mow_entries(c.g, c.eb, c.inv, c.codes, c.lens, c.quals, *c.paths, c.dup, detail)
    m = c.motifs[0]
    d = detail[(c.edge_of[m.e1], c.edge_of[m.e2])]
    n_e1 = int((c.paths[2] == c.edge_of[m.e1]).sum() + (c.paths[2] == c.inv[c.edge_of[m.e1]]).sum())
    assert n_e1 >= 3000 and 100 <= len(d.records) <= 400
    groups: dict = {}
    for fw, off, _ in d.records:
        groups[(fw, off)] = groups.get((fw, off), 0) + 1
    assert max(groups.values()) > 64
    assert cnt["n_entries_in_window"] < cnt["n_entries_on_candidates"] and cnt["n_candidates"] > 300


@pytest.mark.parametrize("name", NAMES)
def test_dup_is_what_mark_dups_gives(name):
    """the fixture's dup -- MarkDups version 2 of the reference -- equals MarkDups as the project has it (version 1, restated)"""
    c = mowref.load(name)
    assert np.array_equal(mowgen.dup_of(c), c.dup)


def test_fuzz_outcomes_all_occur():
    seen = dict.fromkeys(("deleted", "limit", "qss1", "qss2", "void_group", "hq_excluded", "dup"), 0)
    for s in mowgen.FUZZ_SEEDS:
        c = mowref.load(f"fuzz_{s}")
        _, scored, cnt = mowref.restated(f"fuzz_{s}")
        for r in scored:
            seen["deleted" if r[2] >= 300 and r[3] <= 30 else "qss1" if r[2] < 300 else "qss2"] += 1
        seen["limit"] += cnt["n_too_many_reads"]
        seen["void_group"] += cnt["n_groups_mixed_sign"]
        seen["hq_excluded"] += cnt["n_reads_hq_excluded"]
        seen["dup"] += int(c.dup.sum())
    assert all(v >= 1 for v in seen.values()), seen


def test_header_declares_and_lib_binds(snk):
    from supernova_amd import lib
    hdr = (ROOT / "include" / "snk.h").read_text()
    assert re.search(r"\bint snk_dev_mow_lawn\s*\(", hdr) and "typedef struct snk_dev_mow {" in hdr
    assert "snk_dev_mow_lawn" in lib.exported_symbols() and hasattr(snk, "snk_dev_mow_lawn")
    fields = [f for f, _ in lib.SnkDevMow._fields_]
    assert all(k in fields for k in lib.MOW_COUNTERS) and tuple(mowref.COUNTERS) == lib.MOW_COUNTERS
    body = hdr[hdr.index("typedef struct snk_dev_mow {"):hdr.index("} snk_dev_mow;")]
    order = [m for m in re.findall(r"\b(n_[a-z_]+|dels|scored|ms|tables_ms|phase_ms|reserved)\b(?=[\[;,])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))]
    assert order == fields, (order, fields)
