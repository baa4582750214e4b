"""Graph edits on the CPU: the Python restatement of DeleteEdgesParallel + Cleanup and of the hanging-end selection (tests/editref.py)
against what the reference's own functions made of every case (tests/golden/edit/*.npz, written by tests/golden/make_edit_golden.py), and
the cases against what they were made to show.  The hanging-end rule is inline in StageTrim: it is pinned by the restatement and by the
edges the cases name by hand."""
import numpy as np
import pytest

import a48xref
import editref


@pytest.mark.parametrize("key", editref.ALL)
def test_restatement_reproduces_the_reference(key):
    g, mine = editref.golden(key), editref.restated(key)
    assert g.pinned, "the fixture was not made by the reference"
    assert len(mine) == len(g.steps) == (2 if editref.case(key).second else 1)
    for i, (m, r) in enumerate(zip(mine, g.steps)):
        assert m.a_hbv == r.a_hbv, f"edit {i}: a.hbv"
        assert m.a_inv == r.a_inv, f"edit {i}: a.inv"
        assert np.array_equal(m.offset, r.offset) and np.array_equal(m.n_edges, r.n_edges) and np.array_equal(m.edges, r.edges), f"edit {i}: paths"
        idx, data, _ = a48xref.zip_paths(m.offset, m.n_edges, m.edges, a48xref.parse_hbv(m.a_hbv))
        assert a48xref.pathsx_bytes(idx, data, len(m.n_edges)) == r.pathsx, f"edit {i}: a.pathsX bytes"


@pytest.mark.parametrize("key", editref.ALL)
def test_hanging_end_rule(key):
    c, g = editref.case(key), editref.golden(key)
    support, dels = editref.hanging_ends(c.a_hbv, c.inv, c.n_edges, c.edges)
    assert np.array_equal(support, g.support) and np.array_equal(dels, g.hang_dels)
    assert np.array_equal(dels, np.unique(dels)) and np.array_equal(np.sort(c.inv[dels]), dels), "ascending, distinct, closed under inv"
    if c.hang_want is not None:
        assert np.array_equal(dels, c.hang_want), "the edges the case names by hand"


def test_hanging_end_case_is_what_it_says():
    """hang: an unsupported tip of exactly 200 k-mers goes and one of 201 stays; a tip that only its inverse's reads support stays; an
    isolated edge and a self-inverse edge go."""
    for K in (48, 60):
        c = editref.case(f"hang_k{K}")
        g = a48xref.parse_hbv(c.a_hbv)
        km = np.asarray([len(s) for s in editref.patchref.edge_strings(g)]) - K + 1
        support, dels = editref.hanging_ends(c.a_hbv, c.inv, c.n_edges, c.edges)
        bare = np.flatnonzero(support == 0)
        assert 200 in km[dels] and 201 in km[bare] and 201 not in km[dels]
        assert any(c.inv[e] == e for e in dels), "a self-inverse edge"
        counts = np.bincount(c.edges, minlength=g.E)
        assert any(counts[e] == 0 and counts[c.inv[e]] > 0 and support[e] > 0 for e in range(g.E)), "support through the inverse only"
        n_from, n_to = np.diff(g.from_off), np.diff(g.to_off)
        assert any(n_to[g.v_left[e]] == 0 and n_from[g.v_left[e]] == 1 and n_from[g.v_right[e]] == 0 and n_to[g.v_right[e]] == 1 for e in dels), "both ends qualify"
        selfinv = [e for e in range(g.E) if c.inv[e] == e]
        assert selfinv and all(support[e] == 2 * counts[e] for e in selfinv), "a self-inverse edge counts twice per entry"


def test_cases_are_what_they_say():
    r = {k: editref.restated(k) for k in editref.ALL if k.split("_k")[0] not in editref.BIG}
    for K in (48, 60):
        assert r[f"fork_k{K}"][0].counters["max_run"] == 2 and r[f"run3_k{K}"][0].counters["max_run"] == 3 and r[f"run65_k{K}"][0].counters["max_run"] == 65
        assert r[f"selfinv_k{K}"][0].counters["n_runs"] == 0 and len(r[f"selfinv_k{K}"][0].inv) == 3, "a run that is its own reverse complement stays"
        assert any(r[f"selfinv_k{K}"][0].inv[e] == e for e in range(3)), "the palindromic edge is still there"
        for n in (3, 100):
            m = r[f"circle{n}_k{K}"][0]
            assert m.counters["n_runs"] == 2 and m.counters["max_run"] == 1 and len(m.inv) == 2 * n, "a circle of unneeded vertices is not merged"
            assert (m.edge_map >= 2 * n - 2).sum() == 2, "one edge of each circle comes back under a new id"
        assert r[f"two_cycle_k{K}"][0].counters["n_runs"] == 0
        assert r[f"parallel_k{K}"][0].counters["max_run"] == 3
        c, m = editref.case(f"none_k{K}"), r[f"none_k{K}"][0]
        assert m.a_hbv == c.a_hbv and m.a_inv == c.a_inv and np.array_equal(m.edges, c.edges) and np.array_equal(m.offset, c.offset)
        assert len(r[f"all_k{K}"][0].inv) == 0 and int(r[f"all_k{K}"][0].n_edges.sum()) == 0
        # the loop: a path leaves the merged edge and comes back to it, and both visits stay
        m = r[f"loop_k{K}"][0]
        paths = editref.split_paths(m.offset, m.n_edges, m.edges)
        merged = set(m.edge_map[m.edge_koff > 0].tolist())
        assert any(len(p) == 3 and p[0] == p[2] != p[1] and p[0] in merged for _, p in paths)
        assert len(r[f"chain_k{K}"]) == 2 and r[f"chain_k{K}"][1].counters["max_run"] == 5
    # somewhere the order of the new ids (by highest unneeded vertex) is not the order of the runs' first edges
    assert any(m.lefts != sorted(m.lefts, reverse=True) for ms in r.values() for m in ms)
    assert editref.restated("run1025_k48")[0].counters["max_run"] == 1025 and editref.restated("run5000_k60")[0].counters["max_run"] == 5000


def test_paths_cover_the_cuts_and_the_offsets():
    """run65: paths cut at entry 0, at entry 1 and at their last entry; a path wholly inside the run collapses to one edge and its offset
    moves by the k-mers in front of its first edge; negative offsets are there."""
    c, m = editref.case("run65_k48"), editref.restated("run65_k48")[0]
    before, after = editref.split_paths(c.offset, c.n_edges, c.edges), editref.split_paths(m.offset, m.n_edges, m.edges)
    dead = set(c.dels.tolist())
    cut_at = {next(j for j, e in enumerate(p) if e in dead) for _, p in before if dead & set(p)}
    assert {0, 1, 2} <= cut_at
    assert any(len(p) == 3 and p.index(next(e for e in p if e in dead)) == 2 for _, p in before if dead & set(p)), "cut at the last entry"
    inside = [(b, a) for b, a in zip(before, after) if len(b[1]) == 3 and len(a[1]) == 1 and not dead & set(b[1])]
    assert inside and all(a[0] == b[0] + m.edge_koff[b[1][0]] for b, a in inside)
    assert any(m.edge_koff[b[1][0]] > 0 for b, _ in inside) and (c.offset < 0).any() and (m.offset < 0).any()
    assert all(a == (b[0], []) for b, a in zip(before, after) if b[1] and b[1][0] in dead), "a path cut to nothing keeps its offset"
