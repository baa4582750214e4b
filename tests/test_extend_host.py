"""The path-extension fixtures (tests/golden/ext/: bytes the reference's ExtendPathsNew wrote, tests/golden/make_ext_golden.py) against the
Python restatement (tests/extref.py) that the GPU tests use beside them, the metamorphic property of the `_first` cases, and the premises
of the hand-made cases (tests/handext.py).  No GPU."""
import numpy as np
import pytest

import a48ref
import a48xref
import extref
import goldens
import handext


def test_every_case_has_its_fixture():
    assert set(extref.names()) == set(extref.ALL) and extref.GOLDEN == tuple(goldens.CASES)
    for name in goldens.CASES:          # a case without _cut / _first is one where they would be the case itself
        assert (name in extref.BRANCHED) == bool((extref.load(name).paths[1] >= 2).any())


@pytest.mark.parametrize("name", extref.ALL)
def test_restatement_reproduces_the_reference(name):
    """Both flags: the restatement's paths, zipped, are the bytes the reference wrote; and they unzip to the restatement's paths."""
    c = extref.load(name)
    for back in (0, 1):
        o, n, e, _ = extref.restated(name, back)
        idx, data, _ = a48xref.zip_paths(o, n, e, c.g)
        assert a48xref.pathsx_bytes(idx, data, len(n)) == c.pathsx[back], (name, back)
        x_idx, x_data, n_reads = a48xref.parse_pathsx(c.pathsx[back])
        uo, un, ue = a48xref.unzip_paths(x_idx, x_data, n_reads, c.g)
        assert np.array_equal(uo, o) and np.array_equal(un, n) and np.array_equal(ue, e)


@pytest.mark.parametrize("name", goldens.CASES)
def test_inputs_are_what_they_are_said_to_be(name):
    """The un-cut case runs on the reference's own paths; `_cut` and `_first` are derived from them as the maker derived them."""
    base = extref.load(name)
    p0 = extref.golden_input(a48xref.parse_paths(a48ref.load(name)["tmp.paths"]))
    assert all(np.array_equal(a, b) for a, b in zip(base.paths, p0))
    if name not in extref.BRANCHED:
        return
    for tag, want in (("_cut", extref.cut_first_edge(base.g, base.eb, *p0)), ("_first", extref.first_edge_only(*p0))):
        got = extref.load(name + tag).paths
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), name + tag


@pytest.mark.parametrize("name", extref.BRANCHED)
def test_leg_2_looks_at_the_first_edge_only(name):
    """Without the backward leg, cutting every path to its first edge beforehand changes nothing: the reference's own bytes are equal."""
    assert extref.load(name + "_first").pathsx[0] == extref.load(name).pathsx[0]


@pytest.mark.parametrize("name", extref.BRANCHED)
def test_cut_cases_make_the_backward_leg_run(name):
    c = extref.load(name + "_cut")
    many = a48xref.parse_paths(extref.load(name).in_paths)[1] >= 2
    assert many.any()
    assert (c.paths[0][many] < 0).all(), "dropping the first edge leaves the read in front of the path"
    assert extref.restated(name + "_cut", 1)[3]["n_back_extended"] >= 1 and c.pathsx[0] != c.pathsx[1]


def test_golden_cases_raise_every_counter():
    tot = dict.fromkeys(extref.COUNTERS, 0)
    for name in goldens.CASES:
        for k, v in extref.restated(name, 0)[3].items():
            tot[k] += v
    assert all(tot[k] >= 1 for k in ("n_quality_extended", "n_ambiguous", "n_cut_to_first", "n_exact_extended", "n_too_many")), tot
    adv = a48xref.parse_paths(extref.load("adversarial").in_paths)[1].astype(np.int64)
    n = extref.restated("adversarial", 0)[1].astype(np.int64)
    assert (n > adv).sum() >= 1 and (n < adv).sum() >= 1


@pytest.mark.parametrize("name", list(extref.HAND))
def test_hand_made_premises(name, snk, tmp_path):
    """Every hand-made read does what it is there for: the counters it raises and the edges it ends with, per flag; the graph of the
    fixture is the graph the generator makes; the depth-4 tree overflows the list and the depth-3 tree fills it with 85 entries."""
    from supernova_amd import graphio
    K = extref.HAND[name]
    c, h = extref.load(name), handext.case(K)
    assert c.g.K == K and int(np.diff(c.g.from_off).max()) == 4
    graphio.write_hbv(tmp_path / "g.hbv", None, K, h.off, h.bases)
    assert (tmp_path / "g.hbv").read_bytes() == c.a_hbv, "the generator no longer makes the graph the fixture was made on"
    codes, quals, lens, paths = handext.arrays(h, handext.edge_index(c.eb))
    assert np.array_equal(codes, c.codes) and np.array_equal(quals, c.quals) and np.array_equal(lens, c.lens)
    assert all(np.array_equal(a, b) for a, b in zip(paths, c.paths))
    for back in (0, 1):
        hits = []
        o, n, e, cnt = extref.extend(c.g, c.codes, c.lens, c.quals, *c.paths, bool(back), c.eb, hits)
        for i, r in enumerate(h.reads):
            assert hits[i] == r.hits[back] and n[i] == r.n_out[back], (r.name, back, sorted(hits[i]), int(n[i]))
        assert cnt["n_too_many"] >= 1 and cnt["n_ambiguous"] >= 1 and cnt["n_quality_extended"] >= 1 and cnt["n_exact_extended"] >= 1
    assert extref.restated(name, 1)[3]["n_back_extended"] >= 1
    # the lists of the two trees, counted here: 1 + 4 + 16 + 64 entries are expanded below either root; with 256 more the walk reaches entry 101
    names = {r.name: i for i, r in enumerate(h.reads)}
    edge_of = handext.edge_index(c.eb)
    for rd, total in (("tree3_extended", 85), ("tree4_too_many_exact", 341)):
        e0 = edge_of[h.reads[names[rd]].first]
        level, count = [int(c.g.v_right[e0])], 1
        while level:
            nxt = [int(c.g.v_right[f]) for v in level for f in c.g.from_e[c.g.from_off[v]:c.g.from_off[v + 1]]]
            count += len(nxt)
            level = nxt
        assert count == total, (rd, count)


def test_refusals_of_the_restatement():
    """What the reference would read outside a read or an edge with is refused, not computed."""
    c = extref.load("hand_k48")
    e0 = int(c.paths[2][0])
    read, qual = c.codes[0][:100], c.quals[0][:100]
    nb = len(c.eb[e0])
    for off, back, code in ((-100, False, "arg"), (nb, False, "arg"), (40000, False, "unsupported"), (-40000, False, "unsupported")):
        with pytest.raises(extref.Refused) as x:
            extref.extend_read(c.g, c.eb, 48, read, qual, off, [e0], back)
        assert x.value.code == code, off
    with pytest.raises(extref.Refused):
        extref.extend_read(c.g, c.eb, 48, read[:0], qual[:0], 0, [e0], False)
    assert extref.extend_read(c.g, c.eb, 48, read, qual, 0, [], True) == (0, [], set())


def _special(kind, tmp_path):
    from supernova_amd import graphio
    s = handext.special(kind)
    graphio.write_hbv(tmp_path / "s.hbv", None, s.K, *graphio.unitigs_to_arrays(s.unitigs))
    g = a48xref.parse_hbv((tmp_path / "s.hbv").read_bytes())
    eb = extref.edge_bases(g)
    return s, g, eb, handext.special_arrays(s, handext.edge_index(eb))


def test_backward_leg_must_not_move_the_offset_beyond_int16(snk, tmp_path):
    """An in-edge of more than 32767 k-mers put in front: the reference zips the path right there (Extend.cc:57) and the offset wraps.
    Refused with the flag; without it the read is an ordinary one."""
    s, g, eb, (codes, quals, lens, paths) = _special("long_in_edge", tmp_path)
    assert max(len(e) for e in eb) - (s.K - 1) > 32767 + 30
    with pytest.raises(extref.Refused) as x:
        extref.extend(g, codes, lens, quals, *paths, True, eb)
    assert x.value.code == "unsupported"
    o, n, e, cnt = extref.extend(g, codes, lens, quals, *paths, False, eb)
    assert (int(o[0]), int(n[0])) == (-30, 1)


def test_multi_match_premise(snk, tmp_path):
    """Two out-edges with the same base at K-1: the restatement pushes both, as the reference does."""
    s, g, eb, (codes, quals, lens, paths) = _special("multi_match", tmp_path)
    o, n, e, cnt = extref.extend(g, codes, lens, quals, *paths, False, eb)
    assert int(n[0]) == 3 and cnt["n_exact_extended"] == 1 and g.v_left[e[1]] == g.v_left[e[2]] and eb[e[1]][s.K - 1] == eb[e[2]][s.K - 1]
