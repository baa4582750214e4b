"""The seeded cases of tests/patchgen.py without a GPU: the generation reaches every part of gap-patch insertion and of the graph edit (so
the device fuzz, tests/test_gpu_patch_fuzz.py, cannot pass on a constant answer), the expected answers move when a rule of the
restatements (tests/patchref.py, tests/editref.py) is changed, and on the pinned seeds the restatements reproduce what the reference's own
functions wrote (tests/golden/patch/fuzz_<seed>.npz, tests/golden/edit/fuzz_<seed>.npz; tests/golden/make_patch_golden.py and
make_edit_golden.py)."""
import inspect

import numpy as np
import pytest

import a48xref
import editref
import patchgen
import patchref

hu = patchref.hu
_chain: dict = {}


def _expected(seed):
    """patchgen.chain of a sampled seed, computed once per process and left unchanged"""
    if seed not in _chain:
        _chain[seed] = patchgen.chain(patchgen.make_case(seed))
    return _chain[seed]


def _made(seeds):
    return [s for s in seeds if patchgen.make_case(s) is not None]


def probe(c) -> dict:
    """what no counter says, read from the restatements' results on a case"""
    K, m = c.K, patchgen.patched(c)
    d, (support, hang) = patchgen.edited(c)
    ec = patchgen.edit_input(c)
    old = patchref.edge_strings(a48xref.parse_hbv(c.a_hbv))
    e3 = patchref.edge_strings(m.g3)
    forward = set(m.unitigs)                     # an edge that is no unitig as stored is read the other way round
    kmers = lambda seqs: {patchref.canon(s[p:p + K]) for s in seqs for p in range(len(s) - K + 1)}
    on_graph = kmers(old)
    longer = on_graph | kmers(x for x in c.closures if len(x) > K)
    new_kmers = kmers(c.closures) - on_graph
    out = dict(to3_max=max(len(x) for x in m.to3),
               left3_reversed=sum(1 for e, x in enumerate(m.to3) if x and m.left3[e] and e3[x[0]] not in forward),
               self_loops=sum(1 for e in range(m.g3.E) if m.g3.v_left[e] == m.g3.v_right[e]),
               new_one_kmer_edges=sum(1 for s in e3 if len(s) == K and patchref.canon(s) in new_kmers),
               k_closure_on_graph=sum(1 for x in c.closures if len(x) == K and patchref.canon(x) in on_graph),
               n_added=len({patchref.canon(x) for x in c.closures if len(x) == K} - longer),
               pieces_max=max([patchref.n_pieces(len(x), K) for x in c.closures] or [0]), real_overlaps=0)
    # OverlapAppend with a real overlap: a suffix of q is a prefix of v
    plain = patchref.overlap_append

    def counting(q, v):
        out["real_overlaps"] += any(q[len(q) - o:] == v[:o] for o in range(1, min(len(q), len(v)) + 1))
        plain(q, v)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(patchref, "overlap_append", counting)
        patchref.translate_paths(K, c.offset, c.n_edges, c.edges, m.to3, m.left3, np.asarray([len(s) for s in e3], np.int64))
    # a merged run with a member that is read in reverse (on the device: a segment with SEG_RC of the unitig that is stored)
    members: dict = {}
    for e, f in enumerate(d.edge_map):
        if f >= 0 and d.inv[f] >= f:
            members.setdefault(int(f), []).append(e)
    out["runs_with_reversed"] = sum(1 for es in members.values() if len(es) > 1 and any(e3[e] not in forward for e in es))
    out["hang"] = len(hang)
    out["edit"] = d.counters
    return out


def test_generation_reaches_every_part(snk):
    """Conditions on what is generated, over every fourth seed (patchgen.sample: K = 48 and 60 in turn)."""
    seeds = patchgen.sample()
    made = _made(seeds)
    assert len(seeds) - len(made) <= len(seeds) // 20, f"{len(seeds) - len(made)} of {len(seeds)} seeds skipped"
    kinds = {K: set() for K in patchref.KS}
    counters = {K: dict.fromkeys(patchref.COUNTERS, 0) for K in patchref.KS}
    edit = dict.fromkeys(editref.COUNTERS, 0)
    P = dict(to3_max=0, left3_reversed=0, self_loops=0, new_one_kmer_edges=0, k_closure_on_graph=0, n_added=0, pieces_max=0, real_overlaps=0, runs_with_reversed=0)
    hanging = 0
    for s in made:
        c = patchgen.make_case(s)
        kinds[c.K] |= set(c.kinds)
        for k, v in patchgen.patched(c).counters.items():
            counters[c.K][k] += v
        p = probe(c)
        for k in P:
            P[k] = max(P[k], p[k]) if k.endswith("_max") else P[k] + p[k]
        for k in edit:
            edit[k] = max(edit[k], p["edit"][k]) if k == "max_run" else edit[k] + p["edit"][k]
        hanging += p["hang"] > 0
    print(f"patch fuzz generation over {len(made)} of {len(seeds)} seeds: kinds {({K: sorted(v) for K, v in kinds.items()})}; counters {counters}; {P}; edit {edit}; "
          f"the hanging-end rule selects edges in {hanging} cases")
    assert all(kinds[K] == set(patchgen.KINDS) for K in kinds), kinds
    assert all(v >= 1 for K in counters for v in counters[K].values()), counters
    assert P["to3_max"] >= 4 and P["pieces_max"] >= 3, P
    assert all(P[k] >= 1 for k in P), P
    assert all(edit[k] >= 1 for k in ("n_runs", "n_truncated", "n_emptied", "n_collapsed")) and edit["max_run"] >= 3, edit
    assert 3 * hanging >= len(made), hanging


def _planted(mp, module, name, *swaps):
    """the function `name` of `module` with one piece of its text replaced, in the module's own namespace; every piece must occur once"""
    src = inspect.getsource(getattr(module, name))
    for old, new in swaps:
        assert src.count(old) == 1, f"{module.__name__}.{name} no longer reads `{old}`"
        src = src.replace(old, new)
    ns = {}
    exec(compile(src, f"<{module.__name__}.{name}, changed>", "exec"), module.__dict__, ns)
    mp.setattr(module, name, ns[name])


def _shortest_overlap(mp):
    def overlap_append(q, v):
        best = next((o for o in range(1, min(len(q), len(v)) + 1) if q[len(q) - o:] == v[:o]), 0)
        q.extend(v[best:])
    mp.setattr(patchref, "overlap_append", overlap_append)


def _left3_not_mirrored(mp):
    """left3 of an old edge whose first new edge is read the other way round, as an offset on the stored unitig (o, not ulen - K - o)"""
    new_unitigs, path_old_edges = patchref.new_unitigs, patchref.path_old_edges
    last = {}

    def recording(allx, K):
        last["forward"] = set(new_unitigs(allx, K))
        return new_unitigs(allx, K)

    def mirrored(old_edges, g3, e3):
        to3, left3 = path_old_edges(old_edges, g3, e3)
        for e, x in enumerate(to3):
            if x and e3[x[0]] not in last["forward"]:
                left3[e] = len(e3[x[0]]) - g3.K - left3[e]
        return to3, left3
    mp.setattr(patchref, "new_unitigs", recording)
    mp.setattr(patchref, "path_old_edges", mirrored)


CHANGES = {
    "OverlapAppend takes the shortest overlap": _shortest_overlap,
    "start <= len3": lambda mp: _planted(mp, patchref, "translate_paths", ("if start < len3[to3[e][0]]:", "if start <= len3[to3[e][0]]:")),
    "the trim subtracts len3 - K": lambda mp: _planted(mp, patchref, "translate_paths", ("start -= len3[q[trim]] - K + 1", "start -= len3[q[trim]] - K")),
    "left3 of a reversed edge is o, not ulen - K - o": _left3_not_mirrored,
    "pieces overlap by K - 1": lambda mp: _planted(mp, patchref, "piece_spans", ("p += PIECE - K", "p += PIECE - K + 1")),
    "K-base closures are dropped": lambda mp: _planted(mp, patchref, "build_all", ("return allx + list(closures)", "return allx + [x for x in closures if len(x) != K]")),
    "no junction (K+1)-mers in build_all": lambda mp: _planted(mp, patchref, "build_all", ("allx.append(edges[e1][-K:] + edges[e2][K - 1])", "pass")),
    "edit: no collapse of a repeated new id": lambda mp: _planted(mp, editref, "delete_edges", ("if renum[e] != q[-1]:", "if True:")),
    "edit: edge_koff counts bases": lambda mp: _planted(mp, editref, "delete_edges", ("off = hb.kmers(first)", "off = len(hb.edges[first])"),
                                                        ("off += hb.kmers(e)", "off += len(hb.edges[e])")),
    "the hanging-end bound is >=": lambda mp: _planted(mp, editref, "hanging_ends", ("lens[e] - g.K + 1 > max_kmers", "lens[e] - g.K + 1 >= max_kmers")),
}


@pytest.mark.parametrize("change", list(CHANGES))
def test_expected_answers_are_sensitive(snk, change):
    """A restatement with one rule changed gives another expected result -- graph, to3 / left3, translated paths, edited graph and paths,
    maps, counters or hanging-end selection -- on at least 3 of the sampled seeds: a kernel with that mistake cannot pass the fuzz."""
    seeds = _made(patchgen.sample())
    base = {s: _expected(s) for s in seeds}
    moved = []
    with pytest.MonkeyPatch.context() as mp:
        CHANGES[change](mp)
        for s in seeds:
            try:
                moved += [] if patchgen.same(patchgen.chain(patchgen.make_case(s)), base[s]) else [s]
            except (AssertionError, IndexError, KeyError):       # the changed rule leaves a restatement without an answer: no answer is another answer
                moved.append(s)
    print(f"{change}: the expected answers of {len(moved)} of {len(seeds)} seeds change: {moved}")
    assert len(moved) >= 3, (change, moved)


def test_restatements_reproduce_the_reference_on_pinned_seeds(snk):
    """The pinned seeds (patchgen.PINNED, 6 per K): the input made again from the seed is the one the reference ran on (the fixtures'
    digests), and the restatements give the bytes the reference's StageInsertPatch steps and its DeleteEdgesParallel + Cleanup wrote.
    Together the seeds hold every closure kind and every condition of test_generation_reaches_every_part."""
    assert len(patchgen.PINNED) == 12 and sorted(patchgen.make_case(s).K for s in patchgen.PINNED) == [48] * 6 + [60] * 6
    kinds = set()
    have = dict(to3_ge4=0, left3_reversed=0, self_loops=0, new_one_kmer_edges=0, k_closure_on_graph=0, n_added=0, pieces_ge3=0, real_overlaps=0, runs_with_reversed=0, hang=0,
                max_run_ge3=0, **dict.fromkeys(patchref.COUNTERS + ("n_runs", "n_truncated", "n_emptied", "n_collapsed"), 0))
    for seed in patchgen.PINNED:
        c = patchgen.make_case(seed)
        g, m = patchref.golden(c.key), patchgen.patched(c)
        assert m.a_hbv == g.a_hbv and m.a_inv == g.a_inv, (seed, "patched a.hbv / a.inv")
        off, ids = patchref.flat(m.to3)
        assert np.array_equal(off, g.to3_off) and np.array_equal(ids, g.to3) and np.array_equal(m.left3, g.left3), (seed, "to3 / left3")
        assert np.array_equal(m.edge, g.edge) and np.array_equal(a48xref.wrap16(m.offset), g.offset) and m.pathsx == g.pathsx, (seed, "translated paths")
        eg, (d, (support, hang)) = editref.golden(c.key), patchgen.edited(c)
        assert eg.pinned and len(eg.steps) == 1
        step = eg.steps[0]
        assert d.a_hbv == step.a_hbv and d.a_inv == step.a_inv, (seed, "edited a.hbv / a.inv")
        assert np.array_equal(d.offset, step.offset) and np.array_equal(d.n_edges, step.n_edges) and np.array_equal(d.edges, step.edges), (seed, "edited paths")
        idx, data, _ = a48xref.zip_paths(d.offset, d.n_edges, d.edges, a48xref.parse_hbv(d.a_hbv))
        assert a48xref.pathsx_bytes(idx, data, len(d.n_edges)) == step.pathsx, (seed, "edited a.pathsX")
        assert np.array_equal(support, eg.support) and np.array_equal(hang, eg.hang_dels)
        kinds |= set(c.kinds)
        p = probe(c)
        for k in ("left3_reversed", "self_loops", "new_one_kmer_edges", "k_closure_on_graph", "n_added", "real_overlaps", "runs_with_reversed", "hang"):
            have[k] += p[k]
        have["to3_ge4"] += p["to3_max"] >= 4
        have["pieces_ge3"] += p["pieces_max"] >= 3
        have["max_run_ge3"] += d.counters["max_run"] >= 3
        for k in patchref.COUNTERS:
            have[k] += m.counters[k]
        for k in ("n_runs", "n_truncated", "n_emptied", "n_collapsed"):
            have[k] += d.counters[k]
    assert kinds == set(patchgen.KINDS), set(patchgen.KINDS) - kinds
    assert all(v >= 1 for v in have.values()), have
