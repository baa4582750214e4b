"""The seeded gaps of tests/closegen.py without a GPU: the generation reaches every part of CloseGap / CloseGap2 (so the device fuzz,
tests/test_gpu_closures_fuzz.py, cannot pass on a constant answer), the expected answers move when a constant of the restatement
(tests/closeref.py) is off by one, and on the pinned seeds the restatement reproduces what the reference's own functions wrote
(tests/golden/closures/fuzz_<seed>.npz, tests/golden/make_closures_golden.py)."""
import numpy as np
import pytest

import closegen
import closeref

_results: dict = {}


def _expected(seed, cg2=True, width=closeref.MAX_WIDTH):
    """closeref.close_gaps of a sampled seed, computed once per process and left unchanged; None: the seed is skipped"""
    key = (seed, cg2, width)
    if key not in _results:
        c = closegen.make_case(seed)
        _results[key] = None if c is None else closeref.close_gaps(c.I, c.pairs, cg2, width)
    return _results[key]


def _same(a, b) -> bool:
    """closures, pair_first and COUNTERS (not the filters: the device does not report them)"""
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def probe(c, width=closeref.MAX_WIDTH) -> dict:
    """what no counter says, from the restatement's own parts, over the pairs of a case: the widest stack of either side before Trim (M),
    the most gathered rows on a side, the most index entries of an edge a pair reads, whether Trim dropped a gathered row (CloseGap:
    n_rows below the gathered rows), and for CloseGap2 the partners tried that have fewer than 32 bases and those found at two positions
    or more"""
    I = c.I
    out = dict(M=[0, 0], side_rows=0, index_entries=0, dropped=0, short_partner=0, found_twice=0)
    for e1, e2 in c.pairs:
        es = (int(e1), I.inv[int(e2)])
        gathered = 0
        for s, e in enumerate(es):
            locs, _ = closeref._locs(I, e, False)
            gathered += len(locs)
            out["side_rows"] = max(out["side_rows"], len(locs))
            out["index_entries"] = max(out["index_entries"], len(I.pidx[e]), len(I.pidx[I.inv[e]]))
            for rid, pos, fw in locs:
                out["M"][s] = max(out["M"][s], pos + int(I.lens[rid]) if fw else I.ne[e] - pos)
        cnt = dict.fromkeys(closeref.COUNTERS, 0)
        closeref.close_gap(I, int(e1), int(e2), False, width, cnt)
        out["dropped"] += cnt["n_rows"] < gathered
        # the partners, as close_gap looks for them (Closomatic.cc:550-581)
        bod, ids = [{}, {}], [None, None]
        for s, e in enumerate(es):
            locs, prec = closeref._locs(I, e, True)
            ids[s] = sorted({rid for rid, _, fw in locs if fw})
            for g, add in {p for p in prec if prec.count(p) >= closeref.MIN_EDGE_COUNT}:
                E = I.eb[g]
                for l in range(len(E) - closeref.L32 + 1):
                    bod[s].setdefault(bytes(E[l:l + closeref.L32]), set()).add(add + l)
        for s in range(2):
            for id1 in ids[s]:
                if id1 ^ 1 in ids[1 - s]:
                    continue
                b, _ = I.read(id1 ^ 1)
                out["short_partner"] += len(b) < closeref.L32
                finds = {pos - l for l in range(len(b) - closeref.L32 + 1) for pos in bod[1 - s].get(bytes(b[l:l + closeref.L32]), ())}
                out["found_twice"] += len(finds) >= 2
    return out


def test_generation_reaches_every_part(snk):
    """Conditions on what is generated, over every fourth seed (closegen.sample: K = 48 and 60 in turn)."""
    W4, WIDE = closeref.MAX_WIDTH, closeref.WIDE
    seeds = closegen.sample()
    made = [s for s in seeds if closegen.make_case(s) is not None]
    assert len(seeds) - len(made) <= len(seeds) // 20, f"{len(seeds) - len(made)} of {len(seeds)} seeds skipped"
    tot, filt = dict.fromkeys(closeref.COUNTERS, 0), dict.fromkeys(closeref.FILTERS, 0)
    classes = {K: dict.fromkeys(("n_pairs_1", "n_pairs_2", "n_pairs_many"), 0) for K in (48, 60)}
    differ, too_long_wide = {48: 0, 60: 0}, 0
    P = dict(M=[0, 0], side_rows=0, index_entries=0, dropped=0, short_partner=0, found_twice=0)
    for s in made:
        c = closegen.make_case(s)
        r2, r1 = _expected(s), _expected(s, False)
        for k in closeref.COUNTERS:
            tot[k] += r2[3][k]
        for k in closeref.FILTERS:
            filt[k] += r2[4][k]
        for k in classes[c.K]:
            classes[c.K][k] += r2[3][k]
        differ[c.K] += not (np.array_equal(r2[0], r1[0]) and np.array_equal(r2[1], r1[1]))
        too_long_wide += _expected(s, True, WIDE)[3]["n_cons_too_long"]
        p = probe(c)
        P["M"] = [max(a, b) for a, b in zip(P["M"], p["M"])]
        for k in ("side_rows", "index_entries"):
            P[k] = max(P[k], p[k])
        for k in ("dropped", "short_partner", "found_twice"):
            P[k] += p[k]
    print(f"closures fuzz generation over {len(made)} of {len(seeds)} seeds at width {W4}: counters {tot}; filters {filt}; classes {classes}; "
          f"CloseGap2 differs from CloseGap in {differ} cases; n_cons_too_long at {WIDE}: {too_long_wide}; {P}")
    assert all(tot[k] >= 1 for k in closeref.COUNTERS if k != "n_cons_too_long"), tot
    assert too_long_wide >= 1
    assert all(v >= 1 for v in filt.values()), filt
    assert all(v >= 5 for K in classes for v in classes[K].values()), classes
    assert all(v >= 5 for v in differ.values()), differ
    assert P["M"][0] > W4 and P["M"][1] > W4 and P["dropped"] >= 1, P
    assert P["side_rows"] > 256 and P["index_entries"] > 64 and P["short_partner"] >= 1 and P["found_twice"] >= 1, P


def _swapped(m):
    seed, final = closeref.seed_consensus, closeref.final_consensus
    m.setattr(closeref, "seed_consensus", final)
    m.setattr(closeref, "final_consensus", seed)


CHANGES = {
    "MIN_BITS 26": lambda m: m.setattr(closeref, "MIN_BITS", 26.0),
    "MIN_EDGE_COUNT 6": lambda m: m.setattr(closeref, "MIN_EDGE_COUNT", 6),
    "FLANK 9": lambda m: m.setattr(closeref, "FLANK", 9),
    "MAX_EWX 21": lambda m: m.setattr(closeref, "MAX_EWX", 21),
    "MIN_STRETCH 9": lambda m: m.setattr(closeref, "MIN_STRETCH", 9),
    "MIN_ADD 11": lambda m: m.setattr(closeref, "MIN_ADD", 11.0),
    "seed and final consensus swapped": _swapped,
    "Q0 weighs what Q1 and Q2 weigh": lambda m: m.setattr(closeref, "Q0_WEIGHT", closeref.Q12_WEIGHT),
}


@pytest.mark.parametrize("change", list(CHANGES))
def test_expected_answers_are_sensitive(snk, change):
    """A restatement with one constant off by one (or the two consensus rules swapped, or quality 0 weighing 0.2) gives other closures or
    counters for CloseGap2 on at least 3 of the sampled seeds: a kernel with that mistake cannot pass the fuzz."""
    seeds = [s for s in closegen.sample() if closegen.make_case(s) is not None]
    base = {s: _expected(s) for s in seeds}
    with pytest.MonkeyPatch.context() as m:
        CHANGES[change](m)
        moved = [s for s in seeds if not _same(closeref.close_gaps(closegen.make_case(s).I, closegen.make_case(s).pairs, True), base[s])]
    print(f"{change}: the expected answers of {len(moved)} of {len(seeds)} seeds change: {moved}")
    assert len(moved) >= 3, (change, moved)


def test_restatement_reproduces_the_reference_on_pinned_seeds(snk):
    """The pinned seeds (closeref.FUZZ): the input made again from the seed is the one the reference ran on (input_digest), and the
    restatement gives the bytes the reference's CloseGap2 / CloseGap wrote at max_width 400 and 1 200.  Together the seeds hold every class
    of pair, a placed partner that changes bytes, a partner found twice, a dropped row, a self-inverse pair, a bad window and a path [X, X]."""
    assert len(closeref.FUZZ) == 12 and sorted(closegen.generate(s).K for s in closeref.FUZZ) == [48] * 6 + [60] * 6
    have = dict.fromkeys(("n_pairs_0", "n_pairs_1", "n_pairs_2", "n_pairs_many", "placed_changes_bytes", "found_twice", "dropped", "self_inverse", "bad_window", "visited_twice"), 0)
    for seed in closeref.FUZZ:
        c, z = closegen.make_case(seed), closeref.load_fuzz(seed)
        assert z["input_digest"] == closeref.digest(c, c.reads), f"seed {seed}: the generator no longer makes the input the reference ran on"
        for flag in closeref.FLAGS:
            for sfx, width in (("", closeref.MAX_WIDTH), ("_wide", closeref.WIDE)):
                off, bases, first, cnt, _ = closeref.close_gaps(c.I, c.pairs, flag == "cg2", width)
                assert closeref.fastb_bytes(off, bases) == z[f"fastb_{flag}{sfx}"] and np.array_equal(first, z[f"pair_first_{flag}{sfx}"]), (seed, flag, width)
                if flag == "cg2" and not sfx:
                    for k in ("n_pairs_0", "n_pairs_1", "n_pairs_2", "n_pairs_many"):
                        have[k] += cnt[k]
                    have["placed_changes_bytes"] += cnt["n_partners_placed"] >= 1 and z["fastb_cg2"] != z["fastb_cg1"]
        p = probe(c)
        have["found_twice"] += p["found_twice"]
        have["dropped"] += p["dropped"]
        have["self_inverse"] += c.marks["self_inverse"]
        have["bad_window"] += c.marks["bursts"]
        have["visited_twice"] += c.marks["visited_twice"]
    assert all(v >= 1 for v in have.values()), have
