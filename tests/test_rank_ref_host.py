"""tests/rankref.py on the CPU: the reference of the list ranking against a brute-force walk from every state, and the checker against
planted wrong answers -- each must be rejected, and the right answer beside it accepted.  tests/test_gpu_rank_direct.py holds the device
to this reference; a checker that let a wrong answer through would make that suite worthless, so it is tested first."""
import numpy as np
import pytest

import rankref as rr
from rankref import NONE


def brute(link, weights):
    """every state walks on its own: (distance, terminal) or None where it comes back to itself"""
    ns = len(link)
    out = []
    for s0 in range(ns):
        s, d = s0, 0
        for _ in range(ns + 1):
            if link[s] == NONE:
                out.append((d, s))
                break
            s = int(link[s]) ^ 1
            if s == s0:
                out.append(None)
                break
            d += int(weights[s >> 1])
        else:
            raise AssertionError("a walk neither ended nor closed: the links are no involution")
    return out


def _same(link, weights):
    dist, term = rr.ref_rank(link, weights)
    want = brute(link, weights)
    for s, x in enumerate(want):
        if x is None:
            assert term[s] == -1, (link, s)
        else:
            assert (int(dist[s]), int(term[s])) == x, (link, s)
    # the classes: every unranked state in exactly one, a class closed under the mirror, nodes = its states' nodes
    cls = rr.circles(link)
    states = [s for _, st in cls for s in st]
    assert sorted(states) == [s for s, x in enumerate(want) if x is None]
    for nodes, st in cls:
        assert {s ^ 1 for s in st} == st and sorted({s >> 1 for s in st}) == nodes.tolist()
    return len(cls)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_ref_rank_on_every_structure_of_up_to_three_nodes(n):
    count = with_circles = 0
    w = np.array([3, 5, 11][:n], np.uint32)
    for link in rr.all_structures(n):
        assert rr.is_involution(link)
        with_circles += _same(link, w) > 0
        count += 1
    # involutions with optional fixed points on 2n states, each unmatched state free or a turn: sum over matchings of 2^(unmatched)
    assert count == {1: 5, 2: 43, 3: 499}[n] and with_circles > 0


@pytest.mark.parametrize("seed", range(8))
def test_ref_rank_on_random_structures(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 120))
    link = rr.random_mixture(n, rng, max_len=30)
    w = rng.integers(1, 1001, n).astype(np.uint32)
    assert rr.is_involution(link)
    _same(link, w)
    l2, w2 = rr.relabel(link, w, rng)
    assert rr.is_involution(l2) and len(rr.circles(l2)) == len(rr.circles(link))
    _same(l2, w2)
    # the solved structure has no circle left and passes its own check, with the exact cut
    lo, circ, rk, nc = rr.solve(link, w)
    rr.check(link, w, lo, circ, rk, nc, exact_cut=True)
    assert not rr.circles(lo)


def test_the_sample_is_the_one_the_issue_names():
    """split_log2 = 12: the sampled nodes below 4096 are 0, 1626 and 2589 (the GPU tests pin this restatement to the device through m)"""
    assert np.nonzero(rr.sampled(np.arange(4096), 12))[0].tolist() == [0, 1626, 2589]
    assert 20 < int(rr.sampled(np.arange(4096), 5).sum()) < 300 and rr.sampled(np.arange(64), 1).sum() > 10
    def mix(x):          # the same three rounds on Python integers
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ x >> 16
    for x in (0, 1, 2, 1626, 2589, 0x7FFFFFFF, 0xFFFFFFFE):
        assert int(rr.mix32(x)) == mix(x), x


def _job():
    """chains, a chain with a turn, two mirror-pair circles (min nodes 20 and 40), a self-mirror circle (min node 50), a 1-node circle"""
    L = rr.Links(64)
    L.chain(range(0, 9), orient=[1, 0, 1, 1, 0, 0, 1, 0, 1])
    L.chain(range(9, 15), turn_tail=True)
    L.chain([15])
    L.circle([22, 20, 21, 23], orient=[1, 0, 0, 1])
    L.circle(range(40, 47))
    L.chain([52, 50, 51], orient=[0, 1, 1], turn_head=True, turn_tail=True)
    L.circle([60])
    w = (np.arange(64) * 7 % 13 + 1).astype(np.uint32)
    return L.link, w


def _on_list(link, n_th=0):
    """a state of a list that has a successor"""
    lo, _, rk, _ = rr.solve(link)
    return int(np.nonzero((lo != NONE) & (rk[:, 0] > 1))[0][n_th])


def _plant_distance(link, w, lo, circ, rk, nc):
    rk = rk.copy()
    rk[_on_list(link, 5), 0] += 1
    return lo, circ, rk, nc, True


def _plant_mirror_terminal(link, w, lo, circ, rk, nc):
    rk = rk.copy()
    s = _on_list(link, 3)
    assert rk[s ^ 1, 1] != rk[s, 1]
    rk[s, 1] = rk[s ^ 1, 1]
    return lo, circ, rk, nc, True


def _plant_cut_elsewhere(link, w, lo, circ, rk, nc):
    # the circle of node 20 cut at the pair {43, 40} of nodes 21 and 20 instead of {41, 45}: a consistent answer, which only exact_cut refuses
    i = [int(c[0][0]) for c in rr.circles(link)].index(20)
    lo, circ, rk, nc = rr.solve(link, w, cut_at={i: 2 * 21 + 1})
    return lo, circ, rk, nc, True


def _plant_two_cuts(link, w, lo, circ, rk, nc):
    lo, circ = lo.copy(), circ.copy()
    s = 2 * 43 + 1
    for x in (s, int(link[s])):
        lo[x] = NONE
        circ[x] = 1
    d, t = rr.ref_rank(lo, w)
    return lo, circ, np.stack([d, t.astype(np.uint64)], axis=1).astype(np.uint32), nc, False


def _plant_uncut(link, w, lo, circ, rk, nc):
    lo, circ = lo.copy(), circ.copy()
    for x in (2 * 60 + 1, int(link[2 * 60 + 1])):
        lo[x] = link[x]
        circ[x] = 0
    return lo, circ, rk, nc, False


def _plant_missing_mark(link, w, lo, circ, rk, nc):
    circ = circ.copy()
    circ[2 * 40 + 1] = 0
    return lo, circ, rk, nc, True


def _plant_spare_mark(link, w, lo, circ, rk, nc):
    circ = circ.copy()
    circ[3] = 1
    return lo, circ, rk, nc, True


def _plant_count(link, w, lo, circ, rk, nc):
    return lo, circ, rk, nc + 1, True


def _plant_count_low(link, w, lo, circ, rk, nc):
    return lo, circ, rk, nc - 1, True


def _plant_foreign_link(link, w, lo, circ, rk, nc):
    # a list cut in two, ranked consistently with the cut: only the comparison of the links can see it
    lo = lo.copy()
    s = _on_list(link, 2)
    p = int(lo[s])
    lo[s] = lo[p] = NONE
    d, t = rr.ref_rank(lo, w)
    return lo, circ, np.stack([d, t.astype(np.uint64)], axis=1).astype(np.uint32), nc, True


def _plant_rewired_link(link, w, lo, circ, rk, nc):
    lo = lo.copy()
    lo[2 * 15 + 1] = 2 * 15 + 1          # a singleton's free end made a turn
    return lo, circ, rk, nc, True


PLANTS = [_plant_distance, _plant_mirror_terminal, _plant_cut_elsewhere, _plant_two_cuts, _plant_uncut, _plant_missing_mark, _plant_spare_mark,
          _plant_count, _plant_count_low, _plant_foreign_link, _plant_rewired_link]


@pytest.mark.parametrize("plant", PLANTS, ids=lambda f: f.__name__[7:])
def test_checker_rejects_planted_wrong_answers(plant):
    link, w = _job()
    right = rr.solve(link, w)
    rr.check(link, w, *right, exact_cut=True)               # the right answer beside it is accepted
    rr.check(link, w, right[0], None, right[2], right[3], exact_cut=False)
    lo, circ, rk, nc, exact = plant(link, w, *right)
    with pytest.raises(rr.Wrong):
        rr.check(link, w, lo, circ, rk, nc, exact_cut=exact)
    if plant is _plant_cut_elsewhere:
        rr.check(link, w, lo, circ, rk, nc, exact_cut=False)      # ... and is a right answer where the cut is free


def test_checker_takes_a_null_circ_and_refuses_distances_beyond_32_bits():
    link, w = _job()
    lo, circ, rk, nc = rr.solve(link, w)
    rr.check(link, w, lo, None, rk, nc, exact_cut=True)
    L = rr.Links(3).chain([0, 1, 2])
    big = np.array([1, 1 << 31, 1 << 31], np.uint32)
    with pytest.raises(AssertionError):
        rr.solve(L.link, big)
    with pytest.raises(rr.Wrong):
        rr.check(L.link, big, L.link, None, np.zeros((6, 2), np.uint32), 0, exact_cut=False)


def test_builders():
    """a chain is a mirror pair of lists; a turn at one end makes one list of 2n states; a turn at both ends a circle that is its own
    mirror; close makes one class of two cycles"""
    for n in (1, 2, 5):
        a = rr.Links(n).chain(range(n)).link
        d, t = rr.ref_rank(a)
        assert rr.is_involution(a) and not rr.circles(a) and int(d.max()) == n - 1 and len(set(t.tolist())) == 2
        b = rr.Links(n).chain(range(n), turn_tail=True).link
        d, t = rr.ref_rank(b)
        assert rr.is_involution(b) and not rr.circles(b) and int(d.max()) == 2 * n - 1 and len(set(t.tolist())) == 1
        c = rr.Links(n).chain(range(n), turn_head=True, turn_tail=True).link
        cl = rr.circles(c)
        assert rr.is_involution(c) and len(cl) == 1 and len(cl[0][1]) == 2 * n
        lo, _, rk, nc = rr.solve(c)
        assert nc == 1 and len(set(rk[:, 1].tolist())) == (1 if n == 1 else 2)          # cut at a turn: ONE list; at a pair: a mirror pair
        e = rr.Links(n).circle(range(n)).link
        cl = rr.circles(e)
        assert rr.is_involution(e) and len(cl) == 1 and len(cl[0][1]) == 2 * n and (e != NONE).all()
        assert not rr.is_involution(np.array([2, NONE, NONE, NONE], np.uint32)) and not rr.is_involution(np.array([9, NONE], np.uint32))
