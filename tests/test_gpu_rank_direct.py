"""The list ranking on link structures made by hand (csrc/snk_rank.hip through snk_dev_rank_lists), against the sequential reference of
tests/rankref.py.  The read-driven suites (test_gpu_join_mirror.py, test_gpu_handreads.py, test_gpu_sharded.py) reach this code only
through reads -> k-mers -> fragments -> links and cannot choose the structure; here every case chooses it: which states are splitters,
which circles hold none, how long the splitter list is, what the weights are, which owner is empty.  Nothing rotates a circle
afterwards, so a cut in the wrong place or a second cut in one circle shows.

Every comparison is exact integer equality (rankref.check: the links after the cuts, the marks, n_circles, both words of rk for every
state), and every call asserts from the evidence the entry returns that it took the path it is there for.  When the module is done the
evidence of every case is printed, one line for the calls of a case that took the same path under the same options
([rank_direct] ...: profiles/rank_direct.log)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import rankref as rr
from rankref import NONE

pytestmark = pytest.mark.gpu

WYLLIE, RULING, RULING_THEN_WYLLIE = 1, 2, 3
E_ARG = -1


SEEN = {}          # (case, world, options, path taken) -> the calls' sizes and counters


def note(tag, n, world, weights, circ, opts, ev):
    case = re.sub(r"#\d+", "", tag.split(" frag_off=")[0])
    path = tuple(ev[k] for k in ("source", "ruling_attempts", "bad", "part_attempts", "partitioned"))
    g = SEEN.setdefault((case, world, tuple(sorted(opts.items())), path), dict(calls=0, ragged=0, kinds=set(), n=[], n_circles=[], rounds=[], splitters=[], sparse_cut=[]))
    g["calls"] += 1
    g["ragged"] += " frag_off=[" in tag
    g["kinds"].add(("w" if weights is not None else "-") + ("c" if circ else "-"))
    g["n"].append(n)
    for k in ("n_circles", "rounds", "splitters", "sparse_cut"):
        g[k].append(ev[k])


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()
    span = lambda v: str(min(v)) if min(v) == max(v) else f"{min(v)}..{max(v)}"
    for (case, world, opts, path), g in SEEN.items():
        print(f"[rank_direct] {case} world={world} opts={dict(opts)} weights/marks={','.join(sorted(g['kinds']))}: source={path[0]} ruling_attempts={path[1]} "
              f"bad={path[2]} part_attempts={path[3]} partitioned={path[4]} | calls={g['calls']} (uneven frag_off: {g['ragged']}) n={span(g['n'])} "
              + " ".join(f"{k}={span(g[k])}" for k in ("n_circles", "rounds", "splitters", "sparse_cut")))


class Out:
    def __init__(self, rc, msg, link, circ, rk, ev):
        self.rc, self.msg, self.link, self.circ, self.rk, self.ev = rc, msg, link, circ, rk, ev


def call(engine, link, weights=None, circ=True, world=0, frag_off=None, opts=None, n=None):
    """one call of snk_dev_rank_lists under the options of `opts` -> Out (circ: True = a zeroed mark array is given, False = NULL)"""
    import torch
    from supernova_amd import lib as L
    dev = torch.device("cuda", 0)
    link = np.ascontiguousarray(link, dtype=np.uint32)
    n = len(link) // 2 if n is None else n
    d_link = torch.from_numpy(link.view(np.int32).copy()).to(dev)
    d_w = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.uint32).view(np.int32).copy()).to(dev) if weights is not None else None
    d_circ = torch.zeros(len(link) + 16, dtype=torch.uint8, device=dev) if circ else None
    d_rk = torch.full((2 * len(link) + 16,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    fo = (C.c_uint64 * len(frag_off))(*[int(x) for x in frag_off]) if frag_off is not None else None
    ev = L.SnkRankEvidence()
    C.memset(C.byref(ev), 0xEE, C.sizeof(ev))
    err = C.create_string_buffer(512)
    torch.cuda.synchronize()
    opts = dict(opts or {})
    try:
        for k, v in opts.items():
            engine.set_option(k, v)
        rc = engine.lib.snk_dev_rank_lists(engine._ctx, n, d_link.data_ptr(), d_w.data_ptr() if d_w is not None else None,
                                           d_circ.data_ptr() if d_circ is not None else None, world, fo, d_rk.data_ptr(), C.byref(ev), None, err, 512)
    finally:
        for k in opts:
            engine.clear_option(k)
    torch.cuda.synchronize()
    return Out(rc, err.value.decode(errors="replace"), d_link.cpu().numpy().view(np.uint32),
               d_circ.cpu().numpy()[:len(link)] if circ else None, d_rk.cpu().numpy().view(np.uint32)[:2 * len(link)].reshape(-1, 2), ev.to_dict())


def even(n, world):
    return [n * q // world for q in range(world + 1)]


def ragged(n, world):
    """owners without a node first, last and in the middle, and one owner that holds everything"""
    if world == 2:
        return [[0, 0, n], [0, n, n]]
    if world == 3:
        return [[0, 0, n, n], [0, n // 2, n // 2, n], [0, n, n, n]]
    assert world == 8
    return [[0, 0, n // 5, 2 * n // 5, 3 * n // 5, 3 * n // 5, 4 * n // 5, n, n], [0, 0, 0, 0, 0, 0, 0, n, n]]


def verify(tag, link, weights, out, opts=None, world=0, circ=True, expect_bad=False, n_classes=None):
    """rankref.check + the path the evidence must show.  -> the evidence"""
    opts = opts or {}
    n = len(link) // 2
    ev = out.ev
    assert out.rc == 0, (tag, out.rc, out.msg)
    note(tag, n, world, weights, circ, opts, ev)
    sl = opts.get("split_log2", 5)
    wyllie = world == 0 and (n < 2048 or opts.get("rank_wyllie", 0) == 1)
    exact = world == 0 and (wyllie or not circ)
    try:
        rr.check(link, weights, out.link, out.circ, out.rk, ev["n_circles"], exact_cut=exact)
    except rr.Wrong as e:
        raise rr.Wrong(f"{tag} n={n} world={world} weights={weights is not None} circ={circ} opts={opts} {ev}: {e}") from None
    nc = ev["n_circles"] if n_classes is None else n_classes
    assert nc == ev["n_circles"]
    if expect_bad:
        return ev
    assert ev["bad"] == 0, (tag, ev)
    if world == 0:
        assert ev["part_attempts"] == 0 and ev["partitioned"] == 0
        if wyllie:
            assert (ev["source"], ev["ruling_attempts"], ev["sparse_cut"], ev["splitters"]) == (WYLLIE, 0, 0, 0), (tag, ev)
        else:
            assert ev["splitters"] == rr.expected_splitters(link, sl), (tag, ev)
            if nc == 0:
                assert (ev["source"], ev["ruling_attempts"], ev["sparse_cut"]) == (RULING, 1, 0), (tag, ev)
            elif not circ:
                assert (ev["source"], ev["ruling_attempts"], ev["sparse_cut"]) == (RULING_THEN_WYLLIE, 1, 0), (tag, ev)
            else:
                assert (ev["source"], ev["ruling_attempts"], ev["sparse_cut"]) == (RULING, 2, nc), (tag, ev)
    else:
        assert ev["splitters"] == rr.expected_splitters(link, sl), (tag, ev)
        assert (ev["partitioned"], ev["part_attempts"], ev["sparse_cut"], ev["source"]) == (1, 2 if nc else 1, nc, RULING), (tag, ev)
    return ev


def run(engine, tag, link, weights=None, circ=True, world=0, frag_off=None, opts=None, **kw):
    if world and frag_off is None:
        frag_off = even(len(link) // 2, world)
    out = call(engine, link, weights, circ, world, frag_off, opts)
    verify(tag, link, weights, out, opts, world, circ, **kw)
    return out


ONE_GPU = [{}, {"rank_wyllie": 1}, {"split_log2": 1}, {"split_log2": 5}, {"split_log2": 12}, {"rank_round_batch0": 1}, {"rank_round_batch0": 12}]
PART = [(w, b) for w in (1, 2, 3, 8) for b in (1, 8)]


def every_leg(engine, tag, link, weights, part_opts=None):
    """the structure under every leg: the one-GPU options weighted with marks, then unweighted and without marks; worlds 1, 2, 3 and 8
    under rank_round_batch 1 and 8 with even shares, and once more with empty owners and with one owner holding everything"""
    n = len(link) // 2
    first = None
    for o in ONE_GPU:
        out = run(engine, tag, link, weights, opts=o)
        if first is None:
            first = out
        if not first.ev["n_circles"]:
            assert np.array_equal(out.rk, first.rk), (tag, o)          # lists only: nothing is left to choice
    for o in ({}, {"rank_wyllie": 1}, {"split_log2": 1}):
        run(engine, tag, link, None, opts=o)
        run(engine, tag, link, weights, circ=False, opts=o)
        run(engine, tag, link, None, circ=False, opts=o)
    for world, batch in PART:
        o = dict(part_opts or {}, rank_round_batch=batch)
        out = run(engine, tag, link, weights, world=world, opts=o)
        if not first.ev["n_circles"]:
            assert out.rk.tobytes() == first.rk.tobytes(), (tag, world, batch)
        if world > 1 and batch == 8:
            for fo in ragged(n, world):
                out = run(engine, tag + f" frag_off={fo}", link, weights, world=world, frag_off=fo, opts=o)
                if not first.ev["n_circles"]:
                    assert out.rk.tobytes() == first.rk.tobytes(), (tag, world, fo)
    return first


# ---------------------------------------------------------------- structures

def spread(n, parts):
    """parts: (kind, length) with kind in chain / turn / turn_head / turns2 / circle / single, over consecutive nodes; the rest are singletons"""
    L = rr.Links(n)
    at = 0
    for kind, k in parts:
        nodes = range(at, at + k)
        at += k
        if kind == "chain":
            L.chain(nodes)
        elif kind == "turn":
            L.chain(nodes, turn_tail=True)
        elif kind == "turn_head":
            L.chain(nodes, turn_head=True)
        elif kind == "turns2":
            L.chain(nodes, turn_head=True, turn_tail=True)
        elif kind == "circle":
            L.circle(nodes)
        else:
            assert kind == "single"
    assert at <= n
    return L.link


LENGTHS = (1, 2, 31, 32, 33, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def mirror_job(n):
    """mirror pairs and self-mirror lists of the lengths where the walks and the wave reductions turn over, relabelled at random"""
    rng = np.random.default_rng(11)
    kinds = ("chain", "turn", "turn_head") if n >= 3 * sum(LENGTHS) else ("chain", "turn")
    parts = [(kind, k) for k in LENGTHS for kind in kinds]
    link = spread(n, parts)
    w = rng.integers(1, 1001, n).astype(np.uint32)
    link, w = rr.relabel(link, w, rng)
    assert rr.is_involution(link) and not rr.circles(link)
    return link, w


# ---------------------------------------------------------------- the cases

def test_threshold_between_wyllie_and_the_ruling_set(engine):
    """n = 2047 runs pointer jumping, 2048 the ruling set: the same structure, extended by one singleton"""
    rng = np.random.default_rng(5)
    a = rr.random_mixture(2047, rng, max_len=300)
    b = np.concatenate([a, np.full(2, NONE, np.uint32)])
    w = rng.integers(1, 1001, 2048).astype(np.uint32)
    oa = run(engine, "threshold", a, w[:2047])
    ob = run(engine, "threshold", b, w)
    assert oa.ev["source"] == WYLLIE and ob.ev["source"] == RULING and ob.ev["ruling_attempts"] == 2 and oa.ev["n_circles"] == ob.ev["n_circles"] > 0
    # circ NULL: both cut at the minimum node, so the two answers are the same arrays
    oa = run(engine, "threshold", a, w[:2047], circ=False)
    ob = run(engine, "threshold", b, w, circ=False)
    assert (oa.ev["source"], ob.ev["source"]) == (WYLLIE, RULING_THEN_WYLLIE)
    assert np.array_equal(oa.link, ob.link[:-2]) and np.array_equal(oa.rk, ob.rk[:-2])


def test_tiny(engine):
    """n = 1 and 2 in every legal configuration, one GPU and partitioned; all singletons at n = 2048: every state a head, m = 2n"""
    for n in (1, 2):
        for i, link in enumerate(rr.all_structures(n)):
            w = np.array([7, 1000][:n], np.uint32)
            for weights in (w, None):
                for circ in (True, False):
                    run(engine, f"tiny#{i}", link, weights, circ=circ)
            for world in (1, 2, 8):
                run(engine, f"tiny#{i}", link, w, world=world)
    link = np.full(4096, NONE, np.uint32)
    for o in ({}, {"split_log2": 12}, {"split_log2": 1}):
        out = run(engine, "singletons", link, None, opts=o)
        assert out.ev["splitters"] == 4096 and out.ev["source"] == RULING
        assert np.array_equal(out.rk, np.stack([np.zeros(4096, np.uint32), np.arange(4096, dtype=np.uint32)], axis=1))
    out = run(engine, "singletons", link, np.ones(2048, np.uint32), world=3)
    assert out.ev["splitters"] == 4096


ROUND_SIZES = sorted({m + d for m in [1 << k for k in range(0, 11)] + [2048, 4096, 8192] for d in (-1, 0, 1) if m + d >= 1})


@pytest.mark.parametrize("group", [0, 1, 2])
def test_round_bounds(engine, group):
    """One chain with a turn at one end is a single list of 2n states that is its own mirror.  At 2n a power of two (and beside it) both
    Wyllie's max_rounds and the jumping over the splitters with slack 1 are tight: a list that "did not converge" would be taken for a
    circle, cut, and show as n_circles = 1 and a changed link."""
    sizes = [n for n in ROUND_SIZES if (n < 100, 100 <= n < 2000, n >= 2000)[group]]
    for n in sizes:
        for head in (False, True):
            link = rr.Links(n).chain(range(n), turn_head=head, turn_tail=not head).link
            w = (np.arange(n, dtype=np.uint32) % 997) + 1
            legs = [{}, {"rank_wyllie": 1}] + ([{"split_log2": 1}, {"split_log2": 12}, {"rank_round_batch0": 1}] if n >= 2048 else [])
            for o in legs:
                out = run(engine, "round_bounds", link, w, opts=o)
                assert out.ev["n_circles"] == 0 and np.array_equal(out.link, link)
            for o in ({"rank_round_batch": 1}, {"rank_round_batch": 8}, {"rank_round_batch": 1, "split_log2": 1}):
                out = run(engine, "round_bounds", link, w, world=2, opts=o)
                assert out.ev["n_circles"] == 0 and np.array_equal(out.link, link)
    # a chain of singletons-with-turns: n lists of 2 states, and m = 2^k exactly: the splitter list's own bound with slack 1
    for n in (2048, 4096):
        L = rr.Links(n)
        for v in range(n):
            L.chain([v], turn_tail=True)
        out = run(engine, "round_bounds turns", L.link, None)
        assert out.ev["splitters"] >= n


def test_second_batch_of_rounds(engine):
    """One chain of 20 000 nodes at split_log2 = 1: each of its two lists holds some 10 000 splitters, more than the 2^12 the first batch
    of rank_round_batch0 = 12 rounds covers, so the second batch of jump_rounds decides"""
    n = 20000
    rng = np.random.default_rng(3)
    link = rr.Links(n).chain(rng.permutation(n), rng.integers(0, 2, n)).link
    w = rng.integers(1, 1001, n).astype(np.uint32)
    sp = rr.sampled(np.arange(n), 1)
    assert int(sp.sum()) > 4096 + 2
    outs = []
    for b0 in (1, 12):
        out = run(engine, "second_batch", link, w, opts={"split_log2": 1, "rank_round_batch0": b0})
        assert out.ev["rounds"] > b0 and out.ev["rounds"] > 12 and out.ev["source"] == RULING and out.ev["ruling_attempts"] == 1, out.ev
        outs.append(out)
    assert outs[0].rk.tobytes() == outs[1].rk.tobytes()
    for b in (1, 8):
        out = run(engine, "second_batch", link, w, world=3, opts={"split_log2": 1, "rank_round_batch": b})
        assert out.ev["rounds"] > 12 and out.rk.tobytes() == outs[0].rk.tobytes()


@pytest.mark.parametrize("n", [2047, 2048 + 1731])
def test_mirror_pairs_and_self_mirror_lists(engine, n):
    link, w = mirror_job(n)
    every_leg(engine, "mirror", link, w)


def splitter_circle_job():
    """split_log2 = 12: the sampled nodes below 4096 are 0, 1626 and 2589.  Circles through them (their splitters form cycles in the
    splitter list) and circles that avoid them (no walk reaches them), a self-mirror circle of each kind, lists between"""
    n = 4096
    assert np.nonzero(rr.sampled(np.arange(n), 12))[0].tolist() == [0, 1626, 2589]
    L = rr.Links(n)
    L.circle([0, 5, 6, 7])                                        # one sampled node
    L.circle(list(range(1620, 1640)), orient=[i % 2 for i in range(20)])      # through 1626
    L.chain(list(range(2580, 2600)), turn_head=True, turn_tail=True)          # through 2589, two turns: its own mirror
    L.circle([10])                                                # splitter-free, 1 / 2 / 3 / 300 nodes
    L.circle([12, 11])
    L.circle([13, 15, 14], orient=[0, 1, 0])
    L.circle(list(range(400, 700))[::-1])
    L.chain(list(range(100, 140)), turn_head=True, turn_tail=True)            # splitter-free, two turns: its own mirror
    L.chain([20], turn_head=True, turn_tail=True)                 # ... of one node: two fixed points
    L.chain(list(range(1000, 1300)))
    L.chain(list(range(3000, 3257)), turn_tail=True)
    L.chain(list(range(3300, 3333)), turn_head=True)
    w = (np.arange(n, dtype=np.uint32) * 31 % 1000) + 1
    assert len(rr.circles(L.link)) == 9
    return L.link, w


def test_splitter_cycles_and_splitter_free_circles(engine):
    link, w = splitter_circle_job()
    o = {"split_log2": 12}
    out = run(engine, "circles", link, w, opts=o)
    ev = out.ev
    assert (ev["n_circles"], ev["sparse_cut"], ev["ruling_attempts"], ev["bad"], ev["source"]) == (9, 9, 2, 0, RULING), ev
    assert ev["splitters"] == rr.expected_splitters(link, 12)
    run(engine, "circles", link, None, opts=o)
    for b0 in (1, 12):
        run(engine, "circles", link, w, opts=dict(o, rank_round_batch0=b0))
    # the same job under the other spacings: which circles hold a splitter changes, the contract does not
    for sl in (1, 5):
        run(engine, "circles", link, w, opts={"split_log2": sl})
    for world, batch in PART:
        out = run(engine, "circles", link, w, world=world, opts=dict(o, rank_round_batch=batch))
        assert (out.ev["n_circles"], out.ev["part_attempts"], out.ev["partitioned"]) == (9, 2, 1)
        if world > 1 and batch == 1:
            for fo in ragged(4096, world):
                run(engine, f"circles frag_off={fo}", link, w, world=world, frag_off=fo, opts=dict(o, rank_round_batch=batch))


def test_wyllie_cuts_at_the_minimum_node(engine):
    """the same job where pointer jumping does the cutting: no mark array, or rank_wyllie = 1 -- under exact_cut"""
    link, w = splitter_circle_job()
    want = rr.solve(link, w)
    for circ, o in ((False, {"split_log2": 12}), (False, {}), (True, {"rank_wyllie": 1}), (False, {"rank_wyllie": 1})):
        for weights in (w, None):
            out = run(engine, "wyllie_cuts", link, weights, circ=circ, opts=o)
            assert out.ev["source"] == (WYLLIE if "rank_wyllie" in o else RULING_THEN_WYLLIE) and np.array_equal(out.link, want[0])
            if weights is not None:
                assert np.array_equal(out.rk, want[2])
            if circ:
                assert np.array_equal(out.circ, want[1])


@functools.lru_cache(maxsize=None)
def bad_job():
    """2^18 + 2048 circles of one and two nodes, none holding a sampled node at split_log2 = 12: more than the sparse cut's list takes"""
    N = (1 << 18) + 2048
    n = 400000
    free = np.nonzero(~rr.sampled(np.arange(n), 12))[0]
    n1 = N // 2
    link = np.full(2 * n, NONE, np.uint32)
    a = free[:n1]
    link[2 * a], link[2 * a + 1] = 2 * a + 1, 2 * a
    b = free[n1:n1 + 2 * (N - n1)].reshape(-1, 2)
    x, y = b[:, 0], b[:, 1]
    link[2 * x + 1], link[2 * y] = 2 * y, 2 * x + 1
    link[2 * y + 1], link[2 * x] = 2 * x, 2 * y + 1
    assert rr.is_involution(link)
    w = (np.arange(n, dtype=np.uint32) % 1000) + 1
    return link, w, N


def test_bad_branch_counts_the_cuts_already_made(engine):
    """cut_circles_sparse reports `bad` when its list of 2^18 circles is full -- after it has cut those 2^18.  The fallback cuts the
    rest; n_circles must be the number of circle classes, not the rest alone."""
    link, w, N = bad_job()
    out = call(engine, link, w, opts={"split_log2": 12})
    ev = verify("bad", link, w, out, {"split_log2": 12}, expect_bad=True)
    assert (ev["bad"], ev["source"], ev["ruling_attempts"], ev["sparse_cut"]) == (1, RULING_THEN_WYLLIE, 1, 1 << 18), ev
    assert ev["n_circles"] == N


def test_bad_branch_partitioned(engine):
    """the same verdict in the partitioned form: every rank says 1, the replicated ranking finishes on the links as the cuts left them"""
    link, w, N = bad_job()
    o = {"split_log2": 12, "rank_round_batch": 8}
    fo = even(len(link) // 2, 2)
    out = call(engine, link, w, world=2, frag_off=fo, opts=o)
    ev = verify("bad", link, w, out, o, world=2, expect_bad=True)
    assert (ev["bad"], ev["partitioned"], ev["part_attempts"]) == (1, 0, 1) and ev["sparse_cut"] == N and ev["n_circles"] == N, ev


def test_weights(engine):
    rng = np.random.default_rng(9)
    n = 3000
    link = rr.random_mixture(n, rng, max_len=500, p_circle=0.1)
    # all weights 1 equals the unweighted run: the same cuts (the sparse cut does not read weights), so the same arrays
    for o in ({}, {"rank_wyllie": 1}, {"split_log2": 1}):
        a = run(engine, "weights ones", link, np.ones(n, np.uint32), opts=o)
        b = run(engine, "weights ones", link, None, opts=o)
        assert np.array_equal(a.rk, b.rk) and np.array_equal(a.link, b.link)
        run(engine, "weights random", link, rng.integers(1, 1001, n).astype(np.uint32), opts=o)
    # one list of 2 600 nodes whose weights add up to 2^32 - 1, a single node of 2^31 in it: every true distance fits 32 bits, just
    k = 2600
    w = np.ones(n, np.uint32)
    heavy = rng.integers(1, 1 << 19, k).astype(np.uint64)
    heavy[1300] = 1 << 31
    heavy[7] += np.uint64((1 << 32) - 1) - heavy.sum()
    assert heavy.sum() == (1 << 32) - 1 and heavy.min() >= 1 and heavy.max() == 1 << 31
    nodes = rng.permutation(n)
    L = rr.Links(n).chain(nodes[:k], rng.integers(0, 2, k))
    L.chain(nodes[k:k + 300], turn_tail=True)
    w[nodes[:k]] = heavy.astype(np.uint32)
    for o in ({}, {"rank_wyllie": 1}, {"split_log2": 1}, {"split_log2": 12}, {"rank_round_batch0": 1}):
        out = run(engine, "weights 2^32-1", L.link, w, opts=o)
        assert int(out.rk[:, 0].max()) == (1 << 32) - 1 - int(min(heavy[0], heavy[-1]))
    for world in (1, 3):
        run(engine, "weights 2^32-1", L.link, w, world=world)


def test_partitioned_only(engine):
    """n = 1 under world = 8: m = 2, six ranks hold no splitter; m not divisible by the world; more owners than nodes"""
    one = np.full(2, NONE, np.uint32)
    out = run(engine, "partitioned n=1", one, np.array([5], np.uint32), world=8, frag_off=[0, 0, 0, 1, 1, 1, 1, 1, 1])
    assert out.ev["splitters"] == 2 and np.array_equal(out.rk, [[0, 0], [0, 1]])
    link, w = mirror_job(2048 + 1731)
    base = run(engine, "partitioned base", link, w)
    for sl in (5, 12, 1):
        m = rr.expected_splitters(link, sl)
        worlds = [x for x in (3, 7, 8) if m % x]
        assert worlds, m
        for world in worlds[:2]:
            out = run(engine, f"partitioned m={m}", link, w, world=world, opts={"split_log2": sl})
            assert out.ev["splitters"] == m and out.rk.tobytes() == base.rk.tobytes()
    small = rr.Links(3).chain([2, 0, 1], [1, 0, 0]).link
    run(engine, "partitioned n=3", small, np.array([3, 4, 5], np.uint32), world=8)


@pytest.mark.parametrize("seed", range(20))
def test_fuzz(engine, seed):
    """random mixtures of chains, turns, circles and singletons at n = 2047 (pointer jumping), 5000 and 70 000: every one-GPU option at
    every size (weighted with marks, unweighted and without marks in turn), and two of the eight (world, batch) legs per size, which
    rotate with the seed together with the spacing and the shape of frag_off"""
    rng = np.random.default_rng(1000 + seed)
    for n in (2047, 5000, 70000):
        link = rr.random_mixture(n, rng, max_len=(40, 400, 3000)[seed % 3], p_circle=(0.15, 0.02, 0.3)[seed % 3 - 1])
        if seed % 4 == 0:
            link, _ = rr.relabel(link, None, rng)
        w = rng.integers(1, 1001, n).astype(np.uint32)
        for i, o in enumerate(ONE_GPU):
            kind = (seed + i) % 4           # weighted with marks most of the time; unweighted and markless in turn
            run(engine, f"fuzz#{seed}", link, None if kind == 1 else w, circ=kind != 2, opts=o)
        parts = [PART[(seed + i) % len(PART)] for i in (0, 3)]
        for world, batch in parts:
            sl = (5, 12, 1)[(seed + world) % 3]
            fos = [even(n, world)] + (ragged(n, world)[seed % 2:seed % 2 + 1] if world > 1 else [])
            for fo in fos:
                run(engine, f"fuzz#{seed} frag_off={'even' if fo == even(n, world) else fo}", link, w, world=world, frag_off=fo,
                    opts={"rank_round_batch": batch, "split_log2": sl})


def test_refusals(engine):
    """SNK_E_ARG with the evidence zeroed and the caller's arrays untouched; valid links without a circle are not changed either"""
    n = 3000
    link, w = mirror_job(n)
    zero = {f: 0 for f in call(engine, np.full(2, NONE, np.uint32)).ev}

    def refused(tag, lk, weights=w, world=0, frag_off=None, circ=True, nn=None, what=""):
        out = call(engine, lk, weights, circ, world, frag_off, n=nn)
        assert out.rc == E_ARG and what in out.msg, (tag, out.rc, out.msg)
        assert out.ev == zero, (tag, out.ev)
        assert np.array_equal(out.link, lk) and (out.circ is None or not out.circ.any()) and (out.rk == 0x5A5A5A5A).all(), tag

    s = int(np.nonzero(link != NONE)[0][10])
    t = int(np.nonzero((link == NONE))[0][3])
    a = link.copy()
    a[s] = t                                  # link[t] is NONE: link[link[s]] != s
    refused("one-sided link", a, what="involution")
    a = link.copy()
    p = int(a[s])
    q = int(np.nonzero((link != NONE) & (np.arange(2 * n) != s) & (np.arange(2 * n) != p))[0][0])
    a[s] = q                                  # points at a state that is joined to another one
    refused("crossed link", a, what="involution")
    a = link.copy()
    a[t] = 2 * n
    refused("link == 2n", a, what="outside")
    a[t] = 0xFFFFFFFE
    refused("link == 2^32 - 2", a, what="outside")
    for world in (1, 3):
        refused("one-sided link, partitioned", np.where(np.arange(2 * n) == s, t, link).astype(np.uint32), world=world, frag_off=even(n, world))
    refused("frag_off ends before n", link, world=2, frag_off=[0, n // 2, n - 1], what="frag_off")
    refused("frag_off ends after n", link, world=2, frag_off=[0, n // 2, n + 1], what="frag_off")
    refused("frag_off starts after 0", link, world=2, frag_off=[1, n // 2, n], what="frag_off")
    refused("frag_off descends", link, world=3, frag_off=[0, n, n // 2, n], what="frag_off")
    refused("partitioned without weights", link, weights=None, world=2, frag_off=even(n, 2), what="weights")
    refused("partitioned without marks", link, world=2, frag_off=even(n, 2), circ=False, what="circ")
    refused("2n = 2^32", link, nn=1 << 31, what="2^32")
    # n == 0: SNK_OK, nothing written
    out = call(engine, link, w, n=0)
    assert out.rc == 0 and out.ev == zero and np.array_equal(out.link, link) and (out.rk == 0x5A5A5A5A).all()
    # valid links, no circle: link[] comes back as it went in, no mark is set
    for world in (0, 2):
        out = run(engine, "untouched", link, w, world=world)
        assert np.array_equal(out.link, link) and not out.circ.any() and out.ev["n_circles"] == 0
