"""A plain reference of the list ranking (csrc/snk_rank.hip, snk_dev_rank_lists) and the checker of its contract.  Pure Python and numpy,
64-bit sums, sequential walks: no pointer jumping, no splitters.

The structure.  n nodes have 2n directed states s = 2 * node + side.  link[s] is the state that s is joined to, or NONE; the links are
an involution, link[link[s]] == s, and a fixed point link[s] == s is a turn.  The successor of s is link[s] ^ 1: leave the node through
side `s & 1`, arrive at the partner's state, go on through that node's other side.  A head is a state nobody walks into
(link[s ^ 1] == NONE), a terminal one that walks nowhere (link[s] == NONE).  Every walk exists twice, once in each direction (s and the
mirror s ^ 1); a walk through a turn is its own mirror.

The contract.  rk[s] = (the summed weight of the nodes stepped onto after s up to the terminal of its list, that terminal); a terminal
has (0, itself).  A circle class -- a directed cycle and its mirror, which may be the same cycle -- loses exactly one involution pair
{s, link[s]} (one state where that is a fixed point), circ marks the states of those pairs, n_circles counts the classes, and nothing
else in link[] changes."""
import numpy as np

NONE = 0xFFFFFFFF


# ---------------------------------------------------------------- the reference

def ref_rank(link, weights=None):
    """-> (dist u64[2n], term i64[2n]); term == -1: the state was not reached from any head, so it lies on a circle"""
    link = np.asarray(link, dtype=np.uint32)
    ns = len(link)
    w = np.ones(ns // 2, np.uint64) if weights is None else np.asarray(weights).astype(np.uint64)
    ll, wl = link.tolist(), w.tolist()          # Python integers: the sums cannot wrap
    dist, term = [0] * ns, [-1] * ns
    flip = np.arange(ns) ^ 1
    for h in np.nonzero(link[flip] == NONE)[0].tolist():
        path = [h]
        s = h
        while ll[s] != NONE:
            s = ll[s] ^ 1
            path.append(s)
        d = 0
        for x in reversed(path):          # from the terminal back: d = weight of what comes after x
            dist[x] = d
            term[x] = s
            d += wl[x >> 1]
    return np.asarray(dist, dtype=np.uint64), np.asarray(term, dtype=np.int64)


def circles(link):
    """-> the circle classes, each as (sorted node array, set of its states), in the order of their minimum node"""
    link = np.asarray(link, dtype=np.uint32)
    _, term = ref_rank(link)
    ll = link.tolist()
    seen = set()
    out = []
    for s0 in np.nonzero(term < 0)[0].tolist():
        if s0 in seen:
            continue
        cyc = [s0]
        s = ll[s0] ^ 1
        while s != s0:
            cyc.append(s)
            s = ll[s] ^ 1
        states = set(cyc) | {x ^ 1 for x in cyc}
        seen |= states
        out.append((np.unique(np.asarray(cyc) >> 1), states))
    out.sort(key=lambda c: int(c[0][0]))
    return out


def solve(link, weights=None, cut_at=None):
    """The expected answer with every circle cut at state 2 * min_node + 1 (cut_at: {class index: state} cuts elsewhere)
    -> (link_out, circ, rk u32[2n, 2], n_circles)"""
    link_out = np.array(link, dtype=np.uint32)
    circ = np.zeros(len(link_out), np.uint8)
    cls = circles(link)
    for i, (nodes, _) in enumerate(cls):
        s = (cut_at or {}).get(i, 2 * int(nodes[0]) + 1)
        for x in {s, int(link[s])}:
            link_out[x] = NONE
            circ[x] = 1
    dist, term = ref_rank(link_out, weights)
    assert (term >= 0).all() and (dist < 1 << 32).all()
    return link_out, circ, np.stack([dist, term.astype(np.uint64)], axis=1).astype(np.uint32), len(cls)


class Wrong(AssertionError):
    pass


def check(link_in, weights, link_out, circ, rk, n_circles, exact_cut):
    """Raises Wrong with the first difference.  circ None: the ranking was given no mark array."""
    link_in, link_out = np.asarray(link_in, dtype=np.uint32), np.asarray(link_out, dtype=np.uint32)
    ns = len(link_in)
    rk = np.asarray(rk, dtype=np.uint32).reshape(ns, 2)
    if len(link_out) != ns:
        raise Wrong("link_out has another length")
    cls = circles(link_in)
    changed = set(np.nonzero(link_in != link_out)[0].tolist())
    if any(link_out[s] != NONE for s in changed):
        raise Wrong(f"a link was changed to something else than NONE: state {min(s for s in changed if link_out[s] != NONE)}")
    in_class = set()
    for nodes, states in cls:
        in_class |= states
        cut = sorted(changed & states)
        if not cut:
            raise Wrong(f"the circle of node {int(nodes[0])} ({len(nodes)} nodes) was not cut")
        s = cut[0]
        if set(cut) != {s, int(link_in[s])}:
            raise Wrong(f"the circle of node {int(nodes[0])} lost the states {cut[:6]}: not one involution pair")
        if exact_cut and 2 * int(nodes[0]) + 1 not in cut:
            raise Wrong(f"the circle of node {int(nodes[0])} was cut at {cut}, not at state {2 * int(nodes[0]) + 1}")
    outside = changed - in_class
    if outside:
        raise Wrong(f"a link outside any circle changed: state {min(outside)}")
    if circ is not None:
        marked = set(np.nonzero(np.asarray(circ))[0].tolist())
        if marked != changed:
            raise Wrong(f"circ marks {len(marked)} states, the cuts removed {len(changed)}: {sorted(marked ^ changed)[:6]} differ")
        if not np.isin(np.asarray(circ), (0, 1)).all():
            raise Wrong("circ holds something else than 0 and 1")
    if int(n_circles) != len(cls):
        raise Wrong(f"n_circles = {int(n_circles)}, the links hold {len(cls)} circles")
    dist, term = ref_rank(link_out, weights)
    if (term < 0).any():
        raise Wrong(f"state {int(np.nonzero(term < 0)[0][0])} is still on a circle")      # (cannot happen after the above: kept as a guard)
    if (dist >> np.uint64(32)).any():
        raise Wrong("a true distance does not fit 32 bits: the case is outside the contract of rk")
    bad = np.nonzero((rk[:, 0].astype(np.uint64) != dist) | (rk[:, 1].astype(np.int64) != term))[0]
    if len(bad):
        s = int(bad[0])
        raise Wrong(f"rk[{s}] = ({int(rk[s, 0])}, {int(rk[s, 1])}), expected ({int(dist[s])}, {int(term[s])}); {len(bad)} states differ")


# ---------------------------------------------------------------- builders

class Links:
    """link[] of n nodes, filled component by component.  A walk is given by its nodes in order and, per node, the side it leaves
    through (orient, default 1): its states are e_i = 2 * node_i + orient_i and link[e_i] = e_{i+1} ^ 1."""

    def __init__(self, n):
        self.n = n
        self.link = np.full(2 * n, NONE, np.uint32)

    def _join(self, a, b):
        assert self.link[a] == NONE and self.link[b] == NONE, (a, b)
        self.link[a] = b
        self.link[b] = a

    def chain(self, nodes, orient=None, turn_head=False, turn_tail=False, close=False):
        """a chain; with a turn at one end a single self-mirror list; with a turn at both ends a circle that is its own mirror;
        close: a circle (two directed cycles, mirrors of each other)"""
        nodes = [int(x) for x in nodes]
        orient = [1] * len(nodes) if orient is None else [int(o) for o in orient]
        e = [2 * v + o for v, o in zip(nodes, orient)]
        for a, b in zip(e, e[1:]):
            self._join(a, b ^ 1)
        if close:
            assert not (turn_head or turn_tail)
            self._join(e[-1], e[0] ^ 1)
        if turn_tail:
            self._join(e[-1], e[-1])
        if turn_head:
            self._join(e[0] ^ 1, e[0] ^ 1)
        return self

    def circle(self, nodes, orient=None):
        return self.chain(nodes, orient, close=True)


def relabel(link, weights, rng):
    """the same structure under a random renaming of the nodes and a random flip of each node's two sides"""
    link = np.asarray(link, dtype=np.uint32)
    n = len(link) // 2
    perm = rng.permutation(n).astype(np.int64)
    flip = rng.integers(0, 2, n).astype(np.int64)
    s = np.arange(2 * n, dtype=np.int64)
    to = 2 * perm[s >> 1] + ((s & 1) ^ flip[s >> 1])
    out = np.full(2 * n, NONE, np.uint32)
    has = link != NONE
    out[to[has]] = to[link[has].astype(np.int64)].astype(np.uint32)
    w = None
    if weights is not None:
        w = np.empty(n, np.asarray(weights).dtype)
        w[perm] = weights
    return out, w


def is_involution(link):
    link = np.asarray(link, dtype=np.uint32)
    has = np.nonzero(link != NONE)[0]
    return bool((link[has] < len(link)).all() and (link[link[has].astype(np.int64)] == has).all())


def random_mixture(n, rng, max_len=400, p_circle=0.15, p_turn=0.25, p_single=0.1, nodes=None):
    """chains, chains with a turn at one or both ends, circles and singletons over `nodes` (default: all n, shuffled), random sides"""
    L = Links(n)
    pool = rng.permutation(n) if nodes is None else np.asarray(nodes)
    at = 0
    while at < len(pool):
        r = rng.random()
        if r < p_single:
            at += 1
            continue
        k = int(min(len(pool) - at, rng.integers(1, max_len + 1) if rng.random() < 0.5 else rng.integers(1, 9)))
        part = pool[at:at + k]
        at += k
        orient = rng.integers(0, 2, k)
        r = rng.random()
        if r < p_circle:
            L.circle(part, orient)
        elif r < p_circle + p_turn:
            t = int(rng.integers(0, 3))
            L.chain(part, orient, turn_head=t in (0, 2), turn_tail=t in (1, 2))
        else:
            L.chain(part, orient)
    return L.link


def all_structures(n):
    """every link structure of n nodes: each state is free, a turn, or paired with another one"""
    ns = 2 * n

    def rec(s, link):
        if s == ns:
            yield np.array(link, dtype=np.uint32)
            return
        if link[s] is not None:
            yield from rec(s + 1, link)
            return
        for choice in [NONE, s] + [t for t in range(s + 1, ns) if link[t] is None]:
            l2 = list(link)
            l2[s] = choice
            if choice not in (NONE, s):
                l2[choice] = s
            yield from rec(s + 1, l2)

    yield from rec(0, [None] * ns)


# ---------------------------------------------------------------- the device's sample, restated to place nodes on purpose

def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def sampled(node, split_log2):
    """both states of `node` are splitters by the hash (sampled_state in csrc/snk_rank.hip: snk_mix32(s >> 1) >> 7, masked)"""
    return ((mix32(node) >> np.uint64(7)) & np.uint64((1 << split_log2) - 1)) == 0


def expected_splitters(link, split_log2):
    """heads and sampled states: the m that the evidence of a ruling-set run must show"""
    link = np.asarray(link, dtype=np.uint32)
    s = np.arange(len(link))
    return int(((link[s ^ 1] == NONE) | sampled(s >> 1, split_log2)).sum())
