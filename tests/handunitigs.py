"""Hand-made unitig sets for the graph-from-unitigs step (a14: snk_hbv_from_unitigs, snk_dev_hbv; a13: snk_dev_bv_image) -- test
infrastructure (tests/test_hbv_handmade_host.py, tests/test_gpu_hbv_handmade.py, tests/golden/make_hbv_golden.py).  numpy and Python only.

A case is built from a topology, not from reads: junctions are random (K-1)-mers, a unitig is end(a) + interior + end(b) with end(x) the
junction or its reverse complement, chains and rings are a random (circular) string cut into pieces that overlap by K-1.  Random K-mers
never meet by chance at K >= 48, so two k-mers of a case are equal only where the construction makes them so; what the construction must
keep apart is kept apart by _Junction's slots (the four bases that may follow a (K-1)-mer and the four that may precede it: one unitig
strand each).  Every case is then CHECKED to be the unitig set of a de Bruijn graph (check_valid), and carries `facts` -- counted here by a
plain union-find over strings, nothing of the code under test -- which the tests assert, so that a later edit cannot lose what a case is for.

    case(name, K) -> namespace(name, K, unitigs: strings in BVComp order (length descending, then lexicographic), off u64[U + 1],
                               bases u8 codes, facts)
    orders(c)     -> {"bvcomp", "shuffled", "reversed"}: perm with input[i] = c.unitigs[perm[i]]
"""
from __future__ import annotations

import zlib
from types import SimpleNamespace

import numpy as np

KS = (48, 60)
_COMP = str.maketrans("ACGT", "TGCA")
_CODE = np.zeros(256, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def rc(s: str) -> str:
    return s.translate(_COMP)[::-1]


def comp(b: str) -> str:
    return b.translate(_COMP)


def is_palindrome(s: str) -> bool:
    return len(s) % 2 == 0 and s == rc(s)


class _Gen:
    def __init__(self, name, K):
        self.K, self.rng, self.unitigs = K, np.random.default_rng(zlib.crc32(f"{name}/{K}".encode())), []

    def rand(self, n) -> str:
        return "".join("ACGT"[i] for i in self.rng.integers(0, 4, n)) if n > 0 else ""

    def pal(self, n) -> str:
        """a random palindrome of n (even) bases"""
        assert n % 2 == 0
        x = self.rand(n // 2)
        return x + rc(x)

    def junction(self, seq=None):
        return _Junction(self, seq)

    def add(self, s):
        self.unitigs.append(s)
        return s

    def edge(self, a, sa, b, sb, n_interior=None, must=True):
        """the unitig end(a) + interior + end(b); sa / sb = 1: that end is the junction's reverse complement.  The interior's first and last
        base take a free slot of a and of b."""
        n = int(self.rng.integers(1, 20)) if n_interior is None else n_interior
        assert n >= 1
        for _ in range(64):
            i = self.rand(n)
            ka, kb = a.slot(sa, 0, i[0]), b.slot(sb, 1, i[-1])
            if ka != kb and a.free(ka) and b.free(kb):             # (ka == kb: a hairpin whose two ends would be one k-mer, both strands)
                a.take(ka)
                b.take(kb)
                return self.add(a.end(sa) + i + b.end(sb))
        assert not must, "no free slot at a junction"
        return None

    def palindrome_on(self, a, n):
        """a palindromic unitig of n >= 2K bases whose first (K-1)-mer is junction a (and whose last is a's reverse complement: one slot)"""
        assert n % 2 == 0 and n >= 2 * self.K
        for _ in range(64):
            x = a.seq + self.rand(n // 2 - (self.K - 1))
            k = a.slot(0, 0, x[self.K - 1])
            if a.free(k):
                a.take(k)
                return self.add(x + rc(x))
        raise AssertionError("no free slot at a junction")

    def chain(self, n, lo=0, hi=30):
        """n pieces of K + lo .. K + hi bases of one random string, neighbours overlapping by K - 1"""
        K = self.K
        lens = [K + int(x) for x in self.rng.integers(lo, hi + 1, n)]
        s = self.rand(sum(lens) - (n - 1) * (K - 1))
        p = 0
        for L in lens:
            self.add(s[p:p + L])
            p += L - (K - 1)

    def ring(self, n, lo=1, hi=31):
        """n pieces of one random CIRCULAR string, neighbours overlapping by K - 1 (n = 1: the first and last (K-1)-mer of the one unitig
        are equal)"""
        K = self.K
        steps = [int(x) for x in self.rng.integers(lo, hi + 1, n)]
        c = self.rand(sum(steps))
        cc = c * (2 + (K + hi) // len(c))
        p = 0
        for d in steps:
            self.add(cc[p:p + d + K - 1])
            p += d


class _Junction:
    """A (K-1)-mer and the k-mers round it: slot ("out", b) = the k-mer seq + b, slot ("in", b) = b + seq.  A unitig strand that starts
    with seq takes an out slot, one that ends with it an in slot; a unitig that has rc(seq) at an end does so with its other strand."""

    def __init__(self, g, seq=None):
        self.seq = g.rand(g.K - 1) if seq is None else seq
        assert len(self.seq) == g.K - 1
        self.used = set()

    def end(self, s):
        return rc(self.seq) if s else self.seq

    def slot(self, s, right, base):
        """the slot a unitig takes whose left (right = 0) or right end is end(s), `base` being its base next to that end"""
        if not right:
            return ("out", base) if not s else ("in", comp(base))
        return ("in", base) if not s else ("out", comp(base))

    def free(self, k):
        return k not in self.used

    def take(self, k):
        assert k not in self.used
        self.used.add(k)


# ---- the cases

def _single(kind):
    def make(g):
        K = g.K
        g.add({"k": lambda: g.rand(K), "k1": lambda: g.rand(K + 1), "pal_k": lambda: g.pal(K), "pal_2k": lambda: g.pal(2 * K)}[kind]())
    return make


def _hairpin(g):
    v = g.junction()
    g.edge(v, 0, v, 1, 9)


def _hairpin_flanks(g):
    v = g.junction()
    g.edge(v, 0, v, 1, 9)
    g.edge(g.junction(), 0, v, 0, 5)            # into v; its other strand leaves rc(v)
    g.edge(g.junction(), 0, v, 0, 17)


def _bubble(g):
    a, b = g.junction(), g.junction()
    g.edge(a, 0, b, 0, 7)
    g.edge(a, 0, b, 0, 7)                        # equal lengths: ranked by their bases
    g.edge(g.junction(), 0, a, 0, 11)
    g.edge(b, 0, g.junction(), 0, 3)


def _full_vertex(g):
    j = g.junction()
    for n in (1, 2, 3, 4):
        g.edge(g.junction(), 0, j, 0, n + 4)
        g.edge(j, 0, g.junction(), 0, n + 4)


def _palindromes(g):
    K = g.K
    g.add(g.pal(4 * K))                          # rank 0: the longest
    g.add(g.pal(K))                              # the last rank: the only unitig of K bases
    g.add(g.pal(2 * K + 2))                      # isolated
    j = g.junction()
    g.palindrome_on(j, 2 * K + 6)                # on a junction that ordinary unitigs share
    g.edge(g.junction(), 0, j, 0, 4)
    g.edge(j, 0, g.junction(), 0, 6)
    g.edge(g.junction(), 1, j, 0, 8)
    g.add(g.pal(K) + g.rand(13))                 # not a palindrome, but its first k-mer is one
    g.chain(3)


def _forest(m):
    def make(g):
        K = g.K
        L = K + 5
        g.add(g.pal(2 * K))
        g.add(g.pal(K + 6))
        g.add(g.pal(L + 1))                      # (L + 1 is even)
        for d in (-1, 1, -1, 1, 2):
            g.add(g.rand(L + d))
        # two unitigs whose first k-mers differ only at base K - 1 have the same first (K-1)-mer, so they share a vertex: those come in
        # fours round it (components of four nodes); all the others are components of one node
        for _ in range(3):
            q = g.rand(K - 1)
            for b in "ACGT":
                g.add(q + b + g.rand(L - K))
        while len(g.unitigs) < m:                # first k-mers that differ only at base 0 (what follows q differs too: q + t is a k-mer)
            q = g.rand(K - 1)
            for b, t in list(zip("ACGT", g.rng.permutation(list("ACGT"))))[:m - len(g.unitigs)]:
                g.add(b + q + t + g.rand(L - K - 1))
    return make


def _long(g):
    K = g.K
    g.add(g.rand(70000))
    for L in range(K, K + 17):                   # every len % 16
        g.add(g.rand(L))
    g.chain(5, 0, 16)
    g.add(g.pal(K + 16))


def _mixed(g):
    K = g.K
    js = [g.junction() for _ in range(36)]
    # junction pairs that overlap by K - 2: the unitig between them has K bases (one pair per junction: two junctions made from one would
    # share K - 2 bases, and the unitigs that leave their reverse complements a k-mer at the second position)
    for a in js[30:36]:
        x = "ACGT"[int(g.rng.integers(0, 4))]
        b = g.junction(a.seq[1:] + x)
        a.take(("out", x))
        b.take(("in", a.seq[0]))
        g.add(a.seq + x)
        js.append(b)
    hub = js[0]                                  # a star: one junction with all eight ends
    for _ in range(4):
        g.edge(g.junction(), 0, hub, 0)
        g.edge(hub, 0, g.junction(), 0)
    for a in js[2:5]:                            # palindromes on junctions that the multigraph below goes on using
        g.palindrome_on(a, 2 * K + 2 * int(g.rng.integers(0, 6)))
    g.edge(js[1], 0, js[1], 0, 6)                # a self-loop and a hairpin for certain
    g.edge(js[1], 0, js[1], 1, 6)
    while len(g.unitigs) < 150:                  # the random multigraph: more self-loops, hairpins and parallel edges come by themselves
        a, b = (js[int(i)] for i in g.rng.integers(1, len(js), 2))
        sa, sb = (int(i) for i in g.rng.integers(0, 2, 2))
        g.edge(a, sa, b, sb, must=False)
    g.add(g.pal(K))
    g.add(g.pal(2 * K + 4))
    g.chain(12)
    g.chain(7, 0, 0)
    g.ring(3)
    g.ring(1)
    for _ in range(8):
        g.add(g.rand(K + int(g.rng.integers(0, 40))))


_MAKERS = {
    "single_k": _single("k"), "single_k1": _single("k1"), "single_pal_k": _single("pal_k"), "single_pal_2k": _single("pal_2k"),
    "circle": lambda g: g.ring(1, 37, 37), "ring_2": lambda g: g.ring(2), "ring_3": lambda g: g.ring(3),
    "hairpin": _hairpin, "hairpin_flanks": _hairpin_flanks, "bubble": _bubble, "full_vertex": _full_vertex, "palindromes": _palindromes,
    **{f"chain_{n}": (lambda n: lambda g: g.chain(n))(n) for n in (2, 4, 5, 1023, 1024, 1025)},
    **{f"forest_{m}": _forest(m) for m in (255, 256, 257)},
    "long": _long,
    **{f"mixed_seed{s}": _mixed for s in (1, 2, 3, 4)},
}
CASES = tuple(_MAKERS)
# the cases whose reference result is kept under tests/golden/hbv/ (make_hbv_golden.py runs the reference over all of them)
SAVED = CASES[:CASES.index("chain_5") + 1] + ("chain_1025", "forest_257", "long", "mixed_seed1")
UNSAVED = tuple(n for n in CASES if n not in SAVED)


# ---- validity and facts

def _strands(unitigs):
    """the nodes of the (unitig, strand) graph: (rank, rc, sequence); a palindrome has one"""
    for u, s in enumerate(unitigs):
        yield u, 0, s
        if not is_palindrome(s):
            yield u, 1, rc(s)


def check_valid(unitigs, K):
    """Asserts that `unitigs` is the unitig set of a de Bruijn graph as a14 needs it (conditions, not measurements)."""
    assert all(len(s) >= K and set(s) <= set("ACGT") for s in unitigs), "a unitig shorter than K"
    seen = set()
    for s in unitigs:
        last = (len(s) - K) // 2 if is_palindrome(s) else len(s) - K         # (a palindrome's k-mers come in mirrored pairs: the first of each)
        for p in range(last + 1):
            k = s[p:p + K]
            r = rc(k)
            c = k if k <= r else r
            assert c not in seen, f"a k-mer occurs twice: {k}"
            seen.add(c)
    ends: dict = {}
    for _, _, s in _strands(unitigs):
        for v in (s[:K - 1], s[-(K - 1):]):
            ends[v] = ends.get(v, 0) + 1
    assert max(ends.values()) <= 8, "a (K-1)-mer with more than 8 edge ends"
    assert len({s[:K] for s in unitigs}) == len(unitigs), "two unitigs share their first K bases"


def compute_facts(unitigs, K) -> dict:
    """unitigs in BVComp order -> U, palindromes, self_loops (HBV edges whose two vertices are one), parallel_pairs (pairs of HBV edges
    with the same two vertices in the same direction), max_ends (at one vertex), n_vertices, n_edges, components (node counts of the
    connected components of the (unitig, strand) graph, in the order of their seeds: forward copies by rank, then reverse copies)."""
    U = len(unitigs)
    nodes = list(_strands(unitigs))
    ids = {(u, r): i for i, (u, r, _) in enumerate(nodes)}
    parent = list(range(len(nodes)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    at: dict = {}
    ends: dict = {}
    pairs: dict = {}
    loops = 0
    for i, (u, r, s) in enumerate(nodes):
        a, b = s[:K - 1], s[-(K - 1):]
        loops += a == b
        pairs[(a, b)] = pairs.get((a, b), 0) + 1
        for v in (a, b):
            ends[v] = ends.get(v, 0) + 1
            if v in at:
                parent[find(i)] = find(at[v])
            else:
                at[v] = i
    seed = {}
    for (u, r), i in ids.items():
        root = find(i)
        seed[root] = min(seed.get(root, 2 * U), r * U + u)
    size = {}
    for i in range(len(nodes)):
        size[find(i)] = size.get(find(i), 0) + 1
    comps = [size[root] for root in sorted(seed, key=seed.get)]
    return dict(U=U, palindromes=sum(is_palindrome(s) for s in unitigs), self_loops=int(loops),
                parallel_pairs=sum(n * (n - 1) // 2 for n in pairs.values()), max_ends=max(ends.values()), n_vertices=len(ends),
                n_edges=len(nodes), components=comps)


def bvcomp_sorted(unitigs):
    return sorted(unitigs, key=lambda s: (-len(s), s))


def to_arrays(unitigs):
    off = np.zeros(len(unitigs) + 1, np.uint64)
    if unitigs:
        off[1:] = np.cumsum([len(s) for s in unitigs], dtype=np.uint64)
    bases = _CODE[np.frombuffer("".join(unitigs).encode(), np.uint8)] if unitigs else np.zeros(0, np.uint8)
    return off, np.ascontiguousarray(bases)


_made: dict = {}


def case(name, K):
    """Made once per process and left unchanged."""
    if (name, K) not in _made:
        g = _Gen(name, K)
        _MAKERS[name](g)
        us = bvcomp_sorted(g.unitigs)
        check_valid(us, K)
        off, bases = to_arrays(us)
        _made[(name, K)] = SimpleNamespace(name=name, K=K, unitigs=us, off=off, bases=bases, facts=compute_facts(us, K))
    return _made[(name, K)]


ORDERS = ("bvcomp", "shuffled", "reversed")


def orders(c) -> dict:
    U = len(c.unitigs)
    return {"bvcomp": np.arange(U), "shuffled": np.random.default_rng(zlib.crc32(f"order/{c.name}/{c.K}".encode())).permutation(U),
            "reversed": np.arange(U)[::-1].copy()}


def reordered(c, perm):
    """-> (off, bases) of the input whose unitig i is c.unitigs[perm[i]]"""
    return to_arrays([c.unitigs[int(i)] for i in perm])


def flood_split(facts, big):
    """-> (components that device threads flood, components handed to host threads) when components above `big` nodes go to the host"""
    dev = sum(n <= big for n in facts["components"])
    return dev, len(facts["components"]) - dev


def check_facts(c):
    """What every case exists for, asserted (tests/test_hbv_handmade_host.py runs this for every case and K)."""
    f, K, name = c.facts, c.K, c.name
    lens = [len(s) for s in c.unitigs]
    assert f["U"] == len(c.unitigs) and f["n_edges"] == 2 * f["U"] - f["palindromes"] == sum(f["components"])
    if name.startswith("single_"):
        assert f["U"] == 1 and lens == [{"single_k": K, "single_k1": K + 1, "single_pal_k": K, "single_pal_2k": 2 * K}[name]]
        assert f["palindromes"] == int("pal" in name) and f["components"] == ([1] if "pal" in name else [1, 1])
        assert f["n_vertices"] == (2 if "pal" in name else 4)
    elif name == "circle":
        assert f["U"] == 1 and f["self_loops"] == 2 and f["n_vertices"] == 2 and f["components"] == [1, 1]
    elif name.startswith("ring_"):
        n = int(name[5:])
        assert f["U"] == n and f["components"] == [n, n] and f["n_vertices"] == 2 * n and f["self_loops"] == 0
    elif name == "hairpin":
        assert f["U"] == 1 and f["components"] == [2] and f["parallel_pairs"] == 1 and f["n_vertices"] == 2        # both strands in one component
    elif name == "hairpin_flanks":
        assert f["U"] == 3 and f["components"] == [6] and f["parallel_pairs"] == 1
    elif name == "bubble":
        assert f["U"] == 4 and f["components"] == [4, 4] and f["parallel_pairs"] == 2 and lens[1] == lens[2]
    elif name == "full_vertex":
        assert f["U"] == 8 and f["max_ends"] == 8 and f["components"] == [8, 8]
    elif name == "palindromes":
        assert f["palindromes"] == 4 and is_palindrome(c.unitigs[0]) and is_palindrome(c.unitigs[-1]) and lens[-1] == K and lens[-2] > K
        assert sum(n == 1 for n in f["components"]) >= 3                           # isolated palindromes
        on = [s for s in c.unitigs if is_palindrome(s) and sum(t[:K - 1] == s[:K - 1] or t[-(K - 1):] == s[:K - 1] for t in c.unitigs) > 1]
        assert len(on) == 1                                                        # one shares its junction with ordinary unitigs
        assert any(is_palindrome(s[:K]) and not is_palindrome(s) for s in c.unitigs)
    elif name.startswith("chain_"):
        n = int(name[6:])
        assert f["U"] == n and f["components"] == [n, n] and f["palindromes"] == 0 and min(lens) >= K and max(lens) <= K + 30
    elif name.startswith("forest_"):
        m = int(name[7:])
        assert f["U"] == m and f["palindromes"] == 3 and set(f["components"]) == {1, 4} and f["components"].count(4) == 6
        assert len(f["components"]) == 2 * m - 3 - 6 * 3
        common = max(set(lens), key=lens.count)
        assert common == K + 5 and lens.count(common) > m - 12 and {common - 1, common + 1} <= set(lens)
        firsts = sorted(s[:K] for s in c.unitigs if len(s) == common)
        at_last = sum(a[:K - 1] == b[:K - 1] for a, b in zip(firsts, firsts[1:]))          # ties of the ranking decided at base K - 1: bit 0 of the key
        rest: dict = {}
        for k in firsts:
            rest.setdefault(k[1:], set()).add(k[0])
        at_first = sum(len(v) - 1 for v in rest.values())                                  # ... and at base 0: the key's top two bits
        assert at_last == 9 and at_first > m // 2, (at_last, at_first)
    elif name == "long":
        assert lens[0] == 70000 and lens[0] > 2**16 and {n % 16 for n in lens} == set(range(16)) and set(range(K, K + 17)) <= set(lens)
        assert f["palindromes"] == 1
    elif name.startswith("mixed_seed"):
        assert 180 <= f["U"] <= 230 and f["palindromes"] >= 3 and f["self_loops"] >= 2 and f["max_ends"] == 8 and K in lens
        assert max(f["components"]) > 100 and f["components"].count(1) >= 8 and len(set(f["components"])) >= 4      # one hot root among several
        assert lens.count(K) >= 4


# ---- expected values: the reference's (tests/golden/hbv/<case>_k<K>.npz, written by tests/golden/make_hbv_golden.py) or the oracle's

HBV_KEYS = ("v_left", "v_right", "src", "is_rc", "fwd", "rev")


def pack2(bases: np.ndarray) -> np.ndarray:
    """base codes, four to a byte (base j at bits 2 * (j % 4)); the tail is padded with zeros"""
    b = np.zeros((len(bases) + 3) // 4 * 4, np.uint8)
    b[:len(bases)] = bases
    b = b.reshape(-1, 4)
    return (b[:, 0] | (b[:, 1] << 2) | (b[:, 2] << 4) | (b[:, 3] << 6)).astype(np.uint8)


def graph_from_xlat(c, fwd, rev, to_left, to_right, n_vertices) -> dict:
    """the six arrays and two counts of a snk_hbv from what the reference returns: its translation tables (per BVComp rank) and the
    vertices of its edges.  src / is_rc follow from the tables (a palindrome's one edge is a forward copy)."""
    E = len(to_left)
    src, is_rc = np.full(E, -1, np.int32), np.zeros(E, np.uint8)
    for u, (f, r) in enumerate(zip(fwd, rev)):
        assert (f == r) == is_palindrome(c.unitigs[u])
        src[r], is_rc[r] = u, 1
        src[f], is_rc[f] = u, 0
    assert (src >= 0).all()
    return dict(n_vertices=int(n_vertices), n_edges=E, v_left=np.asarray(to_left, np.int32), v_right=np.asarray(to_right, np.int32), src=src, is_rc=is_rc,
                fwd=np.asarray(fwd, np.int32), rev=np.asarray(rev, np.int32))


def golden_path(name, K):
    from pathlib import Path
    return Path(__file__).resolve().parent / "golden" / "hbv" / f"{name}_k{K}.npz"


_gold: dict = {}


def golden(c):
    """The reference's result on a saved case -> namespace(hbv: as graph_from_xlat, edge_lens, a_hbv, a_inv, edges_bv: bytes); the case is
    regenerated from its seed, so the fixture's unitigs are compared with it first."""
    key = (c.name, c.K)
    if key not in _gold:
        z = np.load(golden_path(c.name, c.K))
        assert int(z["K"]) == c.K and np.array_equal(z["unitig_lens"], np.diff(c.off.astype(np.int64))) and np.array_equal(z["unitig_codes2"], pack2(c.bases)), \
            f"{c.name} K={c.K}: the generator no longer makes the unitigs of the fixture"
        _gold[key] = SimpleNamespace(hbv=graph_from_xlat(c, z["fwd"], z["rev"], z["to_left"], z["to_right"], int(z["n_vertices"])), edge_lens=z["edge_lens"],
                                     a_hbv=z["a_hbv"].tobytes(), a_inv=z["a_inv"].tobytes(), edges_bv=z["edges_bv"].tobytes())
    return _gold[key]


def _oracle_unitigs(c):
    import ctypes as C
    import oracle_lib
    return oracle_lib.Unitigs(len(c.unitigs), c.off.ctypes.data_as(C.POINTER(C.c_uint64)), c.bases.ctypes.data_as(C.POINTER(C.c_uint8)))


_orc: dict = {}


def oracle_hbv(c) -> dict:
    """sno_hbv_build on the case (BVComp order), in the layout of graph_from_xlat.  Made once."""
    import ctypes as C
    import oracle_lib
    key = (c.name, c.K)
    if key not in _orc:
        lib = oracle_lib.load()
        h = oracle_lib.Hbv()
        assert lib.sno_hbv_build(C.byref(_oracle_unitigs(c)), c.K, C.byref(h)) == 0
        ne, nu = h.n_edges, len(c.unitigs)
        arr = lambda p, m, dt: (np.ctypeslib.as_array(p, shape=(m,)).astype(dt).copy() if m else np.zeros(0, dt))
        _orc[key] = dict(n_vertices=h.n_vertices, n_edges=ne, v_left=arr(h.v_left, ne, np.int32), v_right=arr(h.v_right, ne, np.int32),
                         src=arr(h.src_unitig, ne, np.int32), is_rc=arr(h.is_rc, ne, np.uint8), fwd=arr(h.fwd_xlat, nu, np.int32), rev=arr(h.rev_xlat, nu, np.int32))
        lib.sno_hbv_free(C.byref(h))
    return _orc[key]


def oracle_bv(c, path) -> bytes:
    """sno_write_bv of the case's unitigs (BVComp order) -> the file's bytes"""
    import ctypes as C
    import oracle_lib
    assert oracle_lib.load().sno_write_bv(str(path).encode(), C.byref(_oracle_unitigs(c))) == 0
    with open(path, "rb") as f:
        return f.read()


def same_graph(a: dict, b: dict):
    """None, or the name of the first thing in which two graphs differ"""
    for k in ("n_vertices", "n_edges"):
        if int(a[k]) != int(b[k]):
            return k
    for k in HBV_KEYS:
        if not np.array_equal(a[k], b[k]):
            return k
    return None


def expected(c) -> dict:
    """the reference's graph where a fixture is kept, else the oracle's (pinned to the reference by tests/test_hbv_handmade_host.py and, for
    the cases that are not kept, by every run of make_hbv_golden.py)"""
    return golden(c).hbv if c.name in SAVED else oracle_hbv(c)
