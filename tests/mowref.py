"""A plain numpy restatement of the reference's MowLawn -- lib/assembly/src/10X/Lawnmower.cc:301-554, the ReadPathVecX overload that
StageTrim calls -- and the fixtures under tests/golden/mow/ (what the reference's own function gave, see
tests/golden/make_mow_golden.py, which asserts that both forms below reproduce it before it saves a case).

Two forms.
  mow_literal   follows the source line by line: the paths index with multiplicity (a read whose path holds e k times is visited k
                times), the per-read filter, both loops of both passes, Sort(oq), the grouping, z1 / z2.
  mow_entries   what the device does: one visit per path entry and role, the window test first, the filter only for an entry whose read
                reaches the window, then the records by (candidate, fw, offset).  It also gives the counters of snk_dev_mow.
Both read the offsets as a ReadPathVecX holds them (static_cast<int16_t>).  They must agree on every fixture (tests/test_mow_host.py).

A candidate is (v, e1, e2): To(v) = {e1, e2}, From(v) has one edge, Kmers(e2) <= Kmers(e1), and ToLeft(e2) has no in-edge and one
out-edge.  n = Kmers(e2), del = Kmers(e1) - n, x1 = e1[del : del + n], x2 = e2[0 : n].
"""
from __future__ import annotations

from pathlib import Path
from types import SimpleNamespace

import numpy as np

import a48xref
import badsref

MOW = Path(__file__).resolve().parent / "golden" / "mow"
MAX_READS2, MAX_QS, MIN_QS_RIGHT, MAX_QS_WRONG, MAX_HQ_DIFFS, MIN_HQ = 2, 50, 300, 30, 5, 30      # Lawnmower.cc:309-314
COUNTERS = ("n_candidates", "n_too_many_reads", "n_entries_on_candidates", "n_entries_in_window", "n_reads_hq_excluded", "n_records", "n_groups",
            "n_groups_mixed_sign", "n_deleted_candidates")


def candidates(g: a48xref.Graph, kmers):
    """-> [(v, e1, e2)] in the order the reference meets them (:407-416)"""
    out = []
    to_n, from_n = np.diff(g.to_off), np.diff(g.from_off)
    for v in range(g.N):
        if to_n[v] != 2:
            continue
        for jj in range(2):
            e1, e2 = int(g.to_e[g.to_off[v] + jj]), int(g.to_e[g.to_off[v] + 1 - jj])
            if kmers[e2] > kmers[e1]:
                continue
            w = g.v_left[e2]
            if to_n[w] > 0 or from_n[w] > 1 or from_n[v] != 1:
                continue
            out.append((v, e1, e2))
    return out


def _hq_diffs(m, read, qual, offset):
    pos = offset + np.arange(len(read), dtype=np.int64)
    ok = (pos >= 0) & (pos < len(m)) & (qual >= MIN_HQ)
    return int((read[ok] != m[pos[ok]]).sum())


def _q1q2(read, qual, first, x1, x2):
    """read base m lies at epos = first + m; over 0 <= epos < n"""
    epos = first + np.arange(len(read), dtype=np.int64)
    ok = (epos >= 0) & (epos < len(x1))
    r, q, p = read[ok], qual[ok].astype(np.int64), epos[ok]
    return int(q[r != x1[p]].sum()), int(q[r != x2[p]].sum())


def _decide(oq):
    """Sort(oq) and :516-531 -> (qss1, qss2, groups, mixed groups)"""
    oq = sorted(oq)
    z1, z2, i, groups, mixed = [], [], 0, 0, 0
    while i < len(oq):
        j = i + 1
        while j < len(oq) and oq[j][:2] == oq[i][:2]:
            j += 1
        groups += 1
        if oq[i][2] / oq[j - 1][2] > 0:
            if oq[i][2] > 0:
                z2.append(min(oq[j - 1][2], MAX_QS))
            else:
                z1.append(min(-oq[i][2], MAX_QS))
        else:
            mixed += 1
        i = j
    z1.sort(), z2.sort()
    return sum(z1[:-1]), sum(z2[:-1]), groups, mixed


class _Input:
    def __init__(self, g, eb, inv, codes, lens, quals, offset, n_edges, edges, dup):
        self.g, self.eb, self.K, self.inv = g, eb, g.K, np.asarray(inv, np.int64)
        self.kmers = np.array([len(b) - g.K + 1 for b in eb], np.int64)
        self.ne = np.asarray(n_edges, np.int64)
        self.n = len(self.ne)
        assert self.n % 2 == 0 and len(codes) == self.n and len(dup) == self.n // 2
        self.start = np.concatenate([[0], np.cumsum(self.ne)])
        self.edges = np.asarray(edges, np.int64)
        self.off = a48xref.wrap16(np.asarray(offset, np.int64)).astype(np.int64)
        self.codes, self.quals, self.lens, self.dup = codes, quals, lens, np.asarray(dup, bool)
        self._cats, self._hq = {}, {}

    def path(self, r):
        return self.edges[self.start[r]:self.start[r + 1]]

    def read(self, r):
        L = int(self.lens[r])
        return np.asarray(self.codes[r][:L], np.uint8), np.asarray(self.quals[r][:L], np.uint8)

    def excluded(self, r):
        """>= 5 mismatches of quality >= 30 against hb.Cat(path) at the path's offset (:452-462)"""
        if r not in self._hq:
            p = self.path(r)
            key = p.tobytes()
            if key not in self._cats:
                self._cats[key] = badsref.cat(self.eb, self.K, p)
            b, q = self.read(r)
            self._hq[r] = _hq_diffs(self._cats[key], b, q, int(self.off[r])) >= MAX_HQ_DIFFS
        return self._hq[r]


def _result(scored, inv):
    scored = sorted(scored, key=lambda s: (s[1], s[0]))
    dels = sorted({x for e1, e2, a, b in scored if a >= MIN_QS_RIGHT and b <= MAX_QS_WRONG for x in (e2, int(inv[e2]))})
    return np.asarray(dels, np.int32), np.asarray(scored, np.int32).reshape(-1, 4)


def mow_literal(g, eb, inv, codes, lens, quals, offset, n_edges, edges, dup):
    """-> (dels i32[] ascending, scored i32[n, 4] = (e1, e2, qss1, qss2) ascending by (e2, e1))"""
    I = _Input(g, eb, inv, codes, lens, quals, offset, n_edges, edges, dup)
    index = [[] for _ in range(g.E)]                     # the paths index: one id per entry
    for r in range(I.n):
        for e in I.path(r):
            index[int(e)].append(r)
    scored = []
    for v, e1, e2 in candidates(g, I.kmers):
        re2 = int(I.inv[e2])
        npe = sum(1 for r in index[e2] if not I.dup[r // 2]) + sum(1 for r in index[re2] if not I.dup[r // 2])
        if npe > MAX_READS2:
            continue
        n = int(I.kmers[e2])
        dl = int(I.kmers[e1]) - n
        x1, x2 = eb[e1][dl:dl + n], eb[e2][:n]
        oq = []
        for pas in (1, 2):
            e = e1 if pas == 1 else e2
            re = int(I.inv[e])
            for r in index[e]:
                if I.dup[r // 2] or I.excluded(r):
                    continue
                p, (b, q) = I.path(r), I.read(r)
                offset_l = int(I.off[r])
                for l in range(len(p) - 1):
                    if p[l] == e:
                        q1, q2 = _q1q2(b, q, offset_l - (dl if pas == 1 else 0), x1, x2)
                        if q1 != q2:
                            oq.append((True, offset_l, q1 - q2))
                    offset_l -= int(I.kmers[p[l]])
            for r in index[re]:
                if I.dup[r // 2] or I.excluded(r):
                    continue
                p, (b, q) = I.path(r), I.read(r)
                b, q = (3 - b)[::-1], q[::-1]
                offset_l = int(I.off[r]) - int(I.kmers[p[0]])
                for l in range(1, len(p)):
                    if p[l] == re:
                        first = len(eb[e]) - offset_l - len(b)
                        q1, q2 = _q1q2(b, q, first - (dl if pas == 1 else 0), x1, x2)
                        if q1 != q2:
                            oq.append((False, offset_l, q1 - q2))
                    offset_l -= int(I.kmers[p[l]])
        qss1, qss2, _, _ = _decide(oq)
        scored.append((e1, e2, qss1, qss2))
    return _result(scored, I.inv)


def mow_entries(g, eb, inv, codes, lens, quals, offset, n_edges, edges, dup, detail: dict | None = None):
    """-> (dels, scored, {counter: value}); detail receives per candidate (e1, e2) its npe and, if it passed, its records and excluded reads"""
    I = _Input(g, eb, inv, codes, lens, quals, offset, n_edges, edges, dup)
    K = I.K
    cands = sorted(candidates(g, I.kmers), key=lambda c: c[2])
    cnt = dict.fromkeys(COUNTERS, 0)
    cnt["n_candidates"] = len(cands)
    role = {}                                            # edge -> [(candidate, pass, fw)]
    npe = np.zeros(len(cands), np.int64)
    as_e2 = {}
    for c, (v, e1, e2) in enumerate(cands):
        for e, pas, fw in ((e1, 1, True), (e2, 2, True), (int(I.inv[e1]), 1, False), (int(I.inv[e2]), 2, False)):
            role.setdefault(e, []).append((c, pas, fw))
            if pas == 2:
                as_e2.setdefault(e, []).append(c)
    for r in range(I.n):
        if I.dup[r // 2]:
            continue
        for e in I.path(r):
            for c in as_e2.get(int(e), ()):
                npe[c] += 1
    cnt["n_too_many_reads"] = int((npe > MAX_READS2).sum())
    recs = [[] for _ in cands]
    excl = [set() for _ in cands]
    for r in range(I.n):
        if I.dup[r // 2] or not I.ne[r]:
            continue
        p = I.path(r)
        if not any(int(e) in role for e in p):
            continue
        b, q = I.read(r)
        L = len(b)
        offset_l = int(I.off[r])
        for l, e in enumerate(p):
            for c, pas, fw in role.get(int(e), ()):
                if npe[c] > MAX_READS2 or (l + 1 >= len(p) if fw else l == 0):
                    continue
                cnt["n_entries_on_candidates"] += 1
                _, e1, e2 = cands[c]
                n = int(I.kmers[e2])
                dl = int(I.kmers[e1]) - n
                first = offset_l - (dl if pas == 1 else 0) if fw else n + K - 1 - offset_l - L
                if L <= 0 or first >= n or first + L <= 0:
                    continue
                cnt["n_entries_in_window"] += 1
                if I.excluded(r):
                    cnt["n_reads_hq_excluded"] += 1
                    excl[c].add(r)
                    continue
                bb, qq = (b, q) if fw else ((3 - b)[::-1], q[::-1])
                q1, q2 = _q1q2(bb, qq, first, eb[e1][dl:dl + n], eb[e2][:n])
                if q1 != q2:
                    cnt["n_records"] += 1
                    recs[c].append((fw, offset_l, q1 - q2))
            offset_l -= int(I.kmers[int(e)])
    scored = []
    for c, (v, e1, e2) in enumerate(cands):
        if detail is not None:
            detail[(e1, e2)] = SimpleNamespace(npe=int(npe[c]), records=sorted(recs[c]), excluded=sorted(excl[c]), qss=None, groups=0, mixed=0)
        if npe[c] > MAX_READS2:
            continue
        qss1, qss2, groups, mixed = _decide(recs[c])
        cnt["n_groups"] += groups
        cnt["n_groups_mixed_sign"] += mixed
        cnt["n_deleted_candidates"] += qss1 >= MIN_QS_RIGHT and qss2 <= MAX_QS_WRONG
        scored.append((e1, e2, qss1, qss2))
        if detail is not None:
            d = detail[(e1, e2)]
            d.qss, d.groups, d.mixed = (qss1, qss2), groups, mixed
    dels, scored = _result(scored, I.inv)
    return dels, scored, {k: int(v) for k, v in cnt.items()}


# ---- the fixtures

_cases: dict = {}
_restated: dict = {}


def names() -> list[str]:
    return sorted(p.stem for p in MOW.glob("*.npz"))


def digest(c) -> str:
    """what identifies a fixture's input: reads, barcodes, paths, graph and inv (dup is the reference's answer, kept in the fixture)"""
    import hashlib
    h = hashlib.sha256(badsref.digest(c).encode())
    h.update(np.ascontiguousarray(c.bc, np.int32).tobytes())
    h.update(np.ascontiguousarray(c.inv, np.int32).tobytes())
    return h.hexdigest()


def load(name: str):
    """-> namespace(name, K, g, eb, inv, a_hbv, unitigs = (off, bases) in the order the graph names them, codes, quals, lens, bc, paths =
    (offset, n_edges, edges), dup, dels, scored, ref_summary).  Loaded once per process and left unchanged."""
    if name in _cases:
        return _cases[name]
    import mowgen
    z = np.load(MOW / f"{name}.npz")
    c = mowgen.inputs(name, bytes(z["a_hbv"]) if "a_hbv" in z.files else None)
    c.name, c.dup, c.dels, c.scored = name, z["dup"].copy(), z["dels"].astype(np.int32), z["scored"].astype(np.int32).reshape(-1, 4)
    c.ref_summary = bytes(z["ref_summary"]).decode()
    assert bytes(z["input_digest"]).decode() == digest(c), f"{name}: the fixture was made from another input"
    _cases[name] = c
    return c


def restated(name: str):
    if name not in _restated:
        c = load(name)
        _restated[name] = mow_entries(c.g, c.eb, c.inv, c.codes, c.lens, c.quals, *c.paths, c.dup)
    return _restated[name]
