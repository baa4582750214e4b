"""CloseGap2 / CloseGap on the device (snk_dev_close_gaps: 10X/Closomatic.cc:356-657).  Bar: closures and pair_first equal what the
reference's own functions wrote (tests/golden/closures/), the counters equal those of the Python restatement that test_closures_host.py
pins to the same closures, with the paths index given and made inside, for both flags, and wherever CloseGap2's partners are placed."""
import ctypes as C

import numpy as np
import pytest

import closeref
import pathgen

pytestmark = pytest.mark.gpu
SNK_E_ARG = -1
BOD_BUDGET = closeref.BOD_BUDGET         # the default, and the most


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.array(a, dtype=dtype))).to(torch.device("cuda", 0))


class _Case:
    """a fixture's unitigs, reads, paths and pairs on the device"""

    def __init__(self, c, paths=None, pairs=None):
        from supernova_amd import graphio
        self.c = c
        self.u = graphio.unitigs_to_arrays(c.unitigs)
        self.d_off, self.d_bases = _dev(self.u[0].astype(np.int64), np.int64), _dev(self.u[1], np.uint8)
        off, ne, edges = c.paths if paths is None else paths
        self.n, self.n_entries = len(ne), len(edges)
        self.paths = (_dev(off, np.int32), _dev(np.asarray(ne, np.uint32).view(np.int32), np.int32), _dev(edges if len(edges) else np.zeros(1, np.int32), np.int32)[:len(edges)])
        self.start = _dev(np.concatenate([[0], np.cumsum(np.asarray(ne, np.int64))]), np.int64)
        codes, quals, lens = closeref.full_reads(c)
        self.read_len = codes.shape[1]
        self.rows, self.quals, self.lens, _ = pathgen.to_device(codes[:max(self.n, 1)], quals[:max(self.n, 1)], lens[:max(self.n, 1)], np.zeros(max(self.n, 1), np.int32))
        pairs = c.pairs if pairs is None else pairs
        self.n_pairs = len(pairs)
        self.pairs = _dev(pairs if len(pairs) else np.zeros((1, 2), np.int32), np.int32)
        self.inv = np.ascontiguousarray(c.inv, dtype=np.int32)

    def tensors(self):
        return (*self.paths, self.rows, self.quals, self.lens, self.pairs, self.d_bases)


_cases: dict = {}


def _case(name) -> _Case:
    if name not in _cases:
        _cases[name] = _Case(closeref.load(name))
    return _cases[name]


def _paths_struct(D, n_reads=None, n_total=None):
    from supernova_amd import lib as _lib
    p = _lib.SnkDevPaths()
    p.n_reads, p.n_edges_total = (D.n if n_reads is None else n_reads), (D.n_entries if n_total is None else n_total)
    p.offset, p.n_edges, p.edges, p.start = D.paths[0].data_ptr(), D.paths[1].data_ptr(), D.paths[2].data_ptr(), D.start.data_ptr()
    return p


def _raw(engine, D, h, flags=0, budget=0, px=None, inv=None, n_total=None, reads=True, max_width=0):
    """the C call itself -> (rc, message, SnkDevClosures, (closure_off, bases, pair_first) or None)"""
    from supernova_amd import lib as _lib
    from supernova_amd.engine import dev_reads
    import devcall
    p = _paths_struct(D, n_total=n_total)
    r = dev_reads(D.rows[:D.n], D.read_len, D.quals[:D.n], D.lens[:D.n])
    out = _lib.SnkDevClosures()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    err = C.create_string_buffer(512)
    inv = D.inv if inv is None else inv
    rc = engine.lib.snk_dev_close_gaps(engine._ctx, D.c.K, len(D.u[0]) - 1, D.d_off.data_ptr(), D.d_bases.data_ptr(), C.byref(h), inv.ctypes.data, C.byref(r) if reads else None,
                                       C.byref(p), C.byref(px) if px is not None else None, D.n_pairs, D.pairs.data_ptr(), max_width, flags, budget, C.byref(out),
                                       engine._stream(), err, 512)
    got = None
    if rc == 0:
        got = (devcall.download(engine, out.closure_off, int(out.n_closures) + 1, np.uint64), devcall.download(engine, out.bases, int(out.n_bases), np.uint8),
               devcall.download(engine, out.pair_first, int(out.n_pairs) + 1, np.uint64))
    return rc, err.value.decode(errors="replace"), out, got


def _index(engine, D):
    return engine._pidx(_paths_struct(D), D.c.g.E, D.inv)


def _counts(out):
    return {k: int(getattr(out, k)) for k in closeref.COUNTERS}


def _want(c, flag):
    return getattr(c, f"closure_off_{flag}"), getattr(c, f"bases_{flag}"), getattr(c, f"pair_first_{flag}")


# the pairs that go to the host routine at the default budget: the hand-made follower edge with more 32-mers than it, and nothing else
_HOST_AT_DEFAULT = {("hand_k48", "cg2"): 1}


def _equal(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("name", closeref.ALL)
def test_closures_match_the_reference(engine, name, tmp_path):
    """Every fixture, both flags: Engine.close_gaps (index made inside) and the C call with the index given return the reference's
    closures and pair_first and the restatement's counters; no placement needed the host at the default budget; a second call gives the
    same bytes; the inputs are untouched; snk_write_bv of the result gives the reference's closures.fastb."""
    from supernova_amd import graphio, lib as _lib
    c, D = closeref.load(name), _case(name)
    with graphio.hbv_handle(c.K, *D.u) as h:
        for flag in closeref.FLAGS:
            want, cnt = _want(c, flag), getattr(c, f"counts_{flag}")
            before = [t.clone() for t in D.tensors()]
            off, bases, first, stats = engine.close_gaps(c.K, h, D.d_off, D.d_bases, D.inv, D.rows[:D.n], D.read_len, D.quals[:D.n], D.lens[:D.n], *D.paths, D.pairs[:D.n_pairs],
                                                         cg1=flag == "cg1")
            assert off.dtype == np.uint64 and bases.dtype == np.uint8 and _equal((off, bases, first), want), (flag, first.tolist(), want[2].tolist())
            assert {k: stats[k] for k in cnt} == cnt, (flag, stats)
            assert stats["n_place_host"] == _HOST_AT_DEFAULT.get((name, flag), 0) and stats["max_width"] == 400 and stats["bod_budget"] == BOD_BUDGET and stats["ms"] > 0
            for a, b in zip(before, D.tensors()):
                assert bool((a == b).all()), "an input changed"
            graphio.write_closures(tmp_path / "closures.fastb", off, bases)
            assert (tmp_path / "closures.fastb").read_bytes() == getattr(c, f"fastb_{flag}")
            px = _index(engine, D)
            flags = _lib.CLOSE_CG1 if flag == "cg1" else 0
            rc, msg, out, got = _raw(engine, D, h, flags, px=px)
            assert rc == 0 and _equal(got, want) and _counts(out) == cnt and out.n_place_host == _HOST_AT_DEFAULT.get((name, flag), 0), msg
            rc, msg, out2, again = _raw(engine, D, h, flags)
            assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(again, got)) and _counts(out2) == cnt, msg


@pytest.mark.parametrize("name", closeref.ALL)
def test_no_result_depends_on_where_the_partners_are_placed(engine, name):
    """SNK_CLOSE_PLACE_HOST: every pair's placement goes through the host routine; bod_budget = 1: every pair with a follower group whose
    edge has a 32-mer does.  Closures and counters are the fixture's every time."""
    from supernova_amd import graphio, lib as _lib
    c, D = closeref.load(name), _case(name)
    want, cnt = _want(c, "cg2"), c.counts_cg2
    with graphio.hbv_handle(c.K, *D.u) as h:
        rc, msg, out, got = _raw(engine, D, h, _lib.CLOSE_PLACE_HOST)
        assert rc == 0 and _equal(got, want) and _counts(out) == cnt, (msg, _counts(out), cnt)
        assert out.n_place_host == len(c.pairs)
        rc, msg, out, got = _raw(engine, D, h, 0, budget=1)
        assert rc == 0 and _equal(got, want) and _counts(out) == cnt and out.bod_budget == 1, (msg, _counts(out), cnt)
        assert out.n_place_host <= len(c.pairs) and (cnt["n_followers"] == 0 or out.n_place_host >= 1), int(out.n_place_host)
        rc, msg, out, got = _raw(engine, D, h, 0, budget=1 << 30)
        assert rc == 0 and _equal(got, want) and out.bod_budget == BOD_BUDGET and out.n_place_host == _HOST_AT_DEFAULT.get((name, "cg2"), 0), msg
        # CloseGap places nobody: the flag and the budget change nothing
        rc, msg, out, got = _raw(engine, D, h, _lib.CLOSE_CG1 | _lib.CLOSE_PLACE_HOST, budget=1)
        assert rc == 0 and _equal(got, _want(c, "cg1")) and _counts(out) == c.counts_cg1 and out.n_place_host == 0, msg


def test_max_width(engine):
    """other widths against the restatement: a window narrower than the reads, and 1200, where a consensus of 1000 columns or more gives
    nothing (synth_4k_dups closes 12 of its 14 pairs at 400)"""
    from supernova_amd import graphio, lib as _lib
    c, D = closeref.load("synth_4k_dups"), _case("synth_4k_dups")
    with graphio.hbv_handle(c.K, *D.u) as h:
        for width in (100, 1200):
            for flag in closeref.FLAGS:
                off, bases, first, cnt, _ = closeref.close_gaps(c.I, c.pairs, flag == "cg2", width)
                rc, msg, out, got = _raw(engine, D, h, _lib.CLOSE_CG1 if flag == "cg1" else 0, max_width=width)
                assert rc == 0 and _equal(got, (off, bases, first)) and _counts(out) == cnt and out.max_width == width, (width, flag, msg, _counts(out), cnt)


@pytest.mark.parametrize("name", closeref.WIDE_CASES)
def test_a_consensus_of_1000_columns_gives_nothing(engine, name):
    """max_width = 1 200 against the reference's own run at that width"""
    from supernova_amd import graphio, lib as _lib
    c, D = closeref.load(name), _case(name)
    with graphio.hbv_handle(c.K, *D.u) as h:
        for flag in closeref.FLAGS:
            rc, msg, out, got = _raw(engine, D, h, _lib.CLOSE_CG1 if flag == "cg1" else 0, max_width=closeref.WIDE)
            cnt = getattr(c, f"counts_{flag}_wide")
            assert rc == 0 and _equal(got, _want(c, flag + "_wide")) and _counts(out) == cnt and out.n_cons_too_long >= 1 and out.max_width == closeref.WIDE, (msg, _counts(out), cnt)


@pytest.mark.parametrize("name", closeref.HAND)
def test_hand_made_items_by_name(engine, name):
    """the stated closures of every hand-made item, by name: CloseGap2 at the default budget (the long follower on the host routine), on
    the host routine throughout and at budget 1, CloseGap, and max_width 1 200"""
    import handclose
    from supernova_amd import graphio
    c, D = closeref.load(name), _case(name)
    hc = handclose.case(c.K)
    with graphio.hbv_handle(c.K, *D.u) as h:
        for which, kw in (("closures", {}), ("closures", dict(place_host=True)), ("closures", dict(bod_budget=1)), ("closures_cg1", dict(cg1=True)),
                          ("closures_wide", dict(max_width=closeref.WIDE))):
            off, bases, first, stats = engine.close_gaps(c.K, h, D.d_off, D.d_bases, D.inv, D.rows[:D.n], D.read_len, D.quals[:D.n], D.lens[:D.n], *D.paths, D.pairs[:D.n_pairs], **kw)
            handclose.assert_items(hc, c.edge_of, c.pairs, off, bases, first, f"the device ({kw})", which)
            if not kw:
                assert stats["n_place_host"] == _HOST_AT_DEFAULT.get((name, "cg2"), 0) and stats["n_partners_placed"] == c.counts_cg2["n_partners_placed"] >= 1, stats


def _all_zero(x) -> bool:
    return bytes(x) == bytes(C.sizeof(x))


def test_refusals(engine):
    """Every refusal returns SNK_E_ARG with *out all zero; the call after it works."""
    from supernova_amd import graphio, lib as _lib
    c, D = closeref.load("synth_4k_dups"), _case("synth_4k_dups")
    off, ne, edges = c.paths
    start = np.concatenate([[0], np.cumsum(np.asarray(ne, np.int64))])
    with graphio.hbv_handle(c.K, *D.u) as h:
        odd = _Case(c, (off[:-1], ne[:-1], edges[:start[-2]]))
        outside = _Case(c, pairs=np.where(np.arange(2 * len(c.pairs)).reshape(-1, 2) == 3, c.g.E, c.pairs).astype(np.int32))
        negative = _Case(c, pairs=np.where(np.arange(2 * len(c.pairs)).reshape(-1, 2) == 0, -1, c.pairs).astype(np.int32))
        edge_outside = _Case(c, (off, ne, np.where(np.arange(len(edges)) == 3, c.g.E, edges).astype(np.int32)))
        not_inv = D.inv.copy()
        not_inv[0] = not_inv[1] if not_inv[1] != not_inv[0] else not_inv[2]
        px = _index(engine, D)
        px_edges, px_entries = _lib.SnkDevPidx.from_buffer_copy(px), _lib.SnkDevPidx.from_buffer_copy(px)
        px_edges.n_hbv_edges += 1
        px_entries.n_entries -= 1
        for what, case, kw in (("odd read count", odd, {}), ("pair id outside", outside, {}), ("negative pair id", negative, {}), ("edge id outside", edge_outside, {}),
                               ("inv", D, dict(inv=not_inv)), ("px edges", D, dict(px=px_edges)), ("px entries", D, dict(px=px_entries)), ("flags", D, dict(flags=4)),
                               ("table", D, dict(n_total=D.n_entries - 1)), ("no reads", D, dict(reads=False))):
            rc, msg, out, _ = _raw(engine, case, h, **kw)
            assert rc == SNK_E_ARG and msg and _all_zero(out), (what, rc, msg)
        rc, msg, out, got = _raw(engine, D, h, px=px)
        assert rc == 0 and _equal(got, _want(c, "cg2")), msg
        # no pairs at all: no reads are needed
        none = _Case(c, pairs=np.zeros((0, 2), np.int32))
        rc, msg, out, got = _raw(engine, none, h, reads=False)
        assert rc == 0 and out.n_closures == 0 and len(got[0]) == 1 and len(got[2]) == 1 and out.n_rows == 0, msg


@pytest.mark.parametrize("name", ("gapped", "synth_4k_dups"))
def test_closures_go_straight_into_insert_patch(engine, name, tmp_path):
    """the chain: what close_gaps returns is what insert_patch takes; the patched a.hbv / a.inv equal what the restatement of
    StageInsertPatch (tests/patchref.py) makes of the reference's closures"""
    import patchref
    from supernova_amd import graphio
    c, D = closeref.load(name), _case(name)
    with graphio.hbv_handle(c.K, *D.u) as h:
        closed = engine.close_gaps(c.K, h, D.d_off, D.d_bases, D.inv, D.rows[:D.n], D.read_len, D.quals[:D.n], D.lens[:D.n], *D.paths, D.pairs[:D.n_pairs])
        out = engine.insert_patch((c.K, h, D.u[0], D.d_bases), closed, D.paths)                # the tuple as it is
        out.write(tmp_path / "a.hbv", tmp_path / "a.inv")
    ro, rb = c.closure_off_cg2, c.bases_cg2
    ref = patchref.insert_patch(c.K, c.a_hbv, [patchref.text(rb[int(ro[i]):int(ro[i + 1])]) for i in range(len(ro) - 1)], c.paths[0], np.asarray(c.paths[1], np.uint32), c.paths[2])
    assert (tmp_path / "a.hbv").read_bytes() == ref.a_hbv and (tmp_path / "a.inv").read_bytes() == ref.a_inv


def test_path_reads_gives_the_closures(engine):
    """count + graph + paths + MarkBads + index + FindEdgePairs + CloseGap2 in one path_reads call on the adversarial case (the device's
    paths ARE the reference's: test_gpu_paths.py): the closures are the fixture's for both flags; without hops the call is refused"""
    import goldens
    c, fx = goldens.load("adversarial"), closeref.load("adversarial")
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    for flag, arg in (("cg2", True), ("cg1", "cg1")):
        _, _, _, info = res.path_reads(rows, c.read_len, dq, lens=dl, bc=dbc, mark_bads="x", hops=True, closures=arg)
        assert np.array_equal(info["hops"], fx.pairs) and _equal(info["closures"], _want(fx, flag))
        assert {k: info["closures_stats"][k] for k in closeref.COUNTERS} == getattr(fx, f"counts_{flag}")
    _, _, _, info2 = res.path_reads(rows, c.read_len, dq, lens=dl, bc=dbc, mark_bads="x", hops=True, closures=True, download=False)
    assert "closures" not in info2 and info2["closures_stats"]["n_closures"] == len(fx.closure_off_cg2) - 1
    with pytest.raises(ValueError):
        res.path_reads(rows, c.read_len, dq, lens=dl, bc=dbc, closures=True)
