"""Read pathing (snk_dev_path_reads) and duplicate marking on the device, on reads walked over hand-made unitig sets (tests/handreads.py):
circles of one to a thousand k-mers, five thousand circles and nothing else, strands that turn round into their own reverse complement,
palindromes on junctions, a vertex with all eight ends, a forest of one- to six-k-mer unitigs -- in three variants each: clean, noisy, and
the pather's own ("paths": random qualities, and a layer of reads with a substituted first / last / inner base, two substitutions near
each other or more than K apart, and chimeras).

Bar: bit-exact.  K=48 against what the REFERENCE's pathReads and MarkDups made of the same reads (tests/golden/handreads/paths/); K=60,
where the reference has no pather, against the C oracle, which tests/test_handreads_paths_host.py holds to those fixtures.  The reads go
up with garbage qualities behind every read's end and behind the row.  info['lookup'], info['n_slow'] and info['retries'] confirm that
a leg was taken; the stages behind the pather are checked on these paths with the restatements of tests/tools/fuzz_paths.py."""
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

import handreads as hr
import oracle_lib
import pathgen

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))

pytestmark = pytest.mark.gpu

ALL = [(n, v) for n in hr.CASES for v in hr.VARIANTS]
IDS = [f"{n}-{hr.vname(v)}" for n, v in ALL]
THREE = ("mixed_seed1", "tiny_circles", "turns")
LOOKUP = {0: "kmer_dictionary", 1: "index"}


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


_dev: dict = {}


def _device(r):
    """the reads on the device (once per read set): garbage qualities behind every read's end, and behind the row (pathgen.to_device)"""
    key = (r.name, r.K, r.noise)
    if key not in _dev:
        seed = zlib.crc32(f"{r.name}/{r.K}/{r.noise}".encode())
        q = np.random.default_rng(seed).integers(0, 42, r.quals.shape, dtype=np.uint8)
        inside = np.arange(r.read_len)[None, :] < r.lens[:, None]
        q[inside] = r.quals[inside]
        _dev[key] = pathgen.to_device(r.codes, q, r.lens, r.bc, pad_seed=seed)
    return _dev[key]


def _count(engine, r, K):
    """(K=60: without barcodes, as the reference's K=60 build has no barcode rule)"""
    from supernova_amd.engine import Params
    rows, dq, dl, dbc = _device(r)
    return engine.count_graph(rows, r.read_len, quals=dq, bc=dbc if K == 48 else None, lens=dl, params=Params(K=K))


def _path(res, r, **more):
    """path_reads, with MarkDups where the reads come in pairs -> (the result in the fixtures' layout, info)"""
    rows, dq, dl, dbc = _device(r)
    n = len(r.lens)
    off, ne, edges, info = res.path_reads(rows, r.read_len, dq, lens=dl, mark_dups=n % 2 == 0, bc=dbc, **more)
    assert off.dtype == np.int32 and edges.dtype == np.int32 and info["n_edges_total"] == len(edges) == int(ne.sum())
    got = dict(path_off=off, path_n=ne.astype(np.int32), path_edges=edges)
    if n % 2 == 0:
        d = info["dups"]
        got.update(dup=d["dup"], interdup=d["interdup_rate"], n_art=d["n_art_pairs"])
        assert d["n_placed"] == int((ne > 0).sum()) and d["n_dup_pairs"] == int(d["dup"].sum())
    return got, info


def _legs(r, got, info, lookup=None):
    """evidence that the legs ran: the look-up asked for; the fast pass left reads of the paths variant to the slow pass; the list of
    second and later edges starts with room for n / 4 + 65536 entries and is regrown (retries & 2) exactly where the paths hold more --
    circles_5000's paths variant, whose reads run round their circles; no other list is regrown"""
    print(f"{r.name} K={r.K} {hr.vname(r.noise)}: lookup {info['lookup']} n_slow {info['n_slow']} retries {info['retries']} "
          f"most edges {int(got['path_n'].max()) if len(got['path_n']) else 0} placed {int((got['path_n'] > 0).sum())} of {len(got['path_n'])}")
    if lookup is not None:
        assert info["lookup"] == LOOKUP[lookup]
    if r.noise == "paths":
        assert info["n_slow"] > 0
    n = len(got["path_n"])
    later = len(got["path_edges"]) - int((got["path_n"] > 0).sum())
    assert info["retries"] == (2 if later > n // 4 + 65536 else 0), (info["retries"], later, n)


@pytest.mark.parametrize("lookup", [0, 1], ids=["dictionary", "index"])
@pytest.mark.parametrize("name,noise", ALL, ids=IDS)
def test_k48_paths_and_dups_equal_the_reference(engine, tune, name, noise, lookup):
    tune("path_index", lookup)
    r, exp = hr.load_paths(name, noise)
    got, info = _path(_count(engine, r, 48), r)
    assert exp.has_dups == ("dup" in got)
    _legs(r, got, info, lookup)
    assert hr.paths_differ(exp, got) is None, hr.paths_differ(exp, got)
    if name == "tiny_circles":
        assert int(got["path_n"].max()) > 16          # more edges than the first passes keep: only the full-capacity pass writes such a path


@pytest.mark.parametrize("name,noise", ALL, ids=IDS)
def test_k60_paths_and_dups_equal_the_oracle(engine, name, noise):
    """The graph is the K=60 handreads fixture's (all three variants: the layer adds no k-mer that is kept)."""
    r = hr.reads(name, 60, noise)
    res = _count(engine, r, 60)
    us = res.unitigs()
    g = hr.golden(name, 60)
    text = np.frombuffer("\n".join(us).encode(), np.uint8)
    assert (hr.sha(text) == g.clean["unitigs"]) if g.hashed else np.array_equal(text, g.clean["unitigs"])
    got, info = _path(res, r)
    _legs(r, got, info)
    off, n, edges = oracle_lib.path_reads(r.codes, r.quals, r.lens, us, K=60)
    for f, want in (("path_off", off), ("path_n", n), ("path_edges", edges)):
        assert np.array_equal(got[f], want), (f, np.nonzero(got["path_n"] != n)[0][:5], np.nonzero(got["path_off"] != off)[0][:5])
    if "dup" in got:
        dup, art, rate, _, _ = oracle_lib.mark_dups(r.codes, r.quals, r.lens, off, n, edges, bc=r.bc)
        assert np.array_equal(got["dup"], dup) and got["interdup"] == rate and got["n_art"] == int(art.sum())


@pytest.mark.parametrize("name", THREE)
def test_paths_do_not_depend_on_the_reads_that_built_the_graph(engine, name):
    """Count the CLEAN reads, path the paths variant's reads on that result: the graph is the same by construction, so the paths are the fixture's."""
    r, exp = hr.load_paths(name, "paths")
    got, info = _path(_count(engine, hr.reads(name, 48, False), 48), r)
    _legs(r, got, info)
    assert hr.paths_differ(exp, got) is None, hr.paths_differ(exp, got)


VARIANTS = {"two_pass_off": {"path_two_pass": 0}, "fast_gs16": {"path_fast_gs": 16}, "slots_x10_11": {"path_slots_x10": 11, "path_index": 0}}
RETRIES = {"path_redo_cap": 1, "path_edge_cap": 2, "path_ubc_cap": 4}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", THREE)
def test_paths_variant_under_the_kernel_variants(engine, tune, name, variant):
    """one pass with the full algorithm, sixteen lanes per read in the first pass, the dictionary at 1.1 slots per k-mer (it sizes the k-mer dictionary)"""
    for o, v in VARIANTS[variant].items():
        tune(o, v)
    r, exp = hr.load_paths(name, "paths")
    got, info = _path(_count(engine, r, 48), r)
    print(f"{name} {variant}: n_slow {info['n_slow']} retries {info['retries']}")
    assert hr.paths_differ(exp, got) is None, hr.paths_differ(exp, got)
    assert info["retries"] == 0 and (info["n_slow"] > 0) == (variant != "two_pass_off")


@pytest.mark.parametrize("name", THREE)
def test_paths_variant_with_the_list_capacities_forced_to_one(engine, tune, name):
    """The three lists of snk_dev_path_reads (reads for the full-capacity pass, second and later edges, (unitig, barcode) keys) start with
    room for one entry: every re-run happens and the paths, duplicate flags and barcode lists are those of the default call.  Before
    that, with the redo list alone at one entry and no read forced onto it: tiny_circles, which has reads of more than 16 edges, overflows
    it by itself -- its long reads have gone through the full-capacity pass."""
    r, exp = hr.load_paths(name, "paths")
    res = _count(engine, r, 48)
    base, info0 = _path(res, r, unitig_bcs=True)
    assert info0["retries"] == 0 and hr.paths_differ(exp, base) is None
    tune("path_redo_cap", 1)
    got, info = _path(res, r)
    print(f"{name}: retries with path_redo_cap=1 alone {info['retries']}")
    assert hr.paths_differ(exp, got) is None and info["retries"] in (0, 1)
    if name == "tiny_circles":
        assert info["retries"] == 1
    for o in RETRIES:
        tune(o, 1)
    tune("path_redo_all", 1)          # (every read on the list: it overflows whatever the data)
    got, info = _path(res, r, unitig_bcs=True)
    assert info["retries"] == 7, info["retries"]
    assert hr.paths_differ(exp, got) is None, hr.paths_differ(exp, got)
    for a, b in zip(info["unitig_bcs"], info0["unitig_bcs"]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("K", hr.KS)
@pytest.mark.parametrize("name", THREE)
def test_stages_behind_the_pather_on_these_paths(engine, name, K):
    """the paths index (a48ref.paths_index), the compressed paths and their unzip (a48xref.zip_paths), the edge -> barcode lists on every
    sort path (ebcxref.edge_barcodes), as tests/tools/fuzz_paths.py checks them on its random genomes"""
    import fuzz_paths
    r = hr.reads(name, K, "paths")
    res = _count(engine, r, K)
    rows, dq, dl, dbc = _device(r)
    off, ne, edges, info = res.path_reads(rows, r.read_len, dq, lens=dl, bc=dbc, paths_index=True, pathsx=True, ebcx=True)
    assert info["pidx"]["n_entries"] == len(edges) > 0
    bad = fuzz_paths.later_stages(dict(K=K, use_bc=K == 48), res.unitigs(), off, ne, edges, r.bc, info, engine=engine)
    assert not bad, bad
