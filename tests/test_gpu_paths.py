"""Read pathing (f1, snk_dev_path_reads) and duplicate marking (f4, snk_dev_mark_dups) outside the golden cases' envelope: reads of up
to 250 bases inside long homopolymers and short-period repeats, K=60 paths against the oracle, the kernel variants the options select,
the re-runs after a list overflowed, and MarkDups' argument checks.  Bar: bit-exact against the reference's dumps or the C oracle."""
import numpy as np
import pytest

import goldens
import oracle_lib
import pathgen

pytestmark = pytest.mark.gpu
SNK_E_ARG = -1


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


def _golden_dev(c):
    return pathgen.to_device(c.codes, c.quals, c.lens, c.bc)


def _check_paths_and_dups(res, rows, dq, dl, dbc, codes, quals, lens, bc, K, unitigs=None):
    """Paths of every read == oracle_lib.path_reads on the result's unitigs; MarkDups == oracle_lib.mark_dups on those paths.
    -> the oracle's edge counts."""
    L = codes.shape[1]
    off, ne, edges, info = res.path_reads(rows, L, dq, lens=dl, mark_dups=True, bc=dbc)
    o_off, o_n, o_edges = oracle_lib.path_reads(codes, quals, lens, unitigs if unitigs is not None else res.unitigs(), K=K)
    bad = np.nonzero((ne.astype(np.int64) != o_n) | (off != o_off))[0]
    assert len(bad) == 0, (len(bad), bad[:5], ne[bad[:5]], o_n[bad[:5]], off[bad[:5]], o_off[bad[:5]])
    assert np.array_equal(edges, o_edges)
    d = info["dups"]
    o_dup, o_art, o_rate, o_nd, o_ni = oracle_lib.mark_dups(codes, quals, lens, o_off, o_n, o_edges, bc=bc)
    assert np.array_equal(d["dup"], o_dup), np.nonzero(d["dup"] != o_dup)[0][:10]
    assert d["interdup_rate"] == o_rate
    assert (d["n_dup_reads"], d["n_interdup_reads"], d["n_dup_pairs"], d["n_art_pairs"], d["n_placed"]) == \
        (o_nd, o_ni, int(o_dup.sum()), int(o_art.sum()), int((o_n > 0).sum()))
    return o_n, d


def _tandem_genome(rng, G=12000):
    """A 230-base homopolymer and period-2 / period-3 repeats of 230 bases in a random genome."""
    g = rng.integers(0, 4, G, dtype=np.uint8)
    g[2000:2230] = 0
    g[5000:5230] = np.resize(np.array([0, 2], np.uint8), 230)
    g[8000:8230] = np.resize(np.array([0, 1, 3], np.uint8), 230)
    return g, [(2000, 230), (5000, 230), (8000, 230)]


@pytest.mark.parametrize("K", [48, 60])
@pytest.mark.parametrize("L", [150, 250])
@pytest.mark.parametrize("lookup", ["1", "0"])
def test_long_tandem_reads(engine, K, L, lookup, tune):
    """Reads inside a homopolymer (one-k-mer unitig with a self-loop: a part per k-mer) and inside period-2 / period-3 repeats (the path
    alternates between short edges: up to ~190 edges for a 250-base read) need more parts and edges than the first passes keep in LDS;
    the full-capacity pass must path every read of up to 256 bases -- no refusal -- exactly as the oracle does."""
    from supernova_amd.engine import Params
    tune("path_index", lookup)
    rng = np.random.default_rng(K * 1000 + L)
    g, spots = _tandem_genome(rng)
    codes, quals, lens, bc = pathgen.pairs(rng, g, int(len(g) * 40 / L / 2), L, 0.002, 6, spots, spot_frac=0.5)
    codes, quals, lens, bc = pathgen.plant_dups(rng, codes, quals, lens, bc, 0.05, 6)
    rows, dq, dl, dbc = pathgen.to_device(codes, quals, lens, bc, pad_seed=K + L)
    res = engine.count_graph(rows, L, quals=dq, bc=dbc, lens=dl, params=Params(K=K))
    o_n, d = _check_paths_and_dups(res, rows, dq, dl, dbc, codes, quals, lens, bc, K)
    assert int(o_n.max()) > 64 and d["n_dup_pairs"] > 0            # the case is what it is meant to be


@pytest.mark.parametrize("lookup", ["1", "0"])
@pytest.mark.parametrize("name", goldens.K60_CASES)
def test_k60_paths_vs_oracle(engine, name, lookup, tune):
    """K=60 paths (the reference has no K=60 pather): the golden base reads on the reference's K=60 unitigs, every read against the
    oracle's restatement of pathReads, and MarkDups over them."""
    from supernova_amd.engine import Params
    tune("path_index", lookup)
    g = goldens.Case60(name)
    c = g.base
    rows, dq, dl, dbc = _golden_dev(c)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=None, lens=dl, params=Params(K=60))
    assert res.unitigs() == g.exp_unitigs
    o_n, _ = _check_paths_and_dups(res, rows, dq, dl, dbc, c.codes, c.quals, c.lens, c.bc, 60, unitigs=g.exp_unitigs)
    assert int((o_n > 0).sum()) > 0


VARIANTS = {"two_pass_off": {"path_two_pass": 0}, "fast_gs16": {"path_fast_gs": 16}, "slots_x10_11": {"path_slots_x10": 11},
            "dups_two_sorts": {"dups_two_sorts": 1}}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", goldens.CASES)
def test_path_and_dups_variants_match_reference(engine, name, variant, tune):
    """Kernel variants a user or the library can select -- one pass with the full algorithm, sixteen lanes per read in the first pass, the
    dictionary at 1.1 slots per k-mer (long probe chains), the two-sort MarkDups (taken by itself on large graphs) -- against the paths
    and duplicate flags the reference dumped."""
    for k, v in VARIANTS[variant].items():
        tune(k, v)
    tune("path_index", 0)       # (path_slots_x10 sizes the k-mer dictionary)
    c = goldens.load(name)
    rows, dq, dl, dbc = _golden_dev(c)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    off, ne, edges, info = res.path_reads(rows, c.read_len, dq, lens=dl, mark_dups=True, bc=dbc)
    assert np.array_equal(ne.astype(np.int64), c.exp_path_n) and np.array_equal(edges, c.exp_path_edges) and np.array_equal(off, c.exp_path_off)
    assert np.array_equal(info["dups"]["dup"], c.exp_dup) and info["dups"]["interdup_rate"] == c.exp_interdup


RETRIES = {"path_redo_cap": 1, "path_edge_cap": 2, "path_ubc_cap": 4}


@pytest.mark.parametrize("which", sorted(RETRIES) + ["all"])
@pytest.mark.parametrize("data", ["adversarial", "synth_200k"])
def test_path_list_overflow_reruns(engine, data, which, tune):
    """snk_dev_path_reads guesses the capacities of three lists (reads for the full-capacity pass, second and later edges, (unitig, barcode)
    keys) and runs the passes again with a longer list when one overflowed.  With the first capacity near zero every re-run happens -- and
    gives the paths, duplicate flags and barcode lists of the default call."""
    from supernova_amd import synth
    if data == "adversarial":
        c = goldens.load(data)
        rows, dq, dl, dbc = _golden_dev(c)
        L, res = c.read_len, engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    else:
        sp = synth.synth_params(200_000, seed=0x5EED0C0D, sub_ppm=6000)
        rows, dq, dbc = engine.synth(sp)
        dl, L = None, sp.read_len
        res = engine.count_graph(rows, L, quals=dq, bc=dbc)

    def run():
        off, ne, edges, info = res.path_reads(rows, L, dq, lens=dl, mark_dups=True, bc=dbc, unitig_bcs=True)
        return (off, ne, edges, info["dups"]["dup"], info["unitig_bcs"][0], info["unitig_bcs"][1]), info

    base, info0 = run()
    assert info0["retries"] == 0 and len(base[2]) > 0
    names = sorted(RETRIES) if which == "all" else [which]
    for o in names:
        tune(o, 1)
    if "path_redo_cap" in names:
        tune("path_redo_all", 1)        # (every read on the list: it overflows whatever the data)
    got, info = run()
    want = 0
    for o in names:
        want |= RETRIES[o]
    assert info["retries"] == want, (info["retries"], want)
    for a, b in zip(got, base):
        assert np.array_equal(a, b)


def test_mark_dups_argument_checks(engine):
    """MarkDups takes pairs (reads 2q, 2q+1) of at least five bases (the mate head): an odd read count and read_len < 5 are refused."""
    from supernova_amd import lib as _lib
    c = goldens.load("adversarial")
    rows, dq, dl, dbc = _golden_dev(c)
    res = engine.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    n = rows.shape[0] - 1 if rows.shape[0] % 2 == 0 else rows.shape[0]
    with pytest.raises(_lib.SnkError) as ex:
        res.path_reads(rows[:n].contiguous(), c.read_len, dq[:n].contiguous(), lens=dl[:n].contiguous(), mark_dups=True, bc=dbc[:n].contiguous())
    assert ex.value.code == SNK_E_ARG and "odd" in str(ex.value)
    with pytest.raises(_lib.SnkError) as ex:
        res.path_reads(rows, 4, dq, lens=dl, mark_dups=True, bc=dbc)
    assert ex.value.code == SNK_E_ARG and "five" in str(ex.value)
    off, ne, edges, info = res.path_reads(rows, c.read_len, dq, lens=dl, mark_dups=True, bc=dbc)      # the context is fine afterwards
    assert np.array_equal(info["dups"]["dup"], c.exp_dup)


def test_dictionary_load_below_eleven_is_refused(engine):
    """path_slots_x10 < 11 could leave the k-mer dictionary without a free slot: the context refuses it and keeps what it had."""
    from supernova_amd import lib as _lib
    engine.set_option("path_slots_x10", 11)
    for v in (10, 0, -5):
        with pytest.raises(_lib.SnkError) as ex:
            engine.set_option("path_slots_x10", v)
        assert ex.value.code == SNK_E_ARG
        assert engine.get_option("path_slots_x10") == 11
    engine.clear_option("path_slots_x10")
