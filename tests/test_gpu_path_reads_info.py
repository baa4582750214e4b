"""The info dict of Result.path_reads: with every stage asked for, exactly the documented keys in each download mode, the same counters in
both, the reference's paths, and one involution for the two stages that take it."""
import numpy as np
import pytest

import goldens
import pathgen

pytestmark = pytest.mark.gpu

BASE = {"dict_ms", "path_ms", "bcs_ms", "hbv_device_ms", "dict_slots", "lookup", "n_slow", "retries", "n_edges_total", "n_unitig_bcs"}
DOWNLOADED = BASE | {"dups", "bads", "pidx", "paths_index", "countsb", "inv", "pathsx", "pathsx_stats", "ebcx", "ebcx_stats", "extended",
                     "extend_stats", "extended_pathsx", "extended_pathsx_stats", "unitig_bcs"}
RESIDENT = BASE | {"dups", "bads", "bads_dev", "pidx", "pathsx_stats", "pathsx_dev", "ebcx_stats", "extend_stats", "extended_pathsx_stats"}
STATS = ("dups", "bads", "pidx", "pathsx_stats", "ebcx_stats", "extend_stats", "extended_pathsx_stats")


@pytest.fixture(scope="module")
def runs(snk):
    """The adversarial case at K = 48, pathed with every stage on in both download modes, and once more with the two stages that take the involution."""
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    c = goldens.load("adversarial")
    rows, dq, dl, dbc = pathgen.to_device(c.codes, c.quals, c.lens, c.bc)
    res = e.count_graph(rows, c.read_len, quals=dq, bc=dbc, lens=dl, ign_bc_below=c.ign_bc_below)
    every = dict(mark_dups=True, bc=dbc, unitig_bcs=True, paths_index=True, pathsx=True, ebcx=True, extend=True, mark_bads="x")
    down = res.path_reads(rows, c.read_len, dq, lens=dl, download=True, **every)
    resident = res.path_reads(rows, c.read_len, dq, lens=dl, download=False, **every)
    two = res.path_reads(rows, c.read_len, dq, lens=dl, paths_index=True, ebcx=True, bc=dbc)
    yield c, down, resident, two
    e.close()


def test_info_keys_are_the_documented_ones_in_each_mode(runs):
    _, down, resident, _ = runs
    assert set(down[3]) == DOWNLOADED
    assert set(resident[3]) == RESIDENT and resident[:3] == (None, None, None)
    assert "dup" in down[3]["dups"] and "dup" not in resident[3]["dups"]
    assert "bad" in down[3]["bads"] and "bad" not in resident[3]["bads"]


def test_counters_agree_between_the_modes(runs):
    _, down, resident, _ = runs
    a, b = down[3], resident[3]
    for k in BASE:
        if not k.endswith("ms"):
            assert a[k] == b[k], k
    for s in STATS:
        want = {k: v for k, v in a[s].items() if not k.endswith("ms") and k not in ("dup", "bad")}
        got = {k: v for k, v in b[s].items() if not k.endswith("ms")}
        assert got == want and want, s


def test_paths_are_the_reference_s(runs):
    c, (off, ne, edges, info), _, _ = runs
    assert off.dtype == np.int32 and ne.dtype == np.uint32 and edges.dtype == np.int32
    assert np.array_equal(off, c.exp_path_off) and np.array_equal(ne, c.exp_path_n) and np.array_equal(edges, c.exp_path_edges)
    assert np.array_equal(info["dups"]["dup"], c.exp_dup)
    assert info["n_edges_total"] == len(c.exp_path_edges)


def test_one_involution_serves_both_stages(runs):
    _, down, _, two = runs
    inv = down[3]["inv"]
    assert len(inv) == down[3]["pidx"]["n_hbv_edges"] > 0 and np.array_equal(inv[inv], np.arange(len(inv)))
    assert np.array_equal(two[3]["inv"], inv)
    assert set(two[3]) == BASE | {"pidx", "paths_index", "countsb", "inv", "ebcx", "ebcx_stats"}
    for k in (0, 1):
        assert np.array_equal(two[3]["paths_index"][k], down[3]["paths_index"][k]) and np.array_equal(two[3]["ebcx"][k], down[3]["ebcx"][k])
