"""The graph verifier's rules, pinned on the host: the restatement (tests/graphcheck_ref.py) finds nothing in the reference's own outputs,
finds every planted corruption, and the numpy digests (supernova_amd/graphcheck.py) agree with it.  The C declarations of the verifier
(include/snk.h) are checked here too; the device side is tests/test_gpu_graph_check.py."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import goldens
import graphcheck_ref as R
from supernova_amd import graphcheck as G
from supernova_amd import lib

ROOT = Path(__file__).resolve().parent.parent
CASES_K = [(n, 48) for n in goldens.CASES] + [(n, 60) for n in goldens.K60_CASES]


def _case(name, K):
    if K == 48:
        c = goldens.load(name)
        return c, c.exp_keys, c.exp_counts, c.exp_ctx, c.exp_unitigs, c.codes
    c = goldens.Case60(name)
    return c, c.exp_keys, c.exp_counts, c.exp_ctx, c.exp_unitigs, c.base.codes


def _by_first(us, K):
    return sorted(us, key=lambda s: s[:K])


@pytest.mark.parametrize("name,K", CASES_K)
def test_reference_outputs_are_clean(name, K):
    c, keys, counts, ctx, us, codes = _case(name, K)
    r = R.check(keys, counts, ctx, _by_first(us, K), K, 3)
    assert not any(r["counters"].values()), r["counters"]
    assert r["n_kmers"] == len(keys) and r["n_unitigs"] == len(us)
    rr = R.recount(keys, counts, ctx, codes, c.exp_goodlens, K, 3)
    assert not any(rr["counters"].values()), rr["counters"]


def test_adversarial_has_circles_and_palindromes():
    c = goldens.load("adversarial")
    r = R.check(c.exp_keys, c.exp_counts, c.exp_ctx, _by_first(c.exp_unitigs, 48), 48, 3)
    assert r["n_circles"] >= 1 and r["n_palindromes"] >= 1


def plants(keys, counts, ctx, us, K):
    """(name, keys, counts, ctx, unitigs in first-K order, counter the plant must raise)."""
    us = _by_first(us, K)
    out = []
    long_i = max(range(len(us)), key=lambda i: len(us[i]))
    s = us[long_i]
    m = len(s) // 2
    flip = s[:m] + "ACGT"[("ACGT".index(s[m]) + 1) & 3] + s[m + 1:]
    out.append(("flip_interior_base", keys, counts, ctx, us[:long_i] + [flip] + us[long_i + 1:], "unitig_kmer_missing"))
    out.append(("drop_unitig", keys, counts, ctx, us[:long_i] + us[long_i + 1:], "kmer_uncovered"))
    out.append(("duplicate_unitig", keys, counts, ctx, us[:long_i + 1] + [s] + us[long_i + 1:], "kmer_repeated"))
    cut = K + (len(s) - K) // 2
    split = _by_first(us[:long_i] + [s[:cut], s[cut - K + 1:]] + us[long_i + 1:], K)
    out.append(("split_unitig", keys, counts, ctx, split, "end_extendable"))
    out.append(("reverse_complement", keys, counts, ctx, us[:long_i] + [R.rc(s)] + us[long_i + 1:], "not_canonical"))
    i = int(np.flatnonzero(ctx)[0])
    b = int(ctx[i]) & -int(ctx[i])
    c2 = ctx.copy()
    c2[i] ^= b
    out.append(("clear_ctx_bit", keys, counts, c2, us, "ctx_not_reciprocal"))
    n2 = counts.copy()
    n2[len(n2) // 2] = 2
    out.append(("count_below_min_freq", keys, n2, ctx, us, "count_below_min_freq"))
    if len(us) > 1:
        out.append(("swap_unitigs", keys, counts, ctx, [us[1], us[0]] + us[2:], "not_ordered"))
    t = R.Table(keys, counts, ctx, K)
    for j, u in enumerate(us):
        if len(u) > K + 1 and u[len(u) - K + 1:] == u[:K - 1]:
            lk = t.lookup(u[-K:], 0)
            if lk[0] is not None and t.down_possible(u[-K:], lk[1], 0):
                rot = u[1:] + u[K - 1]      # start one k-mer later: the same circle, not at its canonical start
                out.append(("rotate_circle", keys, counts, ctx, us[:j] + [rot] + us[j + 1:], "not_canonical"))
                break
    return out


def test_grouped_plant_is_a_group_mismatch():
    """Per-group runs: a unitig given another group than its k-mers carry is a group mismatch, and its k-mers' entries go uncovered."""
    c = goldens.load("adversarial")
    us = _by_first(c.exp_unitigs, 48)
    keys = np.concatenate([c.exp_keys, np.full((len(c.exp_keys), 1), 5, np.uint32)], axis=1)    # every row in group 5
    groups = np.full(len(keys), 5, np.uint32)
    ug = np.full(len(us), 5, np.uint32)
    clean = R.check(keys, c.exp_counts, c.exp_ctx, us, 48, 3, unitig_groups=ug, key_groups=groups)
    assert not any(clean["counters"].values()), clean["counters"]
    j = max(range(len(us)), key=lambda i: len(us[i]))
    ug2 = ug.copy()
    ug2[j] = 9
    got = R.check(keys, c.exp_counts, c.exp_ctx, us, 48, 3, unitig_groups=ug2, key_groups=groups, ordered=False)["counters"]
    assert got["group_mismatch"] == len(us[j]) - 47 and got["unitig_kmer_missing"] == 0 and got["kmer_uncovered"] == len(us[j]) - 47


def test_key_padding_is_found():
    c = goldens.load("synth_2k_err")
    keys = np.concatenate([c.exp_keys, np.zeros((len(c.exp_keys), 1), np.uint32)], axis=1)
    keys[3, 3] = 1
    got = R.check(keys, c.exp_counts, c.exp_ctx, _by_first(c.exp_unitigs, 48), 48, 3)["counters"]
    assert got["key_padding"] == 1


@pytest.mark.parametrize("name", ["synth_20k_err", "adversarial"])
def test_plants_are_found(name):
    c = goldens.load(name)
    found = set()
    for plant, keys, counts, ctx, us, counter in plants(c.exp_keys, c.exp_counts, c.exp_ctx, c.exp_unitigs, 48):
        r = R.check(keys, counts, ctx, us, 48, 3)
        assert r["counters"][counter] > 0, (plant, r["counters"])
        found.add(plant)
    if name == "adversarial":
        assert "rotate_circle" in found


def test_digests_match_restatement_and_are_order_free_and_additive():
    c = goldens.load("adversarial")
    keys, counts, ctx, us = c.exp_keys, c.exp_counts, c.exp_ctx, c.exp_unitigs
    td, ud = R.digests(keys, counts, ctx, us)
    assert G.digest_table(keys, counts, ctx) == td
    assert G.digest_strings(us) == ud
    rng = np.random.default_rng(5)
    p = rng.permutation(len(keys))
    assert G.digest_table(keys[p], counts[p], ctx[p]) == td
    q = [us[i] for i in rng.permutation(len(us))]
    assert G.digest_strings(q) == ud
    h = len(keys) // 3
    M = (1 << 64) - 1
    assert (G.digest_table(keys[:h], counts[:h], ctx[:h]) + G.digest_table(keys[h:], counts[h:], ctx[h:])) & M == td
    assert (G.digest_strings(q[:7]) + G.digest_strings(q[7:])) & M == ud
    # position-sensitive inside a unitig: a rotation changes it
    assert G.digest_strings([us[0][1:] + us[0][0]] + us[1:]) != ud


def test_digest_bv_round_trip(snk, tmp_path):
    from supernova_amd import graphio
    c = goldens.load("synth_4k_dups")
    off, bases = graphio.unitigs_to_arrays(c.exp_unitigs)
    graphio.write_bv(tmp_path / "a.bv", off, bases)
    assert G.digest_bv(str(tmp_path / "a.bv")) == R.digests(c.exp_keys, c.exp_counts, c.exp_ctx, c.exp_unitigs)[1]


def test_header_declares_the_verifier(tmp_path):
    hdr = (ROOT / "include" / "snk.h").read_text()
    assert re.search(r"int snk_dev_check_graph\(", hdr)
    for name in ("snk_check_input", "snk_check_report", "SNK_CHECK_SORTED_TABLE", "SNK_CHECK_ORDERED", "SNK_CHECK_GROUPED", "SNK_CHECK_DIGEST_ONLY"):
        assert name in hdr
    documented = int(re.search(r"sizeof\(snk_check_report\) = (\d+)", hdr).group(1))
    assert C.sizeof(lib.SnkCheckReport) == documented
    src = tmp_path / "sz.c"
    src.write_text(f'#include "{ROOT / "include" / "snk.h"}"\n#include <stdio.h>\n'
                   'int main(void) { printf("%zu %zu %d\\n", sizeof(snk_check_report), sizeof(snk_check_input), SNK_CHECK_KEY_PADDING); return 0; }\n')
    subprocess.run(["cc", str(src), "-o", str(tmp_path / "sz")], check=True)
    got = subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()
    assert int(got[0]) == documented and int(got[1]) == C.sizeof(lib.SnkCheckInput)
    assert int(got[2]) == len(lib.CHECK_COUNTERS) - 1 and lib.CHECK_COUNTERS == R.COUNTERS


def test_verifier_source_is_independent():
    src = (ROOT / "supernova_amd" / "csrc" / "snk_check.hip").read_text()
    includes = re.findall(r'#include\s+"([^"]+)"', src)
    for banned in ("snk_count", "snk_graph", "snk_local", "snk_kernels", "snk_stages"):
        assert not any(banned in i for i in includes), includes
    assert set(includes) <= {"snk_call.h", "snk_common.h"}
    # the call frame it runs in brings nothing but the context with it
    frame = (ROOT / "supernova_amd" / "csrc" / "snk_call.h").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', frame) == ["snk_ctx.h"]
