"""CPU-side checks of the C-ABI shared library: it builds for gfx950, loads, exports every symbol that
include/snk.h declares, and refuses to run without a GPU (no CPU fallback)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def test_exports_match_header(snk):
    hdr = (ROOT / "include" / "snk.h").read_text()
    declared = set(re.findall(r"\b(snk_[a-z0-9_]+)\s*\(", hdr))
    from supernova_amd import lib
    bound = set(lib.exported_symbols())
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(snk, name), f"{name} declared in include/snk.h but not exported by libsnk.so"
    assert declared == bound, (declared ^ bound)


def test_last_hbv_flood_without_a_context(snk):
    """snk_ctx_last_hbv_flood (which id flood the last snk_dev_hbv ran, and the components each side flooded) answers 0 and no components
    for a NULL context and takes NULL for either counter; with a context it is tests/test_gpu_hbv_handmade.py's witness of every leg."""
    dev, host = C.c_uint64(7), C.c_uint64(7)
    assert snk.snk_ctx_last_hbv_flood(None, C.byref(dev), C.byref(host)) == 0 and (dev.value, host.value) == (0, 0)
    assert snk.snk_ctx_last_hbv_flood(None, None, None) == 0


def test_last_local_graph_without_a_context(snk):
    """snk_ctx_last_local_graph (fragment-pass attempts, in-chunk circles and big chunks of the last count-and-graph call) answers 0
    everywhere for a NULL context and takes NULL for either counter; with a context it is tests/test_gpu_handreads.py's witness of the
    circle pool's re-run."""
    circles, big = C.c_uint64(7), C.c_uint32(7)
    assert snk.snk_ctx_last_local_graph(None, C.byref(circles), C.byref(big)) == 0 and (circles.value, big.value) == (0, 0)
    assert snk.snk_ctx_last_local_graph(None, None, None) == 0


def test_no_cpu_fallback(snk):
    import torch
    if torch.cuda.is_available():
        return
    h = C.c_void_p()
    err = C.create_string_buffer(256)
    rc = snk.snk_ctx_create(0, C.byref(h), err, 256)
    assert rc == -3 and b"no CPU fallback" in err.value
    import pytest
    from supernova_amd.engine import Engine
    with pytest.raises(RuntimeError):
        Engine(0)


def test_product_never_imports_oracle():
    for f in (ROOT / "supernova_amd").rglob("*"):
        if f.suffix in (".py", ".h", ".hip", ".cpp") and f.is_file():
            txt = f.read_text(errors="ignore")
            assert "snk_oracle" not in txt and "oracle_lib" not in txt and "libsnkoracle" not in txt, f


def test_synth_host_is_deterministic_and_shaped(snk):
    from supernova_amd import synth
    sp = synth.synth_params(4000, seed=123)
    a = synth.synth_host(sp)
    b = synth.synth_host(sp, first=1000, n=500)
    assert np.array_equal(a[0][1000:1500], b[0]) and np.array_equal(a[1][1000:1500], b[1]) and np.array_equal(a[2][1000:1500], b[2])
    rows, quals, bc = a
    assert rows.shape == (4000, 10) and quals.shape == (4000, 150)
    assert 0.005 < (bc == 0).mean() < 0.05
    assert 0.001 < (quals == 12).mean() < 0.004
    # mates of a pair share the barcode
    assert np.array_equal(bc[0::2], bc[1::2])
    # pack/unpack round trip
    codes = synth.unpack_rows(rows, 150)
    assert np.array_equal(synth.pack_rows(codes), rows)


def test_bench_starts_its_own_ranks(monkeypatch):
    """`python bench.py --gpus N` with no launcher around it (WORLD_SIZE unset) re-runs itself under torch.distributed.run on this node --
    the driver's own N > 1 command line -- and leaves with the ranks' exit code (bench.py::self_launch).  No GPU: the launch is intercepted."""
    import importlib.util
    import sys
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("bench_under_test", root / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = {}

    class R:
        returncode = 7

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return R()

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "2", "--warmup", "1", "--transport", "gloo"])
    assert bench.self_launch(4) == 7
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-8:] == ["--gpus", "4", "--steps", "2", "--warmup", "1", "--transport", "gloo"]
    assert Path(cmd[cmd.index("--master-port") + 2]).name == "bench.py"
    assert seen["env"].get("HSA_ENABLE_IPC_MODE_LEGACY") == "0"


def test_bench_dump_outputs_do_not_depend_on_table_order(monkeypatch, tmp_path):
    """bench.py --dump-outputs: the same retained table in two different orders (the bucket order is the library's to choose) gives the
    same files; the sampled entries are the table's own, in key order, and the files stay under 64 MB.  A plain run has --full off.
    No GPU: the device views bench.py takes of the library's arrays are replaced by host views of host arrays."""
    import ctypes
    import importlib.util
    import sys
    import torch
    import supernova_amd.sharded as sharded
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "4"])
    a = bench.parse()
    assert a.steps == 4 and not a.full and not a.dump_outputs
    monkeypatch.setattr(sharded, "_DevBytes", lambda ptr, n: np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(ptr)))

    class Res:
        def _dl(self, ptr, nbytes, dtype, shape):
            return np.frombuffer(ctypes.string_at(ptr, nbytes), dtype=dtype).reshape(shape).copy()

        def spectrum(self):
            return np.bincount(self.arrays[1], minlength=64)[:64].astype(np.uint64)

    rng = np.random.default_rng(3)
    n = 300_000
    keys = rng.integers(0, 2**62, size=(n, 2), dtype=np.uint64)
    counts = rng.integers(3, 60, size=n, dtype=np.uint32)
    ctx = rng.integers(0, 256, size=n, dtype=np.uint8)
    off = np.cumsum(np.r_[0, rng.integers(48, 500, size=100)]).astype(np.uint64)
    bv = rng.integers(0, 256, size=5_000_000, dtype=np.uint8)
    good = rng.integers(0, 151, size=2_000_000, dtype=np.uint16)
    outs = []
    for seed in (0, 1):
        p = np.random.default_rng(seed).permutation(n)
        r = Res()
        r.arrays = (np.ascontiguousarray(keys[p]), counts[p].copy(), ctx[p].copy(), off, bv, good)
        r.raw = type("Raw", (), {})()
        r.raw.keys, r.raw.counts, r.raw.ctx, r.raw.unitig_off, r.raw.good_len = (x.ctypes.data for x in (*r.arrays[:4], good))
        r.n_kmers, r.n_unitigs, r.n_instances, r.n_circles, r.n_reads = n, 100, 123456, 1, good.size
        r.bv = (bv.ctypes.data, bv.size)
        r.hbv_graph = dict(n_vertices=4, n_edges=2, v_left=np.arange(2), v_right=np.arange(2), src=np.arange(2), is_rc=np.zeros(2, np.uint8),
                           fwd=np.arange(100), rev=np.arange(100), order=np.arange(100))
        nb = bench.dump_outputs(r, tmp_path / str(seed), torch.device("cpu"))
        assert 0 < nb <= 64 << 20
        outs.append({f.name: np.load(f) for f in sorted((tmp_path / str(seed)).glob("*.npy"))})
    assert outs[0].keys() == outs[1].keys() and {"kmer_keys.npy", "spectrum.npy", "bv_image_sample.npy", "scalars.npy"} <= outs[0].keys()
    for name, x in outs[0].items():
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, outs[1][name]), name
    w = outs[0]["kmer_keys.npy"].astype(np.uint64)
    lo, hi = (w[:, 2] << np.uint64(32)) | w[:, 3], (w[:, 0] << np.uint64(32)) | w[:, 1]
    assert 1000 < len(lo) < n and np.all(np.lexsort((lo, hi)) == np.arange(len(lo)))
    table = {(int(k0), int(k1)): (int(c), int(x)) for (k0, k1), c, x in zip(keys, counts, ctx)}
    got = zip(lo, hi, outs[0]["kmer_counts.npy"], outs[0]["kmer_ctx.npy"])
    assert all(table[(int(a), int(b))] == (int(c), int(x)) for a, b, c, x in got)
    assert np.array_equal(outs[0]["unitig_lengths.npy"], np.sort(np.diff(off.astype(np.int64)))[::-1])


def test_options_registry_and_no_environment_switches(snk):
    """include/snk.h "tuning": every option has a name and a description; the product reads the environment for tracing and library paths
    only (67 distinct SNK_* switches were read with getenv inside csrc/) -- every algorithmic choice is a context option."""
    names = []
    i = 0
    while snk.snk_option_name(i):
        names.append(snk.snk_option_name(i).decode())
        assert len(snk.snk_option_doc(i)) > 8
        i += 1
    assert len(names) == len(set(names)) >= 40 and {"count_tight", "target_inst", "minimiser_len", "partition_passes", "path_index"} <= set(names)
    assert snk.snk_option_name(i) is None and snk.snk_option_doc(10_000) is None
    env = set()
    for f in (ROOT / "supernova_amd" / "csrc").rglob("*"):
        if f.suffix in (".hip", ".h", ".cc") and f.is_file():
            env |= set(re.findall(r'getenv\("(SNK_[A-Z0-9_]+)"\)', f.read_text(errors="ignore")))
    allowed = {"SNK_TUNING", "SNK_SYNC_TRACE", "SNK_ARENA_TRACE", "SNK_ARENA_POISON", "SNK_INGEST_TRACE", "SNK_HBV_DEPTH", "SNK_RCCL_LIB",
               "SNK_FASTH_LIBDEFLATE", "SNK_FASTH_WHOLE_MAX_MB"}
    assert env <= allowed, env - allowed
    # stages read options by id (SNK_OPT_<name>: an unknown one does not compile); names are looked up by the registry's by-name ABI only,
    # every registered option is read somewhere, and no option state lives outside the context
    csrc = ROOT / "supernova_amd" / "csrc"
    read = set()
    for f in csrc.rglob("*"):
        if f.suffix in (".hip", ".h", ".cc") and f.is_file() and f.name not in ("snk_opts.hip", "snk_opts.h"):
            text = f.read_text(errors="ignore")
            assert not re.search(r'snk_opt_\w*\(\s*"|snk_opt_index\(|snk_opts_enter|\bopts\.(?:v|set)\[', text), f.name
            read |= set(re.findall(r'\bSNK_OPT_([a-z0-9_]+)\b', text))
    assert read == set(names), (set(names) - read, read - set(names))
    opts_src = (csrc / "snk_opts.hip").read_text()
    assert "thread_local" not in opts_src and "abort(" not in opts_src
    t = __import__("supernova_amd.lib", fromlist=["SnkTuning"]).SnkTuning()
    snk.snk_tuning_default(C.byref(t))
    assert t.count_kernel == 0 and t.target_inst == 0


def test_every_launch_goes_through_the_checked_helper():
    """csrc/snk_launch.h: HIP cuts a launch of 2^32 or more work items short without an error ("round 6" (5)), so the one
    launch of the library sits behind a host-side check of its shape, and the grids are computed by the two shared 64-bit functions -- no
    file launches on its own or keeps a private grid helper."""
    launch = re.compile(r"hipLaunchKernelGGL|<<<|hipLaunchKernel\(|hipModuleLaunchKernel|hipExtLaunch")
    helper = re.compile(r"\b(?:nblk|pidx_grid|ck_grid)\s*\([^;{]*\)\s*\{")
    n_files = 0
    for f in (ROOT / "supernova_amd" / "csrc").rglob("*"):
        if f.suffix in (".hip", ".h", ".cc") and f.is_file():
            text = f.read_text(errors="ignore")
            n_files += 1
            assert not helper.search(text), f.name
            assert len(launch.findall(text)) == (1 if f.name == "snk_launch.h" else 0), f.name
    assert n_files > 20 and (ROOT / "supernova_amd" / "csrc" / "snk_launch.h").is_file()


def test_launch_arithmetic_on_the_host(tmp_path):
    """The arithmetic of csrc/snk_launch.h needs no HIP: tests/launch_shape_host.cc is built with the host compiler and checks the ceiling
    division (64 bits, no truncation), its capped form and which launch shapes are refused."""
    import os
    import subprocess
    exe = tmp_path / "launch_shape_host"
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-O1", f"-I{ROOT / 'supernova_amd' / 'csrc'}",
                    str(ROOT / "tests" / "launch_shape_host.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_tools_and_bench_compile():
    """bench.py runs tools/r6_full_job.py in a process of its own (config.large_job) and the evidence scripts drive the others: a tool that
    does not even compile must not wait for a GPU box to be noticed."""
    import py_compile
    root = Path(__file__).resolve().parent.parent
    files = [root / "bench.py", root / "__graft_entry__.py"] + sorted((root / "tools").glob("*.py")) + sorted((root / "tests" / "tools").glob("*.py"))
    assert (root / "tools" / "r6_full_job.py") in files
    for f in files:
        py_compile.compile(str(f), doraise=True)


def test_dictionary_load_below_eleven_is_refused_without_a_context(snk):
    """path_slots_x10 sizes the pather's k-mer dictionary (nk * x / 10 + 1024 slots for nk unitig k-mers); below 11 it could hold fewer
    slots than k-mers and its insertion would never find a free one.  The registry's range check (snk_ctx_set_option, SNK_TUNING) refuses
    such a value: snk_option_check asks it without a context."""
    err = C.create_string_buffer(256)
    for v in (10, 1, 0, -1):
        assert snk.snk_option_check(b"path_slots_x10", v, err, 256) == -1, v
        assert b"path_slots_x10" in err.value
    for v in (11, 30, 100):
        assert snk.snk_option_check(b"path_slots_x10", v, err, 256) == 0, v
    assert snk.snk_option_check(b"path_fast_gs", 0, err, 256) == 0
    assert snk.snk_option_check(b"no_such_option", 1, err, 256) == -1
    for name in (b"path_edge_cap", b"path_redo_cap", b"path_ubc_cap"):
        assert snk.snk_option_check(name, 1, err, 256) == 0


# ---- the registry's ranges (csrc/snk_opts.h): snk_option_check asks the one range check every setter goes through, without a context

_RANGE = re.compile(r" \[(0 or )?(\d+)\.\.(\d+)( step (\d+))?\]$")


def _registry(snk):
    """-> {name: (doc, zero_also, lo, hi, step)} from snk_option_name / snk_option_doc: every doc string ends with its range."""
    out, i = {}, 0
    while snk.snk_option_name(i):
        name, doc = snk.snk_option_name(i).decode(), snk.snk_option_doc(i).decode()
        m = _RANGE.search(doc)
        assert m, f"the description of option '{name}' does not end with its range: {doc!r}"
        out[name] = (doc, bool(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(5) or 1))
        i += 1
    return out


def _takes(snk, name, value):
    err = C.create_string_buffer(512)
    rc = snk.snk_option_check(name.encode(), value, err, 512)
    assert rc in (0, -1) and (rc == 0 or name.encode() in err.value)
    return rc == 0


def test_every_option_has_a_range_and_refuses_what_lies_outside(snk):
    """include/snk.h: snk_ctx_set_option returns SNK_E_ARG for "a value out of its range" -- for EVERY option: both ends of the range are
    taken, one below, one above, -1 and 2^40 are not (no option is open on either side), a stepped range refuses what lies between its
    steps, and 0 is taken exactly where the range starts there or names it."""
    reg = _registry(snk)
    assert len(reg) >= 70
    for name, (doc, zero, lo, hi, step) in reg.items():
        assert 0 <= lo <= hi < 2**40 and step >= 1 and (hi - lo) % step == 0, (name, doc)
        assert _takes(snk, name, lo) and _takes(snk, name, hi), name
        assert not _takes(snk, name, hi + 1) and not _takes(snk, name, -1) and not _takes(snk, name, 2**40), name
        assert not _takes(snk, name, -2**40) and not _takes(snk, name, 2**63 - 1) and not _takes(snk, name, -2**63), name
        assert _takes(snk, name, 0) == (zero or lo == 0), name
        if lo - 1 > 0:
            assert not _takes(snk, name, lo - 1), name
        if step > 1:
            assert not _takes(snk, name, lo + 1) and _takes(snk, name, lo + step), name


# values that reach a shift, a divisor, a loop bound or a packed field at the call site (file:line as of the commit that added the ranges)
HARMFUL = {
    "split_log2": (0, 32, 40, 64),                   # (1u << v) - 1u, snk_rank.hip rank_setup: undefined from 32 on
    "rank_round_batch0": (0,),                       # no round runs, the flag stays zero, "converged": unconverged ranks go out
    "rank_round_batch": (0,),                        # the same in snk_prank_walk
    "tight_tries": (0, 65536, 1 << 20),              # << 16 into the high half of a 32-bit word (snk_pipeline.hip tight_for)
    "hot_class_inst": (0, 1), "screen_target": (0, 1), "target_inst": (1, 7), "chunk_kmers": (0,),     # divisors and bucket targets
    "bucket_fill_pct": (0, 101, 1000), "msp_cap_pct": (0, 101),
    "count_tight": (1, 255, 1985, 2048, 1 << 16),    # the doc string's own 256 .. slots - 64
    "count_screen": (3,), "count_screen_ng": (3,), "minimiser_len": (1, 15, 17, 18, 24, 32), "path_fast_gs": (4, 12, 32),
    "bl_cpw": (0,), "exchange_ranges": (0, 65), "emit_grid_log2": (23, 32), "partition_passes": (65,), "dbg_fake_segs": (33,),
    "path_slots_x10": (0, 10), "path_fp_mask": (1 << 30,), "rank_wyllie": (2,), "arena_vmm": (2,), "trim_rowwise": (2,),
}


def test_harmful_option_values_are_refused(snk):
    """The values whose call sites cannot take them, read off the code (never run): each is refused by name, so that a range which grows
    back over one of them fails here."""
    reg = _registry(snk)
    for name, values in HARMFUL.items():
        assert name in reg, name
        for v in values:
            assert not _takes(snk, name, v), (name, v)
    # the fields of snk_tuning keep "0 = the library's choice"; by name, 0 is a value like any other
    for name in ("hot_class_inst", "target_inst", "chunk_kmers", "bucket_fill_pct", "exchange_ranges", "hot_min", "hot_factor", "unitig_bc_cut"):
        assert not _takes(snk, name, 0), name


def _registry_defaults():
    src = (ROOT / "supernova_amd" / "csrc" / "snk_opts.h").read_text()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*X\((\w+),\s*(\d+),", src, re.M)}


def test_registry_defaults_lie_in_their_own_range(snk):
    """The default of every entry is a value its setter would take -- except where the entry's 0 is never read because the call site asks
    snk_opt_is_set and chooses from the data (snk_opts.h names them): there the test looks for that question in the sources."""
    reg, dflt = _registry(snk), _registry_defaults()
    assert set(dflt) == set(reg)
    csrc = "".join(f.read_text(errors="ignore") for f in (ROOT / "supernova_amd" / "csrc").glob("*.hip") if f.name != "snk_opts.hip")
    for name, d in dflt.items():
        if _takes(snk, name, d):
            continue
        assert d == 0 and re.search(r"(snk_opt_is_set\(ctx, |cap0\()SNK_OPT_%s\b" % name, csrc), (name, d)


def _values_set_today():
    """(file, option, value) for every literal option value in the tests, the tools, bench.py and the Python package: tune("name", v),
    set_option("name", v), "name": v / "SNK_NAME": "v" in dicts, name=v in SNK_TUNING strings and keyword arguments, name=int(rng.choice([..]))."""
    names = set(_registry_defaults())
    files = [ROOT / "bench.py"] + [f for d in ("tests", "tests/tools", "tools", "supernova_amd") for f in sorted((ROOT / d).glob("*.py"))]
    num = r"(-?(?:0x[0-9a-fA-F]+|\d[\d_]*))"
    pats = [re.compile(r"""(?:tune|set_option)\(\s*["'](?:SNK_)?(\w+)["'],\s*["']?%s["']?\s*\)""" % num),
            re.compile(r"""["'](?:SNK_)?(\w+)["']:\s*["']?%s["']?\s*[,})]""" % num),
            re.compile(r"""\b([a-z][a-z0-9_]+)=%s\b""" % num)]
    lists = re.compile(r"""\b([a-z][a-z0-9_]+)=int\(rng\.choice\(\[([^\]]+)\]\)\)""")
    found = []
    for f in files:
        text = f.read_text(errors="ignore")
        if f.name == "test_abi.py":
            text = text.split("# ---- the registry's ranges", 1)[0]      # (this section names refused values on purpose)
        for p in pats:
            for m in p.finditer(text):
                if m.group(1).lower() in names:
                    found.append((f.name, m.group(1).lower(), int(m.group(2).replace("_", ""), 0)))
        for m in lists.finditer(text):
            if m.group(1) in names:
                found += [(f.name, m.group(1), int(v.strip(), 0)) for v in m.group(2).split(",")]
    return found


def test_every_value_a_caller_sets_today_is_accepted(snk):
    """A range that would refuse what a test, a tool, bench.py or the package sets is wrong, and shows here rather than on the GPU box."""
    found = _values_set_today()
    assert len(found) >= 60 and {"bench.py", "fuzz_parity.py", "test_gpu_parity.py", "msp_probe2.py"} <= {f for f, _, _ in found}, len(found)
    assert ("test_gpu_paths.py", "path_fast_gs", 16) in found and ("test_gpu_sharded.py", "hot_class_inst", 300) in found
    refused_on_purpose = {("test_gpu_paths.py", "path_slots_x10", 10), ("test_gpu_paths.py", "path_slots_x10", 0)}
    bad = [x for x in found if not _takes(snk, x[1], x[2]) and x not in refused_on_purpose]
    assert not bad, bad
    import test_gpu_option_invariance as inv
    for name, spec in inv.NEUTRAL.items():
        for v in spec["values"]:
            assert _takes(snk, name, v), (name, v)
        for k, v in spec.get("with", {}).items():
            assert _takes(snk, k, v), (name, k, v)


INVALIDATING = ("count_dbg", "msp_dbg", "overlap_probe", "overlap_probe_dbg", "path_idx_dbg", "join_dbg", "dbg_fake_segs")
# option -> the existing test that forces it (file::function); the function's source must name the option
ALREADY_FORCED = {
    "count_tight": "test_gpu_parity.py::test_booked_table_slots_count_the_same_table",
    "count_screen": "test_gpu_parity.py::test_grouped_per_barcode_graphs",
    "count_screen_ng": "test_gpu_parity.py::COUNT_VARIANTS",
    "screen_ratio_pct": "test_gpu_parity.py::test_error_rich_reads_are_repartitioned_into_smaller_buckets",
    "target_inst": "test_gpu_dfin.py::test_tuning_struct_and_options",
    "adaptive_buckets": "test_gpu_parity.py::test_error_rich_reads_are_repartitioned_into_smaller_buckets",
    "count_persist": "test_gpu_parity.py::test_count_launch_shapes",
    "minimiser_len": "test_gpu_dfin.py::test_tuning_struct_and_options",
    "global_graph": "test_gpu_parity.py::graph_stage",
    "partition_passes": "test_gpu_parity.py::test_hot_buckets_are_repartitioned_by_kmer_hash",
    "msp_cap_pct": "test_gpu_parity.py::test_partition_overflow_segment",
    "msp_dense": "test_gpu_parity.py::test_dense_partition_mode",
    "msp_hot_factor": "test_gpu_sharded.py::test_sharded_overflowing_buckets_and_the_hot_table",
    "msp_hot_min": "test_gpu_sharded.py::test_sharded_overflowing_buckets_and_the_hot_table",
    "trim_fused": "test_gpu_parity.py::test_trim_inside_the_partition_kernel",
    "hot_min": "test_gpu_sharded.py::test_sharded_hot_buckets_are_repartitioned_on_their_owner",
    "hot_factor": "test_gpu_sharded.py::test_sharded_hot_buckets_are_repartitioned_on_their_owner",
    "hot_class_inst": "test_gpu_sharded.py::test_sharded_hot_buckets_are_repartitioned_on_their_owner",
    "bl_pool": "test_gpu_parity.py::test_circle_pool_retry",
    "emit_grid_log2": "test_gpu_parity.py::test_golden_case_strided_fragment_copy",
    "plan_mem_mb": "test_gpu_parity.py::test_a_small_device_plans_passes_and_probes_its_regions",
    "hbv_huge_pages": "test_gpu_parity.py::test_context_free_hbv_writer_after_a_closed_engine",
    "hbv_short_queue": "test_gpu_parity.py::test_context_free_hbv_writer_after_a_closed_engine",
    "join_replicated": "test_gpu_sharded.py::test_sharded_replicated_ranking_with_circles",
    "path_index": "test_gpu_paths.py::test_long_tandem_reads",
    "path_dict_max_kb": "test_gpu_parity.py::test_read_paths_match_reference",
    "path_slots_x10": "test_gpu_paths.py::VARIANTS",
    "path_two_pass": "test_gpu_paths.py::VARIANTS",
    "path_fast_gs": "test_gpu_paths.py::VARIANTS",
    "path_fused": "test_gpu_parity.py::test_read_paths_full_capacity_pass",
    "path_redo_all": "test_gpu_paths.py::test_path_list_overflow_reruns",
    "path_fp_mask": "test_gpu_parity.py::test_read_paths_with_colliding_fingerprints",
    "path_edge_cap": "test_gpu_paths.py::RETRIES",
    "path_redo_cap": "test_gpu_paths.py::RETRIES",
    "path_ubc_cap": "test_gpu_paths.py::RETRIES",
    "unitig_bc_cut": "test_gpu_parity.py::test_unitig_barcode_lists_two_derivations_200k_parity_unpinned_rust",
    "dups_two_sorts": "test_gpu_paths.py::VARIANTS",
    "hbv_dev_min": "test_gpu_parity.py::HBV_FLOODS",
    "hbv_big": "test_gpu_parity.py::HBV_FLOODS",
    "df_stream": "test_gpu_dfin.py::test_streamed_count_graph_equals_resident",
}


def _source_of(path, symbol):
    """The text of a top-level function, fixture or assignment of a test module (up to the next top-level statement)."""
    text = (ROOT / "tests" / path).read_text()
    m = re.search(r"^(?:def %s\(|%s\s*=)" % (re.escape(symbol), re.escape(symbol)), text, re.M)
    assert m, f"{path} has no top-level '{symbol}'"
    rest = text[m.start():]
    end = re.search(r"^(?=[^\s#)\]}])", rest[rest.index("\n") + 1:], re.M)
    return rest[:rest.index("\n") + 1 + end.start()] if end else rest


def test_every_option_is_classified(snk):
    """Every registered option is in exactly one of: NEUTRAL (tests/test_gpu_option_invariance.py forces it and compares the results),
    ALREADY_FORCED (an existing test does; its source names the option, in either spelling) or INVALIDATING (debug / probe / measurement
    modes, whose description says so).  An option added without a test fails here."""
    import test_gpu_option_invariance as inv
    reg = _registry(snk)
    groups = {"NEUTRAL": set(inv.NEUTRAL), "ALREADY_FORCED": set(ALREADY_FORCED), "INVALIDATING": set(INVALIDATING)}
    for name in reg:
        where = [g for g, s in groups.items() if name in s]
        assert len(where) == 1, f"option '{name}' is in {where or 'no group'}"
    for g, s in groups.items():
        assert s <= set(reg), (g, s - set(reg))
    for name in INVALIDATING:
        assert re.search(r"debug|probe|measurement", reg[name][0]), (name, reg[name][0])
    for name, where in ALREADY_FORCED.items():
        path, symbol = where.split("::")
        src = _source_of(path, symbol)
        assert re.search(r"""["'](?:SNK_%s|%s)["']""" % (name.upper(), name), src) or re.search(r"\b%s=" % name, src), f"{where} does not set '{name}'"
    for name, spec in inv.NEUTRAL.items():
        assert spec["values"] and spec["legs"] and spec["evidence"], name
