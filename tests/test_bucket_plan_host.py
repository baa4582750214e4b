"""The bucket plan (supernova_amd/csrc/snk_plan.h) on the host: tests/plan_host.cc is built from snk_plan.hip and snk_opts.hip with
the host compiler -- no HIP header, no HIP runtime -- and checks values derived by hand from the documented rule and invariants over a
grid of inputs.  The callers' side is read off their sources: each fills the plan's inputs and differs from the others only in the
fields snk_plan.h names as differences.  The device side is tests/test_gpu_bucket_plan.py."""
import os
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "supernova_amd" / "csrc"
HOST_SOURCES = ["snk_plan.hip", "snk_opts.hip"]
# the inputs every caller may fill from its job, and the fields snk_plan.h documents as the present differences between the callers
JOB_FIELDS = {"K", "grouped", "has_bc", "min_freq", "min_bc", "n_buckets", "inst_ub", "world", "ratio", "retain", "may_adapt", "opts", "slots", "plain_limit", "screen_limit"}
NAMED_DIFFERENCES = {"nb_max", "use_retain", "may_book", "book_only_adapting", "screen_needs_tight", "fill_unclamped"}


def test_plan_sources_need_no_hip():
    for name in HOST_SOURCES + ["snk_plan.h", "snk_opts.h"]:
        src = (CSRC / name).read_text()
        if name == "snk_opts.hip":
            assert "#ifndef SNK_OPTS_NO_CTX" in src
            src = re.sub(r"#ifndef SNK_OPTS_NO_CTX.*?#endif", "", src, flags=re.S)      # (what the host build does not see)
        includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)
        assert not any("hip" in i or i in ("snk_ctx.h", "snk_common.h") for i in includes), (name, includes)
        assert "snk_ctx" not in src or name.startswith("snk_opts"), name      # (snk_opts.h declares the context's accessors next to the registry's)


def test_bucket_plan_on_the_host(tmp_path):
    exe = tmp_path / "plan_host"
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-O1", "-DSNK_OPTS_NO_CTX", f"-I{CSRC}", "-x", "c++", str(ROOT / "tests" / "plan_host.cc"),
                    *(str(CSRC / s) for s in HOST_SOURCES), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-4000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) >= 2000          # the grid: a few thousand combinations at the least


def _assigned(text):
    return dict((m.group(1), m.group(2).strip()) for m in re.finditer(r"\bpin\.(\w+) = ([^;]+);", text))


def _function(src, start, end):
    a = src.index(start)
    return src[a:src.index(end, a)]


def test_callers_differ_only_in_the_named_fields():
    pipeline = (CSRC / "snk_pipeline.hip").read_text()
    shard = (CSRC / "snk_shard_step.hip").read_text()
    resident = _assigned(_function(pipeline, 'extern "C" int snk_dev_count_graph(', "// Streamed input"))
    streamed = _assigned(_function(pipeline, 'extern "C" int snk_dev_stream_begin(', 'extern "C" int snk_dev_stream_append('))
    sharded = _assigned(_function(shard, "snk_plan_in shard_plan_in(", "template <typename In, typename Out>"))
    for name, got in (("resident", resident), ("streamed", streamed), ("sharded", sharded)):
        assert got, name
        assert set(got) <= JOB_FIELDS | NAMED_DIFFERENCES, (name, set(got) - JOB_FIELDS - NAMED_DIFFERENCES)
        assert {"K", "n_buckets", "inst_ub", "opts", "slots", "plain_limit", "screen_limit", "nb_max"} <= set(got), name
    # the geometry comes from the same three functions everywhere
    for f in ("slots", "plain_limit", "screen_limit"):
        assert len({re.sub(r"\bp->K\b", "K", g[f]) for g in (resident, streamed, sharded)}) == 1, f
    # the named differences, as the table in snk_plan.h states them (a field a caller leaves alone has the struct's default)
    pick = lambda got: {k: v for k, v in got.items() if k in NAMED_DIFFERENCES}
    assert pick(resident) == {"nb_max": "1ull << 25", "use_retain": "true"}
    assert pick(streamed) == {"nb_max": "1ull << 23", "may_book": "false", "fill_unclamped": "true"}
    assert pick(sharded) == {"nb_max": "1ull << 26", "may_book": "may_book", "book_only_adapting": "true", "screen_needs_tight": "true"}
    hdr = (CSRC / "snk_plan.h").read_text()
    for f in NAMED_DIFFERENCES:
        assert re.search(r"//\s+%s\s+\S" % f, hdr), f                  # a row of the comment block
    # ... and the policy's figures live in snk_plan alone
    for path in sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.h")):
        if path.name.startswith("snk_plan"):
            continue
        text = path.read_text()
        assert not re.search(r"\b5000u\b|\b3500u\b|0\.65 \*|256u \* ctx->mlen", text), path.name
