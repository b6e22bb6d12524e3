"""CPU tier: the decode attention's plan without a device (csrc/attn_plan.h).

tests/attention_plan_check.cpp is a stand-alone program over the header the library itself uses, built with AddressSanitizer and UBSan and
run as its own process.  `check` sweeps head shapes, head sizes, page sizes, page formats, batches and contexts and holds every plan to
what a launch of it needs; `plans` prints the plans of the requests it reads, and tests/golden/attention_plans.json holds what
tl_decode_attention_plan answered before the header existed (tools/record_attention_plans.py): the header must reproduce every one."""

import json
import os
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tests" / "attention_plan_check.cpp"
GOLDEN = ROOT / "tests" / "golden" / "attention_plans.json"
HEADER = ROOT / "tiny-llm_amd" / "csrc" / "attn_plan.h"
FLAGS = ["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "tiny-llm_amd" / "csrc")]
KNOBS = ("TL_ATTN_RQ", "TL_ATTN_MAX_SPLITS", "TL_ATTN_MIN_TOKENS", "TL_ATTN_MFMA")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("attention_plan") / "attention_plan_check"
    subprocess.run([*FLAGS, str(DRIVER), "-o", str(out)], check=True)
    return out


def _env(settings):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(settings)
    return env


def test_every_plan_is_a_launch_the_kernels_take(exe):
    done = subprocess.run([str(exe), "check"], capture_output=True, text=True, timeout=300, env=_env({}))
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    m = re.fullmatch(r"ok plans=(\d+) checks=(\d+)", done.stdout.strip())
    assert m and int(m.group(1)) >= 1_000_000 and int(m.group(2)) >= int(m.group(1)), done.stdout[-400:]


def test_the_header_reproduces_the_recorded_plans(exe):
    golden = json.loads(GOLDEN.read_text())
    shapes = {(c["num_heads"], c["num_kv_heads"]) for c in golden["cases"] if not c["env"]}
    assert shapes >= {(32, 8), (16, 8), (40, 8), (64, 8), (8, 8), (4, 2)} and sum(1 for c in golden["cases"] if c["env"]) >= 3
    records = 0
    for case in golden["cases"]:
        grid = [(batch, ctx) for batch in case["batches"] for ctx in case["contexts"]]
        assert len(case["plans"]) == 3 * len(grid)
        # the entry point plans head_dim 128 on 128-token pages for context + 1 tokens (the token being decoded included)
        lines = [f"{case['num_heads']} {case['num_kv_heads']} 128 128 {batch} {max(1, ctx + 1)} 0 0 0" for batch, ctx in grid]
        done = subprocess.run([str(exe), "plans"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=_env(case["env"]))
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
        got = [json.loads(line) for line in done.stdout.splitlines()]
        assert len(got) == len(grid)
        for i, ((batch, ctx), plan) in enumerate(zip(grid, got)):
            want = case["plans"][3 * i:3 * i + 3]
            assert plan["plan"] == want, f"{case['num_heads']}/{case['num_kv_heads']} heads, {case['env']}, {batch} sequences at {ctx} tokens: {plan['plan']} against {want}"
            assert plan["variant"] == 1 and plan["grid"][2] == batch
        records += len(grid)
    assert records >= 5000


def test_the_plan_header_is_host_only():
    text = HEADER.read_text()
    assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text
    assert '#include "' not in text  # nothing of the project's device code either
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", str(HEADER)], check=True)
