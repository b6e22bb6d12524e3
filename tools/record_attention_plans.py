#!/usr/bin/env python3
"""Record tl_decode_attention_plan over a grid into tests/golden/attention_plans.json (no device, no launch).

    python3 tools/record_attention_plans.py <libtinyllm_hip.so> <commit> [out.json]

The grid: every head shape x batch x context below with the TL_ATTN_* knobs unset, and at 32 / 8 heads each knob setting
tests/test_decode_plans_cpu.py::test_attention_plan_knobs_are_read uses.  A case's plans are one flat list, batch-major:
n_splits, tokens_per_split, heads per workgroup of (batches[0], contexts[0]), (batches[0], contexts[1]), ...
tests/test_attention_plan_cpu.py holds csrc/attn_plan.h to every one of them."""

import ctypes
import json
import os
import sys

HEAD_SHAPES = [(32, 8), (16, 8), (40, 8), (64, 8), (8, 8), (4, 2)]
# both sides of every threshold of the rules (1|2, 2|3, 4|5, 8|9, 16|17, 23|24, 24|25, 32|33, 64) and a spread between and beyond
BATCHES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17, 20, 23, 24, 25, 32, 33, 48, 64, 128, 256]
KNOB_BATCHES = [1, 2, 4, 5, 8, 16, 17, 24, 64]
CONTEXTS = [0, 1] + [c for p in range(6, 18) for b in (1 << p,) for c in (b - 2, b - 1, b, b + 1, 3 * b // 2)]
KNOBS = ("TL_ATTN_RQ", "TL_ATTN_MAX_SPLITS", "TL_ATTN_MIN_TOKENS", "TL_ATTN_MFMA")
KNOB_SETTINGS = [{"TL_ATTN_MIN_TOKENS": "64"}, {"TL_ATTN_MIN_TOKENS": "64", "TL_ATTN_MAX_SPLITS": "8"}, {"TL_ATTN_RQ": "4"}]


def main() -> None:
    lib = ctypes.CDLL(sys.argv[1])
    commit = sys.argv[2]
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "attention_plans.json")
    out3 = (ctypes.c_int * 3)()
    cases = []
    for heads, kv_heads, env, batches in [(h, k, {}, BATCHES) for h, k in HEAD_SHAPES] + [(32, 8, env, KNOB_BATCHES) for env in KNOB_SETTINGS]:
        for name in KNOBS:
            os.environ.pop(name, None)
        os.environ.update(env)
        plans = []
        for batch in batches:
            for ctx in CONTEXTS:
                assert lib.tl_decode_attention_plan(batch, ctx, heads, kv_heads, out3) == 1
                plans += list(out3)
        cases.append({"num_heads": heads, "num_kv_heads": kv_heads, "env": env, "batches": batches, "contexts": CONTEXTS, "plans": plans})
    golden = {
        "what": "tl_decode_attention_plan(batch, context, num_heads, num_kv_heads) -> (n_splits, tokens_per_split, heads per workgroup) "
                "at head_dim 128 on 128-token pages; the planner sees context + 1 tokens",
        "recorded_from": commit,
        "command": "python3 tools/record_attention_plans.py tiny-llm_amd/extensions_hip/tiny_llm_ext_hip/libtinyllm_hip.so " + commit,
        "cases": cases,
    }
    with open(out_path, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
    print(sum(len(c["plans"]) // 3 for c in cases), "plans ->", out_path)


if __name__ == "__main__":
    main()
