"""Generates tests/golden/engine_step_launches.json: which launches a decode step is made of, per model, option set and row count.

The host code that routes a decode step's projections (csrc/decode_linear.h, enqueue_step in csrc/engine.hip) picks a kernel per
projection from the row count, the engine's options and the layer's shapes, and decides whether the step may be replayed without
cache maintenance (`written_once_plan`).  The parity tests pin what the step COMPUTES; this table pins what it LAUNCHES: for every case
the launches per kind of tl_engine_profile_step (qkv, wo, gate|up, w_down, lm_head, attention, merge, step end), its split count,
and tl_engine_check_step's launch count and plan flag.  A change that silently moves a projection to another kernel, or a step off
the per-layer buffers, shows up here even where the numbers still agree.

Cases (tests/test_zz_engine_step_launches_gpu.py runs the same `record`): two layers of the Qwen3-4B widths with the default
options, "qmm6" = 0 and "qmm3" = 0, and with TL_AQL=0 (no per-layer buffers: the batched step on the shared ones); TINY_CFG (the
fallbacks a 256-wide model reaches); TINY_CFG with one dense and one Qwen3-MoE layer.  1, 4, 5, 8, 9, 16, 17, 33 and 64 rows each.

Needs the GPU.  Run from the repository root at the commit whose routing is to be recorded:
    python tests/golden/make_engine_step_launches.py [--out tests/golden/engine_step_launches.json]"""

import argparse
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for extra in (ROOT, ROOT / "tests", ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    if str(extra) not in sys.path:
        sys.path.insert(0, str(extra))

BATCHES = (1, 4, 5, 8, 9, 16, 17, 33, 64)
# (model, label, tl_engine_set_option values, TL_AQL)
SETUPS = (
    ("qwen4b_2_layers", "default", {}, "1"),
    ("qwen4b_2_layers", "qmm6=0", {"qmm6": 0}, "1"),
    ("qwen4b_2_layers", "qmm3=0", {"qmm3": 0}, "1"),
    ("qwen4b_2_layers", "shared_buffers", {}, "0"),
    ("tiny", "default", {}, "1"),
    ("tiny_moe", "default", {}, "1"),
)
PAGE = 64


def models(tmp_dir) -> dict:
    import tiny_llm_ext_hip as ext
    from checkpoint_fixture import MOE_CFG_OVERRIDES, make_moe_weights, write_checkpoint
    from helpers import QWEN4B_CFG, TINY_CFG
    from tiny_llm_hip import load
    from tiny_llm_hip.synthetic import synthetic_qwen3

    ext.load_library(str(ROOT))
    # layer 0 dense, layer 1 sparse (4 experts, top 2)
    moe_cfg = dict(TINY_CFG, **dict(MOE_CFG_OVERRIDES, num_hidden_layers=2, mlp_only_layers=[0]))
    words = [f"w{i}" for i in range(moe_cfg["vocab_size"] - 2)]
    path = write_checkpoint(Path(tmp_dir) / "moe_ckpt", moe_cfg, make_moe_weights(moe_cfg, seed=21), vocab_words=words)
    return {
        "qwen4b_2_layers": (dict(QWEN4B_CFG, num_hidden_layers=2), synthetic_qwen3(dict(QWEN4B_CFG, num_hidden_layers=2), seed=11, device="cuda")),
        "tiny": (TINY_CFG, synthetic_qwen3(TINY_CFG, seed=12, sigma=0.05, device="cuda")),
        "tiny_moe": (moe_cfg, load(str(path))[0]),
    }


def _engine(cfg, model, options, aql):
    """64 slots behind prompts of 31 .. 200 tokens (slot 0: 200, a context a single row splits)."""
    from tiny_llm_hip.engine import DecodeEngine

    old = os.environ.get("TL_AQL")
    os.environ["TL_AQL"] = aql
    try:
        n = max(BATCHES)
        lengths = [200 - (29 * i) % 170 for i in range(n)]
        pages = sum((ln + 4 * len(BATCHES) + PAGE) // PAGE + 1 for ln in lengths) + 2
        eng = DecodeEngine(model, page_size=PAGE, num_pages=pages, max_batch=n, max_prefill_rows=256, options=options)
        rng = np.random.default_rng(7)
        for slot, ln in enumerate(lengths):
            eng.begin(slot)
            eng.prefill(slot, [int(t) for t in rng.integers(2, cfg["vocab_size"], size=ln)])
        return eng
    finally:
        if old is None:
            os.environ.pop("TL_AQL", None)
        else:
            os.environ["TL_AQL"] = old


def record(all_models: dict, log=None) -> dict:
    """{"<model>/<setup>/<rows>": {...}} for every case; a step the engine refuses is recorded by its message."""
    out = {}
    for name, label, options, aql in SETUPS:
        cfg, model = all_models[name]
        eng = _engine(cfg, model, options, aql)
        try:
            for b in BATCHES:
                key = f"{name}/{label}/{b}"
                try:
                    eng.decode(2, batch=b)
                    prof = eng.profile_step(b)
                    chk = eng.check_step(b)
                    out[key] = {"launches": [prof["kinds"][k]["launches"] for k in eng.PROFILE_KINDS], "n_splits": prof["n_splits"],
                                "check_launches": chk["launches"], "check_n_splits": chk["n_splits"], "written_once_plan": chk["written_once_plan"]}
                    if log and chk["double_writes"]:
                        log(f"{key}: {chk['double_writes']} elements written twice, first by launch {chk['first_launch']} (kind {chk['first_kind']})")
                except RuntimeError as err:
                    out[key] = {"error": str(err)}
                    eng.close()
                    eng = _engine(cfg, model, options, aql)
                if log:
                    log(f"{key}: {out[key]}")
        finally:
            eng.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "engine_step_launches.json"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        table = record(models(tmp), log=lambda s: print(s, flush=True))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
    print(f"wrote {args.out} ({len(table)} cases)")


if __name__ == "__main__":
    main()
