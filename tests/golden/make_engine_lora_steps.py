"""Generates tests/golden/engine_lora_steps.json: what a decode step under LoRA adapters launches and produces, per model and row count.

tests/golden/engine_step_launches.json pins the launches of the base program; no case of it holds an adapter.  A step in which a
live slot carries an adapter is another plan: unbatched layers on the shared buffers, a shrink / expand pair behind each of the four
projection groups (enqueue_step in csrc/engine.hip, csrc/lora.h), replayed by hipGraphLaunch.  This table pins that plan: for every
case the launches per kind of tl_engine_profile_step and its split count, tl_engine_check_step's launch count and plan flag (0: an
adapter plan is never written-once), tl_engine_replay_route's text, the ids of 4 greedy captured decode steps for every slot (behind the
engine's one eager warm step; the replays are counted) and the SHA-256 of the bf16 bits of the logits after the last of them.  Host code that builds the step differently shows up here even
where the logits still meet the truth.

Cases (tests/test_zz_lora_step_pin_gpu.py runs the same `record`): TINY_CFG dense and TINY_CFG with one dense and one Qwen3-MoE layer
(the two small models of make_engine_step_launches.py); the mixed batch of test_zz_lora_gpu.py -- adapters X (rank 16, every target),
none, Y (rank 8, q and v), X, none cycling over the slots, prompts of 3 .. 13 tokens; 1, 4, 5 and 17 rows (the GEMV rows, the first
batched row count, the first past 16 where wo changes route).  On the MoE layer X adapts the attention projections only (the engine
refuses MLP targets there).  TL_AQL is left as the environment has it (the default).

Needs the GPU.  `main` records twice and refuses to write a table the engine does not repeat.  Run from the repository root at the
commit whose adapter steps are to be recorded:
    python tests/golden/make_engine_lora_steps.py [--out tests/golden/engine_lora_steps.json]"""

import argparse
import hashlib
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for extra in (ROOT, ROOT / "tests", ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    if str(extra) not in sys.path:
        sys.path.insert(0, str(extra))

BATCHES = (1, 4, 5, 17)
MODELS = ("tiny", "tiny_moe")
CYCLE = ("X", None, "Y", "X", None)
STEPS = 4
MLP_TARGETS = ("gate", "up", "down")


def models(tmp_dir) -> dict:
    """name -> (cfg, model, indices of its MoE layers)"""
    import tiny_llm_ext_hip as ext
    from checkpoint_fixture import MOE_CFG_OVERRIDES, make_moe_weights, write_checkpoint
    from helpers import TINY_CFG
    from tiny_llm_hip import load
    from tiny_llm_hip.synthetic import synthetic_qwen3

    ext.load_library(str(ROOT))
    # layer 0 dense, layer 1 sparse (4 experts, top 2)
    moe_cfg = dict(TINY_CFG, **dict(MOE_CFG_OVERRIDES, num_hidden_layers=2, mlp_only_layers=[0]))
    words = [f"w{i}" for i in range(moe_cfg["vocab_size"] - 2)]
    path = write_checkpoint(Path(tmp_dir) / "moe_ckpt", moe_cfg, make_moe_weights(moe_cfg, seed=21), vocab_words=words)
    return {
        "tiny": (TINY_CFG, synthetic_qwen3(TINY_CFG, seed=12, sigma=0.05, device="cuda"), ()),
        "tiny_moe": (moe_cfg, load(str(path))[0], (1,)),
    }


def mixed_prompt(cfg, i):
    """test_zz_lora_gpu.py's _mixed_prompt"""
    return [int(t) for t in np.random.default_rng(100 + i).integers(0, cfg["vocab_size"], size=3 + (i * 5) % 11)]


def adapters(cfg, moe_layers) -> dict:
    """test_zz_lora_gpu.py's X and Y, without the MLP targets of a MoE layer"""
    import lora_oracle as L

    out = {}
    for key, (rank, targets, seed) in {"X": (16, L.TARGETS, 0), "Y": (8, ("q", "v"), 1)}.items():
        a = L.make_adapter(cfg, rank, targets=targets, seed=seed, sigma=0.05, scale=1.0)
        a["weights"] = {(layer, t): ab for (layer, t), ab in a["weights"].items() if not (layer in moe_layers and t in MLP_TARGETS)}
        out[key] = L.to_lora_adapter(a)
    return out


def record(all_models: dict, log=None) -> dict:
    """{"<model>/<rows>": {...}} for every case"""
    import torch
    from tiny_llm_hip.engine import DecodeEngine

    out = {}
    for name in MODELS:
        cfg, model, moe_layers = all_models[name]
        named = adapters(cfg, moe_layers)
        for b in BATCHES:
            eng = DecodeEngine(model, page_size=128, num_pages=b + 2, max_batch=b, max_prefill_rows=160)
            try:
                ids = {k: eng.load_lora(a) for k, a in named.items()}
                for s in range(b):
                    eng.begin(s)
                    if CYCLE[s % len(CYCLE)] is not None:
                        eng.set_lora(s, ids[CYCLE[s % len(CYCLE)]])
                    eng.prefill(s, mixed_prompt(cfg, s))
                for _ in range(1 + STEPS):  # the first step of an engine is launched eagerly; the next STEPS are graph replays
                    eng.decode(1, batch=b)
                case = {"ids": [eng.read_tokens(s, STEPS) for s in range(b)],
                        "logits_sha256": hashlib.sha256(eng.logits(b).view(torch.int16).cpu().numpy().tobytes()).hexdigest(),
                        "replay_route": eng.replay_route(), "graph_replays": eng.stats()["graph_replays"]}
                prof = eng.profile_step(b)
                chk = eng.check_step(b)
                case.update({"launches": [prof["kinds"][k]["launches"] for k in eng.PROFILE_KINDS], "n_splits": prof["n_splits"],
                             "check_launches": chk["launches"], "check_n_splits": chk["n_splits"], "written_once_plan": chk["written_once_plan"]})
                out[f"{name}/{b}"] = case
                if log:
                    log(f"{name}/{b}: {case}")
            finally:
                eng.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "engine_lora_steps.json"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        all_models = models(tmp)
        table = record(all_models, log=lambda s: print(s, flush=True))
        again = record(all_models)
    if table != again:
        differ = {k: (table[k], again[k]) for k in table if table[k] != again[k]}
        raise SystemExit("not written: two recordings differ (first, second): " + json.dumps(differ, indent=1))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
    print(f"wrote {args.out} ({len(table)} cases, recorded twice)")


if __name__ == "__main__":
    main()
