"""Per-token log-probabilities and prompt scoring against plain decode / prefill on one Qwen3-4B-shaped synthetic engine (the weights
bench.py builds), settings alternated in one process: single-stream decode (128-token prompt, 256 steps in decode(N) calls) and 64
sequences one step per call, greedy against logprobs with top-N 0 and 20; then prefill tokens/s against score tokens/s for 4,096- and
8,192-token prompts in 4,096-token chunks.  Prints one JSON line.

    python tools/logprobs_bench.py [--steps 256] [--rounds 3]

--profile-rows N: only N rows, a few recorded steps -- for `rocprofv3 --kernel-trace --stats -- python tools/logprobs_bench.py
--profile-rows 1` (the recording step end is logprob_step_end_kernel)."""

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip", ROOT / "tests"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

CFG = dict(hidden_size=2560, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128, intermediate_size=9728,
           vocab_size=151936, rope_theta=1000000, rms_norm_eps=1e-6, max_position_embeddings=40960, tie_word_embeddings=True)
SETTINGS = {"greedy": None, "lp0": 0, "lp20": 20}
CHUNK = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--profile-rows", type=int, default=0)
    ap.add_argument("--no-score", action="store_true")
    args = ap.parse_args()
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "logprobs_bench needs a GPU"
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
    B = args.profile_rows or args.batch
    pages = max((128 + args.steps + 256) // 128 * B, 8192 // 128 + 4) + 8
    eng = DecodeEngine(model, page_size=128, num_pages=pages, max_batch=B, max_prefill_rows=CHUNK)
    prompt = [(7 * i + 3) % CFG["vocab_size"] for i in range(128)]

    def start(n, setting):
        for i in range(n):
            eng.begin(i)
            if SETTINGS[setting] is not None:
                eng.set_logprobs(i, SETTINGS[setting])
            eng.prefill(i, prompt)

    def stop(n):
        eng.synchronize()
        for i in range(n):
            eng.release(i)

    if args.profile_rows:
        for setting in SETTINGS:
            start(B, setting)
            eng.decode(8, batch=B)
            stop(B)
        print(json.dumps({"profile_rows": B}))
        return

    def single(setting, calls=8):
        start(1, setting)
        eng.decode(2, batch=1)
        eng.synchronize()
        t0 = time.perf_counter()
        per = args.steps // calls
        for _ in range(calls):
            eng.decode(per, batch=1)
        eng.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / (per * calls)
        stop(1)
        return ms

    def batched(setting, steps=32):
        start(B, setting)
        eng.decode(2, batch=B)
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.decode(1, batch=B)
        eng.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        stop(B)
        return ms

    def prefill_rate(n):
        toks = [(11 * i + 5) % CFG["vocab_size"] for i in range(n)]
        eng.begin(0)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.prefill(0, toks, chunk=CHUNK)
        eng.synchronize()
        dt = time.perf_counter() - t0
        eng.release(0)
        return n / dt

    def score_rate(n):
        toks = [(11 * i + 5) % CFG["vocab_size"] for i in range(n)]
        eng.synchronize()
        t0 = time.perf_counter()
        eng.score(toks, chunk=CHUNK)
        return n / (time.perf_counter() - t0)

    res = {f"single_{s}": [] for s in SETTINGS} | {f"batch{B}_{s}": [] for s in SETTINGS}
    lens = [] if args.no_score else [4096, 8192]
    for n in lens:
        res[f"prefill_{n}"], res[f"score_{n}"] = [], []
        prefill_rate(n), score_rate(n)  # warm-up
    for _ in range(args.rounds):
        for s in SETTINGS:
            res[f"single_{s}"].append(single(s))
        for s in SETTINGS:
            res[f"batch{B}_{s}"].append(batched(s))
        for n in lens:
            res[f"prefill_{n}"].append(prefill_rate(n))
            res[f"score_{n}"].append(score_rate(n))
    out = {k: round(min(v), 4) if not k.startswith(("prefill", "score")) else round(max(v)) for k, v in res.items()}
    out["unit"] = "ms per step (best of rounds); prefill / score: tokens/s (best of rounds)"
    out["route"] = eng.replay_route()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
