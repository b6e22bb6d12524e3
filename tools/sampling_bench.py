"""Device sampling against greedy decode on one Qwen3-4B-shaped synthetic engine (the weights bench.py builds), runs alternated in one
process: single-stream decode (128-token prompt, 256 steps in decode(N) calls), 64 sequences one step per call, and the host loop main.py
ran before the device sampler (decode(1), copy the logits row, torch sampler, set_token) as the baseline.  Prints one JSON line.

    python tools/sampling_bench.py [--steps 256] [--rounds 3] [--profile-rows N]

--profile-rows N: only N rows, a few sampled steps -- for `rocprofv3 --kernel-trace --stats -- python tools/sampling_bench.py
--profile-rows 1` (the sampled step end is sample_step_end_kernel)."""

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
SETTINGS = {"greedy": None, "t0.7_k50_p0.9": (0.7, 50, 0.9), "t1.0": (1.0, None, None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--profile-rows", type=int, default=0)
    args = ap.parse_args()
    from tiny_llm_hip import make_sampler
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "sampling_bench needs a GPU"
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
    B = args.profile_rows or args.batch
    eng = DecodeEngine(model, page_size=128, num_pages=(128 + args.steps + 256) // 128 * B + 8, max_batch=B, max_prefill_rows=128)
    prompt = [(7 * i + 3) % CFG["vocab_size"] for i in range(128)]

    def start(n, setting):
        for i in range(n):
            eng.begin(i)
            if SETTINGS[setting]:
                t, k, p = SETTINGS[setting]
                eng.set_sampling(i, t, k, p, seed=1 + i)
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

    def host_loop(steps=64):
        sample = make_sampler(0.7, top_p=0.9, top_k=50)
        start(1, "greedy")
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            logits = eng.logits(1).float()
            token = int(sample(logits - torch.logsumexp(logits, dim=-1, keepdim=True))[0])
            eng.set_token(0, token)
            eng.decode(1, batch=1)
        eng.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        stop(1)
        return ms

    res = {f"single_{s}": [] for s in SETTINGS} | {f"batch{B}_{s}": [] for s in SETTINGS} | {"host_loop": []}
    for _ in range(args.rounds):
        for s in SETTINGS:
            res[f"single_{s}"].append(single(s))
        for s in SETTINGS:
            res[f"batch{B}_{s}"].append(batched(s))
        res["host_loop"].append(host_loop())
    out = {k: round(min(v), 4) for k, v in res.items()}
    out["unit"] = "ms per step (best of rounds)"
    out["route"] = eng.replay_route()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
