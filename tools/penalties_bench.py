"""Logit processing (repetition / presence / frequency penalties + a logit bias, on the device) against the same decode without it, on one
Qwen3-4B-shaped synthetic engine (the weights bench.py builds), settings alternated in one process: single-stream decode (128-token
prompt, 256 steps in decode(N) calls) and 64 sequences one step per call, greedy and T 0.7 / top-k 50 / top-p 0.9, each with processing
off and on (all three penalties + 16 bias entries), and the host loop the device path replaces (decode(1), copy the logits row, process
it in torch, set_token).  Prints one JSON line.

    python tools/penalties_bench.py [--steps 256] [--rounds 3] [--profile-rows N]

--profile-rows N: only N rows, a few processing steps -- for `rocprofv3 --kernel-trace --stats -- python tools/penalties_bench.py
--profile-rows 1` (the new launch is logit_process_kernel)."""

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
SAMPLING = {"greedy": None, "t0.7_k50_p0.9": (0.7, 50, 0.9)}
PENALTIES = (1.2, 0.5, 0.2)
BIAS = {1000 * i + 7: (-1.0) ** i * 0.5 * i for i in range(16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--profile-rows", type=int, default=0)
    args = ap.parse_args()
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "penalties_bench needs a GPU"
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
    B = args.profile_rows or args.batch
    eng = DecodeEngine(model, page_size=128, num_pages=(128 + args.steps + 256) // 128 * B + 8, max_batch=B, max_prefill_rows=128)
    prompt = [(7 * i + 3) % CFG["vocab_size"] for i in range(128)]

    def start(n, sampling, processing):
        for i in range(n):
            eng.begin(i)
            if processing:
                eng.set_penalties(i, *PENALTIES)
                eng.set_logit_bias(i, BIAS)
            if SAMPLING[sampling]:
                t, k, p = SAMPLING[sampling]
                eng.set_sampling(i, t, k, p, seed=1 + i)
            eng.prefill(i, prompt)

    def stop(n):
        eng.synchronize()
        for i in range(n):
            eng.release(i)

    if args.profile_rows:
        for sampling in SAMPLING:
            start(B, sampling, True)
            eng.decode(8, batch=B)
            stop(B)
        print(json.dumps({"profile_rows": B}))
        return

    def single(sampling, processing, calls=8):
        start(1, sampling, processing)
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

    def batched(sampling, processing, steps=32):
        start(B, sampling, processing)
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
        """the loop the device path replaces: greedy over the row processed in torch (the same rules, fp32)"""
        r, p, f = PENALTIES
        dev = torch.device("cuda")
        bias = torch.zeros(CFG["vocab_size"], device=dev)
        for t, v in BIAS.items():
            bias[t] = v
        seen = torch.zeros(CFG["vocab_size"], dtype=torch.bool, device=dev)
        seen[torch.tensor(prompt, device=dev)] = True
        count = torch.zeros(CFG["vocab_size"], device=dev)
        start(1, "greedy", False)
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            v = eng.logits(1).float()[0]
            v = torch.where(seen | (count > 0), torch.where(v > 0, v / r, v * r), v)
            v = v - f * count - p * (count > 0) + bias
            token = int(torch.argmax(v))
            count[token] += 1
            eng.set_token(0, token)
            eng.decode(1, batch=1)
        eng.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        stop(1)
        return ms

    keys = [(kind, s, on) for kind in ("single", f"batch{B}") for s in SAMPLING for on in (False, True)]
    res = {f"{kind}_{s}_{'processing' if on else 'off'}": [] for kind, s, on in keys} | {"host_loop": []}
    for _ in range(args.rounds):
        for kind, s, on in keys:
            res[f"{kind}_{s}_{'processing' if on else 'off'}"].append(single(s, on) if kind == "single" else batched(s, on))
        res["host_loop"].append(host_loop())
    out = {k: round(min(v), 4) for k, v in res.items()}
    out["unit"] = "ms per step (best of rounds)"
    out["route"] = eng.replay_route()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
