"""min-p, typical-p and Mirostat v2 against the plain device sampler on one Qwen3-4B-shaped synthetic engine (the weights bench.py builds),
runs alternated in one process at one temperature: single-stream decode (128-token prompt, 256 steps in decode(N) calls) and 64 sequences
one step per call.  Prints one JSON line: ms per step (best of rounds) per setting, the difference to the sampled step without
truncation in microseconds, and the replay route each setting ran on.

    python tools/truncation_bench.py [--steps 256] [--rounds 3] [--batch 64] [--out profiles/truncation.json]

Under `rocprofv3 --kernel-trace` run it with TL_AQL=0 (the sampled step end is sample_step_end_kernel on either route): the run submits
more packets than the engine's 8,192-slot AQL ring holds, and the profiler's queue interception faults on the first submission that
wraps the ring.  (The --profile-rows runs of sampling_bench / logprobs_bench and bench.py's own rocprofv3 child stay below one ring.)"""

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
TEMPERATURE = 0.8
SETTINGS = {"sampled": {}, "min_p0.05": {"min_p": 0.05}, "typical0.9": {"typical_p": 0.9}, "mirostat_tau5": {"tau": 5.0}}
# ~12 us per pass of one workgroup over a 304 KB row; three to four passes plus the write
EXPECTED_US = [40, 60]


def kernel_times(V=151936, iters=50):
    """truncate_rows_kernel alone over caller rows (tl_truncate_rows), microseconds per launch by stream events: 1 and 64 rows of
    N(0, 2^2) logits with one token raised by 6 ("spread") and of N(0, 0.5^2) logits ("flat": the kept band crosses zero, where bf16 has
    128 keys per binade and the typical walk needs more rounds).  "copy" (temperature 0) is one read and one write of the row."""
    import tiny_llm_ext_hip as ext

    nan = float("nan")
    settings = {"copy": (0.0, 0.0, 1.0, nan), "min_p0.05": (TEMPERATURE, 0.05, 1.0, nan), "typical0.9": (TEMPERATURE, 0.0, 0.9, nan),
                "min_p0.05+typical0.9": (TEMPERATURE, 0.05, 0.9, nan), "mirostat_mu10": (TEMPERATURE, 0.0, 1.0, 10.0)}
    g = torch.Generator(device="cuda").manual_seed(1)
    out = {}
    for rows in (1, 64):
        spread = torch.randn((rows, V), generator=g, device="cuda") * 2.0
        spread[:, 1234] += 6.0
        for name, x in (("spread", spread.bfloat16()), ("flat", (torch.randn((rows, V), generator=g, device="cuda") * 0.5).bfloat16())):
            for s, p in settings.items():
                ext.truncate_rows(x, *p)
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(iters):
                    ext.truncate_rows(x, *p)
                t1.record()
                torch.cuda.synchronize()
                out[f"{name}_rows{rows}_{s}"] = round(t0.elapsed_time(t1) * 1e3 / iters, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the result (with \"measured\": true) to this file")
    args = ap.parse_args()
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "truncation_bench needs a GPU"
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
    B = args.batch
    eng = DecodeEngine(model, page_size=128, num_pages=(128 + args.steps + 256) // 128 * B + 8, max_batch=B, max_prefill_rows=128)
    prompt = [(7 * i + 3) % CFG["vocab_size"] for i in range(128)]
    routes = {}

    def start(n, setting):
        s = SETTINGS[setting]
        for i in range(n):
            eng.begin(i)
            eng.set_sampling(i, TEMPERATURE, seed=1 + i)
            if "tau" in s:
                eng.set_mirostat(i, s["tau"])
            elif s:
                eng.set_truncation(i, s.get("min_p", 0.0), s.get("typical_p", 1.0))
            eng.prefill(i, prompt)
        routes[setting] = eng.replay_route().split(":")[0]

    def stop(n):
        eng.synchronize()
        for i in range(n):
            eng.release(i)

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

    res = {f"single_{s}": [] for s in SETTINGS} | {f"batch{B}_{s}": [] for s in SETTINGS}
    for _ in range(args.rounds):
        for s in SETTINGS:
            res[f"single_{s}"].append(single(s))
        for s in SETTINGS:
            res[f"batch{B}_{s}"].append(batched(s))
    out = {"measured": True, "temperature": TEMPERATURE, "ms_per_step": {k: round(min(v), 4) for k, v in res.items()}}
    ms = out["ms_per_step"]
    out["added_us"] = {k: round((ms[k] - ms[k.split("_")[0] + "_sampled"]) * 1e3, 1) for k in ms if not k.endswith("_sampled")}
    out["expected_added_us_single"] = EXPECTED_US
    out["route"] = routes
    out["unit"] = "ms per step, best of rounds; added_us against the sampled step without truncation in the same process"
    eng.close()
    out["kernel_us"] = kernel_times()
    text = json.dumps(out)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
