"""LoRA adapters against the base step on one Qwen3-4B-shaped synthetic engine (the weights bench.py builds), every comparison inside
one process: ms per decode step at 1, 8 and 64 sequences with no adapter / one adapter slot among base slots / all slots on one rank-16
adapter / 8 distinct rank-16 adapters / all slots on one rank-64 adapter -- with the launches per step (captured graph nodes are not
readable from here: the adapter plan's added launches are counted from the plan, 8 per dense layer), the algorithmic adapter bytes per
step and the replay route -- and prefill tokens/s of a 2,048-token prompt with and without a rank-16 adapter.  The speed ratio against
the no-adapter step of the same process is RECORDED, not gated.  Prints one JSON line.

    python tools/lora_bench.py [--steps 64] [--rounds 3] [--out profiles/lora.json] [--bench-json FILE ...]

--bench-json: result lines of bench.py runs to fold in as the regression gate ("this commit" / "parent", interleaved on one box):
pairs LABEL=FILE, e.g. new=runs/new_1.json old=runs/old_1.json; the ranges of `value` per label go into the output."""

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
TARGETS = ("q", "k", "v", "o", "gate", "up", "down")
ADDED_LAUNCHES_PER_LAYER = 8  # shrink + expand around qkv, wo, gate|up and w_down (csrc/lora.h)


def make_adapter(rank, seed):
    from tiny_llm_hip.lora import LoraAdapter

    H, I = CFG["hidden_size"], CFG["intermediate_size"]
    q, kv = CFG["num_attention_heads"] * CFG["head_dim"], CFG["num_key_value_heads"] * CFG["head_dim"]
    shapes = {"q": (H, q), "k": (H, kv), "v": (H, kv), "o": (q, H), "gate": (H, I), "up": (H, I), "down": (I, H)}
    g = torch.Generator().manual_seed(seed)
    w = {}
    for layer in range(CFG["num_hidden_layers"]):
        for t in TARGETS:
            n_in, n_out = shapes[t]
            w[(layer, t)] = ((torch.randn((rank, n_in), generator=g) * 0.02).bfloat16(), (torch.randn((n_out, rank), generator=g) * 0.02).bfloat16())
    return LoraAdapter(rank=rank, scale=1.0, weights=w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result (with \"measured\": true) to this file")
    ap.add_argument("--bench-json", nargs="*", default=[], metavar="LABEL=FILE")
    args = ap.parse_args()
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "lora_bench needs a GPU"
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
    B = 64
    eng = DecodeEngine(model, page_size=128, num_pages=3 * B + 24, max_batch=B, max_prefill_rows=2048)
    r16 = [eng.load_lora(make_adapter(16, 10 + i)) for i in range(8)]
    r64 = eng.load_lora(make_adapter(64, 99))
    per_adapter_bytes = {16: make_adapter(16, 10).nbytes(), 64: None}
    per_adapter_bytes[64] = per_adapter_bytes[16] * 4
    prompt = [(7 * i + 3) % CFG["vocab_size"] for i in range(128)]
    cases = {
        "none": lambda i, n: None,
        "one_slot_r16": lambda i, n: r16[0] if i == 0 else None,
        "all_one_r16": lambda i, n: r16[0],
        "eight_r16": lambda i, n: r16[i % 8],
        "all_one_r64": lambda i, n: r64,
    }
    info = {}

    def step_ms(n, case):
        pick = cases[case]
        distinct = set()
        for i in range(n):
            eng.begin(i)
            a = pick(i, n)
            if a is not None:
                eng.set_lora(i, a)
                distinct.add(a)
            eng.prefill(i, prompt)
        route = eng.replay_route().split(":")[0]
        eng.decode(2, batch=n)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.decode(args.steps, batch=n)
        eng.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        for i in range(n):
            eng.release(i)
        info[f"{case}_x{n}"] = {"route": route, "added_launches_per_step": ADDED_LAUNCHES_PER_LAYER * CFG["num_hidden_layers"] if distinct else 0,
                                "adapter_bytes_per_step": sum(per_adapter_bytes[64 if a == r64 else 16] for a in distinct)}
        return ms

    res = {f"{c}_x{n}": [] for n in (1, 8, 64) for c in cases}
    for _ in range(args.rounds):
        for n in (1, 8, 64):
            for c in cases:
                res[f"{c}_x{n}"].append(step_ms(n, c))
    out = {"measured": True, "ms_per_step": {k: round(min(v), 4) for k, v in res.items()}, "cases": info}
    ms = out["ms_per_step"]
    out["ratio_to_no_adapter"] = {k: round(ms[k] / ms["none_x" + k.rsplit("_x", 1)[1]], 3) for k in ms if not k.startswith("none_")}
    out["added_launches_per_layer"] = ADDED_LAUNCHES_PER_LAYER
    out["base_step_bytes"] = eng.step_bytes(1)

    long_prompt = [(11 * i + 5) % CFG["vocab_size"] for i in range(2048)]
    pre = {"base": [], "r16": []}
    for _ in range(args.rounds):
        for name, a in (("base", None), ("r16", r16[0])):
            eng.begin(0)
            if a is not None:
                eng.set_lora(0, a)
            eng.synchronize()
            t0 = time.perf_counter()
            eng.prefill(0, long_prompt)
            eng.synchronize()
            pre[name].append(len(long_prompt) / (time.perf_counter() - t0))
            eng.release(0)
    out["prefill_2048_tokens_per_s"] = {k: round(max(v)) for k, v in pre.items()}
    out["lora_stats"] = eng.lora_stats()
    out["unit"] = "ms per step, best of rounds, 128-token contexts; ratios against the no-adapter step of the same process (recorded, not gated)"
    eng.close()
    gate = {}
    for item in args.bench_json:
        label, path = item.split("=", 1)
        line = [l for l in Path(path).read_text().splitlines() if l.startswith("{")][-1]
        gate.setdefault(label, []).append(json.loads(line)["value"])
    if gate:
        out["bench_py_single_stream"] = {k: {"runs": v, "min": min(v), "max": max(v)} for k, v in gate.items()}
    text = json.dumps(out)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
