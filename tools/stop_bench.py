"""What arming a slot with stop conditions costs, on Qwen3-4B-shaped synthetic engines (the weights bench.py builds), every setting
alternated in one process: ms per step for 1 and 64 sequences at 128-token prompts
    (a) unarmed on the default replay route, (b) unarmed on hipGraphLaunch (an engine made under TL_AQL=0),
    (c) every slot armed with 8 stop ids and 4 stop strings that never match (on the default engine: the plan keeps hipGraphLaunch).
(c) - (b) is the cost of the launch, (c) - (a) what arming really costs, the route included.  Also generate() of a 256-token budget whose
stop id falls near token 64, against the unarmed call.  Prints one JSON line.

    python tools/stop_bench.py [--steps 256] [--rounds 3] [--batch 64] [--out profiles/stop.json]"""

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip", ROOT / "tests"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

CFG = dict(hidden_size=2560, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128, intermediate_size=9728,
           vocab_size=151936, rope_theta=1000000, rms_norm_eps=1e-6, max_position_embeddings=40960, tie_word_embeddings=True)
# the yardstick beside (a) and (b): the Mirostat update, another single launch behind the step end that keeps hipGraphLaunch
# (profiles/truncation.json: added microseconds per step at 1 / 64 sequences)
MIROSTAT_ADDED_US = [86, 146]


def vocabulary(V):
    """Token i spells 3-6 lowercase letters derived from i; the stop strings below hold capitals, so none ever matches."""
    out = []
    for i in range(V):
        n, x, s = 3 + i % 4, i * 2654435761 % (1 << 32), bytearray()
        for _ in range(n):
            s.append(97 + x % 26)
            x //= 26
        out.append(bytes(s))
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

    assert torch.cuda.is_available(), "stop_bench needs a GPU"
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
    B, V = args.batch, CFG["vocab_size"]

    def engine(aql):
        old = os.environ.pop("TL_AQL", None)
        if not aql:
            os.environ["TL_AQL"] = "0"
        try:
            return DecodeEngine(model, page_size=128, num_pages=(128 + args.steps + 256) // 128 * B + 8, max_batch=B, max_prefill_rows=128)
        finally:
            os.environ.pop("TL_AQL", None)
            if old is not None:
                os.environ["TL_AQL"] = old

    engines = {"unarmed": engine(True), "unarmed_hipgraph": engine(False)}
    engines["armed"] = engines["unarmed"]
    eng = engines["armed"]
    eng.make_vocab(vocabulary(V))
    never = eng.make_stop_set([V - 1 - 7 * k for k in range(8)], [b"STOP", b"\n\nUser:", b"</Answer>", b"###END"])
    prompt = [(7 * i + 3) % V for i in range(128)]
    routes = {}

    def start(name, n):
        e = engines[name]
        for i in range(n):
            e.begin(i)
            if name == "armed":
                e.set_stop(i, never, 0)
            e.prefill(i, prompt)
        routes[name] = e.replay_route().split(":")[0]
        return e

    def finish(name, e, n):
        e.synchronize()
        if name == "armed":  # the figure is a step's only while every slot ran every step
            assert all(not e.stop_state(i).stopped for i in range(n)), "a slot stopped: choose other ids"
        for i in range(n):
            e.release(i)

    def single(name, calls=8):
        e = start(name, 1)
        e.decode(2, batch=1)
        e.synchronize()
        per = args.steps // calls
        t0 = time.perf_counter()
        for _ in range(calls):
            e.decode(per, batch=1)
        e.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / (per * calls)
        finish(name, e, 1)
        return ms

    def batched(name, steps=32):
        e = start(name, B)
        e.decode(2, batch=B)
        e.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            e.decode(1, batch=B)
        e.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        finish(name, e, B)
        return ms

    res = {f"single_{s}": [] for s in engines} | {f"batch{B}_{s}": [] for s in engines}
    for _ in range(args.rounds):
        for s in engines:
            res[f"single_{s}"].append(single(s))
        for s in engines:
            res[f"batch{B}_{s}"].append(batched(s))
    ms = {k: round(min(v), 4) for k, v in res.items()}
    out = {"measured": True, "ms_per_step": ms, "route": routes}
    out["launch_us"] = {k: round((ms[f"{k}_armed"] - ms[f"{k}_unarmed_hipgraph"]) * 1e3, 1) for k in ("single", f"batch{B}")}
    out["arming_us"] = {k: round((ms[f"{k}_armed"] - ms[f"{k}_unarmed"]) * 1e3, 1) for k in ("single", f"batch{B}")}
    out["yardstick_mirostat_added_us"] = MIROSTAT_ADDED_US

    # generate(): a 256-token budget whose stop id falls near token 64, against the unarmed call (which decodes all 256)
    full = eng.generate(prompt, 256)
    at = min((k for k in range(16, 256) if full[k] not in full[:k]), key=lambda k: abs(k - 63))
    early = eng.make_stop_set([full[at]])
    times = {"unarmed": [], "stop": []}
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        eng.generate(prompt, 256)
        times["unarmed"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        got = eng.generate(prompt, 256, stop=early)
        times["stop"].append((time.perf_counter() - t0) * 1e3)
        assert got == full[:at + 1]
    out["generate_ms"] = {"budget": 256, "stop_at_token": at + 1, "decode_block": 32, "unarmed": round(min(times["unarmed"]), 2),
                          "stop": round(min(times["stop"]), 2)}
    out["unit"] = "ms per step, best of rounds; launch_us = armed - unarmed on hipGraphLaunch, arming_us = armed - unarmed on the default route"
    for e in set(engines.values()):
        e.close()
    text = json.dumps(out)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
