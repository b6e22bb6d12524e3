"""DRY and the n-gram ban (tl_engine_set_dry, csrc/dry.h) against the same sampled decode step without them, on one Qwen3-4B-shaped synthetic
engine (the weights bench.py builds), armed and unarmed alternated in one process:

  * one sequence and 64 sequences after 128-token prompts (nothing repeats in them: the walk finds few candidates);
  * one sequence at contexts of 1,024 and 16,384 tokens of a period-61 pattern (the walk grows with the context, and every 61st position
    is a candidate whose match runs to the cap of 64);
  * each on the engine's own replay route and on an engine that keeps hipGraphLaunch for every plan (TL_AQL=0): an armed plan always
    replays through hipGraphLaunch, so the second engine's difference is the launches' cost and the first one's adds the route's.

Every slot samples at T 0.7 / top-k 50 / top-p 0.9; an armed slot has DRY (0.8, 1.75, 2) and no_repeat_ngram 4 on.  Writes one JSON
object (ms per step, best of rounds) to --out.

    python tools/dry_bench.py [--steps 128] [--rounds 3] [--out profiles/dry.json]
    python tools/dry_bench.py --bench-json NEW.json ... --parent-json A.json B.json    (adds the headline bench.py comparison to --out)

--profile-rows N: only N armed rows at a 1,024-token context and a few steps -- for `rocprofv3 --kernel-trace --stats -- python
tools/dry_bench.py --profile-rows 1` (the launches are dry_record_kernel, dry_match_kernel and dry_apply_kernel)."""

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip", ROOT / "tests"):
    sys.path.insert(0, str(p))

CFG = dict(hidden_size=2560, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128, intermediate_size=9728,
           vocab_size=151936, rope_theta=1000000, rms_norm_eps=1e-6, max_position_embeddings=40960, tie_word_embeddings=True)
SAMPLING = (0.7, 50, 0.9)
DRY = dict(multiplier=0.8, base=1.75, allowed_length=2, range=0, no_repeat_ngram=4)
YARDSTICKS = ["profiles/stop.json (one launch behind the step end, hipGraphLaunch)", "profiles/truncation.json (one or two launches behind the lm_head)"]


def last_json_line(path):
    lines = [l for l in Path(path).read_text().splitlines() if l.strip().startswith("{")]
    return json.loads(lines[-1])


def headline(out_path, new, parents):
    """bench.py's headline value of this tree against two runs of the parent commit, built and run in the same visit, alternating"""
    doc = json.loads(Path(out_path).read_text()) if Path(out_path).exists() else {"tool": "tools/dry_bench.py"}
    n, p = [last_json_line(x) for x in new], [last_json_line(x) for x in parents]
    mine, vals = [x["value"] for x in n], [x["value"] for x in p]
    diff = sum(mine) / len(mine) - sum(vals) / len(vals)
    doc["headline_bench"] = {
        "command": "bench.py --gpus 1 --steps K --warmup W (the plans of an unarmed engine are unchanged)", "unit": n[0].get("unit", "tokens/s"),
        "this_tree_runs": mine, "this_tree_ms_per_step": [x.get("ms_per_step") for x in n], "parent_runs": vals,
        "parent_ms_per_step": [x.get("ms_per_step") for x in p], "parent_spread": round(max(vals) - min(vals), 3),
        "difference_of_means": round(diff, 3), "difference_inside_parent_spread": abs(diff) <= max(vals) - min(vals),
    }
    Path(out_path).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc["headline_bench"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--profile-rows", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dry.json"))
    ap.add_argument("--bench-json", nargs="*", default=[])
    ap.add_argument("--parent-json", nargs="*", default=[])
    args = ap.parse_args()
    if args.bench_json:
        return headline(args.out, args.bench_json, args.parent_json)

    import torch

    if not torch.cuda.is_available():  # nothing here may be stated from a CPU run
        Path(args.out).write_text(json.dumps({"tool": "tools/dry_bench.py", "measured": False, "why": "no MI355X in this process: the tool has not run",
                                              "yardsticks": YARDSTICKS}, indent=1) + "\n")
        return
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    V = CFG["vocab_size"]
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
    B = args.profile_rows or args.batch
    long_ctx = (1024,) if args.profile_rows else (1024, 16384)
    pages = max((128 + args.steps + 256) // 128 * B, (max(long_ctx) + args.steps + 256) // 128 + 1) + 8
    prompts = {128: [(7 * i + 3) % V for i in range(128)]}
    for n in long_ctx:
        prompts[n] = [(7 * (i % 61) + 3) % V for i in range(n)]

    def engine(route):
        old = os.environ.pop("TL_AQL", None)
        if route == "hipgraph":
            os.environ["TL_AQL"] = "0"
        try:
            return DecodeEngine(model, page_size=128, num_pages=pages, max_batch=B, max_prefill_rows=2048)
        finally:
            os.environ.pop("TL_AQL", None)
            if old is not None:
                os.environ["TL_AQL"] = old

    def start(eng, n, ctx, armed):
        for i in range(n):
            eng.begin(i)
            if armed:
                eng.set_dry(i, **DRY)
            eng.set_sampling(i, *SAMPLING, seed=1 + i)
            eng.prefill(i, prompts[ctx], chunk=2048)

    def stop(eng, n):
        eng.synchronize()
        for i in range(n):
            eng.release(i)

    def timed(eng, n, ctx, armed, steps):
        start(eng, n, ctx, armed)
        eng.decode(2, batch=n)
        eng.synchronize()
        t0 = time.perf_counter()
        if n == 1:  # decode(N) calls
            for _ in range(4):
                eng.decode(steps // 4, batch=1)
        else:       # one step per call, as a serving loop issues them
            for _ in range(steps):
                eng.decode(1, batch=n)
        eng.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / (steps // 4 * 4 if n == 1 else steps)
        route = eng.replay_route()
        stop(eng, n)
        return ms, route

    if args.profile_rows:
        eng = engine("default")
        start(eng, B, 1024, True)
        eng.decode(8, batch=B)
        stop(eng, B)
        eng.close()
        print(json.dumps({"profile_rows": B, "context": 1024}))
        return

    cases = [("single_128", 1, 128, args.steps), (f"batch{B}_128", B, 128, max(8, args.steps // 4)), ("single_1k", 1, 1024, args.steps)] + \
            [("single_16k", 1, 16384, args.steps)] * (16384 in long_ctx)
    doc = {"tool": "tools/dry_bench.py", "measured": True, "unit": "ms per step (best of rounds)", "sampling": list(SAMPLING), "dry": DRY,
           "ms_per_step": {}, "added_us": {}, "route": {}, "yardsticks": YARDSTICKS}
    for route in ("default", "hipgraph"):
        eng = engine(route)
        for name, n, ctx, steps in cases:
            res = {False: [], True: []}
            routes = {}
            try:
                for _ in range(args.rounds):
                    for armed in (False, True):  # alternating
                        ms, routes[armed] = timed(eng, n, ctx, armed, steps)
                        res[armed].append(ms)
            except RuntimeError as exc:  # (a shape this engine does not take: said, not hidden)
                doc["ms_per_step"][f"{route}_{name}"] = {"unarmed": None, "armed": None, "why": str(exc)}
                for i in range(n):
                    try:
                        eng.release(i)
                    except RuntimeError:
                        pass
                continue
            off, on = min(res[False]), min(res[True])
            doc["ms_per_step"][f"{route}_{name}"] = {"unarmed": round(off, 4), "armed": round(on, 4)}
            doc["added_us"][f"{route}_{name}"] = round((on - off) * 1e3, 1)
            doc["route"][f"{route}_{name}"] = {"unarmed": routes[False].split(":")[0], "armed": routes[True].split(":")[0]}
        eng.close()
    keep = json.loads(Path(args.out).read_text()) if Path(args.out).exists() else {}
    for k in ("headline_bench", "kernel_times_us"):  # (filled by the other invocations of the same visit)
        if k in keep:
            doc[k] = keep[k]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
