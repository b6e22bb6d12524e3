"""Batched speculative verification against its two yardsticks on Qwen3-4B-shaped synthetic engines (the weights bench.py builds for the
target, a 4-layer model of the same width as the draft), 128-token contexts, all in one process:

  new  ms per tl_engine_verify_batch call over (slots x tokens) = 1x2, 1x4, 1x8, 4x4, 8x4, 8x8, 16x4;
  (a)  the same rows through tl_engine_verify, one call per slot (the only way before; the entry point is unchanged);
  (b)  one tl_engine_decode step with batch = the row count (what the decode route costs for that many rows once it is captured: the
       ratio new / (b) is what eager launching and the un-fused hand-overs cost, the yardstick for a later captured version);
  and the draft's decode(k) time, from which the break-even tokens per round = (verify ms + draft ms) / single-sequence step ms.

The three arms of a shape alternate inside every round; each timed call ends in a synchronisation and is followed by the rewind that
restores the state (not timed).  Medians over --rounds rounds after --warmup warm rounds.  Prints one JSON line; --out also writes it
(with "measured": true).

    python tools/verify_batch_bench.py [--rounds 15] [--warmup 3] [--out profiles/verify_batch.json]"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

CFG = dict(hidden_size=2560, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128, intermediate_size=9728,
           vocab_size=151936, rope_theta=1000000, rms_norm_eps=1e-6, max_position_embeddings=40960, tie_word_embeddings=True)
DRAFT_LAYERS = 4
CONTEXT = 128
SHAPES = [(1, 2), (1, 4), (1, 8), (4, 4), (8, 4), (8, 8), (16, 4)]
SLOTS = 64


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result (with \"measured\": true) to this file")
    args = ap.parse_args()
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "verify_batch_bench needs a GPU"
    target = DecodeEngine(synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda"), page_size=128, num_pages=2 * SLOTS + 4, max_batch=SLOTS,
                          max_prefill_rows=128)
    draft = DecodeEngine(synthetic_qwen3(dict(CFG, num_hidden_layers=DRAFT_LAYERS), seed=1, sigma=0.02, device="cuda"), page_size=128,
                         num_pages=2 * 16 + 4, max_batch=16, max_prefill_rows=128)
    result = {"tool": "tools/verify_batch_bench.py",
              "shape": {"layers": CFG["num_hidden_layers"], "draft_layers": DRAFT_LAYERS, "vocab": CFG["vocab_size"], "context": CONTEXT},
              "method": {"rounds": args.rounds, "warmup": args.warmup, "statistic": "median ms per call, arms alternating inside a round",
                         "a": "tl_engine_verify, one call per slot, over the same rows", "b": "one tl_engine_decode step with batch = rows"}}
    try:
        for slot in range(SLOTS):
            target.begin(slot)
            target.prefill(slot, [(7 * i + 3 + slot) % CFG["vocab_size"] for i in range(CONTEXT)])
        for slot in range(16):
            draft.begin(slot)
            draft.prefill(slot, [(7 * i + 3 + slot) % CFG["vocab_size"] for i in range(CONTEXT)])
        target.synchronize()
        draft.synchronize()

        def rewind_all(engine, slots, n):
            for s in range(slots):
                engine.rewind(s, n)

        def step(engine, batch, steps=1):
            engine.decode(steps, batch=batch)
            engine.synchronize()

        single = []
        for i in range(args.warmup + args.rounds):
            single.append(timed(lambda: step(target, 1)))
            target.rewind(0, 1)
        single_ms = statistics.median(single[args.warmup:])
        result["single_sequence_step_ms"] = round(single_ms, 4)

        table = {}
        for slots, n in SHAPES:
            rows = slots * n
            chunks = [(s, [(11 * j + 5 + s) % CFG["vocab_size"] for j in range(n)]) for s in range(slots)]
            arms = {"verify_batch_ms": [], "verify_per_slot_ms": [], "decode_step_ms": [], "draft_decode_ms": []}
            for i in range(args.warmup + args.rounds):
                arms["verify_batch_ms"].append(timed(lambda: target.verify_batch(chunks)))
                rewind_all(target, slots, n)
                arms["verify_per_slot_ms"].append(timed(lambda: [target.verify(s, toks) for s, toks in chunks]))
                rewind_all(target, slots, n)
                arms["decode_step_ms"].append(timed(lambda: step(target, rows)))
                rewind_all(target, rows, 1)
                if n > 1:  # the draft proposes n - 1 tokens for each of the slots in one call
                    arms["draft_decode_ms"].append(timed(lambda: step(draft, slots, n - 1)))
                    rewind_all(draft, slots, n - 1)
            med = {k: round(statistics.median(v[args.warmup:]), 4) for k, v in arms.items() if v}
            med["rows"] = rows
            med["ratio_to_per_slot_verify"] = round(med["verify_batch_ms"] / med["verify_per_slot_ms"], 3)
            med["ratio_to_decode_step"] = round(med["verify_batch_ms"] / med["decode_step_ms"], 3)
            med["beats_per_slot_verify"] = med["verify_batch_ms"] < med["verify_per_slot_ms"]
            # a round costs one verification and one draft call and yields between 1 and n tokens per slot: the break-even tokens per
            # round against single-sequence steps, and -- for several slots -- per slot against plain batched steps over the same slots
            round_ms = med["verify_batch_ms"] + med.get("draft_decode_ms", 0.0)
            med["break_even_tokens_per_round"] = round(round_ms / single_ms, 3)
            if slots > 1:
                plain_step_ms = statistics.median([timed(lambda: step(target, slots)) for _ in range(5)][1:])
                rewind_all(target, slots, 5)
                med["plain_step_ms_same_slots"] = round(plain_step_ms, 4)
                med["break_even_tokens_per_slot_vs_batched_steps"] = round(round_ms / plain_step_ms, 3)
            table[f"{slots}x{n}"] = med
        result["shapes"] = table
        result["acceptance"] = {"1x4_beats_a": table["1x4"]["beats_per_slot_verify"], "1x8_beats_a": table["1x8"]["beats_per_slot_verify"],
                                "shapes_that_do_not_beat_a": [k for k, v in table.items() if not v["beats_per_slot_verify"]]}
    finally:
        target.close()
        draft.close()
    result["measured"] = True
    print(json.dumps(result))
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
