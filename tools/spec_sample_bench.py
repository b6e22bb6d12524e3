"""Speculative sampling against its yardsticks on Qwen3-4B-shaped synthetic engines (the weights bench.py builds for the target, a
4-layer model of the same width as the draft), all in one process:

  (a) ms per verify_sampled call at n = 2, 4, 8 rows against tl_engine_verify at the same n on a greedy twin slot -- the difference
      is what the one new launch (and its parameter copy) costs;
  (b) ms for k draft steps as k one-step decode calls plus row copies against one decode(k) call, k = 3, 7;
  (c) the acceptance and residual-draw shares of speculative_generate_ids(temperature = 0.8) with this draft.  Random weights make the
      two models unrelated, so (c) says nothing about a real draft: it only shows the loop running.

Prints one JSON line; --out also writes it (with "measured": true).

    python tools/spec_sample_bench.py [--rounds 20] [--out profiles/spec_sample.json]"""

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
DRAFT_LAYERS = 4
SAMPLING = (0.8, 50, 0.95)
PROMPT_LEN = 128


def best_ms(fn, undo, rounds):
    """Best wall time of fn() over `rounds` runs, each followed by undo(); fn synchronises."""
    best = float("inf")
    for _ in range(rounds + 2):  # (two warm runs: captures, first-use allocations)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
        undo()
    return round(best * 1e3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the result (with \"measured\": true) to this file")
    args = ap.parse_args()
    from tiny_llm_hip.engine import DecodeEngine, speculative_generate_ids
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "spec_sample_bench needs a GPU"
    target = DecodeEngine(synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda"), page_size=128, num_pages=16, max_batch=2, max_prefill_rows=128)
    draft = DecodeEngine(synthetic_qwen3(dict(CFG, num_hidden_layers=DRAFT_LAYERS), seed=1, sigma=0.02, device="cuda"), page_size=128,
                         num_pages=16, max_batch=1, max_prefill_rows=128)
    prompt = [(7 * i + 3) % CFG["vocab_size"] for i in range(PROMPT_LEN)]
    T, k, p = SAMPLING
    result = {"tool": "tools/spec_sample_bench.py", "shape": {"layers": CFG["num_hidden_layers"], "draft_layers": DRAFT_LAYERS,
                                                             "vocab": CFG["vocab_size"], "prompt": PROMPT_LEN, "sampling": list(SAMPLING)}}
    try:
        # slot 0 samples, slot 1 is its greedy twin; the draft samples
        for slot in (0, 1):
            target.begin(slot)
            if slot == 0:
                target.set_sampling(0, T, k, p, 1)
            target.prefill(slot, prompt)
        draft.begin(0)
        draft.set_sampling(0, T, k, p, 2)
        draft.prefill(0, prompt, want_logits=False)
        rows = draft.logits_buffer(7)
        token = target.read_tokens(0, 1)[0]

        def draft_steps(n):
            draft.set_token(0, token)
            for i in range(n):
                draft.decode(1, batch=1)
                draft.copy_logits_into(rows[i], 1)
            return draft.read_tokens(0, n)

        verify = {}
        for n in (2, 4, 8):
            fed = [token] + draft_steps(n - 1)
            draft.rewind(0, n - 1)
            sampled = best_ms(lambda: target.verify_sampled(0, fed, rows, SAMPLING), lambda: target.rewind(0, n), args.rounds)
            greedy = best_ms(lambda: target.verify(1, fed), lambda: target.rewind(1, n), args.rounds)
            verify[f"n{n}"] = {"verify_sampled_ms": sampled, "verify_greedy_ms": greedy, "difference_us": round((sampled - greedy) * 1e3, 1)}
        result["verify"] = verify
        stepping = {}
        for n in (3, 7):
            one_by_one = best_ms(lambda: draft_steps(n), lambda: draft.rewind(0, n), args.rounds)

            def fused():
                draft.set_token(0, token)
                draft.decode(n, batch=1)
                draft.read_tokens(0, n)

            stepping[f"k{n}"] = {"one_step_calls_with_copies_ms": one_by_one, "one_decode_call_ms": best_ms(fused, lambda: draft.rewind(0, n), args.rounds)}
        result["draft_stepping"] = stepping
        for slot in (0, 1):
            target.release(slot)
        draft.release(0)
        stats = {}
        t0 = time.perf_counter()
        out = speculative_generate_ids(target, draft, prompt, 128, proposal_length=4, temperature=T, top_k=k, top_p=p, seed=3, stats=stats)
        result["generate"] = {"tokens": len(out), "seconds": round(time.perf_counter() - t0, 4), **stats,
                              "acceptance": round(stats["accepted"] / max(stats["proposed"], 1), 4),
                              "residual_draw_share_of_rounds": round(stats["resampled"] / max(stats["target_calls"] - 1, 1), 4),
                              "note": "random weights: the draft is unrelated to the target, the acceptance rate means nothing"}
    finally:
        target.close()
        draft.close()
    result["measured"] = True
    print(json.dumps(result))
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
