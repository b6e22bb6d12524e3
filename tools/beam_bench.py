"""Beam search (tl_engine_beam_select / tl_engine_beam_reorder, csrc/beam.h) against its yardstick, on one Qwen3-4B-shaped synthetic
engine (the weights bench.py builds), 128-token pages, a 128-token prompt, 4 and 8 beams.  The feature has no parent to compare with, so
the yardstick is the plain greedy decode(1) of the same batch of slots IN THE SAME PROCESS: a beam step is that step plus the
selection and the reorder.  Per width:

    beam_step_ms     select + reorder + decode(1) over the group, wall clock per step, nothing synchronised but what the calls
                     synchronise themselves (the selection returns its records; a step on the AQL route returns drained)
    greedy_step_ms   decode(1) over the same slots at the same contexts + a stream synchronise, per step
    select_ms        the selection alone (upload of the scores, two launches, the records' copy, the synchronise)
    reorder_ms       the reorder alone + a stream synchronise (block-table pokes and one tail-copy launch per further child)
    shares           select_ms and reorder_ms over the phase-split step (which synchronises after every phase and is therefore
                     recorded beside beam_step_ms, not instead of it)

The beams follow the search's own rule without EOS ids: the next beams are the best B candidates, so parents fan out and die as in
a real search.  Everything is RECORDED, no threshold is asserted.  Writes profiles/beam.json and prints it as one JSON line; without
a GPU the file says "measured": false and why.

    python tools/beam_bench.py [--beams 4,8] [--steps 48]"""

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    sys.path.insert(0, str(p))

CFG = dict(hidden_size=2560, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128, intermediate_size=9728,
           vocab_size=151936, rope_theta=1000000, rms_norm_eps=1e-6, max_position_embeddings=40960, tie_word_embeddings=True)
PAGE, PROMPT = 128, 128


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def run_width(model, beams, steps, rng):
    from tiny_llm_hip.beam import beam_candidates
    from tiny_llm_hip.engine import DecodeEngine

    n_cand = beam_candidates(beams, 2)  # Qwen3 chat: two EOS ids
    eng = DecodeEngine(model, page_size=PAGE, num_pages=beams * 3 + 2, max_batch=beams, max_prefill_rows=2048)
    try:
        eng.begin(0)
        eng.prefill(0, [int(t) for t in rng.integers(0, CFG["vocab_size"], PROMPT)])
        cands = eng.beam_select(0, 1, [0.0], n_cand)[:beams]
        eng.beam_reorder(0, 1, [c[0] for c in cands], [c[1] for c in cands])
        eng.decode(1, batch=beams)
        scores = [c[2] for c in cands]
        distinct_parents, copies0 = [], eng.stats()["page_allocations"]

        def beam_step(split):
            nonlocal scores
            t0 = time.perf_counter()
            cands = eng.beam_select(0, beams, scores, n_cand)[:beams]
            t1 = time.perf_counter()
            eng.beam_reorder(0, beams, [c[0] for c in cands], [c[1] for c in cands])
            if split:
                eng.synchronize()
            t2 = time.perf_counter()
            eng.decode(1, batch=beams)
            eng.synchronize()
            t3 = time.perf_counter()
            scores = [c[2] for c in cands]
            distinct_parents.append(len({c[0] for c in cands}))
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3

        for _ in range(4):  # warm: the plan of this batch is captured, the scratch allocated
            beam_step(False)
        whole = [beam_step(False)[3] for _ in range(steps)]
        split = [beam_step(True) for _ in range(steps)]
        pages_taken = eng.stats()["page_allocations"] - copies0

        def greedy_step():
            t0 = time.perf_counter()
            eng.decode(1, batch=beams)
            eng.synchronize()
            return (time.perf_counter() - t0) * 1e3

        greedy_step()
        greedy = [greedy_step() for _ in range(steps)]
        select_ms, reorder_ms, split_ms = median([s[0] for s in split]), median([s[1] for s in split]), median([s[3] for s in split])
        return {"n_cand": n_cand, "steps": steps, "route": eng.replay_route(), "beam_step_ms": round(median(whole), 4),
                "greedy_step_ms": round(median(greedy), 4), "beam_over_greedy": round(median(whole) / median(greedy), 4),
                "phase_split_step_ms": round(split_ms, 4), "select_ms": round(select_ms, 4), "reorder_ms": round(reorder_ms, 4),
                "decode_ms": round(median([s[2] for s in split]), 4), "select_share": round(select_ms / split_ms, 4),
                "reorder_share": round(reorder_ms / split_ms, 4), "mean_distinct_parents": round(sum(distinct_parents) / len(distinct_parents), 3),
                "pages_taken_per_step": round(pages_taken / len(distinct_parents), 3), "context_at_end": eng.context_len(0)}
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="4,8")
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "beam.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    result = {"tool": "tools/beam_bench.py", "shape": {"model": "Qwen3-4B (synthetic weights)", "page_size": PAGE, "prompt_tokens": PROMPT},
              "unit": "ms of wall clock per step, median over the steps",
              "yardstick": "greedy decode(1) of the same slots in the same process (the feature has no parent)"}
    if not torch.cuda.is_available():
        result.update(measured=False, reason="no GPU in this process")
    else:
        from tiny_llm_hip.synthetic import synthetic_qwen3

        model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
        rng = np.random.default_rng(3)
        result.update(measured=True, widths={str(b): run_width(model, int(b), args.steps, rng) for b in args.beams.split(",")})
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
