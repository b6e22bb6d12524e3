"""Prompt-lookup speculative decoding (tl_engine_lookup_propose, csrc/lookup.h) measured three ways, every comparison inside one process:

  (a) the propose launch alone -- tl_lookup_rows, the engine launch's rule over caller rows -- for 1, 16 and 64 rows with 128-, 8,192- and
      32,768-id histories, against a numpy proposer over the same ids (and required to give the same proposals).  Two kinds of ids:
      "random" (the 151,936-id vocabulary: hardly a candidate) and "periodic" (period 61: every 61st position is a candidate whose
      compare runs to max_ngram);
  (b) one round -- tl_engine_lookup_propose plus tl_engine_verify_batch with k proposals per slot -- against one captured decode step
      over the same slots of the same Qwen3-4B-shaped synthetic engine (the weights bench.py builds), alternating.  So that EVERY timed
      round has k proposals per slot whatever the random weights answer, each slot's pending token is set to the id that continues its
      period-61 prompt, and the round undoes itself (verify_batch without commit, then the rewind and the set_token a commit would
      have issued, back to the state before: two host calls per slot, which a commit makes inside the library).  A round yields 1 + (accepted proposals) ids per slot and a step yields one, so lookup
      pays from the acceptance break_even = (ms_round / ms_step - 1) / k per proposal on;
  (c) tokens/s of lookup_generate_ids against batch_generate_ids on that engine over prompts that repeat themselves (period 61), with the
      acceptance that was observed -- on the random weights, whose own output nothing makes repeat the prompt, and on bench.py's PEAKED
      checkpoint (a larger embedding, damped residual writers, a permuted head), whose greedy output walks the head's permutation -- a cycle
      far longer than 128 ids, so nothing repeats there either.  Neither is a trained model on text that quotes its prompt; the one
      checkpoint whose output is known to repeat is the tiny one of tests/test_zz_lookup_gpu.py.

Writes one JSON object to --out.  No ratio is fixed in advance; the yardsticks are the same-process runs above.

    python tools/lookup_bench.py [--rounds 3] [--out profiles/lookup.json] [--skip-engine]"""

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip", ROOT / "tests"):
    sys.path.insert(0, str(p))

CFG = dict(hidden_size=2560, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128, intermediate_size=9728,
           vocab_size=151936, rope_theta=1000000, rms_norm_eps=1e-6, max_position_embeddings=40960, tie_word_embeddings=True)
PARAMS = dict(max_ngram=3, min_ngram=1, num_proposals=4)


def numpy_propose(T, s0, e, max_ngram, min_ngram, num_proposals):
    """The rule of csrc/lookup.h over T[s0 .. e], vectorised over the candidates."""
    import numpy as np

    cand = np.flatnonzero(T[s0:e] == T[e]) + s0
    if cand.size == 0:
        return []
    raw = np.ones(cand.size, dtype=np.int64)
    alive = np.ones(cand.size, dtype=bool)
    for j in range(1, max_ngram):
        if e - j < s0:
            break
        alive &= cand - j >= s0
        alive[alive] = T[cand[alive] - j] == T[e - j]
        raw += alive
    avail = np.minimum(num_proposals, e - cand)
    key = np.where(raw >= min_ngram, raw << 27 | avail << 24 | cand, 0)
    best = int(key.max())
    if best == 0:
        return []
    i, n = best & ((1 << 24) - 1), best >> 24 & 7
    return [int(t) for t in T[i + 1:i + 1 + n]]


def launch_alone(rounds):
    import numpy as np
    import torch
    import tiny_llm_ext_hip as ext

    out = {}
    rng = np.random.default_rng(0)
    for kind in ("random", "periodic"):
        for hist in (128, 8192, 32768):
            for rows in (1, 16, 64):
                if kind == "random":
                    ids = rng.integers(0, CFG["vocab_size"], size=(rows, hist), dtype=np.int32)
                else:
                    ids = np.stack([np.resize(rng.integers(0, CFG["vocab_size"], size=61, dtype=np.int32), hist) for _ in range(rows)])
                dev = torch.from_numpy(ids).cuda()
                start = torch.zeros(rows, dtype=torch.int32, device="cuda")
                end = torch.full((rows,), hist - 1, dtype=torch.int32, device="cuda")
                got_dev, counts_dev = ext.lookup_rows(dev, start, end, **PARAMS)
                got, counts = got_dev.cpu().numpy(), counts_dev.cpu().numpy()
                t0 = time.perf_counter()
                want = [numpy_propose(ids[r], 0, hist - 1, **PARAMS) for r in range(rows)]
                numpy_ms = (time.perf_counter() - t0) * 1e3
                equal = all(got[r, :counts[r]].tolist() == want[r] for r in range(rows))
                reps, best = 200, None
                stream = torch.cuda.current_stream().cuda_stream
                for _ in range(rounds):  # (the C entry point: the binding's own check of `end` reads it back)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        ext.check(ext.lib().tl_lookup_rows(dev.data_ptr(), rows, hist, start.data_ptr(), end.data_ptr(), PARAMS["max_ngram"], PARAMS["min_ngram"],
                                                           PARAMS["num_proposals"], got_dev.data_ptr(), counts_dev.data_ptr(), None, stream))
                    torch.cuda.synchronize()
                    us = (time.perf_counter() - t0) * 1e6 / reps
                    best = us if best is None else min(best, us)
                out[f"{kind}_{rows}x{hist}"] = {"launch_us": round(best, 2), "numpy_us": round(numpy_ms * 1e3, 1), "equal": bool(equal),
                                                "proposals": int(counts.sum())}
    return out


def engine_parts(rounds, k, peaked=False):
    import torch
    from tiny_llm_hip.engine import DecodeEngine, batch_generate_ids, lookup_generate_ids
    from tiny_llm_hip.synthetic import synthetic_qwen3

    V = CFG["vocab_size"]
    recipe = dict(embed_sigma=0.25, residual_gain=0.2, head_permutation=(48271, 11)) if peaked else {}  # (bench.py PEAKED_RECIPE)
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda", **recipe)
    B = 8
    eng = DecodeEngine(model, page_size=128, num_pages=(B + 1) * 16 + 8, max_batch=B + 1, max_prefill_rows=2048)
    prompt = [(7 * (i % 61) + 3) % V for i in range(1024)]
    doc = {"round_vs_step": {}, "generation": {}}

    def begin(n):
        for s in range(n):
            eng.begin(s)
            eng.set_lookup(s)
            eng.prefill(s, [(t + s) % V for t in prompt], chunk=2048)

    def end(n):
        eng.synchronize()
        for s in range(n):
            eng.release(s)

    for n in () if peaked else (1, B):
        steps, reps = [], []
        proposed = accepted = calls = 0
        propose_ms = []
        for _ in range(rounds):  # alternating
            begin(n)
            eng.decode(4, batch=n)
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(32):
                eng.decode(1, batch=n)
            eng.synchronize()
            steps.append((time.perf_counter() - t0) * 1e3 / 32)
            live = list(range(n))
            for s in live:  # the pending token continues the slot's pattern: every round finds a 3-gram and k ids behind it
                eng.set_token(s, (prompt[eng.context_len(s) % 61] + s) % V)

            def one_round():
                fed = eng.lookup_propose(live, [k + 1] * n, PARAMS["max_ngram"], PARAMS["min_ngram"], k)
                t2 = time.perf_counter()
                res = eng.verify_batch(list(zip(live, fed)))  # (synchronises)
                for s, f in zip(live, fed):  # what commit issues, here back to the state before the round
                    eng.rewind(s, len(f))
                    eng.set_token(s, f[0])
                return fed, res, t2

            for _ in range(2):  # warm: the verification scratch and its routes
                one_round()
            t0 = time.perf_counter()
            tp = 0.0
            for _ in range(16):
                t1 = time.perf_counter()
                fed, res, t2 = one_round()
                tp += t2 - t1
                proposed += sum(len(f) - 1 for f in fed)
                accepted += sum(len(r) - 1 for r in res)
                calls += 1
            eng.synchronize()
            reps.append((time.perf_counter() - t0) * 1e3 / 16)
            propose_ms.append(tp * 1e3 / 16)
            end(n)
        step, rnd = min(steps), min(reps)
        per_slot = proposed / max(calls * n, 1)
        doc["round_vs_step"][f"slots_{n}"] = {
            "ms_step": round(step, 4), "ms_round": round(rnd, 4), "ms_propose_call": round(min(propose_ms), 4), "k": k,
            "proposals_per_slot_and_round": round(per_slot, 2), "accepted_per_proposal": round(accepted / max(proposed, 1), 3),
            "break_even_accepted_per_proposal": round((rnd / step - 1) / max(per_slot, 1e-9), 3), "route": eng.replay_route().split(":")[0]}

    prompts = [[(t + s) % V for t in prompt[:256]] for s in range(4)]
    new = 128
    for _ in range(rounds):
        for name in ("plain", "lookup"):
            stats = {}
            eng.synchronize()
            t0 = time.perf_counter()
            if name == "plain":
                outs = [ids for _, ids in sorted(batch_generate_ids(eng, prompts, new, batch_size=4, prefill_step=2048))]
            else:
                outs = lookup_generate_ids(eng, prompts, new, proposal_length=k, max_ngram=PARAMS["max_ngram"], min_ngram=PARAMS["min_ngram"], stats=stats)
            eng.synchronize()
            dt = time.perf_counter() - t0
            rec = doc["generation"].setdefault(name, {"tokens_per_s": 0.0})
            rec["tokens_per_s"] = max(rec["tokens_per_s"], round(sum(len(o) for o in outs) / dt, 1))  # (prefill included, in both)
            rec["tokens"] = sum(len(o) for o in outs)
            doc["generation"]["_outs_" + name] = outs
            if stats:
                rec.update(stats, accepted_per_proposal=round(stats["accepted"] / max(stats["proposed"], 1), 3))
    doc["generation"]["note"] = "4 prompts of 256 ids (period 61), 128 new ids each; tokens/s include the prefill, in both loops; best of rounds"
    doc["generation"]["outputs_equal"] = bool(doc["generation"].pop("_outs_plain") == doc["generation"].pop("_outs_lookup"))
    eng.close()
    del model
    torch.cuda.empty_cache()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lookup.json"))
    args = ap.parse_args()

    import torch

    doc = {"tool": "tools/lookup_bench.py", "params": PARAMS}
    if not torch.cuda.is_available():  # nothing here may be stated from a CPU run
        doc.update(measured=False, why="no MI355X in this process: the tool has not run")
    else:
        doc.update(measured=True, launch_alone=launch_alone(args.rounds),
                   launch_alone_unit="us per call of tl_lookup_rows (best of rounds, 200 calls each, enqueue to synchronise) / us of the numpy proposer over all rows")
        if not args.skip_engine:
            doc.update(engine_parts(args.rounds, args.k))
            doc["generation"] = {"random_weights": doc["generation"], "peaked_checkpoint": engine_parts(args.rounds, args.k, peaked=True)["generation"]}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
