"""Batched speculative sampling against its yardsticks on a Qwen3-4B-shaped synthetic engine (the weights bench.py builds), 128-token
contexts, one MI355X, all in one process; the method of tools/verify_batch_bench.py (warm-up, then the median of calls that end in a
device synchronisation, the arms of a shape alternating inside every round).

  (1) the acceptance launches alone at V = 151,936 for 1 / 8 / 64 rows (sequences of min(rows, 8) rows), each arm one C call
      over preallocated device arrays, enqueue to synchronise:
        greedy   tl_verify_accept_rows (verify_accept_kernel + scan; the routine allocates and uploads its descriptors per call)
        two_row  tl_spec_sample_rows over materialised one-hot draft rows (parent-commit code: the yardstick)
        point    tl_verify_sample_rows with no draft rows (verify_sample_kernel + scan; its sequences ride in the kernel arguments)
      The point pair reads half the bytes: its median must not exceed the two-row routine's at any row count.
  (2) the call: verify_batch_sampled (every slot at T = 0.8, top-k 50) against verify_batch (the same slots greedy) at 1x5, 8x5 and 12x5
      rows, with the spread (min, max) of each.  Expected: the difference of (1).
  (3) the round: lookup_propose(sampled) + verify_batch_sampled of 1x(1+4) and 8x(1+4) rows against the captured sampled step of equal
      sequences, and the accepted-per-proposal figure from which a round pays: (round / step - 1) / 4, as profiles/lookup.json reports it.
      Random weights do not repeat their prompt: acceptance is about zero, and no speed-up is claimed.

Prints one JSON line; --out also writes it (with "measured": true).

    python tools/verify_sampled_bench.py [--rounds 15] [--warmup 3] [--out profiles/verify_batch_sampled.json]"""

import argparse
import ctypes
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
CONTEXT = 128
V = CFG["vocab_size"]
SAMPLING = (0.8, 50, None)
SLOTS = 12


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(values, warmup):
    v = values[warmup:]
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def acceptance_launches(ext, rounds, warmup):
    lib = ext.lib()
    dev = "cuda"
    out = {}
    gen = torch.Generator(device=dev).manual_seed(1)
    for rows in (1, 8, 64):
        target = (torch.randn((rows, V), device=dev, generator=gen) * 2.0).bfloat16()
        # rows / n sequences of n = min(rows, 8) rows each, as a real pass has them: every row but a sequence's last carries a proposal --
        # the third most likely token of its row, so both branches occur -- and the last is a bonus row, in all three arms
        n = min(rows, 8)
        n_seqs = rows // n
        third = torch.argsort(target.float(), dim=1, descending=True)[:, 2].to(torch.int32)
        proposal = third.clone()
        proposal[n - 1::n] = -1
        tokens = torch.cat([torch.full((1,), 7, device=dev, dtype=torch.int32), proposal[:-1]]).clamp(min=0).contiguous()  # tokens[r + 1] = row r's proposal
        draft = torch.full((rows, V), -4.0, device=dev, dtype=torch.bfloat16)  # one-hot draft rows, materialised: 304 KB each
        draft[torch.arange(rows, device=dev), third.long()] = 9.0
        temp = torch.full((rows,), SAMPLING[0], device=dev)
        top_k = torch.full((rows,), SAMPLING[1], device=dev, dtype=torch.int32)
        top_p = torch.ones(rows, device=dev)
        zero_f, zero_i = torch.zeros(rows, device=dev), torch.zeros(rows, device=dev, dtype=torch.int32)
        seed = torch.arange(rows, device=dev, dtype=torch.int64)
        pos = torch.arange(1, rows + 1, device=dev, dtype=torch.int32)
        accept, alt = torch.zeros(rows, device=dev, dtype=torch.int32), torch.zeros(rows, device=dev, dtype=torch.int32)
        results = torch.zeros((rows, 9), device=dev, dtype=torch.int32)
        arr = lambda v: (ctypes.c_int * len(v))(*v)
        row0, lens, starts = arr([i * n for i in range(n_seqs)]), arr([n] * n_seqs), arr([CONTEXT] * n_seqs)
        stream = ext._stream()
        arms = {
            "greedy": lambda: lib.tl_verify_accept_rows(target.data_ptr(), V, n_seqs, row0, lens, tokens.data_ptr(), results.data_ptr(), stream),
            "two_row": lambda: lib.tl_spec_sample_rows(target.data_ptr(), draft.data_ptr(), rows, V, proposal.data_ptr(), temp.data_ptr(), top_k.data_ptr(),
                                                       top_p.data_ptr(), zero_f.data_ptr(), zero_i.data_ptr(), top_p.data_ptr(), seed.data_ptr(),
                                                       pos.data_ptr(), accept.data_ptr(), alt.data_ptr(), stream),
            "point": lambda: lib.tl_verify_sample_rows(target.data_ptr(), None, V, n_seqs, row0, lens, starts, tokens.data_ptr(), temp.data_ptr(),
                                                       top_k.data_ptr(), top_p.data_ptr(), seed.data_ptr(), 0.0, 0, 1.0, accept.data_ptr(), alt.data_ptr(),
                                                       results.data_ptr(), stream),
        }
        times = {k: [] for k in arms}
        for _ in range(warmup + rounds):
            for name, fn in arms.items():
                rc = []
                times[name].append(timed(lambda: rc.append(fn())))
                assert rc == [0], (name, rc)
        rec = {k: summary(v, warmup) for k, v in times.items()}
        rec["sequences_x_rows"] = f"{n_seqs}x{n}"
        rec["point_not_slower_than_two_row"] = rec["point"]["median_ms"] <= rec["two_row"]["median_ms"]
        rec["point_minus_greedy_ms"] = round(rec["point"]["median_ms"] - rec["greedy"]["median_ms"], 4)
        out[str(rows)] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result (with \"measured\": true) to this file")
    args = ap.parse_args()
    import tiny_llm_ext_hip as ext
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "verify_sampled_bench needs a GPU"
    result = {"tool": "tools/verify_sampled_bench.py", "shape": {"layers": CFG["num_hidden_layers"], "vocab": V, "context": CONTEXT},
              "method": {"rounds": args.rounds, "warmup": args.warmup,
                         "statistic": "median (min, max) ms per call ending in a device synchronisation, arms alternating inside a round"}}
    result["acceptance_launches"] = acceptance_launches(ext, 4 * args.rounds, args.warmup)
    eng = DecodeEngine(synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda"), page_size=128, num_pages=2 * SLOTS + 4, max_batch=SLOTS,
                       max_prefill_rows=128)
    try:
        period = 16
        prompts = [[(7 * (i % period) + 3 + 31 * s) % V for i in range(CONTEXT)] for s in range(SLOTS)]
        for s in range(SLOTS):
            eng.begin(s)
            eng.set_lookup(s)
            eng.prefill(s, prompts[s])
            eng.set_token(s, prompts[s][CONTEXT - period])  # the id the period continues with: every lookup finds 4 proposals
        eng.synchronize()

        def sampling(on, slots):
            for s in range(slots):
                eng.set_sampling(s, *(SAMPLING if on else (0.0, None, None)), 100 + s)

        def rewind(slots, n):
            for s in range(slots):
                eng.rewind(s, n)
                eng.set_token(s, prompts[s][CONTEXT - period])

        calls = {}
        for slots in (1, 8, 12):
            chunks = [(s, [prompts[s][CONTEXT - period + j] for j in range(5)]) for s in range(slots)]
            arms = {"verify_batch": [], "verify_batch_sampled": []}
            for _ in range(args.warmup + args.rounds):
                sampling(False, slots)
                arms["verify_batch"].append(timed(lambda: eng.verify_batch(chunks)))
                rewind(slots, 5)
                sampling(True, slots)
                arms["verify_batch_sampled"].append(timed(lambda: eng.verify_batch_sampled(chunks)))
                rewind(slots, 5)
            rec = {k: summary(v, args.warmup) for k, v in arms.items()}
            rec["difference_ms"] = round(rec["verify_batch_sampled"]["median_ms"] - rec["verify_batch"]["median_ms"], 4)
            calls[f"{slots}x5"] = rec
        result["call"] = calls

        rounds = {}
        accepted = proposed = 0
        for slots in (1, 8):
            sampling(True, slots)
            arms = {"round": [], "propose": [], "sampled_step": []}
            for _ in range(args.warmup + args.rounds):
                fed = []

                def one_round():
                    fed[:] = eng.lookup_propose(list(range(slots)), [5] * slots, 3, 1, 4, sampled=True)
                    return eng.verify_batch_sampled(list(enumerate(fed)))

                out = []
                arms["round"].append(timed(lambda: out.extend(one_round())))
                assert all(len(f) == 5 for f in fed), "every timed round carries 4 proposals per slot"
                accepted += sum(len(r) - 1 for r in out)
                proposed += 4 * slots
                rewind(slots, 5)
                arms["propose"].append(timed(lambda: eng.lookup_propose(list(range(slots)), [5] * slots, 3, 1, 4, sampled=True)))
                arms["sampled_step"].append(timed(lambda: eng.decode(1, batch=slots)))
                rewind(slots, 1)
            rec = {k: summary(v, args.warmup) for k, v in arms.items()}
            rec["break_even_accepted_per_proposal"] = round((rec["round"]["median_ms"] / rec["sampled_step"]["median_ms"] - 1.0) / 4.0, 3)
            rounds[f"{slots}x(1+4)"] = rec
        result["round"] = rounds
        result["acceptance_on_random_weights"] = {"accepted": accepted, "proposed": proposed,
                                                  "note": "random weights do not continue their prompt: no speed-up is claimed"}
    finally:
        eng.close()
    result["measured"] = True
    print(json.dumps(result))
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
