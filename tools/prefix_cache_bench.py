"""Cross-request prefix caching (csrc/prefix_cache.h, csrc/kv_copy.h) against the same serving loop without it, on one Qwen3-4B-shaped
synthetic engine (the weights bench.py builds): 64 decode slots, R requests of one shared prefix of S tokens + U unique tokens, 64 new
tokens each, through benches/serving.py:serve_requests with packed admission.  In ONE process, on ONE engine:

    warm     the cache-off run once, unrecorded (graph captures, first-use allocations)
    off      cache off: the code path of an engine that never heard of the cache -- the yardstick of everything below
    on       cache on, the same requests
    unique   cache on, R prompts of the same lengths that share nothing: the zero-hit overhead (lookups, registrations, retention
             and eviction with nothing gained), against `off`

The counters are exact and ASSERTED: prefill_tokens(on) == prefill_tokens(off) - tokens_matched, and tokens_matched >=
(R - 64) * floor(S / page) * page (every request admitted after the first wave finds the whole-page prefix).  Times are RECORDED, never
asserted: total and prefill tokens/s of each run, and -- on the populated cache -- the host time of one prefix_attach without and with
a tail copy (the call alone, and the call + a stream synchronise), beside tl_engine_fork copying the same 64-row tail through copy_page
(2 x layers whole-page hipMemcpyAsync calls: what a tail copy cost before kv_copy_rows_kernel).

Writes profiles/prefix_cache.json and prints it as one JSON line.

    python tools/prefix_cache_bench.py [--requests 128] [--shared 1024] [--unique 128] [--new-tokens 64]"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CFG = dict(hidden_size=2560, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128, intermediate_size=9728,
           vocab_size=151936, rope_theta=1000000, rms_norm_eps=1e-6, max_position_embeddings=40960, tie_word_embeddings=True)
PAGE, SLOTS, STAGING = 128, 64, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=128)
    ap.add_argument("--shared", type=int, default=1024)
    ap.add_argument("--unique", type=int, default=128)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--prefill-step", type=int, default=128)
    ap.add_argument("--prefill-budget", type=int, default=2048)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "prefix_cache.json"))
    args = ap.parse_args()
    from benches.serving import serve_requests
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "prefix_cache_bench needs a GPU"
    R, S, U, V = args.requests, args.shared, args.unique, CFG["vocab_size"]
    per_seq = (S + U + args.new_tokens + PAGE - 1) // PAGE
    num_pages = per_seq * (SLOTS + STAGING) + 2 * per_seq  # every live sequence, and a little to retain; the rest is evicted
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
    eng = DecodeEngine(model, page_size=PAGE, num_pages=num_pages, max_batch=SLOTS + STAGING, max_prefill_rows=args.prefill_budget)
    rng = np.random.default_rng(7)
    shared = [int(t) for t in rng.integers(0, V, S)]

    def requests(share):
        return [SimpleNamespace(prompt_token_ids=(shared if share else [int(t) for t in rng.integers(0, V, S)]) +
                                [int(t) for t in rng.integers(0, V, U)], max_new_tokens=args.new_tokens) for _ in range(R)]

    def run(reqs):
        before, pbefore = eng.stats(), eng.prefix_stats()
        eng.synchronize()
        t0 = time.perf_counter()
        m = serve_requests(eng, reqs, batch_size=SLOTS, prefill_step=args.prefill_step, prefill_budget=args.prefill_budget, page_size=PAGE,
                           staging_slots=STAGING)
        eng.synchronize()
        dt = time.perf_counter() - t0
        after, pafter = eng.stats(), eng.prefix_stats()
        prompt = sum(len(r.prompt_token_ids) for r in reqs)
        prefilled = after["prefill_tokens"] - before["prefill_tokens"]
        out = {"seconds": round(dt, 4), "prompt_tokens": prompt, "generated_tokens": m.generated_tokens, "prefill_tokens": prefilled,
               "total_tokens_per_s": round((prompt + m.generated_tokens) / dt, 1), "prefill_seconds": round(m.prefill_time, 4),
               "prompt_tokens_per_prefill_s": round(prompt / m.prefill_time, 1), "prefilled_tokens_per_prefill_s": round(prefilled / m.prefill_time, 1),
               "decode_step_median_ms": round(m.decode_step_median_ms, 4), "peak_active_requests": m.peak_active_requests}
        out.update({k: pafter[k] - pbefore[k] for k in ("lookups", "hits", "tokens_matched", "tail_rows_copied", "pages_registered", "pages_evicted")})
        out["pages_retained_at_end"] = pafter["pages_retained"]
        assert after["pages_in_use"] == 0 and after["pages_in_use"] + after["pages_free"] + pafter["pages_retained"] == num_pages
        return out

    reqs = requests(True)
    run(reqs)  # warm
    result = {"tool": "tools/prefix_cache_bench.py", "shape": {"requests": R, "shared": S, "unique": U, "new_tokens": args.new_tokens, "slots": SLOTS,
              "staging_slots": STAGING, "page_size": PAGE, "num_pages": num_pages, "prefill_step": args.prefill_step, "prefill_budget": args.prefill_budget},
              "route": eng.replay_route(), "unit": "seconds of wall clock per run of serve_requests; tokens/s = (prompt + generated) / seconds"}
    result["off"] = run(reqs)
    eng.set_prefix_cache(True)
    result["on"] = run(reqs)
    # the exact counters
    on, off = result["on"], result["off"]
    assert off["lookups"] == 0 and off["prefill_tokens"] == off["prompt_tokens"]
    assert on["prefill_tokens"] == off["prefill_tokens"] - on["tokens_matched"], (on, off)
    assert on["tokens_matched"] >= (R - SLOTS) * (S // PAGE) * PAGE, on
    assert on["lookups"] == R and on["generated_tokens"] == off["generated_tokens"]

    # one attach on the populated cache: whole pages only, then whole pages + a 64-row tail; and the fork that copies such a tail
    def timed(fn, n=20):
        host, synced = [], []
        for _ in range(n):
            eng.synchronize()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            eng.synchronize()
            t2 = time.perf_counter()
            host.append((t1 - t0) * 1e6)
            synced.append((t2 - t0) * 1e6)
            eng.release(0)
        return {"host_us_median": round(statistics.median(host), 2), "host_us_min": round(min(host), 2),
                "with_synchronize_us_median": round(statistics.median(synced), 2)}

    fresh = [int(t) for t in rng.integers(0, V, U)]
    no_tail = shared[:S // PAGE * PAGE] + fresh
    half = PAGE // 2
    published = shared[:S // PAGE * PAGE] + [int(t) for t in rng.integers(0, V, PAGE)]  # one more full page behind the shared ones, cached now
    eng.begin(0)
    eng.prefill(0, published[eng.prefix_attach(0, published):], chunk=args.prefill_step, want_logits=False)
    eng.release(0)
    with_tail = published[:S // PAGE * PAGE + half] + fresh

    def attach(tokens, want):
        def go():
            eng.begin(0)
            got = eng.prefix_attach(0, tokens)
            assert got == want, (got, want)
        return go

    micro = {"attach_whole_pages": timed(attach(no_tail, S // PAGE * PAGE))}
    micro["attach_with_tail_copy"] = timed(attach(with_tail, S // PAGE * PAGE + half))
    micro["attach_with_tail_copy"]["rows"] = half
    eng.begin(1)
    eng.prefix_attach(1, with_tail)  # slot 1: S + 64 tokens, its last page partly filled

    def fork():
        eng.fork(1, 0)
    micro["fork_copy_page_same_tail"] = timed(fork)
    micro["fork_copy_page_same_tail"]["memcpy_calls"] = 2 * CFG["num_hidden_layers"]
    eng.release(1)
    result["microseconds"] = micro

    eng.prefix_clear()
    result["unique"] = run(requests(False))
    assert result["unique"]["tokens_matched"] <= R  # nothing to find but a chance first token
    result["zero_hit_overhead_vs_off"] = round(result["unique"]["seconds"] / off["seconds"] - 1.0, 4)
    result["speedup_on_vs_off"] = round(off["seconds"] / on["seconds"], 3)
    eng.close()
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
