"""KV swap (csrc/kv_swap.h, tl_engine_park / tl_engine_unpark) against its two yardsticks, on one Qwen3-4B-shaped synthetic engine (the
weights bench.py builds), 128-token pages, bf16 and FP8 pages, contexts of 1k / 8k / 32k tokens.  In ONE process, per format and context:

    prefill      the context prefilled in 2,048-token chunks (after one unrecorded warm run): ms
    park         tl_engine_park of that slot, wall clock around the call + a stream synchronise: ms, GB/s of KV bytes moved
    unpark       tl_engine_unpark likewise
    recompute    the slot released and the same context prefilled again: the alternative to swapping, and the yardstick that decides
                 whether a swap is worth having at a given length (swap_vs_recompute = (park + unpark) / recompute)
    per_pool     (bf16 only) the same bytes, device to pinned host, by one hipMemcpyAsync per (page, pool) as tl_engine_fork's copy_page
                 would issue them (72 pools), over caller pools of the engine's shape -- beside tl_kv_gather_pages over the SAME pools
                 + one copy per 32 MiB group: the yardstick for the gather kernel

Everything is RECORDED, nothing asserted but the byte counts and that the resumed sequence continues with the ids of an uninterrupted
one.  Writes profiles/kv_swap.json and prints it as one JSON line.

    python tools/kv_swap_bench.py [--contexts 1024,8192,32768] [--formats bf16,fp8]"""

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CFG = dict(hidden_size=2560, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128, intermediate_size=9728,
           vocab_size=151936, rope_theta=1000000, rms_norm_eps=1e-6, max_position_embeddings=40960, tie_word_embeddings=True)
PAGE, CHUNK = 128, 2048
HIP_D2H = 2


def timed(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    fn()
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3


def per_pool_yardstick(ext, n_pages, repeats=3):
    """n_pages pages of 72 bf16 pools [pages][8][128][256 B], device to pinned host: one hipMemcpyAsync per (page, pool), and the gather
    launch + one copy per group over the same pools.  Median of `repeats`, ms."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    heads, row = CFG["num_key_value_heads"], CFG["head_dim"] * 2
    n_pools = 2 * CFG["num_hidden_layers"]
    page_bytes = heads * PAGE * row
    pools = [torch.randint(0, 256, (n_pages * page_bytes,), dtype=torch.uint8, device="cuda") for _ in range(n_pools)]
    record = n_pools * page_bytes
    host = torch.empty(n_pages * record, dtype=torch.uint8).pin_memory()
    stream = torch.cuda.current_stream().cuda_stream

    def per_pool():
        for j in range(n_pages):
            for i, pool in enumerate(pools):
                rc = hip.hipMemcpyAsync(host.data_ptr() + j * record + i * page_bytes, pool.data_ptr() + j * page_bytes, page_bytes, HIP_D2H, stream)
                assert rc == 0
        torch.cuda.synchronize()

    table = (ext.TlKvPoolDesc * n_pools)(*[ext.TlKvPoolDesc(p.data_ptr(), row) for p in pools])
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    offsets_dev = torch.arange(n_pools, dtype=torch.int64, device="cuda") * page_bytes
    ids_dev = torch.arange(n_pages, dtype=torch.int32, device="cuda")
    group = max(1, min(n_pages, (32 << 20) // record))
    staging = torch.empty(group * record, dtype=torch.uint8, device="cuda")

    def gathered():
        for j0 in range(0, n_pages, group):
            n = min(group, n_pages - j0)
            ext.check(ext.lib().tl_kv_gather_pages(table_dev.data_ptr(), offsets_dev.data_ptr(), n_pools, heads, PAGE, ids_dev.data_ptr() + 4 * j0, n,
                                                   PAGE, staging.data_ptr(), record, stream))
            assert hip.hipMemcpyAsync(host.data_ptr() + j0 * record, staging.data_ptr(), n * record, HIP_D2H, stream) == 0
        torch.cuda.synchronize()

    out = {}
    for name, fn in (("per_pool_memcpy", per_pool), ("gather_and_group_copy", gathered)):
        fn()  # warm
        times = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e3)
        ms = float(np.median(times))
        out[name] = {"ms": round(ms, 3), "gb_per_s": round(n_pages * record / ms / 1e6, 2)}
    out["per_pool_memcpy"]["memcpy_calls"] = n_pages * n_pools
    out["gather_and_group_copy"]["launches"] = (n_pages + group - 1) // group
    # the gathered copy holds the pools' bytes
    assert torch.equal(host[:page_bytes], pools[0][:page_bytes].cpu())
    assert torch.equal(host[(n_pages - 1) * record + (n_pools - 1) * page_bytes:], pools[-1][(n_pages - 1) * page_bytes:].cpu())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", default="1024,8192,32768")
    ap.add_argument("--formats", default="bf16,fp8")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kv_swap.json"))
    args = ap.parse_args()
    import tiny_llm_ext_hip as ext
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "kv_swap_bench needs a GPU"
    contexts = [int(c) for c in args.contexts.split(",")]
    pages = max(contexts) // PAGE + 2
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
    rng = np.random.default_rng(3)
    result = {"tool": "tools/kv_swap_bench.py", "measured": True, "shape": {"model": "Qwen3-4B", "page_size": PAGE, "prefill_chunk": CHUNK, "contexts": contexts},
              "unit": "ms of wall clock around the call + a stream synchronise; GB/s = KV bytes of the context's pages / ms",
              "yardsticks": ["recompute: re-prefill of the same context in the same process", "per_pool: one hipMemcpyAsync per (page, pool)"],
              "formats": {}}
    for fmt in args.formats.split(","):
        eng = DecodeEngine(model, page_size=PAGE, num_pages=pages, max_batch=2, max_prefill_rows=CHUNK, kv_format=fmt, swap_pages=pages)
        record = eng.swap_stats()["record_bytes"]
        rows = {"record_bytes": record, "route": eng.replay_route()}
        eng.begin(0)
        eng.prefill(0, [int(t) for t in rng.integers(0, CFG["vocab_size"], 1024)], chunk=CHUNK)  # warm
        eng.park(0)
        eng.unpark(0)
        eng.release(0)
        for ctx in contexts:
            tokens = [int(t) for t in rng.integers(0, CFG["vocab_size"], ctx)]
            n = (ctx + PAGE - 1) // PAGE
            eng.begin(0)
            prefill_ms = timed(eng, lambda: eng.prefill(0, tokens, chunk=CHUNK))
            eng.decode(4, batch=1)
            want = eng.read_tokens(0, 5)
            eng.rewind(0, 4)
            eng.set_token(0, want[0])
            before = eng.swap_stats()
            park_ms = timed(eng, lambda: eng.park(0))
            unpark_ms = timed(eng, lambda: eng.unpark(0))
            after = eng.swap_stats()
            assert after["pages_out"] - before["pages_out"] == n and after["pages_in"] - before["pages_in"] == n
            eng.decode(4, batch=1)
            assert eng.read_tokens(0, 4) == want[1:], "the resumed sequence does not continue like the uninterrupted one"
            eng.release(0)
            eng.begin(0)
            recompute_ms = timed(eng, lambda: eng.prefill(0, tokens, chunk=CHUNK))
            eng.release(0)
            moved = n * record
            rows[str(ctx)] = {"pages": n, "bytes": moved, "prefill_ms": round(prefill_ms, 3), "recompute_ms": round(recompute_ms, 3),
                              "park_ms": round(park_ms, 3), "park_gb_per_s": round(moved / park_ms / 1e6, 2),
                              "unpark_ms": round(unpark_ms, 3), "unpark_gb_per_s": round(moved / unpark_ms / 1e6, 2),
                              "swap_vs_recompute": round((park_ms + unpark_ms) / recompute_ms, 4)}
        eng.close()
        result["formats"][fmt] = rows
    del model
    torch.cuda.empty_cache()
    result["per_pool"] = {str(ctx): per_pool_yardstick(ext, (ctx + PAGE - 1) // PAGE) for ctx in contexts}
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
