"""Measure the FP8-activation prefill GEMM (csrc/gemm_fp8.h) against the two kernels prefill runs on today -> profiles/prefill_fp8.json.

Kernel level: the four projections of one Qwen3-4B layer (qkv, wo, gate|up, down) at 512 / 1,024 / 2,048 / 4,096 rows, in layer order so that every
launch meets weights the previous one did not touch; per row count the time of the four launches on the bf16 GEMM (tl_prefill_matmul_bf16), on the
W4 GEMM (tl_quantized_matmul) and on quantise + FP8 GEMM (the quantise launches INSIDE the FP8 time), device events around `iters` rounds after
`warmup`, the three routes alternating inside a round.  FLOP/s = 2 M N K over the four projections / time.
Engine level: a config-3-shaped prompt (8,192 tokens in 4,096-row chunks) through a Qwen3-4B-shaped engine with the option off and on, host clock
around prefill + synchronise.  A run without a GPU fails: nothing here falls back.

    python tools/prefill_fp8_bench.py [--rows 512 1024 2048 4096] [--layers 36] [--out profiles/prefill_fp8.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    sys.path.insert(0, str(p))

SHAPES = (("qkv", 6144, 2560, 0), ("wo", 2560, 4096, 1), ("gate_up", 19456, 2560, 2), ("down", 2560, 9728, 1))  # name, weight rows, columns, epilogue
FP8_PEAK_TFLOPS = 5033.0  # AMD's published dense FP8 matrix peak of the MI355X (twice the 2,516 of bf16)


def kernel_level(ext, torch, rows_list, warmup, iters):
    from tiny_llm_hip.synthetic import quantize

    dev = "cuda"
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    mats = []
    for name, n, k, epi in SHAPES:
        w = (torch.randn((n, k), generator=gen, device=dev, dtype=torch.float32) * 0.02).to(torch.bfloat16)
        packed, scales, biases = quantize(w)
        mats.append(dict(name=name, n=n, k=k, epi=epi, packed=packed, scales=scales, biases=biases,
                         bf16=ext.prefill_weights_bf16(packed, scales, biases), fp8=ext.prefill_weights_fp8(packed, scales, biases)))
    table = []
    for M in rows_list:
        acts = [torch.randn((M, m["k"]), generator=gen, device=dev, dtype=torch.float32).to(torch.bfloat16) for m in mats]
        res = [torch.randn((M, m["n"]), generator=gen, device=dev, dtype=torch.float32).to(torch.bfloat16) for m in mats]

        def run_bf16():
            for m, a, r in zip(mats, acts, res):
                ext.prefill_matmul_bf16(a, m["bf16"], epilogue=m["epi"], residual=r if m["epi"] == 1 else None)

        def run_w4():  # (plain store: the W4 GEMM's fused epilogues are engine-internal; its residual / SwiGLU passes are small against the product)
            for m, a in zip(mats, acts):
                ext.quantized_matmul(m["scales"], m["biases"], 128, 4, a, m["packed"], True)

        def run_fp8():
            for m, a, r in zip(mats, acts, res):
                ext.prefill_matmul_fp8(*ext.prefill_quantize_rows_fp8(a), m["fp8"], m["n"], epilogue=m["epi"], residual=r if m["epi"] == 1 else None)

        def run_fp8_gemm_only(q):
            for m, qr, r in zip(mats, q, res):
                ext.prefill_matmul_fp8(*qr, m["fp8"], m["n"], epilogue=m["epi"], residual=r if m["epi"] == 1 else None)

        quantised = [ext.prefill_quantize_rows_fp8(a) for a in acts]
        routes = {"bf16_gemm8": run_bf16, "w4_gemm": run_w4, "fp8_with_quantise": run_fp8, "fp8_gemm_only": lambda: run_fp8_gemm_only(quantised)}
        for _ in range(warmup):
            for f in routes.values():
                f()
        torch.cuda.synchronize()
        ms = {k: 0.0 for k in routes}
        for _ in range(iters):
            for k, f in routes.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                f()
                t1.record()
                t1.synchronize()
                ms[k] += t0.elapsed_time(t1) / iters
        flop = sum(2.0 * M * m["n"] * m["k"] for m in mats)
        row = {"rows": M, "ms": {k: round(v, 4) for k, v in ms.items()}, "tflops": {k: round(flop / (v * 1e-3) / 1e12, 1) for k, v in ms.items()}}
        row["fp8_share_of_fp8_peak"] = round(row["tflops"]["fp8_with_quantise"] / FP8_PEAK_TFLOPS, 3)
        table.append(row)
        print(json.dumps(row), flush=True)
    return table


def engine_level(torch, layers, prompt_len, chunk, repeats):
    import numpy as np

    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import QWEN3_CONFIGS, synthetic_qwen3

    cfg = dict(QWEN3_CONFIGS["qwen3-4b"], num_hidden_layers=layers)
    model = synthetic_qwen3(cfg, seed=1, device="cuda")
    prompt = [int(t) for t in np.random.default_rng(3).integers(1, cfg["vocab_size"], size=prompt_len)]
    out = {"layers": layers, "prompt_tokens": prompt_len, "chunk_rows": chunk}
    for name, flag in (("option_off", 0), ("option_on", 1)):
        eng = DecodeEngine(model, page_size=128, num_pages=prompt_len // 128 + 4, max_batch=1, max_prefill_rows=chunk, options={"prefill_fp8": flag})
        try:
            best = None
            for _ in range(repeats + 1):  # the first pass warms every shape
                eng.begin(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.prefill(0, prompt, chunk=chunk)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                eng.release(0)
                best = dt if best is None or _ == 1 else min(best, dt)
            out[name] = {"prefill_s": round(best, 5), "tokens_per_s": round(prompt_len / best, 1), "workspace_bytes": int(eng.stats()["workspace_bytes"])}
        finally:
            eng.close()
        print(json.dumps({name: out[name]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[512, 1024, 2048, 4096])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--prompt-len", type=int, default=8192)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "prefill_fp8.json"))
    args = ap.parse_args()
    import torch

    import tiny_llm_ext_hip as ext

    if not torch.cuda.is_available():
        raise SystemExit("prefill_fp8_bench: needs a GPU (nothing is measured without one)")
    ext.load_library(str(ROOT))
    result = {"what": "FP8-activation prefill GEMM against the bf16 GEMM and the W4 GEMM", "device": torch.cuda.get_device_name(0),
              "fp8_peak_tflops_published": FP8_PEAK_TFLOPS, "kernel_level": kernel_level(ext, torch, args.rows, args.warmup, args.iters),
              "engine_level": engine_level(torch, args.layers, args.prompt_len, args.chunk, args.repeats)}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
