"""The experts of a MoE MLP on the three routes -- GEMV (tl_moe_experts_rows), grouped tile GEMM (tl_moe_experts_rows_grouped), decode-shaped
(tl_moe_experts_rows_decode) -- at decode row counts and the Qwen3-30B-A3B layer shape (128 experts, top 8, hidden 2,048, expert width
768), alternating in one process.

    python tools/moe_decode_bench.py [--out profiles/moe_decode.json] [--iters 50]

Ids: once from the device router over random logits, once skewed (half the rows on eight experts).  Times: the median of device-event
times after a warm-up of every shape.  The yardsticks are the two existing routes; beside each time stands the floor -- the bytes of
the distinct experts named over the measured copy rate of 6.29 TB/s -- and the fraction of it the new route reaches.  The derived
result is the smallest row count from which the new route beats the better existing route on both id sets at every larger count
measured: the recommended ``moe_decode_rows`` (null when it loses at the largest)."""

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    sys.path.insert(0, str(p))

E, K, D, I = 128, 8, 2048, 768
ROWS = [1, 2, 4, 8, 16, 32, 64]
COPY_RATE = 6.29e12  # bytes / s, the measured copy rate the floor is taken against
ROUTES = ("gemv", "grouped", "decode")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "moe_decode.json"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rows", default=",".join(str(r) for r in ROWS), help="row counts, comma separated (a kernel trace of one count)")
    args = ap.parse_args()
    rows_list = [int(r) for r in args.rows.split(",")]
    import torch

    import tiny_llm_ext_hip as ext

    ext.load_library(str(ROOT))
    lib, dev = ext.lib(), "cuda"
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def w4(out_dim, in_dim):  # random codes, scales and biases of plausible size: the timing does not depend on the values
        words = torch.randint(-2 ** 31, 2 ** 31 - 1, (E, out_dim, in_dim // 8), generator=gen, device=dev, dtype=torch.int32)
        scales = (torch.rand((E, out_dim, in_dim // 128), generator=gen, device=dev) * 0.01 + 0.002).to(torch.bfloat16)
        return words, scales, (scales.float() * -7.5).to(torch.bfloat16)

    gate, up, down = w4(I, D), w4(I, D), w4(D, I)
    w = ext.TlMoeWeights(ext.TlW4(), gate[0].data_ptr(), up[0].data_ptr(), down[0].data_ptr(), gate[1].data_ptr(), gate[2].data_ptr(),
                         up[1].data_ptr(), up[2].data_ptr(), down[1].data_ptr(), down[2].data_ptr(), E, K, I, 0)
    expert_bytes = 3 * (I * D // 2 + 2 * 2 * I * D // 128)  # W4 words, bf16 scales and biases of gate, up and down
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = [lib.tl_moe_experts_rows, lib.tl_moe_experts_rows_grouped, lib.tl_moe_experts_rows_decode]

    cases = []
    for rows in rows_list:
        for kind in ("router", "skewed"):
            logits = torch.randn((rows, E), generator=gen, device=dev).to(torch.bfloat16)
            if kind == "skewed":  # half the rows choose among eight experts only
                logits[: rows // 2, 8:] = -30.0
            ids, scores = ext.moe_route_rows(logits, K, True)
            xn = torch.randn((rows, D), generator=gen, device=dev).to(torch.bfloat16)
            h = torch.randn((rows, D), generator=gen, device=dev).to(torch.bfloat16)
            outs = [torch.empty_like(xn) for _ in ROUTES]
            nb = [lib.tl_moe_experts_workspace_bytes(rows, K, D, I), lib.tl_moe_grouped_workspace_bytes(rows, K, D, I, E),
                  lib.tl_moe_decode_workspace_bytes(rows, K, D, I)]
            ws = [torch.empty(n, dtype=torch.uint8, device=dev) for n in nb]

            def run(which, a=(xn, h, ids, scores, outs, ws, nb, rows)):
                xn, h, ids, scores, outs, ws, nb, rows = a
                ext.check(fn[which](xn.data_ptr(), h.data_ptr(), ids.data_ptr(), scores.data_ptr(), ctypes.byref(w), rows, D, outs[which].data_ptr(),
                                    ws[which].data_ptr(), nb[which], stream))

            hit = int((torch.bincount(ids.reshape(-1).long(), minlength=E) > 0).sum())
            cases.append(dict(rows=rows, ids=kind, run=run, experts_hit=hit, outs=outs))
    for c in cases:  # warm-up of every shape on every route; the new route's output against the GEMV route's on the same inputs
        for which in range(3):
            c["run"](which)
        torch.cuda.synchronize()
        c["max_abs_vs_gemv"] = float((c["outs"][2].float() - c["outs"][0].float()).abs().max())
    results = []
    for c in cases:
        times = [[], [], []]
        for _ in range(args.iters):
            for which in range(3):  # alternating
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                c["run"](which)
                t1.record()
                t1.synchronize()
                times[which].append(t0.elapsed_time(t1) * 1e3)
        us = [statistics.median(t) for t in times]
        floor_us = c["experts_hit"] * expert_bytes / COPY_RATE * 1e6
        results.append(dict(rows=c["rows"], ids=c["ids"], experts_hit=c["experts_hit"], gemv_us=round(us[0], 1), grouped_us=round(us[1], 1),
                            decode_us=round(us[2], 1), decode_us_min=round(min(times[2]), 1), speedup_vs_better=round(min(us[0], us[1]) / us[2], 3),
                            distinct_expert_bytes=c["experts_hit"] * expert_bytes, floor_us=round(floor_us, 1), fraction_of_floor=round(floor_us / us[2], 3),
                            decode_tb_per_s=round(c["experts_hit"] * expert_bytes / (us[2] * 1e-6) / 1e12, 2), max_abs_vs_gemv=c["max_abs_vs_gemv"]))
        print(json.dumps(results[-1]), flush=True)
    wins = {rows: all(r["speedup_vs_better"] > 1.0 for r in results if r["rows"] == rows) for rows in rows_list}
    recommended = None
    for rows in reversed(rows_list):
        if not wins[rows]:
            break
        recommended = rows
    doc = dict(measured=True, what="experts of one MoE MLP on three routes, same process, alternating: tl_moe_experts_rows (GEMV) and "
               "tl_moe_experts_rows_grouped (tile GEMM), the yardsticks, vs tl_moe_experts_rows_decode; times include the combine launch",
               shape=dict(num_experts=E, top_k=K, hidden=D, intermediate=I), timing=f"median of {args.iters} device-event times after a warm-up of every shape",
               floor="bytes of the distinct experts named / 6.29 TB/s (the measured copy rate)", device=torch.cuda.get_device_name(0), results=results,
               loses_at_rows=[rows for rows in rows_list if not wins[rows]], recommended_moe_decode_rows=recommended)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(f"recommended moe_decode_rows: {recommended}")


if __name__ == "__main__":
    main()
