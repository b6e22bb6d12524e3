"""The experts of a MoE MLP on the GEMV route (tl_moe_experts_rows) against the grouped-expert route (tl_moe_experts_rows_grouped) at the
Qwen3-30B-A3B layer shape (128 experts, top 8, hidden 2,048, expert width 768), alternating in one process.

    python tools/moe_grouped_bench.py [--out profiles/moe_grouped.json] [--iters 20]

Ids: once from the device router over random logits, once skewed (half the rows on eight experts).  Times: the median of device-event
times after a warm-up of every shape.  Beside each time the counted weight bytes of both routes (GEMV: every expert row reads its
expert; grouped: every tile of at most TM rows reads its expert) and the grouped kernels' FLOP/s.  The yardstick is the GEMV route in
the same process; the derived result is the smallest row count from which the grouped route wins on both id sets at every larger
count measured -- the recommended ``moe_grouped_rows``."""

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
ROWS = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "moe_grouped.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", default=",".join(str(r) for r in ROWS), help="row counts, comma separated (a kernel trace of one count)")
    args = ap.parse_args()
    rows_list = [int(r) for r in args.rows.split(",")]
    import torch

    import tiny_llm_ext_hip as ext

    ext.load_library(str(ROOT))
    lib, dev = ext.lib(), "cuda"
    TM = lib.tl_moe_grouped_tile_rows()
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

    def ids_for(rows, kind):
        logits = torch.randn((rows, E), generator=gen, device=dev).to(torch.bfloat16)
        if kind == "skewed":  # half the rows choose among eight experts only
            logits[: rows // 2, 8:] = -30.0
        ids, scores = ext.moe_route_rows(logits, K, True)
        return ids, scores

    cases = []
    for rows in rows_list:
        for kind in ("router", "skewed"):
            ids, scores = ids_for(rows, kind)
            xn = torch.randn((rows, D), generator=gen, device=dev).to(torch.bfloat16)
            h = torch.randn((rows, D), generator=gen, device=dev).to(torch.bfloat16)
            out = torch.empty_like(xn)
            nb = [lib.tl_moe_experts_workspace_bytes(rows, K, D, I), lib.tl_moe_grouped_workspace_bytes(rows, K, D, I, E)]
            ws = [torch.empty(n, dtype=torch.uint8, device=dev) for n in nb]
            fn = [lib.tl_moe_experts_rows, lib.tl_moe_experts_rows_grouped]

            def run(which, a=(xn, h, ids, scores, out, ws, nb, rows)):
                xn, h, ids, scores, out, ws, nb, rows = a
                ext.check(fn[which](xn.data_ptr(), h.data_ptr(), ids.data_ptr(), scores.data_ptr(), ctypes.byref(w), rows, D, out.data_ptr(),
                                    ws[which].data_ptr(), nb[which], stream))

            counts = torch.bincount(ids.reshape(-1).long(), minlength=E).cpu()
            tiles = int(((counts + TM - 1) // TM).sum())
            cases.append(dict(rows=rows, ids=kind, run=run, experts_hit=int((counts > 0).sum()), tiles=tiles))
    for c in cases:  # warm-up of every shape on both routes
        for which in (0, 1):
            c["run"](which)
    torch.cuda.synchronize()
    results = []
    for c in cases:
        times = [[], []]
        for _ in range(args.iters):
            for which in (0, 1):  # alternating
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                c["run"](which)
                t1.record()
                t1.synchronize()
                times[which].append(t0.elapsed_time(t1) * 1e3)
        gemv_us, grouped_us = statistics.median(times[0]), statistics.median(times[1])
        rows = c["rows"]
        results.append(dict(rows=rows, ids=c["ids"], experts_hit=c["experts_hit"], tiles=c["tiles"], gemv_us=round(gemv_us, 1), grouped_us=round(grouped_us, 1),
                            speedup=round(gemv_us / grouped_us, 3), gemv_weight_bytes=rows * K * expert_bytes, grouped_weight_bytes=c["tiles"] * expert_bytes,
                            grouped_tflops=round(2.0 * rows * K * 3 * I * D / (grouped_us * 1e-6) / 1e12, 2)))
        print(json.dumps(results[-1]))
    wins = {rows: all(r["speedup"] > 1.0 for r in results if r["rows"] == rows) for rows in rows_list}
    recommended = None
    for rows in reversed(rows_list):
        if not wins[rows]:
            break
        recommended = rows
    doc = dict(measured=True, what="experts of one MoE MLP: tl_moe_experts_rows (GEMV route, the yardstick) vs tl_moe_experts_rows_grouped, same process, alternating",
               shape=dict(num_experts=E, top_k=K, hidden=D, intermediate=I, tile_rows=TM), timing=f"median of {args.iters} device-event times after a warm-up of every shape",
               device=torch.cuda.get_device_name(0), results=results, recommended_moe_grouped_rows=recommended,
               wins_by_256_rows=bool(recommended is not None and recommended <= 256))
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(f"recommended moe_grouped_rows: {recommended}")


if __name__ == "__main__":
    main()
