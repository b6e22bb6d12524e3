"""The device W4 quantiser (tl_quantize_w4, csrc/quantize_w4.h) on the matrices of Qwen3-4B -- 2560->9728, 9728->2560, 2560->4096,
4096->2560 and the 151,936 x 2,560 table, bf16 sources -- against two yardsticks on the same device tensors in the same process,
alternated round by round:

  * `tiny_llm_hip.synthetic.quantize`, the torch restatement that was the only quantiser on a GPU machine before the kernel;
  * a plain device copy (`Tensor.copy_`) that moves the same number of bytes (half of them read, half written): what a
    bandwidth-bound kernel could reach in that run.

Per matrix: median microseconds per call (device events around `--reps` calls, after `--warmup` calls, over `--rounds` rounds), the
bytes the algorithm needs (source read + words, scales and biases written), achieved GB/s and its share of the 8 TB/s HBM peak, and the
same for the copy.  Once per matrix the kernel's output is compared with the torch quantiser's on the device, and for one matrix both
with the torch quantiser's on the CPU (counts of differing words / scales / biases: the kernel is held to the numpy oracle by
tests/test_zz_quantize_w4_gpu.py; torch's device division is not promised to be correctly rounded).  Writes one JSON object to --out; without a GPU it writes `"measured": false` and nothing else may be stated.

    python tools/quantize_bench.py [--reps 20] [--rounds 5] [--out profiles/quantize_w4.json]"""

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    sys.path.insert(0, str(p))

SHAPES = {"gate_up 9728x2560": (9728, 2560), "down 2560x9728": (2560, 9728), "q 4096x2560": (4096, 2560), "o 2560x4096": (2560, 4096),
          "embed 151936x2560": (151936, 2560)}
PEAK_GBS = 8000.0
YARDSTICKS = ["tiny_llm_hip.synthetic.quantize on the same device tensor", "Tensor.copy_ of the same number of bytes (half read, half written)"]


def algorithm_bytes(rows: int, cols: int, src_bytes: int = 2) -> int:
    return rows * cols * src_bytes + rows * cols // 2 + 2 * 2 * rows * cols // 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "quantize_w4.json"))
    args = ap.parse_args()

    import torch

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    if not torch.cuda.is_available():  # nothing here may be stated from a CPU run
        Path(args.out).write_text(json.dumps({"tool": "tools/quantize_bench.py", "measured": False, "why": "no MI355X in this process: the tool has not run",
                                              "yardsticks": YARDSTICKS, "shapes": {k: list(v) for k, v in SHAPES.items()}}, indent=1) + "\n")
        return
    import tiny_llm_ext_hip as ext
    from tiny_llm_hip.synthetic import quantize as torch_quantize

    def timed_us(fn, reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / reps

    doc = {"tool": "tools/quantize_bench.py", "measured": True, "device": torch.cuda.get_device_name(0), "source_dtype": "bfloat16",
           "unit": "median us per call over rounds; GB/s = algorithm bytes / that", "peak_GBs": PEAK_GBS, "yardsticks": YARDSTICKS,
           "note": "a call of a few microseconds is bounded by the host loop's launch rate, for the kernel and the copy alike: the table is the bandwidth figure",
           "reps": args.reps, "rounds": args.rounds, "matrices": {}}
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, (rows, cols) in SHAPES.items():
        w = (torch.randn((rows, cols), device="cuda", generator=gen) * 0.02).to(torch.bfloat16)
        nbytes = algorithm_bytes(rows, cols)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda").random_(0, 255)
        dst = torch.empty_like(src)
        slow_reps = max(1, args.reps // 10)  # (the torch quantiser takes many launches and gigabytes of temporaries per call)
        out = ext.quantize_w4(w)  # the timed calls go to the C entry point with these outputs: no allocation inside the window
        call = (w.data_ptr(), rows, cols, ext.TL_BF16, *(t.data_ptr() for t in out), torch.cuda.current_stream().cuda_stream)
        runs = {"kernel": (lambda: ext.check(ext.lib().tl_quantize_w4(*call)), args.reps), "torch": (lambda: torch_quantize(w), slow_reps), "copy": (lambda: dst.copy_(src), args.reps)}
        # how many packed words / scales / biases differ, bit for bit: the kernel and the torch quantiser ON THE DEVICE, and (one matrix
        # only: the host takes seconds) each of them against the torch quantiser on the CPU, whose divisions are correctly rounded
        def differing(a, b):
            return [int((x.view(torch.int16) != y.to(x.device).view(torch.int16)).sum()) if x.dtype == torch.bfloat16 else int((x != y.to(x.device)).sum()) for x, y in zip(a, b)]

        want = torch_quantize(w)
        diff = {"kernel_vs_torch_on_device": differing(out, want)}
        if name.startswith("q "):
            host = torch_quantize(w.cpu())
            diff.update(kernel_vs_torch_on_cpu=differing(out, host), torch_on_device_vs_torch_on_cpu=differing(want, host))
            del host
        del want
        for fn, _ in runs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in runs}
        for _ in range(args.rounds):  # alternating
            for k, (fn, reps) in runs.items():
                us[k].append(timed_us(fn, reps))
        med = {k: statistics.median(v) for k, v in us.items()}
        gbs = {k: nbytes / med[k] * 1e-3 for k in ("kernel", "copy")}
        doc["matrices"][name] = {
            "rows": rows, "cols": cols, "algorithm_bytes": nbytes, "differing_words_scales_biases": diff,
            "kernel_us": round(med["kernel"], 2), "kernel_us_min_max": [round(min(us["kernel"]), 2), round(max(us["kernel"]), 2)],
            "torch_us": round(med["torch"], 1), "copy_us": round(med["copy"], 2),
            "kernel_GBs": round(gbs["kernel"], 1), "kernel_share_of_peak": round(gbs["kernel"] / PEAK_GBS, 3),
            "copy_GBs": round(gbs["copy"], 1), "kernel_over_copy": round(gbs["kernel"] / gbs["copy"], 3),
            "speedup_over_torch": round(med["torch"] / med["kernel"], 1),
            "under_half_of_copy": gbs["kernel"] < 0.5 * gbs["copy"],
        }
        del w, src, dst, out
        torch.cuda.empty_cache()
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
