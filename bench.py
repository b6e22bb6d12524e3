#!/usr/bin/env python3
"""Headline benchmark: Qwen3-4B int4 (W4A16, group 128) single-stream KV-cache decode on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times exactly K decode steps and prints the line; `--dump-outputs DIR` also writes what the
last timed step computed (DIR/logits.npy: its logits [1, vocab] as float32; DIR/tokens.npy: the ids of the timed steps, up to
the last 4,096, as float64), for comparing two builds output for output -- the weights and the prompt derive from --seed only.
`--full` adds everything else below (roofline leg and its rocprofv3 child, GPU clocks, the short configs[2] / configs[4] /
64-sequence runs, the CPU baselines and checkers): runs of their own that the headline figure does not need.

Workload (BASELINE.json configs[1], the configuration the metric is quoted on): one request per GPU, a
128-token synthetic prompt (token ids drawn like the reference's build_requests, benches/bench.py:201-225),
chunked prefill, then greedy decode.  A "step" is one decode step = one generated token per GPU.  Weights are
random-init Qwen3-4B-shaped W4 tensors (N(0, 0.02) bf16 -> affine group-128 quantizer); no checkpoint can be
downloaded here.  N > 1: one process per GPU (torch.distributed.run), every rank decodes its own request —
request-level data parallelism with NO collective on the data path; RCCL is used only for the
barrier and the max-over-ranks of the elapsed time.

One JSON line on stdout (rank 0).  Extra objects (filled by --full; a plain run keeps roofline.step_* only):
  roofline     — the dominant kernel (tl::qmv3_kernel, the W4A16 decode GEMV: 145 launches per step streaming
                 all 2.137 GB of weights).  `achieved` / `frac` = algorithmic bytes of those launches / the sum of
                 their durations in a `rocprofv3 --kernel-trace --stats` run of THIS command, taken by this process
                 right after the timed region (a child process under rocprofv3: `roofline.rocprof.measured_in_this_run`)
                 -- the conservative figure: rocprofv3 brackets every dispatch, ramp and write-back included.  If
                 rocprofv3 cannot run, the newest committed summary is replayed and labelled so.
                 `frac_in_kernel_stamps` is the same ratio from tl_engine_profile_step (every kernel stamps the device
                 wall clock at its first workgroup's start and last wave's end; hipEvents cannot bracket kernels inside
                 a replayed graph).  `step_*` give the ratio for the whole production step (graph replay, launch gaps
                 included) — that is the number `value` follows.
  cpu_baseline — oracle/qwen3_decode.c (plain-C OpenMP port of the same decode step) on the host cores, on a
                 bounded sample at the bench's own prompt length; also the checker: GPU logits against the float64
                 truth beside the port's.  `cpu_baseline.torch_week2_kv_cache`: the torch-CPU restatement of the
                 reference's CPU-runnable Week-2 `kv-cache` path on all host cores.
"""

from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec (guides/MI355X_MICROARCH.md); measured copy ceiling 6290
HBM_COPY_GBPS = 6290.0


_T0 = time.perf_counter()


def progress(msg: str) -> None:
    """Timestamped progress on stderr (stdout carries exactly one JSON line): where a slow host spends the command's time."""
    print(f"[bench +{time.perf_counter() - _T0:6.1f}s] {msg}", file=sys.stderr, flush=True)


class time_box:
    """`with time_box(seconds):` raises TimeoutError inside the block once the wall clock is spent (SIGALRM; main thread only --
    elsewhere it does nothing).  Every CPU leg of this file runs in one: a reported baseline must never take the measurement
    with it (round 4: a leg that overran on one GPU box cost the whole line twice)."""

    def __init__(self, seconds: float):
        self.seconds = max(1, int(seconds))
        self.armed = False

    def _fire(self, signum, frame):
        raise TimeoutError(f"time box of {self.seconds} s exceeded")

    def __enter__(self):
        import signal
        import threading

        if threading.current_thread() is threading.main_thread() and hasattr(signal, "SIGALRM"):
            self.prev = signal.signal(signal.SIGALRM, self._fire)
            signal.alarm(self.seconds)
            self.armed = True
        return self

    def __exit__(self, *exc):
        if self.armed:
            import signal

            signal.alarm(0)
            signal.signal(signal.SIGALRM, self.prev)
        return False


def build_prompt(rng: random.Random, length: int, vocab: int) -> list[int]:
    """Synthetic prompt ids in [256, vocab) like the reference harness (benches/bench.py:201-225)."""
    return [rng.randrange(256, vocab) for _ in range(length)]


def timed_steps(run, sync, steps: int, dist=None, device=None):
    """The driver's timing contract: barrier + device sync on both sides of EXACTLY `steps` steps, MAX over ranks.
    `run(steps)` enqueues the work, `sync()` blocks until the device is idle.  Returns (elapsed_max_s, elapsed_local_s)."""
    import torch

    sync()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    run(steps)
    sync()
    local = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
        t = torch.tensor([local], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()), local
    return local, local


def rocprof_gemv_rate(stats_csv: Path, kinds: dict, num_layers: int, live: bool = False) -> dict | None:
    """GEMV-stream rate recomputed from a COMMITTED `rocprofv3 --kernel-trace --stats` summary of this same command
    (profiles/<round>_rocprofv3/bench_config<N>_kernel_stats.csv).  NOT measured in this run: the block is labelled so, carries
    the file's modification time, and is only as fresh as that file.  Decode steps in the trace = calls of the gate|up GEMV
    (the only kernel with the SwiGLU epilogue, one per layer and step) / layers -- prefill launches a step_end_kernel and an
    lm_head GEMV of its own, so neither of those counts steps.  rocprofv3 brackets each dispatch (wave launch ramp +
    end-of-kernel write-back): its durations are ~1 us per launch longer than the in-kernel stamps.
    Kernel names carry the template arguments <MR, KS, CW, PRO, EPI, LM>: EPI 2 = SwiGLU (gate|up), EPI 1 = residual (KS 8:
    w_down, else wo), PRO 1 + EPI 0 = RMSNorm prologue + plain store (qkv and lm_head share that instantiation)."""
    import csv
    import re

    try:
        rows = list(csv.DictReader(open(stats_csv)))
    except OSError:
        return None
    gemv = []
    for r in rows:
        m = re.search(r"tl::qmv3_kernel<(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)", r["Name"])
        if not m:
            continue
        mr, ks, cw, pro, epi, lm = (int(x) for x in m.groups())
        which = "gate_up" if epi == 2 else ("down" if epi == 1 and ks >= 8 else ("o" if epi == 1 else "qkv+lm_head"))
        gemv.append((which, r))
    gu_calls = sum(int(r["Calls"]) for w, r in gemv if w == "gate_up")
    if not gu_calls or gu_calls % num_layers:
        return None
    steps = gu_calls // num_layers
    b = {k: kinds[f"gemv_{k}"]["bytes"] for k in ("qkv", "o", "gate_up", "down", "lm_head")}
    per_step_bytes = {"gate_up": b["gate_up"], "down": b["down"], "o": b["o"], "qkv+lm_head": b["qkv"] + b["lm_head"]}
    total_ns = sum(float(r["TotalDurationNs"]) for _, r in gemv)
    launches = sum(int(r["Calls"]) for _, r in gemv)
    us_per_step = total_ns / 1e3 / steps
    g_bytes = sum(b.values())
    ach = g_bytes / us_per_step / 1e3
    per = {}
    for which in per_step_bytes:
        ns = sum(float(r["TotalDurationNs"]) for w, r in gemv if w == which)
        calls = sum(int(r["Calls"]) for w, r in gemv if w == which)
        if ns > 0:
            gbps = per_step_bytes[which] * steps / ns
            per[which] = {"avg_launch_us": round(ns / 1e3 / calls, 3), "GBps": round(gbps, 1), "frac": round(gbps / HBM_PEAK_GBPS, 4)}
    try:
        shown = str(stats_csv.relative_to(ROOT))
    except ValueError:  # a summary outside the repository (--rocprof-stats, or the live run's temporary directory)
        shown = str(stats_csv)
    return {"measured_in_this_run": live,
            "source": "rocprofv3 --kernel-trace --stats of this command, run by this process after the timed region" if live
                      else "committed rocprofv3 --kernel-trace --stats summary of this command (replayed, NOT measured now)",
            "file": shown,
            "steps_in_trace": steps, "gemv_launches_per_step": round(launches / steps, 2),
            "gemv_us_per_step": round(us_per_step, 1), "avg_launch_us": round(total_ns / 1e3 / launches, 3),
            "achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBPS, 4), "per_projection": per}


def latest_rocprof_stats(config: int) -> Path | None:
    """The newest committed profiles/r<NN>_rocprofv3/bench_config<N>_kernel_stats.csv."""
    found = sorted((ROOT / "profiles").glob(f"r*_rocprofv3/bench_config{config}_kernel_stats.csv"))
    return found[-1] if found else None


def rocprof_live(args) -> Path | None:
    """Run this very command once more as a child under `rocprofv3 --kernel-trace --stats` (20 decode steps, no CPU legs) and
    return its kernel-stats CSV, or None when rocprofv3 is missing or fails (the caller then replays the committed summary)."""
    import glob
    import shutil
    import subprocess
    import tempfile

    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not Path(exe).exists():
        return None
    tmp = tempfile.mkdtemp(prefix="bench_rocprof_", dir="/tmp")
    cmd = [exe, "--kernel-trace", "--stats", "-d", tmp, "-o", "bench", "--output-format", "csv", "--", sys.executable,
           str(Path(__file__).resolve()), "--config", str(args.config), "--steps", "20", "--warmup", "5", "--seed", str(args.seed),
           "--model", args.model, "--prompt-len", str(args.prompt_len), "--prefill-step", str(args.prefill_step),
           "--no-cpu-baseline", "--no-extra-configs", "--no-clocks", "--profile-steps", "0", "--rocprof", "off"]
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    try:
        subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300, check=True)
    except (OSError, subprocess.SubprocessError):
        return None
    found = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
    if not found:
        return None
    keep = ROOT / "gpurun_out" / "bench_rocprof"  # scratch copy: what gets committed under profiles/ is taken from here
    try:
        keep.mkdir(parents=True, exist_ok=True)
        dst = keep / f"bench_config{args.config}_kernel_stats.csv"
        shutil.copyfile(found[-1], dst)
        return dst
    except OSError:
        return Path(found[-1])


def self_launch(argv: list[str], n: int) -> None:
    """`python bench.py --gpus N` without a launcher: start N ranks of this script under torch.distributed.run (one per GPU,
    rendezvous on 127.0.0.1) and hand their exit status on.  Rank 0's JSON line goes to this process's stdout."""
    import socket
    import subprocess

    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this host driver (RCCL needs it)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve()), *argv]
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


class SleepEngine:
    """--engine sleep: a stand-in with the call surface main() uses and a fixed cost per step, so that the launch / rendezvous /
    timing / reporting path of this file can be exercised without a GPU (tests/test_bench_dist_cpu.py).  Its line says
    "data": "none (--engine sleep ...)" and is never a measurement."""

    def __init__(self, step_s: float = 0.002):
        self.step_s = step_s
        self.steps = 0

    def begin(self, slot): pass
    def prefill(self, slot, prompt, chunk=None): time.sleep(self.step_s)
    def decode(self, k, batch=1, use_graph=True):
        time.sleep(self.step_s * k)
        self.steps += k
    def synchronize(self): pass
    def step_bytes(self, batch): return 0
    def read_tokens(self, slot, n): return [0] * n
    def stats(self): return {"graph_captures": 0, "graph_replays": 0, "decode_steps": self.steps, "kv_bytes": 0}
    def release(self, slot): pass


def dump_outputs(out_dir: Path, engine, steps: int, dry: bool) -> None:
    """--dump-outputs: what a caller of the timed path receives from its last step -- the logits [1, vocab] (bf16 on the device,
    exact in float32) and the greedy ids of the timed steps (the engine's ring holds the last 4,096) -- as DIR/<name>.npy."""
    import numpy as np

    out_dir.mkdir(parents=True, exist_ok=True)
    ids = engine.read_tokens(0, min(steps, 4096))
    np.save(out_dir / "tokens.npy", np.asarray(ids, dtype=np.float64))
    if not dry:
        np.save(out_dir / "logits.npy", engine.logits(1).float().cpu().numpy().astype(np.float32))


def aggregate_value(n_gpus: int, steps: int, elapsed_max_s: float) -> float:
    """Whole-job tokens/s: every rank decodes its own request (weak scaling), the job takes as long as its slowest rank."""
    return n_gpus * steps / elapsed_max_s


def host_weights(mlx_model) -> dict:
    """The checkpoint as host numpy arrays in the layout oracle/c_oracle.py takes."""
    import numpy as np
    import torch

    def host_w4(layer):
        return (layer.weight.cpu().numpy().view(np.uint32), layer.scales.view(torch.int16).cpu().numpy().view(np.uint16),
                layer.biases.view(torch.int16).cpu().numpy().view(np.uint16))

    def host_norm(t):
        return t.to(torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16)

    layers = []
    for layer in mlx_model.model.layers:
        a, m = layer.self_attn, layer.mlp
        layers.append(dict(q=host_w4(a.q_proj), k=host_w4(a.k_proj), v=host_w4(a.v_proj), o=host_w4(a.o_proj),
                           gate=host_w4(m.gate_proj), up=host_w4(m.up_proj), down=host_w4(m.down_proj),
                           q_norm=host_norm(a.q_norm.weight), k_norm=host_norm(a.k_norm.weight),
                           input_norm=host_norm(layer.input_layernorm.weight),
                           post_norm=host_norm(layer.post_attention_layernorm.weight)))
    return dict(embed=host_w4(mlx_model.model.embed_tokens), layers=layers, norm=host_norm(mlx_model.model.norm.weight))


def dense_host_weights(mlx_model) -> dict:
    """The checkpoint dequantised to dense bf16 on the device (quantize.py:103-121: fp32 q * scale + bias, one cast) and moved to
    host memory: what the reference's Week-2 `kv-cache` checkpoint computes with (oracle/torch_week2_cpu.py)."""
    import torch

    def dq(layer):
        packed, scales, biases = layer.weight, layer.scales, layer.biases
        shifts = torch.arange(0, 32, 4, device=packed.device, dtype=torch.int32)
        q = ((packed.to(torch.int32).unsqueeze(-1) >> shifts) & 0xF).reshape(packed.shape[0], -1).float()
        w = q * scales.float().repeat_interleave(128, dim=1) + biases.float().repeat_interleave(128, dim=1)
        return w.to(torch.bfloat16).cpu()

    def nw(t):
        return t.to(torch.bfloat16).cpu()

    layers = []
    for layer in mlx_model.model.layers:
        a, m = layer.self_attn, layer.mlp
        layers.append(dict(q=dq(a.q_proj), k=dq(a.k_proj), v=dq(a.v_proj), o=dq(a.o_proj), gate=dq(m.gate_proj), up=dq(m.up_proj),
                           down=dq(m.down_proj), q_norm=nw(a.q_norm.weight), k_norm=nw(a.k_norm.weight),
                           input_norm=nw(layer.input_layernorm.weight), post_norm=nw(layer.post_attention_layernorm.weight)))
    out = dict(embed=dq(mlx_model.model.embed_tokens), layers=layers, norm=nw(mlx_model.model.norm.weight))
    if hasattr(mlx_model, "lm_head"):
        out["lm_head"] = dq(mlx_model.lm_head)
    return out


def torch_week2_leg(mlx_model, cfg: dict, prompt: list[int], fed: list[int], gpu_first_logits, dense: dict | None = None) -> dict:
    """SURVEY.md section 8d's baseline: the reference's CPU-runnable Week-2 `kv-cache` path (dense bf16 linears, fp32 attention,
    concatenating cache; benches/bench.py:158-169,277-312) restated on torch-CPU, on ALL host cores of this box, at the bench's
    own prompt length.  A restatement, not MLX (which cannot be installed here).  Bounded: torch's CPU bf16 GEMM has no fast path
    on every host (a 128-token prefill took more than ten minutes on one GPU box), so a probe picks the faster of bf16 / fp32
    storage for the linears (same bf16-valued weights; fp32 streams twice the bytes) and the prompt is cut to what TORCH_BUDGET_S
    affords (a prefix of the same prompt; the line says which)."""
    import numpy as np
    import torch

    from oracle.torch_week2_cpu import TorchWeek2KvCacheCPU

    cores = os.cpu_count() or 1
    hs, inter = cfg["hidden_size"], cfg["intermediate_size"]

    def probe(dtype, rows):
        a, w = torch.randn((rows, hs)).to(dtype), torch.randn((inter, hs)).to(dtype)
        a @ w.T
        t0 = time.perf_counter()
        for _ in range(2):
            a @ w.T
        return (time.perf_counter() - t0) / 2

    # "all host cores": every logical CPU is offered; the thread count is the fastest of {all, half (one per physical core), 64, 32}
    # on a GEMV probe -- on a 256-thread two-socket host a small op on 256 threads costs more in fork / join than it computes
    threads_tried = {}
    for n in sorted({cores, max(1, cores // 2), min(cores, 64), min(cores, 32)}, reverse=True):
        try:
            torch.set_num_threads(n)
        except RuntimeError:
            continue
        threads_tried[n] = min(probe(torch.bfloat16, 1), probe(torch.float32, 1))
    best_threads = min(threads_tried, key=threads_tried.get) if threads_tried else torch.get_num_threads()
    try:
        torch.set_num_threads(best_threads)
    except RuntimeError:
        pass
    gemv = {d: probe(d, 1) for d in (torch.bfloat16, torch.float32)}
    dtype = min(gemv, key=gemv.get)
    if dense is None:
        dense = dense_host_weights(mlx_model)
    if dtype != torch.bfloat16:
        for lw in dense["layers"]:
            for k in ("q", "k", "v", "o", "gate", "up", "down"):
                lw[k] = lw[k].to(dtype)
        dense["embed_linear"] = dense["embed"].to(dtype)
    model = TorchWeek2KvCacheCPU(cfg, dense, linear_dtype=dtype)
    # prefill cost: one matmul of `rows` x hidden x intermediate is 1 / 145 of the whole model's linears for those rows
    per_layer_unit = (3 * inter * hs + 2 * hs * cfg["num_attention_heads"] * cfg["head_dim"] + 2 * hs * cfg["num_key_value_heads"] * cfg["head_dim"]) / (inter * hs)
    L = len(prompt)
    while L > 8 and probe(dtype, L) * per_layer_unit * cfg["num_hidden_layers"] > TORCH_BUDGET_S:
        L = max(8, L // 2)
    used = prompt[:L]
    t0 = time.perf_counter()
    logits = model.forward(used)
    prefill_s = time.perf_counter() - t0
    steps = len(fed)
    dt, ids, first = model.timed_decode(int(torch.argmax(logits.float())), steps, fed=fed if L == len(prompt) else None)
    diff = None
    if gpu_first_logits is not None and L == len(prompt):
        diff = float(np.abs(first.float().numpy().astype(np.float64) - np.asarray(gpu_first_logits, dtype=np.float64)).max())
    bytes_per_token = 2 if dtype == torch.bfloat16 else 4
    return {"value": round(steps / dt, 3), "unit": "tokens/s", "cores": cores, "torch_threads": torch.get_num_threads(),
            "os_cpu_count": os.cpu_count(), "kind": "port",
            "label": "torch-CPU restatement of tiny_llm_ref (Qwen3ModelWeek2, checkpoint kv-cache: dense bf16-valued linears, fp32 attention, concatenating KV cache) -- NOT MLX",
            "linear_storage": str(dtype).replace("torch.", ""),
            "gemv_probe_ms": {str(d).replace("torch.", ""): round(v * 1e3, 2) for d, v in gemv.items()},
            "gemv_probe_ms_by_threads": {str(n): round(v * 1e3, 2) for n, v in threads_tried.items()},
            "sample": f"{steps} decode steps after a {L}-token prompt" + ("" if L == len(prompt) else f" (cut from {len(prompt)}: prefill budget {TORCH_BUDGET_S:.0f} s)")
                      + f" (prefill {round(L / prefill_s, 1)} tokens/s), the same checkpoint dequantised to dense weights "
                      + f"({round(4.022e9 * bytes_per_token / 1e9, 1)} GB streamed per token)",
            "max_abs_logit_vs_gpu_first_decode_step": None if diff is None else round(diff, 4)}


def walk_prompt_bounded(models, prompt: list[int], budget_s: float, floor: int = 8):
    """Feed `prompt` token by token to every model of `models` IN LOCK STEP until it ends or `budget_s` of wall clock are spent
    (never fewer than `floor` tokens): all of them end on the same prefix.  Returns (tokens fed, [(last id, last logits) per model])."""
    t0 = time.perf_counter()
    fed, last = 0, [(0, None)] * len(models)
    for t in prompt:
        last = [m.step(t) for m in models]
        fed += 1
        if fed >= floor and time.perf_counter() - t0 > budget_s:
            break
    return fed, last


def cpu_baseline_leg(mlx_model, cfg: dict, engine, sample_prompt: int, sample_steps: int, prefill_chunk: int = 8, fp8_engine=None) -> dict:
    """Time the plain-C port (oracle/) on the host cores on a bounded sample and use it as a checker: the engine is prefilled
    through the bench's own path (`prefill_chunk` rows per pass) and decodes at the bench's own attention plan."""
    import numpy as np
    import torch

    from oracle import c_oracle

    if not c_oracle.available():
        return {"value": None, "unit": "tokens/s", "cores": 0, "kind": "port",
                "sample": "oracle/libqwen3_oracle.so missing (run __graft_entry__.build())"}

    weights = host_weights(mlx_model)
    # OpenMP fork/join per matvec (7 x 36 per token) stops scaling long before a 2-socket host runs out of cores
    cores = min(os.cpu_count() or 1, 32)
    model = c_oracle.COracleQwen3(cfg, weights, max_ctx=sample_prompt + sample_steps + 1, threads=cores)
    # ground truth beside it: oracle/qwen3_truth.c, float64 with no intermediate rounding.  The bf16 port and the HIP engine both
    # round at every reference op boundary; their distances from THIS are what can be compared.
    truth_steps = min(sample_steps, 8)
    truth = c_oracle.CTruthQwen3(cfg, weights, max_ctx=sample_prompt + truth_steps + 1, threads=cores)
    prompt = build_prompt(random.Random(1234), sample_prompt, cfg["vocab_size"])
    # Token-by-token prefill of both C checkers in lock step: untimed warm-up of the CPU path.  BOUNDED: they walk the prompt one
    # token at a time (~0.3-0.5 s each on 32 threads, each), and this line must come out within minutes on any host -- after
    # PROMPT_BUDGET_S the prompt is cut where it stands (never below 8 tokens; a prefix of the same seeded prompt), and the line
    # says which length was checked.
    progress(f"cpu_baseline: C port + C truth walk the {sample_prompt}-token prompt on {cores} threads (budget {PROMPT_BUDGET_S:.0f} s)")
    fed_prompt, ((tid, logits), (_, tl)) = walk_prompt_bounded([model, truth], prompt, PROMPT_BUDGET_S)
    prompt = prompt[:fed_prompt]
    sample_prompt = fed_prompt
    progress(f"cpu_baseline: {fed_prompt} prompt tokens walked; timing {sample_steps} decode steps of the port")
    cpu_ids, cpu_logits = [tid], [logits]
    t0 = time.perf_counter()
    for _ in range(sample_steps):
        tid, logits = model.step(cpu_ids[-1])
        cpu_ids.append(tid)
        cpu_logits.append(logits)
    dt = time.perf_counter() - t0
    model.close()
    truth_logits = [tl]
    for s in range(truth_steps):
        _, tl = truth.step(cpu_ids[s])
        truth_logits.append(tl)
    truth.close()
    progress("cpu_baseline: C legs done; engine checked against them")

    # checker: the engine on the same prompt, teacher-forced on the CPU ids, must give the same logits (log-softmax
    # within the band one bf16 ulp of a logit can move it) and the same greedy id wherever the top-2 margin is clear
    def logsm(x):
        x = np.asarray(x, dtype=np.float64)
        return x - x.max() - np.log(np.exp(x - x.max()).sum())

    engine.begin(0)
    engine.prefill(0, prompt, chunk=prefill_chunk)
    gpu_ids, gpu_logits = engine.read_tokens(0, 1), [engine.logits(1)[0].float().cpu().numpy()]
    for s in range(sample_steps):
        engine.set_token(0, cpu_ids[s])
        engine.decode(1, batch=1)
        gpu_ids.append(engine.read_tokens(0, 1)[0])
        gpu_logits.append(engine.logits(1)[0].float().cpu().numpy())
    n_splits_checked = engine.profile_step(1)["n_splits"]  # the attention plan of the steps just checked (one more step, unchecked)
    engine.release(0)
    # The same sample once more with the prompt prefilled the way the TIMED run prefills it -- whole chunks through the tile GEMM (rows > 8:
    # quantize.py:54-65 -> quantized_matmul.metal:96-249, weights rounded to bf16 first, split-K partials in bf16) and the FlashAttention
    # kernel -- so that the line's own check also covers the prefill kernels the timed numbers use (round-5 review).  Same truth; the
    # reference-mandated extra roundings of that path sit in the cached K/V, so its distance is reported beside the matvec-form one, not
    # folded into it.
    gemm_chunk = max(int(getattr(engine, "timed_prefill_chunk", 0) or 0), 9)
    gemm_logits = []
    engine.begin(0)
    engine.prefill(0, prompt, chunk=gemm_chunk)
    gemm_logits.append(engine.logits(1)[0].float().cpu().numpy())
    for s in range(truth_steps):
        engine.set_token(0, cpu_ids[s])
        engine.decode(1, batch=1)
        gemm_logits.append(engine.logits(1)[0].float().cpu().numpy())
    engine.release(0)
    # ... and once more on an engine whose K / V pages are FP8 (E4M3) codes (an extension -- the reference has no
    # quantised cache): the same prompt, the same teacher-forced steps, the same truth.  What the quantised cache costs in logits.
    fp8_sample = None
    if fp8_engine is not None:
        fp8_logits = []
        fp8_engine.begin(0)
        fp8_engine.prefill(0, prompt, chunk=prefill_chunk)
        fp8_logits.append(fp8_engine.logits(1)[0].float().cpu().numpy())
        for s in range(truth_steps):
            fp8_engine.set_token(0, cpu_ids[s])
            fp8_engine.decode(1, batch=1)
            fp8_logits.append(fp8_engine.logits(1)[0].float().cpu().numpy())
        fp8_engine.release(0)
        e8 = max(float(np.abs(np.asarray(g, np.float64) - t).max()) for g, t in zip(fp8_logits, truth_logits))
        rms8 = float(np.sqrt(np.mean([np.mean((np.asarray(g, np.float64) - t) ** 2) for g, t in zip(fp8_logits, truth_logits)])))
        same_ids = sum(int(np.argmax(g) == np.argmax(b)) for g, b in zip(fp8_logits, gpu_logits))
        fp8_sample = {"what": "the same prompt and teacher-forced steps on an engine with FP8 (E4M3) K / V pages (tl_engine_create_kv; extension, no reference behaviour)",
                      "steps": len(fp8_logits), "max_abs_logit_gpu_vs_truth": round(e8, 5), "rms_logit_gpu_vs_truth": round(rms8, 5),
                      "greedy_ids_equal_the_bf16_engine": f"{same_ids}/{len(fp8_logits)}"}
    worst, worst_logit = 0.0, 0.0
    for cl, gl in zip(cpu_logits, gpu_logits):
        worst = max(worst, float(np.abs(logsm(cl) - logsm(gl)).max()))
        worst_logit = max(worst_logit, float(np.abs(np.asarray(cl, np.float64) - gl).max()))
    e_gpu = max(float(np.abs(np.asarray(g, np.float64) - t).max()) for g, t in zip(gpu_logits, truth_logits))
    e_cpu = max(float(np.abs(np.asarray(c, np.float64) - t).max()) for c, t in zip(cpu_logits, truth_logits))
    # the same comparison on a statistic that does not hang on ONE of 151,936 x steps logits: root mean square error over all of them
    rms_gpu = float(np.sqrt(np.mean([np.mean((np.asarray(g, np.float64) - t) ** 2) for g, t in zip(gpu_logits, truth_logits)])))
    rms_cpu = float(np.sqrt(np.mean([np.mean((np.asarray(c, np.float64) - t) ** 2) for c, t in zip(cpu_logits, truth_logits)])))
    e_gemm = max(float(np.abs(np.asarray(g, np.float64) - t).max()) for g, t in zip(gemm_logits, truth_logits))
    rms_gemm = float(np.sqrt(np.mean([np.mean((np.asarray(g, np.float64) - t) ** 2) for g, t in zip(gemm_logits, truth_logits)])))
    # greedy ids: the engine's choice must be the truth's argmax or lie within the engine's own measured error of it
    near, exact = 0, 0
    for gi, t in zip(gpu_ids, truth_logits):
        gap = float(t.max() - t[gi])
        exact += int(gap == 0.0)
        near += int(gap <= 2.0 * e_gpu)
    return {"value": round(sample_steps / dt, 3), "unit": "tokens/s", "cores": cores, "os_cpu_count": os.cpu_count(), "kind": "port",
            "sample": f"{sample_steps} decode steps after a {sample_prompt}-token prompt, same Qwen3-4B W4 checkpoint, "
                      f"oracle/qwen3_decode.c with OpenMP on {cores} threads",
            "n_splits_checked": n_splits_checked, "engine_prefill_rows_per_pass_checked": prefill_chunk, "_prompt": prompt, "_fed": cpu_ids[:sample_steps], "_gpu_first_decode_logits": gpu_logits[1],
            "truth": f"oracle/qwen3_truth.c (float64, no intermediate rounding), first {len(truth_logits)} steps",
            "oracle_pins": "the numpy / C checkers are bit-identical in 16 bits to the reference's own Metal kernels compiled for the host (oracle/_ref) for the "
                           "vanilla matmul, decode matvec, embedding, split-K reduce, RMSNorm, RoPE, SwiGLU, dense and paged decode attention; the tile GEMM and "
                           "the MMA FlashAttention restatements follow the .metal text and are pinned by PyTorch only (MLX's steel headers are not in the reference tree)",
            "max_abs_logit_gpu_vs_truth": round(e_gpu, 5), "max_abs_logit_cpu_vs_truth": round(e_cpu, 5),
            "gpu_error_over_cpu_error": round(e_gpu / e_cpu, 3) if e_cpu > 0 else None,
            "rms_logit_gpu_vs_truth": round(rms_gpu, 5), "rms_logit_cpu_vs_truth": round(rms_cpu, 5),
            "gpu_rms_error_over_cpu_rms_error": round(rms_gpu / rms_cpu, 3) if rms_cpu > 0 else None,
            "max_abs_logit_gpu_vs_cpu": round(worst_logit, 5), "gpu_vs_cpu_max_logprob_diff": round(worst, 4),
            "gemm_prefill_sample": {"engine_prefill_rows_per_pass": min(gemm_chunk, sample_prompt), "steps": len(gemm_logits),
                                    "what": "the same prompt prefilled in whole chunks (tile GEMM + FlashAttention: the timed run's prefill kernels), then the same teacher-forced steps",
                                    "max_abs_logit_gpu_vs_truth": round(e_gemm, 5), "rms_logit_gpu_vs_truth": round(rms_gemm, 5),
                                    "gpu_error_over_cpu_error": round(e_gemm / e_cpu, 3) if e_cpu > 0 else None,
                                    "gpu_rms_error_over_cpu_rms_error": round(rms_gemm / rms_cpu, 3) if rms_cpu > 0 else None},
            "kv_fp8_sample": fp8_sample,
            "gpu_greedy_ids_vs_truth": f"{exact}/{len(truth_logits)} are the truth's argmax, {near}/{len(truth_logits)} within "
                                       f"2 x the engine's measured error of it"}


PROMPT_BUDGET_S = 30.0  # wall-clock bound of the C port's + C truth's walk over the prompt (cpu_baseline_leg)
TORCH_BUDGET_S = 10.0    # ... and of the torch-CPU restatement's prefill (torch_week2_leg)
PEAKED_RECIPE = dict(embed_sigma=0.25, residual_gain=0.2, head_permutation=(48271, 11))


def peaked_checkpoint_leg(cfg: dict, device: str, seed: int, steps: int = 8) -> dict:
    """Greedy ids on a PEAKED synthetic checkpoint must EQUAL the float64 truth's.  With N(0, 0.02) weights the top two of 151,936
    logits lie within a rounding error of each other and id agreement says little.  Round 3's recipe (residual writers damped by
    0.02, tied head) echoed ONE id with a margin of 460 logit units: a kernel wrong by a hundred would have passed.  This recipe
    (tiny_llm_hip/synthetic.py: embedding N(0, 0.25), o_proj / down_proj x 0.2, an untied head that is the embedding with its rows
    permuted) walks a permutation -- every step a different id -- with a top-2 margin of 5-50 x the engine's measured error
    (tools/r4/peaked_recipe_probe.py: margin 21-46, error ~1.9 on logits of ~90).  The engine and the truth each follow their OWN ids."""
    import numpy as np
    import torch

    from oracle import c_oracle
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    if not c_oracle.available():
        return {"checked": False, "why": "oracle/libqwen3_oracle.so missing"}
    model = synthetic_qwen3(cfg, seed=seed + 7, sigma=0.02, device=device, **PEAKED_RECIPE)
    prompt = build_prompt(random.Random(4321), 8, cfg["vocab_size"])
    eng = DecodeEngine(model, page_size=128, num_pages=4, max_batch=1, max_prefill_rows=8)
    try:
        eng.begin(0)
        eng.prefill(0, prompt, chunk=8)
        gpu_logits = [eng.logits(1)[0].float().cpu().numpy()]
        eng.decode(steps, batch=1)
        gpu_ids = eng.read_tokens(0, steps + 1)
        eng.release(0)
    finally:
        eng.close()
    # the same walk on an engine whose K / V pages are FP8 (E4M3) codes (an extension): its own ids, its own first logits
    fp8_ids, fp8_first = None, None
    if cfg.get("head_dim") == 128:
        eng = DecodeEngine(model, page_size=128, num_pages=4, max_batch=1, max_prefill_rows=8, kv_format="fp8")
        try:
            eng.begin(0)
            eng.prefill(0, prompt, chunk=8)
            fp8_first = eng.logits(1)[0].float().cpu().numpy()
            eng.decode(steps, batch=1)
            fp8_ids = eng.read_tokens(0, steps + 1)
            eng.release(0)
        finally:
            eng.close()
    cores = min(os.cpu_count() or 1, 32)
    weights = host_weights(model)
    head = model.lm_head
    weights["lm_head"] = (head.weight.cpu().numpy().view(np.uint32), head.scales.view(torch.int16).cpu().numpy().view(np.uint16),
                          head.biases.view(torch.int16).cpu().numpy().view(np.uint16))
    truth = c_oracle.CTruthQwen3(dict(cfg, tie_word_embeddings=False), weights, max_ctx=len(prompt) + steps + 2, threads=cores)
    tid, tl = 0, None
    for t in prompt:
        tid, tl = truth.step(t)
    truth_ids, margins = [tid], []
    first_tl = tl
    first_err = float(np.abs(gpu_logits[0].astype(np.float64) - tl).max())
    for _ in range(steps):
        top2 = np.partition(tl, -2)[-2:]
        margins.append(float(top2[1] - top2[0]))
        tid, tl = truth.step(truth_ids[-1])
        truth_ids.append(tid)
    truth.close()
    same = sum(int(a == b) for a, b in zip(gpu_ids, truth_ids))
    ratio = min(margins) / first_err if first_err > 0 else None
    fp8 = None
    if fp8_ids is not None:
        fp8 = {"greedy_ids_equal_truth": f"{sum(int(a == b) for a, b in zip(fp8_ids, truth_ids))}/{len(truth_ids)}",
               "max_abs_logit_gpu_vs_truth_first_step": round(float(np.abs(fp8_first.astype(np.float64) - first_tl).max()), 4)}
    return {"checked": True, "recipe": "embed_sigma 0.25, residual_gain 0.2 (o_proj, down_proj), untied head = embedding rows permuted by t -> 48271 t + 11 mod V, else N(0, 0.02); W4 g128",
            "greedy_ids_equal_truth": f"{same}/{len(truth_ids)}", "all_equal": same == len(truth_ids), "kv_fp8_pages": fp8,
            "distinct_ids": len(set(int(t) for t in truth_ids)),
            "min_top2_margin_of_truth": round(min(margins), 3), "max_abs_logit_gpu_vs_truth_first_step": round(first_err, 4),
            "margin_over_error": None if ratio is None else round(ratio, 1),
            "discriminating": bool(ratio is not None and 5.0 <= ratio <= 50.0 and len(set(int(t) for t in truth_ids)) >= 4),
            "gpu_ids": gpu_ids, "truth_ids": [int(t) for t in truth_ids]}


def extra_configs_leg(mlx_model, cfg: dict, device: str, seed: int, page: int = 128) -> dict:
    """BASELINE.json configs[2], configs[4] and a 64-sequence step of configs[3], on the GPU only, after the timed region (a few
    seconds together): each on its own engine over the same checkpoint.  Shapes: book/src/appendix-performance.md:18-27,555-561
    (8k static prefill + decode; 64 concurrent requests); SURVEY.md section 8d for the byte model.  `--config 3` / `--config 5` time
    the same steps as the headline workload (profiles/r05_bench_config{3,5}.json); these are the short driver-observed twins."""
    import torch

    from tiny_llm_hip.engine import DecodeEngine

    out = {}
    rng = random.Random(seed * 1000 + 77)

    def sync(e):
        e.synchronize()
        torch.cuda.synchronize()

    # config5_kv_fp8: configs[4] once more with the K / V pages as FP8 E4M3 codes + one power-of-two scale per row (SURVEY section 8 f4,
    # tl_engine_create_kv): NOT the reference's arithmetic (it has no quantised cache, README.md:134-135) -- an opt-in extension reported
    # beside the bf16 figure, never instead of it; its algorithmic bytes are its own (132 instead of 256 bytes per cached row)
    for name, plen, steps, chunk, kv_format in (("config3", 8192, 16, 4096, "bf16"), ("config5", 32768, 16, 4096, "bf16"),
                                                ("config5_kv_fp8", 32768, 16, 4096, "fp8")):
        eng = None
        try:
            with time_box(60):
                eng = DecodeEngine(mlx_model, page_size=page, num_pages=(plen + steps + 96 + page - 1) // page + 2, max_batch=1, max_prefill_rows=chunk,
                                   kv_format=kv_format)
                prompt = build_prompt(rng, plen, cfg["vocab_size"])
                eng.begin(0)  # one chunk, untimed: code objects and workspaces of the full-chunk prefill kernels
                eng.prefill(0, prompt[:chunk], chunk=chunk)
                sync(eng)
                eng.release(0)
                eng.begin(0)
                t0 = time.perf_counter()
                eng.prefill(0, prompt, chunk=chunk)
                sync(eng)
                prefill_s = time.perf_counter() - t0
                eng.decode(4, batch=1)  # eager warm step + graph capture
                sync(eng)
                b0 = eng.step_bytes(1)
                t0 = time.perf_counter()
                eng.decode(steps, batch=1)
                sync(eng)
                dt = time.perf_counter() - t0
                step_bytes = 0.5 * (b0 + eng.step_bytes(1))
                prof = eng.profile_step(1)
                kinds = prof["kinds"]
                g_bytes = sum(v["bytes"] for k, v in kinds.items() if k.startswith("gemv_"))
                kv_bytes = max(step_bytes - g_bytes, 0.0)
                attn_us = kinds["attention"]["us"] + kinds["attention_merge"]["us"]
                out[name] = {"prompt_tokens": plen, "decode_steps": steps, "prefill_step": chunk, "kv_pages": kv_format,
                             "ms_per_step": round(dt * 1e3 / steps, 4), "tokens_per_s": round(steps / dt, 1),
                             "prefill_tokens_per_s": round(plen / prefill_s, 1),
                             "step_bytes": int(step_bytes), "step_frac": round(step_bytes / (dt / steps) / 1e9 / HBM_PEAK_GBPS, 4),
                             "kv_bytes_per_step": int(kv_bytes), "attention_us_per_step_in_kernel_stamps": round(attn_us, 1),
                             "kv_frac": round(kv_bytes / attn_us / 1e3 / HBM_PEAK_GBPS, 4) if attn_us else None,
                             "attention_launches_per_step": kinds["attention"]["launches"] + kinds["attention_merge"]["launches"],
                             "n_splits": prof.get("n_splits")}
                eng.release(0)
        except Exception as exc:
            out[name] = {"ms_per_step": None, "why": f"{type(exc).__name__}: {exc}"}
        finally:
            if eng is not None:
                eng.close()
    for name, kv_format in (("batch64", "bf16"), ("batch64_kv_fp8", "fp8")):
        eng = None
        try:
            with time_box(60):
                B, plen, steps = 64, 128, 16
                per_seq = (plen + steps + 8 + 2 * page) // page + 1
                eng = DecodeEngine(mlx_model, page_size=page, num_pages=per_seq * B + 2, max_batch=B, max_prefill_rows=128, kv_format=kv_format)
                for slot in range(B):
                    eng.begin(slot)
                    eng.prefill(slot, build_prompt(rng, plen, cfg["vocab_size"]), chunk=128)
                eng.decode(4, batch=B)
                sync(eng)
                b0 = eng.step_bytes(B)
                t0 = time.perf_counter()
                eng.decode(steps, batch=B)
                sync(eng)
                dt = time.perf_counter() - t0
                step_bytes = 0.5 * (b0 + eng.step_bytes(B))
                out[name] = {"sequences": B, "prompt_tokens": plen, "decode_steps": steps, "kv_pages": kv_format,
                             "ms_per_step": round(dt * 1e3 / steps, 4), "tokens_per_s": round(B * steps / dt, 1),
                             "step_bytes": int(step_bytes), "step_frac": round(step_bytes / (dt / steps) / 1e9 / HBM_PEAK_GBPS, 4)}
        except Exception as exc:
            out[name] = {"ms_per_step": None, "why": f"{type(exc).__name__}: {exc}"}
        finally:
            if eng is not None:
                eng.close()
    return out


def gpu_clocks(device_index: int = 0) -> dict:
    """Shader / memory clock, power and power cap of one GPU as rocm-smi reports them NOW (one call, bounded at 10 s): read before and after
    the timed region so that a box whose matrix-core-heavy legs run slow (profiles/README.md: the 64-sequence step measured 2.5 ms on
    three boxes of the pool and 4.3-4.5 ms on two others with the same binaries) can be told from the line itself."""
    import shutil
    import subprocess

    exe = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    try:
        r = subprocess.run([exe, "-d", str(device_index), "--showclocks", "--showpower", "--showmaxpower", "--showperflevel", "--json"],
                           capture_output=True, text=True, timeout=10)
        card = next(iter(json.loads(r.stdout).values()))
        out = {}
        for key, val in card.items():
            k = key.lower()
            mhz = "".join(ch for ch in str(val) if ch.isdigit())
            if "sclk clock speed" in k: out["sclk_mhz"] = int(mhz) if mhz else val
            elif "mclk clock speed" in k: out["mclk_mhz"] = int(mhz) if mhz else val
            elif "fclk clock speed" in k: out["fclk_mhz"] = int(mhz) if mhz else val
            elif "max graphics package power" in k: out["power_cap_w"] = float(val)
            elif "power" in k and "(w)" in k and "max" not in k: out["power_w"] = float(val)
            elif "performance level" in k: out["perf_level"] = val
        return out or {"why": "rocm-smi --json returned no clock field", "keys": sorted(card)[:12]}
    except Exception as exc:
        return {"why": f"{type(exc).__name__}: {exc}"}


def gpu_clocks_under_load(device: str, device_index: int) -> dict:
    """The same reading while the GPU runs ~0.7 s of bf16 matrix products (torch.mm, enqueued first): the shader clock the matrix cores
    actually get on THIS box -- an idle reading says 95 MHz on every box."""
    import torch

    try:
        a = torch.randn((8192, 8192), dtype=torch.bfloat16, device=device)
        b = torch.randn((8192, 8192), dtype=torch.bfloat16, device=device)
        for _ in range(8):
            c = a @ b
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(64):
            c = a @ b
        torch.cuda.synchronize()
        per = (time.perf_counter() - t0) / 64
        n = max(64, min(4096, int(1.2 / per)))
        for _ in range(n):
            c = a @ b
        time.sleep(0.25)
        out = gpu_clocks(device_index)
        torch.cuda.synchronize()
        del a, b, c
        out["load"] = "torch.mm 8192^3 bf16, %.0f TFLOP/s" % (2 * 8192 ** 3 / per / 1e12)
        return out
    except Exception as exc:
        return {"why": f"{type(exc).__name__}: {exc}"}


def serving64_leg(mlx_model, cfg: dict, device: str, seed: int, page: int = 128) -> dict:
    """BASELINE.json configs[3] on ONE GPU as the reference runs it (benches/bench.py:351-572 -> benches/serving.py): the reference's
    serving trace scaled to 64 decode slots -- `--num-seqs 128 --batch-size 64`, 128-1,024 tokens in / 32-128 out, 128-token chunks,
    seed 0 (book/src/appendix-performance.md:22-27,528-541) -- under the reference's admission rule (one chunk of one request per turn)
    and under the 2,048-token admission budget with 8 staging slots (one packed multi-token pass per turn); since the end of round 6 also under a
    4,096-token budget in chunks of up to 1,024 tokens over 16 staging slots (the plain bf16 prefill GEMM is at its best from 3,072 rows).  GPU only, after
    the timed region; one engine for all; a complete-request warm-up of 32 requests first (graph captures of every row bucket)."""
    import torch
    from random import Random

    from benches.bench import build_requests
    from benches.serving import serve_requests, nearest_rank, median
    from tiny_llm_hip.engine import DecodeEngine

    B, staging, staging_max = 64, 8, 16
    trace = build_requests(rng=Random(0), num_seqs=128, vocab_size=cfg["vocab_size"], eos_token_id=cfg["vocab_size"] - 1,
                           min_input_len=128, max_input_len=1024, min_output_len=32, max_output_len=128)
    longest = max(len(r.prompt_token_ids) + r.max_new_tokens for r in trace)
    pages_per_seq = (longest + page - 1) // page + 1
    slots = B + staging_max
    kv_page_bytes = 2 * cfg["num_hidden_layers"] * cfg["num_key_value_heads"] * page * cfg["head_dim"] * 2
    out = {"requests": len(trace), "decode_slots": B, "prompt_tokens": sum(len(r.prompt_token_ids) for r in trace),
           "shape": "128-1,024 tokens in / 32-128 out, 128-token chunks, seed 0 (the reference's serving trace at 64 slots)"}
    eng = None
    try:
        eng = DecodeEngine(mlx_model, page_size=page, num_pages=pages_per_seq * slots + 2, max_batch=slots, max_pages_per_seq=pages_per_seq,
                           max_prefill_rows=4096)
        notes = {"reference_admission": "one 128-token chunk of one request per turn (batch.py:48-76)",
                 "budget_2048": "up to 2,048 prompt tokens per turn over 8 staging slots, one packed pass",
                 "budget_4096": "up to 4,096 prompt tokens per turn in chunks of up to 1,024 over 16 staging slots, one packed pass"}
        for name, kw in (("reference_admission", dict(prefill_step=128, prefill_budget=128, staging_slots=1)),
                         ("budget_2048", dict(prefill_step=512, prefill_budget=2048, staging_slots=staging)),
                         ("budget_4096", dict(prefill_step=1024, prefill_budget=4096, staging_slots=staging_max))):
            def run(reqs):
                return serve_requests(eng, reqs, batch_size=B, page_size=page, kv_bytes_per_page=kv_page_bytes, capacity_pages=pages_per_seq * slots + 2, **kw)
            run(trace[:32])
            eng.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = run(trace)
            eng.synchronize()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            steps = m.decode_step_ms
            out[name] = {"admission": notes[name],
                         "wall_s": round(wall, 3), "output_tok_s": round(m.generated_tokens / wall, 1),
                         "total_tok_s": round((out["prompt_tokens"] + m.generated_tokens) / wall, 1),
                         "decode_tok_s": round(m.decode_tokens / m.decode_time, 1) if m.decode_time else None,
                         "prefill_tok_s": round(out["prompt_tokens"] / m.prefill_time, 1) if m.prefill_time else None,
                         "req_s": round(len(trace) / wall, 2), "step_p50_ms": round(median(steps), 3) if steps else None,
                         "step_p95_ms": round(nearest_rank(steps, 0.95), 3) if steps else None, "decode_steps": m.decode_step_count,
                         "peak_active_requests": m.peak_active_requests,
                         "decode_bytes_per_step": int(m.decode_bytes / m.decode_step_count) if m.decode_step_count else None}
    except Exception as exc:
        out["why"] = f"{type(exc).__name__}: {exc}"
    finally:
        if eng is not None:
            eng.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed decode steps (default 256; 64 / 32 for --config 3 / 5)")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--model", default="qwen3-4b")
    ap.add_argument("--config", type=int, default=2, choices=(2, 3, 5),
                    help="BASELINE.json workload: 2 = configs[1] single-prompt decode (the metric's configuration, default), "
                         "3 = configs[2] 8k chunked prefill + paged decode, 5 = configs[4] 32k prefill + split-K decode")
    ap.add_argument("--prompt-len", type=int, default=None)
    ap.add_argument("--prefill-step", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--profile-steps", type=int, default=8)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra-configs", action="store_true", help="skip the short configs[2] / configs[4] / 64-sequence runs behind the timed region")
    ap.add_argument("--cpu-legs-budget", type=float, default=60.0,
                    help="seconds the CPU legs may take together (C port + float64 truth, peaked checkpoint, torch-CPU restatement of the "
                         "Week-2 kv-cache path): a leg that would start past its share is skipped and says so; 300 runs all three")
    ap.add_argument("--cpu-prompt", type=int, default=32,
                    help="prompt tokens the C checkers walk (token by token, ~0.4 s each per checker): 32 keeps the CPU legs near a minute; "
                         "128 checks the engine at the timed steps' own attention plan (4 windows) -- the GPU suite holds that plan against "
                         "the float64 truth in tests/test_zz_engine_windows_vs_truth_gpu.py")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly (for rocprofv3 kernel traces)")
    ap.add_argument("--no-clocks", action="store_true", help="skip the rocm-smi clock / power readings (the rocprofv3 child of this command: its trace should hold the bench's own kernels only)")
    ap.add_argument("--rocprof-stats", default=None,
                    help="rocprofv3 --kernel-trace --stats CSV of this command to recompute the GEMV rate from (default: the newest "
                         "committed profiles/r*_rocprofv3/bench_config<N>_kernel_stats.csv; 'none' to leave the block out)")
    ap.add_argument("--rocprof", default="live", choices=("live", "committed", "off"),
                    help="live (default): run this command once more under rocprofv3 after the timed region and take roofline.achieved / "
                         "frac from its kernel durations; committed: replay the newest committed summary; off: in-kernel stamps only")
    ap.add_argument("--engine", default="hip", choices=("hip", "sleep"),
                    help="sleep = launch-path plumbing test without a GPU (gloo); never a measurement")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (logits float32, token ids float64)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: roofline leg + rocprofv3 child, GPU clocks, extra configs, "
                         "CPU baselines / checkers (a plain run only sets up, warms up and times --steps steps)")
    args = ap.parse_args()
    t_start = time.perf_counter()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(sys.argv[1:], args.gpus)  # does not return
    workload = {2: ("Qwen3-4B int4 single-prompt KV-cache decode (BASELINE.json configs[1])", 128, 128, 256),
                # (4,096-token prefill chunks since round 6: from 3,072 rows a chunk's projections run on the plain bf16 GEMM over the bf16 weight
                # copy -- csrc/gemm8.h --, 987 against 742 TFLOP/s for a layer; --prefill-step 2048 is the round-5 shape)
                3: ("Qwen3-4B int4 chunked-prefill 8k + paged-KV decode (BASELINE.json configs[2])", 8192, 4096, 64),
                5: ("Qwen3-4B 32k long-context paged FlashAttention prefill + split-K decode (BASELINE.json configs[4])",
                    32768, 4096, 32)}[args.config]
    if args.prompt_len is None:
        args.prompt_len = workload[1]
    if args.prefill_step is None:
        args.prefill_step = workload[2]
    if args.steps is None:
        args.steps = workload[3]

    import torch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("bench.py --gpus N>1 must be launched with torch.distributed.run (one rank per GPU)")
        args.gpus = world
    dry = args.engine == "sleep"
    if not dry and not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    if not dry:
        torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if dry:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from tiny_llm_hip.synthetic import QWEN3_CONFIGS

    cfg = dict(QWEN3_CONFIGS[args.model])
    device = "cpu" if dry else f"cuda:{local_rank}"
    total_ctx = args.prompt_len + args.warmup + args.steps + args.profile_steps + 64
    page = 128
    if dry:
        mlx_model, engine = None, SleepEngine()
        args.profile_steps, args.no_cpu_baseline = 0, True
    else:
        from tiny_llm_hip.engine import DecodeEngine
        from tiny_llm_hip.synthetic import synthetic_qwen3

        mlx_model = synthetic_qwen3(cfg, seed=args.seed, sigma=0.02, device=device)
        engine = DecodeEngine(mlx_model, page_size=page, num_pages=(total_ctx + page - 1) // page + 2, max_batch=1,
                              max_prefill_rows=max(args.prefill_step, 8))
    prompt = build_prompt(random.Random(args.seed * 1000 + rank), args.prompt_len, cfg["vocab_size"])
    use_graph = not args.no_graph
    engine.timed_prefill_chunk = args.prefill_step  # cpu_baseline_leg checks a second sample prefilled at this chunk size

    def sync():
        engine.synchronize()
        if not dry:
            torch.cuda.synchronize()

    engine.begin(0)  # untimed pass first: code objects, workspace first touch (the reported prefill rate is the warm one)
    engine.prefill(0, prompt, chunk=args.prefill_step)
    engine.synchronize()
    engine.release(0)
    engine.begin(0)
    t_p0 = time.perf_counter()
    engine.prefill(0, prompt, chunk=args.prefill_step)
    engine.synchronize()
    prefill_s = time.perf_counter() - t_p0
    engine.decode(max(args.warmup, 2), batch=1, use_graph=use_graph)  # >= 2: eager warm step + graph capture
    sync()
    bytes_first = engine.step_bytes(1)
    clocks = None if dry or args.no_clocks or not args.full else {"before": gpu_clocks(local_rank)}
    progress("timed region")
    elapsed, local_elapsed = timed_steps(lambda k: engine.decode(k, batch=1, use_graph=use_graph), sync, args.steps, dist, device)
    bytes_last = engine.step_bytes(1)
    if args.dump_outputs and rank == 0:  # before anything else runs on the engine: the last timed step's logits and the timed ids
        dump_outputs(Path(args.dump_outputs), engine, args.steps, dry)
    if clocks is not None:
        clocks["after"] = gpu_clocks(local_rank)
        if rank == 0:
            clocks["under_matmul_load"] = gpu_clocks_under_load(device, local_rank)
    route_here = engine.replay_route() if hasattr(engine, "replay_route") else "none"
    per_rank = None
    if dist is not None:  # every rank's own clock over the timed region (one all_gather AFTER it): a straggler GPU shows here
        # ... and every rank's replay route: a rank that fell back to hipGraphLaunch (no code objects, no HSA agent for its device) is slower
        # by ~6 % and would otherwise show only as a slower entry (1 = AQL packets, 0 = anything else)
        t = torch.tensor([local_elapsed, 1.0 if route_here == "aql" else (0.0 if route_here.startswith("hipgraph") else -1.0)], dtype=torch.float64, device=device)
        gathered = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(gathered, t)
        secs = [float(g[0].item()) for g in gathered]
        rates = [args.steps / x for x in secs]
        per_rank = {"ms_per_step": [round(x * 1e3 / args.steps, 4) for x in secs], "tokens_per_s": [round(r, 2) for r in rates],
                    "min_tokens_per_s": round(min(rates), 2), "max_tokens_per_s": round(max(rates), 2),
                    "slowest_rank": int(max(range(world), key=lambda i: secs[i])),
                    "replay_route": [{1.0: "aql", 0.0: "hipgraph"}.get(float(g[1].item()), "none") for g in gathered]}
    ids = engine.read_tokens(0, 8)

    # ---- roofline leg: per-kernel device-clock durations of real decode steps (not part of the timed region)
    prof = None
    for _ in range(max(args.profile_steps, 0) if args.full else 0):
        p = engine.profile_step(1)
        if prof is None:
            prof = p
        else:
            for k, v in p["kinds"].items():
                prof["kinds"][k]["us"] += v["us"]
            prof["span_us"] += p["span_us"]
    stats = engine.stats()
    # "aql": the captured step replays as hand-written AQL packets on the engine's own HSA queue, no cache maintenance between its
    # launches (the default; csrc/aql.h); "hipgraph...": hipGraphLaunch (TL_AQL=0, or the route was not available: the text says why)
    replay_route = engine.replay_route() if hasattr(engine, "replay_route") else "none"
    engine.release(0)

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    ms_per_step = elapsed * 1e3 / args.steps
    step_bytes = 0.5 * (bytes_first + bytes_last)
    step_gbps = step_bytes / (elapsed / args.steps) / 1e9
    roofline = {"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": None, "traffic": None}
    if prof:
        n = max(args.profile_steps, 1)
        kinds = prof["kinds"]
        gemv = [k for k in kinds if k.startswith("gemv_")]
        g_us = sum(kinds[k]["us"] for k in gemv) / n
        g_bytes = sum(kinds[k]["bytes"] for k in gemv)
        g_launch = sum(kinds[k]["launches"] for k in gemv)
        ach = g_bytes / g_us / 1e3
        kv_bytes = max(step_bytes - g_bytes, 0.0)  # K and V of the cached context, read once per step
        attn_us = (kinds["attention"]["us"] + kinds["attention_merge"]["us"]) / n
        roofline.update({
            "kernel": "tl::qmv3_kernel<...> (W4A16 decode GEMV on MFMA over the tiled weight layout; fused RMSNorm / residual / SwiGLU variants)",
            "achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBPS, 4),
            "frac_of_measured_copy_peak": round(ach / HBM_COPY_GBPS, 4),
            "launches_per_step": g_launch, "launches_per_step_all_kernels": sum(v["launches"] for v in kinds.values()),
            "bytes_per_launch_avg": round(g_bytes / g_launch),
            "avg_launch_us": round(g_us / g_launch, 3),
            "timing": "in-kernel device wall clock, tl_engine_profile_step, mean of %d steps" % n,
            "per_kind": {k: {"us_per_step": round(v["us"] / n, 2), "launches": v["launches"],
                             "GBps": round(v["bytes"] / (v["us"] / n) / 1e3, 1) if v["bytes"] and v["us"] else None}
                         for k, v in kinds.items()},
            "kernel_time_us_per_step": round(sum(v["us"] for v in kinds.values()) / n, 1),
            "attention_kv": {"bytes_per_step": int(kv_bytes), "us_per_step": round(attn_us, 2),
                             "GBps": round(kv_bytes / attn_us / 1e3, 1) if attn_us else None,
                             "frac": round(kv_bytes / attn_us / 1e3 / HBM_PEAK_GBPS, 4) if attn_us else None,
                             "n_splits": prof.get("n_splits")},
        })
        if kv_bytes > g_bytes:  # long contexts: the K/V stream, not the weights, is the dominant traffic
            roofline["dominant"] = "decode attention (K/V pages): see attention_kv; achieved/frac stay the GEMV stream's"
        progress("roofline: rocprofv3 child")
        # rocprofv3-derived rate: measured now (a child of this process under rocprofv3), else the newest committed summary
        stats_csv, live = None, False
        if args.rocprof_stats == "none" or args.rocprof == "off":
            stats_csv = None
        elif args.rocprof_stats:
            stats_csv = Path(args.rocprof_stats).resolve()
        else:
            if args.rocprof == "live" and args.gpus == 1:
                stats_csv = rocprof_live(args)
                live = stats_csv is not None
            if stats_csv is None:
                stats_csv = latest_rocprof_stats(args.config)
        rp = rocprof_gemv_rate(stats_csv, kinds, cfg["num_hidden_layers"], live=live) if stats_csv else None
        if rp:
            meta = Path(str(stats_csv) + ".meta.json")
            if live:
                rp["captured_utc"] = time.strftime("%Y-%m-%d %H:%M", time.gmtime())
                try:
                    meta.write_text(json.dumps({"captured_utc": rp["captured_utc"], "command": "bench.py --config %d --steps 20 --warmup 5 (child of bench.py under rocprofv3 --kernel-trace --stats)" % args.config}))
                except OSError:
                    pass
            elif meta.exists():
                try:
                    rp["captured_utc"] = json.loads(meta.read_text()).get("captured_utc")
                except Exception:
                    pass
            rp["stamp_minus_rocprof_us_per_launch"] = round(rp["avg_launch_us"] - g_us / g_launch, 3)
            roofline["rocprof"] = rp
            if live:
                # the headline figure is the conservative one: rocprofv3's dispatch durations (ramp and write-back included), measured in this run
                roofline["achieved_in_kernel_stamps"], roofline["frac_in_kernel_stamps"] = roofline["achieved"], roofline["frac"]
                roofline["achieved"], roofline["frac"] = rp["achieved"], rp["frac"]
                roofline["frac_of_measured_copy_peak"] = round(rp["achieved"] / HBM_COPY_GBPS, 4)
                roofline["avg_launch_us_in_kernel_stamps"], roofline["avg_launch_us"] = roofline["avg_launch_us"], rp["avg_launch_us"]
                roofline["frac_source"] = "rocprofv3 --kernel-trace --stats of this command, measured in this run"
            else:
                # a replayed summary is NOT this run: it stays a side block; the headline keeps this run's own in-kernel stamps
                roofline["frac_source"] = ("in-kernel device wall-clock stamps of this run (optimistic by ~0.8 us per launch); roofline.rocprof is "
                                           "replayed from " + rp["file"] + " (rocprofv3 did not run here) and is not this run's figure")
        else:
            roofline["frac_source"] = "in-kernel device wall-clock stamps (no rocprofv3 summary available): optimistic by ~0.8 us per launch"
        # HBM bytes by hardware counters.  First choice: the passes over the ENGINE's own decode step (tools/lab/pmc_engine_step.sh drives
        # the C ABI without Python: rocprofv3's counter mode crashes under this bench); fallback: the GEMV lab's replay of the kernels.
        engine_traffic = ROOT / "profiles" / "traffic_engine.json"
        traffic_file = ROOT / "profiles" / "traffic.json"
        try:
            if engine_traffic.exists():
                et = json.loads(engine_traffic.read_text())
                ctx = min(et["contexts"], key=lambda c: abs(int(c) - args.prompt_len))
                row = et["contexts"][ctx]
                roofline["traffic"] = row["gemv_hbm_bytes_per_launch"]
                roofline["traffic_step"] = {"context_tokens": int(ctx), "hbm_read_bytes": row["step_hbm_read_bytes"], "hbm_write_bytes": row["step_hbm_write_bytes"],
                                            "algorithmic_bytes": row["step_algorithmic_bytes"], "hbm_over_algorithmic": row["hbm_over_algorithmic"],
                                            "launches": row["launches_per_step"]}
                roofline["traffic_note"] = ("HBM bytes per GEMV launch (and per whole decode step: traffic_step) from rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over the "
                                            "engine's own decode step at " + ctx + " tokens of context (tools/lab/engine_step_lab through the C ABI); NOT measured in this run: "
                                            "replayed from the committed profiles/traffic_engine.json (" + str(et.get("collected", "")) + ")")
            elif traffic_file.exists():
                traffic = json.loads(traffic_file.read_text())
                roofline["traffic"] = traffic.get("qmv_hbm_bytes_per_launch")
                roofline["traffic_note"] = ("HBM bytes per GEMV launch from rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over tools/lab/gemv_lab; NOT measured in "
                                            "this run: replayed from the committed profiles/traffic.json (" + str(traffic.get("collected", "round 3")) + ")")
        except Exception:
            roofline["traffic"] = None
    roofline["step_achieved"] = round(step_gbps, 1)
    roofline["step_frac"] = round(step_gbps / HBM_PEAK_GBPS, 4)
    roofline["step_bytes"] = int(step_bytes)

    extra = None
    if args.full and args.gpus == 1 and not dry and args.config == 2 and not args.no_extra_configs:
        progress("extra configs: 8k, 32k, 64 sequences")
        extra = extra_configs_leg(mlx_model, cfg, device, args.seed, page)
        progress("extra configs done; serving trace at 64 slots")
        try:
            with time_box(90):
                extra["serving64"] = serving64_leg(mlx_model, cfg, device, args.seed, page)
        except Exception as exc:
            extra["serving64"] = {"why": f"{type(exc).__name__}: {exc}"}
        progress("serving trace done")

    cpu = None
    if args.full and args.gpus == 1 and not args.no_cpu_baseline:
        # at the bench's own prompt length (bounded at 128 tokens: the C checkers walk the prompt token by token), through the
        # bench's own prefill chunking, so that the checked decode steps run the attention plan of the timed ones
        sample_prompt = min(args.prompt_len, max(8, args.cpu_prompt))
        t_cpu0 = time.perf_counter()
        try:
            with time_box(max(90, int(1.5 * args.cpu_legs_budget))):
                # the checked engine is prefilled in 8-row passes: rows <= 8 take the matvec arithmetic (quantize.py:54-65), which is what the
                # C port walks the prompt with -- a 128-row chunk takes the tile GEMM, whose weights are rounded to bf16 first
                # (quantized_matmul.metal:96-249): reference-mandated extra rounding in the cached K/V that is not the decode kernels' error
                fp8_engine = None
                if device != "cpu" and cfg.get("head_dim") == 128:
                    try:
                        from tiny_llm_hip.engine import DecodeEngine as _DE

                        fp8_engine = _DE(mlx_model, page_size=page, num_pages=4, max_batch=1, max_prefill_rows=8, kv_format="fp8")
                    except Exception:
                        fp8_engine = None
                try:
                    cpu = cpu_baseline_leg(mlx_model, cfg, engine, sample_prompt=sample_prompt, sample_steps=16, prefill_chunk=8, fp8_engine=fp8_engine)
                finally:
                    if fp8_engine is not None:
                        fp8_engine.close()
        except Exception as exc:
            cpu = {"value": None, "unit": "tokens/s", "cores": 0, "kind": "port", "sample": f"failed: {type(exc).__name__}: {exc}"}
        cpu["n_splits_timed"] = prof.get("n_splits") if prof else None
        c_prompt, c_fed, c_first = cpu.pop("_prompt", None), cpu.pop("_fed", None), cpu.pop("_gpu_first_decode_logits", None)
        if c_prompt is None:  # the C checkers are not built: same sample, greedy on its own ids
            c_prompt, c_fed = build_prompt(random.Random(1234), sample_prompt, cfg["vocab_size"]), None
        # the optional legs run only while the whole command is inside its time box (the driver expects a line within minutes).
        # The torch leg comes LAST: its thread pool keeps spinning on every logical CPU afterwards and starves the C checkers
        # (round 4: the peaked leg's 16 truth steps did not finish in 90 s behind it).
        if time.perf_counter() - t_start > 300 or time.perf_counter() - t_cpu0 > 0.8 * args.cpu_legs_budget:
            cpu["peaked_checkpoint"] = {"checked": False, "why": "skipped: the CPU legs had used their minute (tests/test_engine_qwen4b_gpu.py holds the same check)"}
        else:
            try:
                progress("peaked_checkpoint leg")
                with time_box(max(30, int(0.5 * args.cpu_legs_budget))):
                    cpu["peaked_checkpoint"] = peaked_checkpoint_leg(cfg, device, args.seed, steps=6)
            except Exception as exc:
                cpu["peaked_checkpoint"] = {"checked": False, "why": f"{type(exc).__name__}: {exc}"}
        if time.perf_counter() - t_start > 360 or time.perf_counter() - t_cpu0 > 0.7 * args.cpu_legs_budget:
            cpu["torch_week2_kv_cache"] = {"value": None, "why": "skipped: the CPU legs had used their minute (python bench.py --cpu-legs-budget 300 runs it; "
                                                                  "profiles/r04_bench_config2.json holds round 4's figure)"}
        else:
            try:
                progress("torch_week2_kv_cache leg")
                with time_box(max(40, int(0.7 * args.cpu_legs_budget))):
                    cpu["torch_week2_kv_cache"] = torch_week2_leg(mlx_model, cfg, c_prompt, c_fed[:8] if c_fed else [0] * 8, c_first)
            except Exception as exc:  # a reported baseline must not take the measurement with it (e.g. a host without 9 GB to spare)
                cpu["torch_week2_kv_cache"] = {"value": None, "why": f"{type(exc).__name__}: {exc}"}
        progress("CPU legs done")
        cpu["seconds_since_start"] = round(time.perf_counter() - t_start, 1)
        cpu["cpu_legs_seconds"] = round(time.perf_counter() - t_cpu0, 1)

    out = {
        "metric": "Qwen3-4B int4 decode tokens/sec/GPU; achieved HBM GB/s vs roofline",
        "value": round(aggregate_value(args.gpus, args.steps, elapsed), 2),
        "unit": "tokens/s",
        "n_gpus": args.gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16",
        "dtype_note": "int4 (W4A16, group 128) weights x bf16 activations on bf16 MFMA, fp32 accumulate",
        "data": "none (--engine sleep: launch-path plumbing test, NOT a measurement)" if dry else
                "synthetic (random-init Qwen3-4B-shaped W4 weights, synthetic token ids)",
        "config": {"workload": workload[0],
                   "prompt_tokens": args.prompt_len, "decode_steps": args.steps, "batch_per_gpu": 1,
                   "parallelism": f"request-parallel x{args.gpus} (no collective on the data path)",
                   "page_size": page, "graph_replay": use_graph, "prefill_step": args.prefill_step, "replay_route": replay_route},
        "tokens_per_s_per_gpu": round(args.steps / elapsed, 2),
        "per_rank": per_rank,
        "prefill_tokens_per_s": round(args.prompt_len / prefill_s, 1),
        "roofline": roofline,
        "cpu_baseline": cpu,
        "extra_configs": extra,
        "clocks": clocks,
        "engine": dict({k: stats[k] for k in ("graph_captures", "graph_replays", "decode_steps", "kv_bytes")}, aql_steps=stats.get("aql_steps"),
                       replay_route=replay_route),
        "first_ids": ids,
    }
    print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
