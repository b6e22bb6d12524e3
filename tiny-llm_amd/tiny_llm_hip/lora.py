"""LoRA adapters for the decode engine (include/tinyllm_engine.h "LoRA adapters", csrc/lora.h).

``load_adapter(dir)`` reads an adapter directory into a ``LoraAdapter`` -- per (layer, target) the matrices A [r, in] and B [out, r] in
the PEFT orientation, bf16 on the CPU, plus rank and scale -- and ``DecodeEngine.load_lora`` hands it to the engine, which keeps it in
the fused layouts of the base weights.  ``fused_group`` builds those layouts on the host, for tests and for the routine over caller rows
(``tiny_llm_ext_hip.lora_rows``).

Two on-disk layouts are read.  BOTH ARE WRITTEN FROM MEMORY OF THE TWO PROJECTS: neither ``peft`` nor ``mlx_lm`` is installed here, no
adapter file was at hand, and no real adapter has ever been loaded.
  PEFT    ``adapter_config.json`` (``r``, ``lora_alpha``, ``use_rslora``, ``target_modules``) + ``adapter_model.safetensors`` with keys
          ``base_model.model.model.layers.N.{self_attn,mlp}.X_proj.lora_A.weight`` [r, in] / ``lora_B.weight`` [out, r];
          scale = alpha / r, or alpha / sqrt(r) with rsLoRA.
  mlx_lm  ``adapter_config.json`` with ``lora_parameters`` (``rank``, ``scale``) + ``adapters.safetensors`` with keys
          ``model.layers.N.{self_attn,mlp}.X_proj.lora_a`` [in, r] / ``lora_b`` [r, out] (the transposes); scale = lora_parameters.scale.
"""

from __future__ import annotations

import json
import math
import re
from dataclasses import dataclass, field
from pathlib import Path

import torch

TARGETS = ("q", "k", "v", "o", "gate", "up", "down")  # TL_LORA_Q .. TL_LORA_DOWN
GROUPS = {"qkv": ("q", "k", "v"), "o": ("o",), "gate_up": ("gate", "up"), "down": ("down",)}
MAX_RANK = 64
MAX_ADAPTERS = 32

_KEY = re.compile(r"(?:^|\.)layers\.(\d+)\.(?:self_attn|mlp)\.(q|k|v|o|gate|up|down)_proj\.(lora_A\.weight|lora_B\.weight|lora_a|lora_b)$")


@dataclass
class LoraAdapter:
    """One adapter: ``weights[(layer, target)] = (A [rank, in], B [out, rank])`` bf16 CPU tensors, PEFT orientation."""
    rank: int
    scale: float
    weights: dict = field(default_factory=dict)
    name: str = ""

    def targets(self) -> tuple[str, ...]:
        return tuple(t for t in TARGETS if any(k[1] == t for k in self.weights))

    def nbytes(self) -> int:
        return sum(a.numel() * 2 + b.numel() * 2 for a, b in self.weights.values())


def check_adapter(adapter: LoraAdapter) -> None:
    """ValueError unless the adapter is one the engine takes: rank a multiple of 8 up to 64, a finite scale, A [rank, in] and B [out, rank]
    for every pair, at least one pair."""
    r = adapter.rank
    if isinstance(r, bool) or not isinstance(r, int) or not 8 <= r <= MAX_RANK or r % 8:
        raise ValueError(f"LoRA rank must be a multiple of 8 up to {MAX_RANK}, got {r!r}")
    if not isinstance(adapter.scale, (int, float)) or not math.isfinite(adapter.scale):
        raise ValueError(f"LoRA scale must be finite, got {adapter.scale!r}")
    if not adapter.weights:
        raise ValueError("the adapter adapts nothing")
    for (layer, target), (a, b) in adapter.weights.items():
        if target not in TARGETS or not isinstance(layer, int) or layer < 0:
            raise ValueError(f"unknown LoRA target {(layer, target)!r}")
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != r or b.shape[1] != r:
            raise ValueError(f"layer {layer} {target}: A must be [rank, in] and B [out, rank], got {tuple(a.shape)} and {tuple(b.shape)}")


def load_adapter(path) -> LoraAdapter:
    """Read a PEFT or an mlx_lm adapter directory (module docstring) into a LoraAdapter."""
    from safetensors.torch import load_file

    d = Path(path)
    cfg_file = d / "adapter_config.json"
    if not cfg_file.exists():
        raise FileNotFoundError(f"no adapter_config.json in {d}")
    cfg = json.loads(cfg_file.read_text())
    peft_file, mlx_file = d / "adapter_model.safetensors", d / "adapters.safetensors"
    if peft_file.exists():
        tensors, peft = load_file(str(peft_file)), True
    elif mlx_file.exists():
        tensors, peft = load_file(str(mlx_file)), False
    else:
        raise FileNotFoundError(f"neither adapter_model.safetensors (PEFT) nor adapters.safetensors (mlx_lm) in {d}")
    halves: dict = {}
    for key, t in tensors.items():
        m = _KEY.search(key)
        if not m:
            raise ValueError(f"{d}: unsupported adapter tensor {key!r} (only q/k/v/o/gate/up/down_proj of the decoder layers are adapted)")
        layer, target, kind = int(m.group(1)), m.group(2), m.group(3)
        is_a = kind in ("lora_A.weight", "lora_a")
        if kind in ("lora_a", "lora_b"):  # mlx_lm stores the transposes
            t = t.t()
        halves.setdefault((layer, target), {})["a" if is_a else "b"] = t.to(torch.bfloat16).contiguous()
    weights = {}
    for k, h in halves.items():
        if "a" not in h or "b" not in h:
            raise ValueError(f"{d}: layer {k[0]} {k[1]}_proj has only one of its two matrices")
        weights[k] = (h["a"], h["b"])
    if not weights:
        raise ValueError(f"{d}: the adapter holds no tensors")
    rank = int(next(iter(weights.values()))[0].shape[0])
    if peft:
        if int(cfg.get("r", rank)) != rank:
            raise ValueError(f"{d}: adapter_config.json says r = {cfg.get('r')}, the tensors have rank {rank}")
        alpha = float(cfg.get("lora_alpha", rank))
        scale = alpha / math.sqrt(rank) if cfg.get("use_rslora") else alpha / rank
        listed = cfg.get("target_modules")
        if isinstance(listed, (list, tuple)):
            for t in {k[1] for k in weights}:
                if f"{t}_proj" not in listed:
                    raise ValueError(f"{d}: tensors for {t}_proj, which target_modules does not list")
    else:
        params = cfg.get("lora_parameters") or {}
        if "scale" not in params:
            raise ValueError(f"{d}: adapter_config.json has no lora_parameters.scale")
        scale = float(params["scale"])
        if int(params.get("rank", rank)) != rank:
            raise ValueError(f"{d}: lora_parameters.rank = {params.get('rank')}, the tensors have rank {rank}")
    adapter = LoraAdapter(rank=rank, scale=scale, weights=weights, name=d.name)
    check_adapter(adapter)
    return adapter


def fused_group(adapter: LoraAdapter, layer: int, group: str, widths: dict | None = None):
    """The fused layout the engine keeps for one projection group (csrc/lora.h): (A [rank * present targets, in], B [out, rank],
    seg_mask), or None when the adapter has no target of the group in that layer.  A is the present targets' A stacked in target
    order.  B holds the targets' rows one block after the other ("qkv") or interleaved 2i / 2i + 1 ("gate_up"); a missing target
    contributes no rows to A, zero rows to B -- ``widths[target]`` says how many -- and a cleared bit of seg_mask."""
    names = GROUPS[group]
    present = [t for t in names if (layer, t) in adapter.weights]
    if not present:
        return None
    r = adapter.rank
    a = torch.cat([adapter.weights[(layer, t)][0] for t in present], 0).contiguous()
    blocks = []
    for t in names:
        if t in present:
            blocks.append(adapter.weights[(layer, t)][1])
        elif widths is None or t not in widths:
            raise ValueError(f"fused_group: {t} is missing from the adapter; its output width must be given in widths")
        else:
            blocks.append(torch.zeros((int(widths[t]), r), dtype=torch.bfloat16))
    if group == "gate_up":
        if blocks[0].shape != blocks[1].shape:
            raise ValueError("fused_group: gate and up must have the same output width")
        b = torch.stack(blocks, dim=1).reshape(2 * blocks[0].shape[0], r)
    else:
        b = torch.cat(blocks, 0)
    mask = sum(1 << i for i, t in enumerate(names) if t in present)
    return a, b.contiguous(), mask


def request_loras(sampling, n_prompts: int) -> list[int] | None:
    """The ``"lora"`` key of batch_generate_ids' ``sampling``: one dict whose ``lora`` is an adapter id (or None / -1) for every request
    or a list with one id per request, or one dict per prompt.  Returns per prompt an id or -1; None when nothing asks for an adapter."""
    if sampling is None:
        return None
    if isinstance(sampling, dict):
        v = sampling.get("lora")
        per = list(v) if isinstance(v, (list, tuple)) else [v] * n_prompts
    else:
        per = [d.get("lora") if isinstance(d, dict) else None for d in sampling]
    if len(per) != n_prompts:
        raise ValueError("sampling['lora'] needs one adapter id per prompt (or one for all)")
    out = []
    for v in per:
        if v is None:
            v = -1
        if isinstance(v, bool) or not isinstance(v, int) or not -1 <= v < MAX_ADAPTERS:
            raise ValueError(f"sampling['lora'] must be None, -1 or an adapter id below {MAX_ADAPTERS}, got {v!r}")
        out.append(v)
    return out if any(v >= 0 for v in out) else None


def assign_adapters(n_requests: int, adapter_ids, policy: str = "round-robin") -> list[int]:
    """batch_main's --lora-assign: which adapter each of ``n_requests`` requests gets -- "round-robin": request i gets adapter
    i mod n; "first": request 0 gets the first adapter, every other request none (-1)."""
    ids = [int(a) for a in adapter_ids]
    if policy not in ("round-robin", "first"):
        raise ValueError(f"--lora-assign must be round-robin or first, got {policy!r}")
    if not ids:
        return [-1] * n_requests
    if policy == "first":
        return [ids[0] if i == 0 else -1 for i in range(n_requests)]
    return [ids[i % len(ids)] for i in range(n_requests)]
