"""Test-only oracles for LoRA adapters (csrc/lora.h; tl_lora_rows, tl_engine_lora_load, tl_engine_set_lora).

An adapter is a dict ``{(layer, target): (A [r, in], B [out, r])}`` of float32 arrays holding bf16 values, a rank and a scale; targets
are q, k, v, o, gate, up, down.  ``LoraOracleQwen3`` is the bf16 oracle with ``bf16(y + scale * (B (A x)))`` behind every adapted
projection (t = A x kept in fp32), ``LoraTruthQwen3`` the float64 truth over ``W + scale * B @ A``.  ``lora_rows_reference`` is the
float64 arithmetic of the routine over caller rows with the per-element allowance of its test.
"""

from __future__ import annotations

import numpy as np

from oracle import tiny_oracle as O

TARGETS = ("q", "k", "v", "o", "gate", "up", "down")


def target_shapes(cfg: dict) -> dict:
    """target -> (in, out) of a Qwen3 layer."""
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    q, kv = cfg["num_attention_heads"] * cfg["head_dim"], cfg["num_key_value_heads"] * cfg["head_dim"]
    return {"q": (H, q), "k": (H, kv), "v": (H, kv), "o": (q, H), "gate": (H, I), "up": (H, I), "down": (I, H)}


def make_adapter(cfg: dict, rank: int, targets=TARGETS, seed: int = 0, sigma: float = 0.05, scale: float = 1.0) -> dict:
    """A, B ~ N(0, sigma) rounded to bf16, for every layer and every target of ``targets``."""
    rng = np.random.default_rng(seed)
    shapes = target_shapes(cfg)
    weights = {}
    for layer in range(cfg["num_hidden_layers"]):
        for t in TARGETS:  # (drawn for every target so that a subset shares its matrices with the full adapter of the same seed)
            n_in, n_out = shapes[t]
            a = O.bf16(rng.standard_normal((rank, n_in), dtype=np.float32) * sigma)
            b = O.bf16(rng.standard_normal((n_out, rank), dtype=np.float32) * sigma)
            if t in targets:
                weights[(layer, t)] = (a, b)
    return dict(rank=rank, scale=float(scale), weights=weights)


def to_lora_adapter(adapter: dict):
    """The oracle's adapter as the product's ``tiny_llm_hip.lora.LoraAdapter`` (bf16 CPU tensors)."""
    import torch
    from tiny_llm_hip.lora import LoraAdapter

    w = {k: tuple(torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(torch.bfloat16) for m in ab) for k, ab in adapter["weights"].items()}
    return LoraAdapter(rank=int(adapter["rank"]), scale=float(adapter["scale"]), weights=w)


def _by_weight(weights: dict, adapter: dict | None) -> dict:
    """id(packed words of a base projection) -> (A, B, scale)."""
    out = {}
    if adapter is None:
        return out
    for (layer, t), (a, b) in adapter["weights"].items():
        out[id(weights["layers"][layer][t][0])] = (np.asarray(a, np.float64), np.asarray(b, np.float64), float(adapter["scale"]))
    return out


class LoraOracleQwen3(O.OracleQwen3):
    """OracleQwen3 with an adapter: every adapted projection returns bf16(y + scale * (B (A x))), t = A x in fp32."""

    def __init__(self, cfg, weights, adapter=None, **kw):
        super().__init__(cfg, weights, **kw)
        self._lora = _by_weight(weights, adapter)

    def _linear(self, x, wt):
        y = super()._linear(x, wt)
        hit = self._lora.get(id(wt[0]))
        if hit is None:
            return y
        a, b, scale = hit
        t = (np.asarray(x, np.float64) @ a.T).astype(np.float32)  # fp32 t
        d = (t.astype(np.float64) @ b.T).astype(np.float32) * np.float32(scale)
        return O.bf16(y.astype(np.float32) + d)


class LoraTruthQwen3(O.TruthQwen3):
    """TruthQwen3 over the merged weights W + scale * B @ A, in float64."""

    def __init__(self, cfg, weights, adapter=None):
        super().__init__(cfg, weights)
        self._lora = _by_weight(weights, adapter)
        self._merged = {}

    def _weight(self, wt):
        w = super()._weight(wt)
        hit = self._lora.get(id(wt[0]))
        if hit is None:
            return w
        key = id(wt[0])
        if key not in self._merged:
            a, b, scale = hit
            self._merged[key] = w + scale * (b @ a)
        return self._merged[key]


def merged_weights_truth(cfg, weights, adapter):
    """A TruthQwen3 whose dense weights were replaced by W + scale * B @ A ahead of time: what LoraTruthQwen3 must equal."""
    truth = O.TruthQwen3(cfg, weights)
    for (layer, t), (a, b) in adapter["weights"].items():
        wt = weights["layers"][layer][t]
        truth._dense[id(wt[0])] = O.TruthQwen3._weight(truth, wt) + float(adapter["scale"]) * (np.asarray(b, np.float64) @ np.asarray(a, np.float64))
    return truth


# ---- the routine over caller rows ------------------------------------------------------------------------------------
def segment_of(out_cols: int, seg_mode: str, seg_ends=(0, 0)) -> np.ndarray:
    o = np.arange(out_cols)
    if seg_mode == "blocks":
        return (o >= seg_ends[0]).astype(int) + (o >= seg_ends[1]).astype(int)
    return o & 1 if seg_mode == "interleaved" else np.zeros(out_cols, dtype=int)


def lora_rows_reference(x, row_adapter, adapters, base, *, mode: str, seg_mode: str = "plain", seg_ends=(0, 0), norm_weight=None,
                        eps: float = 1e-6):
    """(want, allowed) in float64 for tiny_llm_ext_hip.lora_rows: ``adapters`` = (A_fused, B_fused, scale, seg_mask) float arrays.
    want: base + scale * B (A x) per row and segment (x normalised in float64 when ``norm_weight`` is given), through the SwiGLU for
    mode "swiglu".  allowed per element: one bf16 ulp of the result per store rounding (one; "swiglu" stores g', u' and the product:
    the ulps of g' and u' are carried through the product's derivatives, plus the product's own) plus
    (in + r) * 2^-23 * (|base| + |scale| * sum_j |B_oj| * sum_c |A_jc| |x_c|)."""
    from helpers import bf16_ulp

    x = np.asarray(x, np.float64)
    base = np.asarray(base, np.float64)
    rows, n_in = x.shape
    out_cols = base.shape[1]
    if norm_weight is not None:
        x = x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + eps) * np.asarray(norm_weight, np.float64)
    seg = segment_of(out_cols, seg_mode, seg_ends)
    d = np.zeros((rows, out_cols))
    mag = np.zeros((rows, out_cols))
    rank_of = np.zeros(rows)
    for i in range(rows):
        ad = int(row_adapter[i])
        if ad < 0:
            continue
        a, b, scale, mask = adapters[ad]
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        r = b.shape[1]
        rank_of[i] = r
        t = a @ x[i]
        t_abs = np.abs(a) @ np.abs(x[i])
        off = 0
        for s in range(3):
            if not (mask >> s) & 1:
                continue
            cols = np.nonzero(seg == s)[0]
            d[i, cols] = scale * (b[cols] @ t[off:off + r])
            mag[i, cols] = abs(scale) * (np.abs(b[cols]) @ t_abs[off:off + r])
            off += r
    fp32 = (n_in + rank_of[:, None]) * 2.0 ** -23 * (np.abs(base) + mag)
    y = base + d
    if mode != "swiglu":
        return y, bf16_ulp(y) + fp32
    g, u = y[:, 0::2], y[:, 1::2]
    sig = 1.0 / (1.0 + np.exp(-g))
    silu = g * sig
    dsilu = sig * (1.0 + g * (1.0 - sig))
    want = silu * u
    eg = bf16_ulp(g) + fp32[:, 0::2]
    eu = bf16_ulp(u) + fp32[:, 1::2]
    # first order in the stored g' and u', the cross term, the fp32 steps of the product (expf, the division, the multiply: 8 ulp_f32) and its rounding
    allowed = np.abs(dsilu * u) * eg + np.abs(silu) * eu + 1.1 * eg * eu + 8 * 2.0 ** -23 * np.abs(want) + bf16_ulp(want)
    return want, allowed
