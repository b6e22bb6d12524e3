"""Test-only oracles for the engine's MoE kernels (csrc/engine_kernels.h: moe_route_kernel, moe_silu_mul_kernel, moe_combine_kernel;
tl_moe_route_rows, tl_moe_experts_rows).  Plain numpy restatements of what the kernels' comments and include/tinyllm_engine.h state:

* the router in float64 -- softmax, each probability rounded to bf16, a stable descending top-k (equal probabilities: the lower expert
  index first), the scores, and the renormalisation with the kernel's two roundings (the float32 sum in selection order rounded to bf16,
  each float32 quotient rounded to bf16);
* which rows a float32 softmax decides the same way (`robust_rows`): every float64 probability stands clear of a bf16 rounding boundary;
* SiLU x up and the weighted sum + residual in float32, operation by operation as the kernels state them.

bf16 values travel as float32 arrays (oracle.tiny_oracle.bf16); nothing here runs on a device."""

import numpy as np

from oracle import tiny_oracle as O

ROBUST_MARGIN = 2.0 ** -17


def probs64(logits) -> np.ndarray:
    """Float64 softmax over the last axis of finite bf16 logits."""
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def stable_topk(probs, top_k: int) -> np.ndarray:
    """[rows, top_k] indices of the largest values, descending; equal values in ascending index order."""
    return np.argsort(-np.asarray(probs), axis=-1, kind="stable")[..., :top_k]


def renormalise(picked) -> np.ndarray:
    """The kernel's renormalisation of the selected bf16 probabilities [rows, k]: float32 sum in selection order, rounded to bf16;
    every float32 quotient rounded to bf16."""
    q = np.asarray(picked, dtype=np.float32)
    tot = np.zeros(q.shape[:-1], dtype=np.float32)
    for j in range(q.shape[-1]):
        tot = tot + q[..., j]
    den = O.bf16(tot)
    return O.bf16(q / den[..., None])


def route(logits, top_k: int, norm: bool):
    """(ids [rows, top_k], scores [rows, top_k] bf16, bf16 probabilities [rows, E], float64 probabilities) of the router."""
    p64 = probs64(logits)
    pb = O.bf16(p64)
    ids = stable_topk(pb, top_k)
    picked = np.take_along_axis(pb, ids, axis=-1)
    return ids, (renormalise(picked) if norm else picked), pb, p64


def robust_rows(p64, margin: float = ROBUST_MARGIN) -> np.ndarray:
    """Rows whose bf16 probabilities any softmax within a relative `margin` of the float64 one rounds to the same values:
    bf16(p (1 - margin)) == bf16(p (1 + margin)) for every expert."""
    p64 = np.asarray(p64, dtype=np.float64)
    return (O.bf16(p64 * (1.0 - margin)) == O.bf16(p64 * (1.0 + margin))).all(axis=-1)


def silu_mul(gate, up) -> np.ndarray:
    """act = bf16(bf16(silu(gate)) * up) with silu(g) = g / (1 + exp(-g)) in float32 (moe_silu_mul_kernel)."""
    g, u = np.asarray(gate, dtype=np.float32), np.asarray(up, dtype=np.float32)
    with np.errstate(over="ignore"):
        s = g / (np.float32(1.0) + np.exp(-g))
    return O.bf16(O.bf16(s) * u)


def silu_candidates(gate, rel: float = 2.0 ** -21):
    """The bf16 values bf16(silu(gate)) can take when the float32 evaluation stands within a relative `rel` of the float64 one
    (expf, one add, one divide: a few float32 steps): (low, high) -- equal wherever the rounding is decided."""
    g = np.asarray(gate, dtype=np.float64)
    s = g / (1.0 + np.exp(-g))
    return O.bf16(s * (1.0 - rel)), O.bf16(s * (1.0 + rel))


def combine(y, scores, h) -> np.ndarray:
    """out = bf16(h + bf16(sum_j bf16(y[:, j] * score[:, j]))) -- y [rows, k, D], scores [rows, k], h [rows, D]; the sum in float32
    from 0 in expert order, rounded once (moe_combine_kernel)."""
    y, sc, h = (np.asarray(a, dtype=np.float32) for a in (y, scores, h))
    acc = np.zeros(h.shape, dtype=np.float32)
    for j in range(y.shape[1]):
        acc = acc + O.bf16(y[:, j] * sc[:, j, None])
    return O.bf16(h + O.bf16(acc))


def weighted_sum(y, scores, per_add: bool = False) -> np.ndarray:
    """bf16(sum_j bf16(y_j * score_j)) in float32 in expert order, rounded once; per_add=True: the form that rounds to bf16 after
    every add (what oracle.moe_block stated before it took the kernel's definition -- the same operation for k <= 2)."""
    y, sc = np.asarray(y, dtype=np.float32), np.asarray(scores, dtype=np.float32)
    w = O.bf16(y * sc[..., None])
    acc = w[:, 0]
    for j in range(1, y.shape[1]):
        acc = O.bf16(acc + w[:, j]) if per_add else acc + w[:, j]
    return O.bf16(acc)


def selection_ratio(p64, ids) -> np.ndarray:
    """Per row max over chosen i and unchosen j of p64[j] / p64[i]: how far a selection stands from a top-k of the float64
    probabilities (<= 1 for an exact one)."""
    p64, ids = np.asarray(p64, dtype=np.float64), np.asarray(ids)
    chosen = np.zeros(p64.shape, dtype=bool)
    np.put_along_axis(chosen, ids, True, axis=-1)
    if chosen.all():
        return np.zeros(p64.shape[0])
    lowest = np.take_along_axis(p64, ids, axis=-1).min(axis=-1)
    return np.where(chosen, 0.0, p64).max(axis=-1) / lowest
