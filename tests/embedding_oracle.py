"""Test-only oracles for text embeddings (csrc/pool.h; tl_pool_rows, tl_engine_embed, tl_engine_embed_packed).

* ``final_rows``: the model's output rows -- the final RMSNorm of the last layer's hidden rows -- out of the existing oracles without
  touching them: the weight dict gets an identity ``lm_head`` (W4 codes of eye(hidden): code 1 on the diagonal, scale 1, bias 0), so
  ``forward(tokens, logits_to_keep=None)`` returns the rows themselves -- OracleQwen3 the bf16 rows exactly (a row times the identity is
  the row, at any accumulation precision), TruthQwen3 the float64 rows.
* ``pool`` / ``finish``: the pooling definition in float64 numpy.
* ``pool_allowance``: the per-element allowance of an fp32 kernel against ``pool``, derived from the magnitudes that were summed.
"""

import numpy as np

from oracle import tiny_oracle as O


def identity_head(hidden: int):
    """(packed, scales, biases) of eye(hidden) as a W4 tensor of the mlx_lm layout: 8 nibbles per uint32 word, element 8 j + i in bits
    [4 i, 4 i + 4); one (scale 1, bias 0) per group of 128."""
    assert hidden % 128 == 0
    codes = np.eye(hidden, dtype=np.uint32).reshape(hidden, hidden // 8, 8)
    packed = np.zeros((hidden, hidden // 8), dtype=np.uint32)
    for i in range(8):
        packed |= codes[..., i] << np.uint32(4 * i)
    assert np.array_equal(O.unpack_codes(packed), np.eye(hidden, dtype=np.uint32))
    return packed, np.ones((hidden, hidden // 128), dtype=np.float32), np.zeros((hidden, hidden // 128), dtype=np.float32)


def with_identity_head(weights: dict, hidden: int) -> dict:
    return dict(weights, lm_head=identity_head(hidden))


def final_rows(model_cls, cfg: dict, weights: dict, tokens, **kwargs) -> np.ndarray:
    """[len(tokens), hidden] final-norm rows of ``model_cls`` (O.OracleQwen3: exact bf16 values; O.TruthQwen3: float64)."""
    model = model_cls(cfg, with_identity_head(weights, cfg["hidden_size"]), **kwargs)
    return np.asarray(model.forward([int(t) for t in tokens], logits_to_keep=None)[0], dtype=np.float64)


def finish(vector, dim: int | None = None, normalize: bool = True) -> np.ndarray:
    """The first ``dim`` components in float64, divided by their Euclidean norm when ``normalize`` (a zero vector stays zeros)."""
    v = np.asarray(vector, dtype=np.float64)
    v = v[: v.shape[0] if dim is None else dim].copy()
    if not normalize:
        return v
    norm = np.sqrt(np.sum(v * v))
    return v if norm == 0 else v / norm


def pool(rows, pooling: str = "last", dim: int | None = None, normalize: bool = True) -> np.ndarray:
    """The embedding of one text from its final-norm rows [len, hidden], in float64."""
    rows = np.asarray(rows, dtype=np.float64)
    assert rows.ndim == 2 and rows.shape[0] >= 1 and pooling in ("last", "mean")
    return finish(rows[-1] if pooling == "last" else rows.mean(axis=0), dim, normalize)


def pool_allowance(rows, pooling: str, dim: int | None, normalize: bool) -> np.ndarray:
    """Per element, how far an fp32 implementation of ``pool`` may lie from it.

    last, not normalised   0: the widened bf16 row is exact.
    mean, not normalised   the worst-case bound of an fp32 summation of len terms in any order, len * 2^-24 * mean_r |x_rc| (each of
                           the len - 1 additions rounds a partial sum of at most sum_r |x_rc|, relative 2^-24; the division by len
                           is the last of the len roundings), plus one fp32 ulp of the result.
    normalised             the un-normalised allowance carried through the division (by the norm), plus dim * 2^-24 relative for the
                           fp32 sum of dim squares, its square root and the division -- and, where the un-normalised components
                           themselves carry an error (mean), that error's effect on the norm, bounded by its Euclidean length."""
    rows = np.asarray(rows, dtype=np.float64)
    n, hidden = rows.shape
    dim = hidden if dim is None else dim
    u = 2.0 ** -24
    if pooling == "last":
        raw, base = rows[-1, :dim], np.zeros(dim)
    else:
        raw = rows.mean(axis=0)[:dim]
        base = n * u * np.abs(rows).mean(axis=0)[:dim] + 2.0 ** (np.floor(np.log2(np.maximum(np.abs(raw), 2.0 ** -126))) - 23)
    if not normalize:
        return base
    norm = np.sqrt(np.sum(raw * raw))
    if norm == 0:
        return base
    want = raw / norm
    return base / norm + np.abs(want) * (dim * u + np.sqrt(np.sum(base * base)) / norm)
