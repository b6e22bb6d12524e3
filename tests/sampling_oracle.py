"""numpy restatement of the decode engine's device sampler (include/tinyllm_engine.h tl_engine_set_sampling, csrc/sample.h): Philox4x32-10,
the kept set (rank by logit then id, exact top-k, top-p over the full-vocabulary temperature-1 probabilities), and the float64 inverse CDF.
Each draw also says whether it is ambiguous: u W within 1e-5 W of a boundary of the cumulative weights, or a top-p decision whose mass
before the token lies within 1e-5 of top_p -- where the device's fp32 arithmetic may fall on either side."""

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
TAG = 0x53414D50
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c = [int(x) & MASK for x in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c[3] ^ k1) & MASK, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def uniform(seed: int, position: int) -> float:
    out = philox4x32_10((position, 0, TAG, 0), (seed & MASK, (seed >> 32) & MASK))
    return (out[0] >> 8) * 2.0 ** -24


def kept_set(logits, top_k: int = 0, top_p: float = 1.0):
    """logits: float array (bf16 values).  Returns (kept ids in rank order, ambiguous top-p decision)."""
    l = np.asarray(logits, dtype=np.float64)
    V = l.size
    ids = np.arange(V)
    valid = ~np.isnan(l)
    order = ids[valid][np.lexsort((ids[valid], -l[valid]))]
    m = l[valid].max()
    n = order.size
    if 0 < top_k < V:
        n = min(n, top_k)
    amb = False
    if 0.0 < top_p < 1.0:
        p = np.exp(l[valid] - m)
        p = np.exp(l - m) / p.sum()
        before = np.concatenate([[0.0], np.cumsum(p[order])[:-1]])
        keep = before < top_p
        keep[0] = True
        lp = int(np.argmin(keep)) if not keep.all() else keep.size
        amb = bool(np.any(np.abs(before[1:n] - top_p) < 1e-5)) if n > 1 else False
        n = min(n, lp)
    return order[:n], amb


def sample(logits, temperature: float, top_k: int = 0, top_p: float = 1.0, seed: int = 0, position: int = 0):
    """(token id, ambiguous) of one row."""
    l = np.asarray(logits, dtype=np.float64)
    valid = ~np.isnan(l)
    if not valid.any() or not (l[valid].max() > -np.inf):
        return 0, False
    m = l[valid].max()
    if temperature == 0 or m == np.inf:
        return int(np.flatnonzero(l == m)[0]), False
    kept, amb = kept_set(l, top_k, top_p)
    kept = np.sort(kept)
    w = np.exp((l[kept] - m) / temperature)
    cum = np.cumsum(w)
    W = cum[-1]
    t = uniform(seed, position) * W
    hit = np.flatnonzero(cum > t)
    tok = int(kept[hit[0]]) if hit.size else int(kept[-1])
    amb = amb or bool(np.any(np.abs(cum[:-1] - t) < 1e-5 * W))
    return tok, amb
