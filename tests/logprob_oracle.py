"""numpy restatement of the decode engine's per-token log-probabilities (include/tinyllm_engine.h tl_engine_set_logprobs, csrc/logprob.h):
for a logits row l with m its maximum over non-NaN entries, lse = m + log(sum exp(l - m)) over non-NaN entries and logprob(t) = l_t - lse;
a NaN logit gives NaN, a row without a finite maximum (all NaN / -inf, or holding +inf) NaN everywhere.  The top-N list is the first N
tokens of the sampler's order (logit descending, equal logits by the lower id, NaN never ranked), padded with (-1, -inf) to N."""

import numpy as np

MAX_TOP = 20


def lse(logits) -> float:
    l = np.asarray(logits, dtype=np.float64)
    valid = l[~np.isnan(l)]
    if valid.size == 0:
        return float("nan")
    m = valid.max()
    if not np.isfinite(m):
        return float("nan")
    return float(m + np.log(np.sum(np.exp(valid - m))))


def logprob(logits, token: int) -> float:
    return float(np.float64(logits[token]) - lse(logits))


def order(logits):
    """Rankable ids in the sampler's order."""
    l = np.asarray(logits, dtype=np.float64)
    ids = np.flatnonzero(~np.isnan(l))
    return ids[np.lexsort((ids, -l[ids]))]


def top(logits, n: int):
    """(ids, logprobs) of the first n tokens of the order, padded with -1 / -inf to n entries."""
    l = np.asarray(logits, dtype=np.float64)
    z = lse(l)
    ids = order(l)[:n]
    out_ids = np.full(n, -1, dtype=np.int64)
    out_lp = np.full(n, -np.inf)
    out_ids[:ids.size] = ids
    out_lp[:ids.size] = l[ids] - z
    return out_ids, out_lp


def greedy(logits) -> int:
    """The first maximum (0 for a row without one above -inf), the engine's greedy id."""
    l = np.asarray(logits, dtype=np.float64)
    valid = ~np.isnan(l)
    if not valid.any() or not l[valid].max() > -np.inf:
        return 0
    return int(np.flatnonzero(l == l[valid].max())[0])
