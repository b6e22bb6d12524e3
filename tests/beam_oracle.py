"""A numpy float64 restatement of beam-search candidate selection (include/tinyllm_engine.h "Beam search", csrc/beam.h) and of the
genealogy a reorder leaves (csrc/slot_table.h, beam_reorder).  Independent of the library: the tests compare the device against it."""

from __future__ import annotations

import numpy as np

EMPTY = (-1, -1, float("-inf"), float("-inf"))


def row_order(row: np.ndarray) -> np.ndarray:
    """Token ids of one row in the sampler's order: logit descending, equal logits by the lower id, NaN never ranked."""
    ids = np.flatnonzero(~np.isnan(row))
    return ids[np.lexsort((ids, -row[ids]))]


def row_lse(row: np.ndarray) -> float:
    """m + log(sum exp(l - m)) over the non-NaN entries; NaN without a finite maximum."""
    vals = row[~np.isnan(row)]
    if vals.size == 0 or not np.isfinite(vals.max()):
        return float("nan")
    m = vals.max()
    return float(m + np.log(np.exp(vals - m).sum()))


def beam_select(logits, scores, n_cand: int, with_logits: bool = False):
    """The first ``n_cand`` (parent, token, score, logprob) over all rows x vocab pairs of ``logits`` [rows, vocab] (any float array;
    computed in float64) with cumulative ``scores`` [rows]: score descending, equal scores by the lower parent, then by the row's own
    order; EMPTY past the rankable pairs.  A row without a finite maximum or with a score that is not finite contributes nothing.
    ``with_logits``: each entry carries its logit as a fifth field."""
    logits = np.asarray(logits, dtype=np.float64)
    scores = np.asarray(scores, dtype=np.float64)
    found = []
    for p, row in enumerate(logits):
        lse = row_lse(row)
        if not np.isfinite(scores[p]) or not np.isfinite(lse):
            continue
        for rank, t in enumerate(row_order(row)[:n_cand]):
            lp = row[t] - lse
            found.append((-(scores[p] + lp), p, rank, int(t), float(scores[p] + lp), float(lp), float(row[t])))
    found.sort(key=lambda c: c[:3])
    out = [((c[1], c[3], c[4], c[5], c[6]) if with_logits else (c[1], c[3], c[4], c[5])) for c in found[:n_cand]]
    return out + [EMPTY + ((float("nan"),) if with_logits else ())] * (n_cand - len(out))


def reorder(sequences, n_src: int, parents, tokens):
    """The genealogy of a reorder: ``sequences[i]`` is what slot i of the group holds (a list of ids, or None for a free slot); after
    it slot i holds ``sequences[parents[i]]`` followed by the pending token ``tokens[i]``, and slots past the new width are free."""
    assert all(s is not None for s in sequences[:n_src]) and all(s is None for s in sequences[n_src:len(parents)])
    assert all(0 <= p < n_src for p in parents) and len(parents) == len(tokens)
    span = max(n_src, len(parents))
    return [list(sequences[p]) + [t] for p, t in zip(parents, tokens)] + [None] * (span - len(parents))


def reorder_pages_needed(contexts, parents, page_size: int) -> int:
    """Pages a reorder must obtain: one per further child of a parent whose tail page is partial."""
    need = 0
    for p in set(parents):
        children = sum(1 for q in parents if q == p)
        need += children - 1 if contexts[p] % page_size else 0
    return need
