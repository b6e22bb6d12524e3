"""The prompt-lookup proposal rule in plain Python (csrc/lookup.h; include/tinyllm_engine.h "Prompt lookup"), written from the contract
and from nothing else: the tests hold the kernel and the engine against it.

T[s0 .. e] are a row's ids and last = T[e].  A candidate is every i in [s0, e) with T[i] == last; raw(i) is the largest
m <= min(N, i - s0 + 1) with T[i - j] == T[e - j] for all 0 <= j < m; it is eligible with raw(i) >= min_ngram; avail(i) = min(K, e - i).
The choice is the eligible candidate with the largest (raw, avail, i); the proposals are T[i + 1 .. i + avail]."""
from __future__ import annotations

MAX_NGRAM = 16
MAX_PROPOSALS = 7


def check_params(max_ngram, min_ngram, num_proposals):
    if not 1 <= max_ngram <= MAX_NGRAM:
        raise ValueError("max_ngram must be 1 .. 16")
    if not 1 <= min_ngram <= max_ngram:
        raise ValueError("min_ngram must be 1 .. max_ngram")
    if not 1 <= num_proposals <= MAX_PROPOSALS:
        raise ValueError("num_proposals must be 1 .. 7")


def choose(T, s0, e, max_ngram=3, min_ngram=1, num_proposals=4):
    """(i, raw, avail) of the choice over T[s0 .. e], or None.  Only T[s0 .. e] is read."""
    check_params(max_ngram, min_ngram, num_proposals)
    if e < s0:
        return None
    last, best = T[e], None
    for i in range(s0, e):
        if T[i] != last:
            continue
        raw = 0
        while raw < min(max_ngram, i - s0 + 1) and T[i - raw] == T[e - raw]:
            raw += 1
        if raw < min_ngram:
            continue
        key = (raw, min(num_proposals, e - i), i)
        if best is None or key > best:
            best = key
    return None if best is None else (best[2], best[0], best[1])


def propose(T, s0, e, max_ngram=3, min_ngram=1, num_proposals=4):
    """The proposals over T[s0 .. e]: a list of 0 .. num_proposals ids."""
    c = choose(T, s0, e, max_ngram, min_ngram, num_proposals)
    if c is None:
        return []
    i, _, avail = c
    return [int(t) for t in T[i + 1:i + 1 + avail]]


def propose_ids(ids, max_ngram=3, min_ngram=1, num_proposals=4, start=0):
    """... over a whole sequence ``ids`` whose last id is the pending token; ids before ``start`` are unknown."""
    return propose(list(ids), start, len(ids) - 1, max_ngram, min_ngram, num_proposals)
