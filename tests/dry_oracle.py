"""numpy restatement of DRY and the n-gram ban as include/tinyllm_engine.h defines them ("DRY and the n-gram ban"; csrc/dry.h).

A slot's recorded ids are S[s0 .. e]; ``seq`` below is the list S[0 .. e] (entries before ``start`` = s0 are never looked at),
``last = seq[-1]`` the token the step has just fed.  Everything is plain Python over the positions; the penalty is a chain of float32
products rounded one by one, and the row rule works on bf16 bit patterns, so the device's rows can be compared bit for bit."""

import numpy as np

MAX_MATCH = 64      # TL_DRY_MAX_MATCH
MAX_BREAKERS = 64   # TL_MAX_DRY_BREAKERS
NEG_INF = 0xFF80    # bf16 -inf


def bits(x) -> np.ndarray:
    """float32 -> bf16 bits, round to nearest even (NaN stays NaN)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def from_bits(b) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def raw_match(seq, i, start):
    """raw(i): the largest m in [1, min(M, i - s0 + 1)] with S[i - j] == S[e - j] for all 0 <= j < m (S[i] == S[e] is given)."""
    e = len(seq) - 1
    m, lim = 1, min(MAX_MATCH, i - start + 1)
    while m < lim and seq[i - m] == seq[e - m]:
        m += 1
    return m


def banned(seq, start=0, ngram=0):
    """The tokens no_repeat_ngram = ngram bans: every continuation with raw(i) >= ngram - 1."""
    out = set()
    if ngram <= 0:
        return out
    e = len(seq) - 1
    if e < start:
        return out
    for i in range(start, e):
        if seq[i] == seq[e] and raw_match(seq, i, start) >= ngram - 1:
            out.add(seq[i + 1])
    return out


def dry_lengths(seq, start=0, multiplier=0.0, allowed_length=2, range_=0, breakers=()):
    """{t: L[t]} for the tokens whose L[t] >= allowed_length."""
    L = {}
    e = len(seq) - 1
    if multiplier <= 0 or e < start:
        return L
    brk = set(breakers)
    lo = max(start, e + 1 - range_) if range_ > 0 else start
    B = 0
    while B < MAX_MATCH and e - B >= lo and seq[e - B] not in brk:
        B += 1
    if B == 0:
        return L
    for i in range(lo, e):
        if seq[i] != seq[e] or seq[i + 1] in brk:
            continue
        d = min(raw_match(seq, i, start), B, i - lo + 1)
        t = seq[i + 1]
        L[t] = max(L.get(t, 0), d)
    return {t: d for t, d in L.items() if d >= allowed_length}


def penalty(multiplier, base, length, allowed_length) -> np.float32:
    """p = multiplier, then length - allowed_length times p = p * base: float32 products, rounded one by one."""
    p, b = np.float32(multiplier), np.float32(base)
    with np.errstate(over="ignore"):
        for _ in range(length - allowed_length):
            p = np.float32(p * b)
    return p


def apply(row_bits, seq, start=0, multiplier=0.0, base=1.75, allowed_length=2, range_=0, ngram=0, breakers=()):
    """The processed row's bf16 bits [V] -> the bits after DRY and the n-gram ban.  Ids outside the row are ignored."""
    out = np.array(row_bits, dtype=np.uint16, copy=True)
    V = out.shape[0]
    ban = banned(seq, start, ngram)
    for t in ban:
        if 0 <= t < V:
            out[t] = NEG_INF
    for t, d in dry_lengths(seq, start, multiplier, allowed_length, range_, breakers).items():
        if t in ban or not 0 <= t < V:
            continue
        v = from_bits(out[t:t + 1])[0]
        if np.isnan(v):
            continue
        p = penalty(multiplier, base, d, allowed_length)
        if not np.isfinite(p):
            out[t] = NEG_INF
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                out[t] = bits(np.array([np.float32(v) - p], dtype=np.float32))[0]
    return out
