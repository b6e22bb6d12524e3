"""numpy (float64) restatement of the decode engine's truncation (include/tinyllm_engine.h "truncation", csrc/truncate.h): min-p, locally
typical sampling closed under ties, Mirostat v2 and its update.  ``kept`` sorts every token of a row into surely kept, surely dropped and
UNDECIDED -- the tokens the device's fp32 arithmetic may decide either way:
  * min-p / Mirostat: the threshold lies within relative 1e-5 of the token's own value;
  * typical-p: the token's deviation lies between the boundaries for mass typical_p - 1e-5 and typical_p + 1e-5 (the band
    tests/sampling_oracle.py uses for top-p).
Also the rows and per-row parameters the CPU cap test and the GPU tests share."""

import numpy as np

LOG2E = 1.0 / np.log(2.0)
BAND = 1e-5
NEG_INF_BITS = 0xFF80


def bf16_bits(x) -> np.ndarray:
    """float32 -> bf16 bits (uint16), round to nearest even (NaN stays NaN)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    return np.where(nan, np.uint16(0x7FC0), r)


def bf16_values(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def kept(x, T, min_p=0.0, typical_p=1.0, mu=float("nan")):
    """Boolean masks (kept, dropped, undecided) over the row ``x`` (bf16 values; NaN allowed), disjoint and complete.  A row that is not
    filtered -- T == 0, every parameter off, or a maximum that is not finite -- is all kept (it is copied bit for bit, NaN included)."""
    x = np.asarray(x, dtype=np.float64)
    V = x.size
    all_kept = (np.ones(V, bool), np.zeros(V, bool), np.zeros(V, bool))
    mir = not np.isnan(mu)
    use_minp = not mir and min_p > 0.0
    use_typ = not mir and 0.0 < typical_p < 1.0
    valid = ~np.isnan(x)
    if not T > 0 or not (mir or use_minp or use_typ) or not valid.any():
        return all_kept
    m = x[valid].max()
    if not np.isfinite(m):
        return all_kept
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = (x - m) / T
        keep = valid.copy()
        und = np.zeros(V, bool)
        if mir:
            s = np.log2(np.exp(t[valid]).sum()) - t * LOG2E  # -log2 p_i
            keep &= s <= mu
            und |= valid & (np.abs(s - mu) < BAND * np.abs(s))
            g = int(np.flatnonzero(x == m)[0])  # the first maximum always stays
            keep[g], und[g] = True, False
        else:
            if use_minp:
                lnmp = np.log(min_p)
                keep &= t >= lnmp
                und |= valid & (np.abs(t - lnmp) < BAND * np.abs(t))
            if use_typ:
                if und.any():  # the survivors themselves are in doubt: so is everything computed over them
                    und = valid.copy()
                else:
                    S = np.flatnonzero(keep & (t > -np.inf))
                    p = np.exp(t[S])
                    p /= p.sum()
                    tbar = (p * t[S]).sum()  # d_i = |(-ln p_i) - H| = |t_i - tbar|
                    d = np.abs(t[S] - tbar)
                    order = np.argsort(d, kind="stable")
                    cum = np.cumsum(p[order])

                    def boundary(target):
                        i = int(np.searchsorted(cum, target, side="left"))
                        return d[order[i]] if i < cum.size else np.inf

                    d_star, d_lo, d_hi = boundary(typical_p), boundary(typical_p - BAND), boundary(typical_p + BAND)
                    keep_s = np.zeros(V, bool)
                    keep_s[S[d <= d_star]] = True
                    keep &= keep_s
                    und[S[(d > d_lo) & (d <= d_hi)]] = True
    keep &= ~und
    return keep, ~keep & ~und, und


def typical_set(x, T, typical_p):
    """(kept mask of the typical stage alone, boundary deviation, deviations) -- for the comparison with transformers."""
    x = np.asarray(x, dtype=np.float64)
    t = (x - x.max()) / T
    p = np.exp(t)
    p /= p.sum()
    tbar = (p * t).sum()
    d = np.abs(t - tbar)
    order = np.argsort(d, kind="stable")
    cum = np.cumsum(p[order])
    i = int(np.searchsorted(cum, typical_p, side="left"))
    d_star = d[order[i]] if i < cum.size else np.inf
    return d <= d_star, d_star, d


def filtered_bits(bits, masks):
    """(expected bf16 bits where the token is decided, decided mask): kept tokens keep their bits, dropped ones are -inf."""
    k, dr, und = masks
    out = np.where(k, np.asarray(bits, dtype=np.uint16), np.uint16(NEG_INF_BITS))
    return out, ~und


def mirostat_update(filtered_row, token, T, tau, eta, mu):
    """mu after the draw of ``token`` from the filtered row: s = -log2(p_t / sum_kept p), mu - eta (s - tau)."""
    f = np.asarray(filtered_row, dtype=np.float64)
    k = ~np.isnan(f) & (f > -np.inf)
    a = f[k] / T
    L = a.max() + np.log(np.exp(a - a.max()).sum())
    s = (L - f[token] / T) * LOG2E
    return mu - eta * (s - tau)


# ---- the rows the tests share -------------------------------------------------------------------------------------------------------
TEMPERATURES = (0.7, 1.0, 1.3)
TYPICAL_PS = (0.2, 0.5, 0.9, 0.95)
MIN_PS = (0.02, 0.1, 0.3)
MUS = (2.0, 6.0, 10.0, 16.0)
VOCABS = (1024, 151936, 151941)
N_ROWS = 12
COMBOS = ("min_p", "typical_p", "both", "mirostat")


def make_rows(V, n=N_ROWS, seed=0):
    """bf16 bits [n, V]: N(0, 2^2) logits rounded to bf16 with one token per row raised by 6."""
    rng = np.random.default_rng(1000 + seed + V)
    x = bf16_values(bf16_bits((2.0 * rng.standard_normal((n, V))).astype(np.float32)))
    up = rng.integers(0, V, size=n)
    x[np.arange(n), up] += 6.0
    return bf16_bits(x)


def row_params(i, combo):
    """(T, min_p, typical_p, mu) of row i under ``combo``."""
    T = TEMPERATURES[i % 3]
    min_p = MIN_PS[(i // 4) % 3] if combo in ("min_p", "both") else 0.0
    typ = TYPICAL_PS[i % 4] if combo in ("typical_p", "both") else 1.0
    mu = MUS[i % 4] if combo == "mirostat" else float("nan")
    return T, min_p, typ, mu
