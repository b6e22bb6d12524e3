"""numpy float64 restatement of speculative sampling as the engine defines it (include/tinyllm_engine.h tl_spec_sample_rows,
csrc/spec_sample.h), on top of sampling_oracle (kept_set, philox4x32_10): the kept sets and weights of a target and a draft row, the
accept test, the residual draw.  Each result also says whether it is ambiguous -- either kept set's top-p decision is, u q_x lies within
1e-5 (relative) of p_x, or u R lies within 1e-5 R of a boundary of the cumulative residual -- where the device's fp32 arithmetic may
fall on either side.  Also the case lists the CPU and the GPU tier share."""

import numpy as np

import sampling_oracle as S

ACCEPT_TAG = 0x53504143  # 'SPAC'
RESIDUAL_TAG = 0x53505253  # 'SPRS'
MARGIN = 1e-5


def uniform(seed: int, position: int, tag: int) -> float:
    out = S.philox4x32_10((position, 0, tag, 0), (seed & S.MASK, (seed >> 32) & S.MASK))
    return (out[0] >> 8) * 2.0 ** -24


def weights(logits, temperature: float, top_k: int = 0, top_p: float = 1.0):
    """(w float64 [V], ambiguous, one-hot id or -1): w = exp((l - m) / T) on the sampler's kept set, 0 elsewhere; a row with T == 0,
    without a finite maximum or holding +inf is one-hot at the sampler's id."""
    l = np.asarray(logits, dtype=np.float64)
    w = np.zeros(l.size)
    valid = ~np.isnan(l)
    hot = -1
    if not valid.any() or not (l[valid].max() > -np.inf):
        hot = 0
    else:
        m = l[valid].max()
        if temperature == 0 or m == np.inf:
            hot = int(np.flatnonzero(l == m)[0])
    if hot >= 0:
        w[hot] = 1.0
        return w, False, hot
    kept, amb = S.kept_set(l, top_k, top_p)
    w[kept] = np.exp((l[kept] - m) / temperature)
    return w, amb, -1


def inverse_cdf(w, u: float):
    """(first id whose inclusive cumulative w exceeds u sum(w) -- rounding leaving none: the last id with w > 0 --, ambiguous)."""
    cum = np.cumsum(w)
    total = cum[-1]
    t = u * total
    hit = np.flatnonzero(cum > t)
    tok = int(hit[0]) if hit.size else int(np.flatnonzero(w > 0)[-1])
    return tok, bool(np.any(np.abs(cum[:-1] - t) < MARGIN * total))


class Pair:
    """A target row and the draft row proposals are drawn from, each with its (temperature, top_k, top_p): the weights are formed once,
    verify() may be called for many (proposal, seed, position)."""

    def __init__(self, target, draft, target_params, draft_params):
        self.target = np.asarray(target, dtype=np.float64)
        self.target_params = tuple(target_params)
        self.V = self.target.size
        self.wp, self.amb_p, self.hot = weights(self.target, *target_params)
        self.p = self.wp / self.wp.sum()
        if self.hot < 0:  # (a one-hot target never looks at the draft row)
            wq, self.amb_q, _ = weights(draft, *draft_params)
            self.q = wq / wq.sum()
            self.r = np.maximum(self.p - self.q, 0.0)

    def verify(self, x: int, seed: int, position: int):
        """(accept, alt, ambiguous) of one row."""
        if x < 0:  # a bonus row: the sampler's own draw
            tok, amb = S.sample(self.target, *self.target_params, seed, position)
            return 0, tok, amb
        if self.hot >= 0:
            return (1, -1, False) if x == self.hot else (0, self.hot, False)
        amb = self.amb_p or self.amb_q
        if x < self.V:
            u = uniform(seed, position, ACCEPT_TAG)
            px, uq = self.p[x], u * self.q[x]
            amb = amb or abs(uq - px) < MARGIN * max(px, uq)
            if uq < px:
                return 1, -1, amb
        u = uniform(seed, position, RESIDUAL_TAG)
        tok, amb_r = inverse_cdf(self.r if self.r.sum() > 0 else self.wp, u)
        return 0, tok, amb or amb_r


def verify(target, draft, x, target_params, draft_params, seed: int = 0, position: int = 0):
    return Pair(target, draft, target_params, draft_params).verify(x, seed, position)


def g_statistic(tokens, p):
    """G = 2 sum obs ln(obs / expected) of observed token ids against the distribution p (df = support - 1); inf for a token outside
    the support."""
    tokens = np.asarray(tokens)
    support = np.flatnonzero(p > 0)
    obs = np.array([(tokens == t).sum() for t in support])
    if obs.sum() != tokens.size:
        return float("inf")
    expect = p[support] * tokens.size
    nz = obs > 0
    return float(2.0 * np.sum(obs[nz] * np.log(obs[nz] / expect[nz])))


# ---- the shared cases ---------------------------------------------------------------------------------------------------------
COMBOS = [(0, 1.0), (50, 1.0), (0, 0.9), (20, 0.8)]  # (top_k, top_p): neither, top-k, top-p, both
TEMPERATURES = (0.3, 1.0, 2.0)
UNEQUAL_DRAFT = {0.3: 0.5, 1.0: 0.7, 2.0: 1.5}  # the draft's temperature where it differs from the target's
VOCABS = [1024, 8200, 151936, 151941]
ROWS_PER_PAIR = 6

DIST_PARAMS = (0.8, 16, 1.0)
DIST_V, DIST_ROWS = 1024, 1500
PROPOSAL_SEED = 1 << 20  # the draft's draws: seeds disjoint from the verification's 0 .. DIST_ROWS - 1


def bf16(x):
    import torch

    return torch.from_numpy(np.asarray(x, dtype=np.float32)).bfloat16().float().numpy()


def rows(V, rng):
    """rand / peaked / ties target rows, as tests/test_zz_device_sampling_gpu.py draws them (bf16 values)."""
    rand = rng.standard_normal(V).astype(np.float32) * 2.0
    peaked = rand.copy()
    peaked[rng.integers(0, V, 3)] += 12.0
    ties = np.round(rng.standard_normal(V) * 2.0).astype(np.float32)
    return {"rand": bf16(rand), "peaked": bf16(peaked), "ties": bf16(ties)}


def combos(V, kind, T):
    """The (top_k, top_p) a vocabulary of V takes.  A kept set of thousands of tokens puts u R within 1e-5 R of some boundary in a large
    share of draws, so beyond 1,024 tokens the sets are cut by top-k <= 50 -- or the row is peaked and cold, its mass on three tokens."""
    if V <= 1024:
        return COMBOS
    return [c for c in COMBOS if c[0] > 0 or (kind == "peaked" and T == 0.3 and c[1] == 1.0)]


def kernel_cases(V):
    """The rows of the kernel-against-oracle test at vocabulary V: a list of (Pair, target row, draft row, target params, draft params,
    [(proposal, seed, position)]).  Of each pair's proposals a third is drawn from the draft's distribution (mostly accepted), a third is
    the draft's most over-weighted tokens (mostly rejected), a third lies outside the target's kept set (ids past the vocabulary where
    the kept set is everything)."""
    rng = np.random.default_rng(V)
    base = rows(V, rng)
    out = []
    n = 0
    for kind, target in base.items():
        draft = bf16(target + rng.standard_normal(V).astype(np.float32))
        for T in TEMPERATURES:
            for k, p in combos(V, kind, T):
                for Tq in (T, UNEQUAL_DRAFT[T]):
                    pair = Pair(target, draft, (T, k, p), (Tq, k, p))
                    inside = np.flatnonzero((pair.p > 0) & (pair.q > 0))
                    over = inside[np.argsort(-(pair.q[inside] / pair.p[inside]))[:2]]
                    outside = np.flatnonzero(pair.p == 0)
                    xs = list(rng.choice(V, 2, p=pair.q)) + list(over) + \
                        (list(rng.choice(outside, 2)) if outside.size else [V, V + 5])
                    props = []
                    for x in xs:
                        props.append((int(x), 5000 + n, 13 * n + 2))
                        n += 1
                    out.append((pair, target, draft, (T, k, p), (Tq, k, p), props))
    return out


def distribution_case(data_seed=0):
    """The fixed pair of the distribution property: V = 1,024, target row N(0, 2), draft row = target + N(0, 1), both under DIST_PARAMS;
    returns (Pair, target row, draft row, proposals drawn by sampling_oracle.sample from the draft row with seeds of their own)."""
    rng = np.random.default_rng(1000 + data_seed)
    target = bf16(rng.standard_normal(DIST_V) * 2.0)
    draft = bf16(target + rng.standard_normal(DIST_V).astype(np.float32))
    pair = Pair(target, draft, DIST_PARAMS, DIST_PARAMS)
    proposals = [S.sample(draft, *DIST_PARAMS, PROPOSAL_SEED + i, i)[0] for i in range(DIST_ROWS)]
    return pair, target, draft, proposals
