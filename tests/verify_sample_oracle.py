"""numpy float64 restatement of batched speculative sampling as the engine defines it (include/tinyllm_engine.h
tl_engine_verify_batch_sampled, csrc/verify_sample.h), on top of spec_sample_oracle (weights, uniforms, the inverse CDF) and
sampling_oracle (the bonus row's draw): the point rule -- a proposal whose draft distribution is one-hot at the proposed id -- written
from its own definition, the scan that composes a sequence's result from its rows, and the case lists the CPU and the GPU tier share."""

import numpy as np

import sampling_oracle as S
import spec_sample_oracle as SS


class Point:
    """A target row with its (temperature, top_k, top_p): the weights are formed once, verify() may be called for many (proposal, seed,
    position)."""

    def __init__(self, target, params):
        self.target, self.params = np.asarray(target, dtype=np.float64), tuple(params)
        self.wp, self.amb, self.hot = SS.weights(self.target, *self.params)
        self.p = self.wp / self.wp.sum()

    def verify(self, x: int, seed: int, position: int):
        """(accept, alt, ambiguous) of one row whose proposal x is certain under the draft: accepted iff u_acc < p_x; rejected, the
        inverse-CDF draw with u_res over p with x removed (x >= V: never accepted, nothing to remove); x < 0: the sampler's own draw."""
        if x < 0:
            tok, amb = S.sample(self.target, *self.params, seed, position)
            return 0, tok, amb
        if self.hot >= 0:
            return (1, -1, False) if x == self.hot else (0, self.hot, False)
        amb = self.amb
        r = self.p
        if x < r.size:
            u = SS.uniform(seed, position, SS.ACCEPT_TAG)
            amb = amb or abs(u - r[x]) < SS.MARGIN * max(r[x], u)
            if u < r[x]:
                return 1, -1, amb
            r = r.copy()
            r[x] = 0.0
        tok, amb_r = SS.inverse_cdf(r if r.sum() > 0 else self.wp, SS.uniform(seed, position, SS.RESIDUAL_TAG))
        return 0, tok, amb or amb_r


def point_verify(target, x: int, params, seed: int, position: int):
    return Point(target, params).verify(x, seed, position)


def compose(row0, lens, tokens, accept, alt):
    """Per sequence the accepted proposals tokens[row0 + 1 .. row0 + a] followed by row a's alt, a = the first row j < len - 1 that
    rejects (len - 1 when none does): tl_verify_result's ids[:count]."""
    out = []
    for r0, n in zip(row0, lens):
        a = next((j for j in range(n - 1) if not accept[r0 + j]), n - 1)
        out.append([int(tokens[r0 + j + 1]) for j in range(a)] + [int(alt[r0 + a])])
    return out


def verify_sequences(targets, row0, lens, starts, tokens, params, seeds):
    """The whole stage over rows `targets` [R, V]: (accept [R], alt [R], ambiguous [R], results); params[i] / seeds[i] are sequence i's.
    Rows that are the same array object share one Point."""
    R = len(tokens)
    accept, alt, amb = [0] * R, [-1] * R, [False] * R
    points = {}
    for i, (r0, n) in enumerate(zip(row0, lens)):
        for j in range(n):
            x = int(tokens[r0 + j + 1]) if j < n - 1 else -1
            key = (id(targets[r0 + j]), tuple(params[i]))
            if key not in points:
                points[key] = Point(targets[r0 + j], params[i])
            accept[r0 + j], alt[r0 + j], amb[r0 + j] = points[key].verify(x, seeds[i], starts[i] + j + 1)
    return accept, alt, amb, compose(row0, lens, tokens, accept, alt)


def peaked_row(V: int, x: int):
    """A draft row whose first maximum is x: under draft temperature 0 its distribution is one-hot there."""
    row = np.full(V, -4.0, dtype=np.float32)
    row[x] = 9.0
    return row


def point_cases(V: int):
    """The rows of the point tests at vocabulary V: a list of (target row, (T, top_k, top_p), [(proposal, seed, position)]) over
    SS.rows(V, default_rng(V + 7)), every SS.TEMPERATURES x SS.combos.  Six proposals per case: two drawn from p, the two most likely
    tokens, two outside the kept set (V and V + 5 where the kept set is everything)."""
    rng = np.random.default_rng(V + 7)
    out, n = [], 0
    for kind, target in SS.rows(V, rng).items():
        for T in SS.TEMPERATURES:
            for k, p in SS.combos(V, kind, T):
                wp, _, _ = SS.weights(target, T, k, p)
                prob = wp / wp.sum()
                outside = np.flatnonzero(prob == 0)
                xs = list(rng.choice(V, 2, p=prob)) + list(np.argsort(-prob, kind="stable")[:2]) + \
                    (list(rng.choice(outside, 2)) if outside.size else [V, V + 5])
                props = []
                for x in xs:
                    props.append((int(x), 7000 + n, 11 * n + 3))
                    n += 1
                out.append((target, (T, k, p), props))
    return out


def two_row_twin(target, x: int, params):
    """(draft row, draft params) with which the two-row rule (SS.Pair, tl_spec_sample_rows) is the point rule for proposal x: a row
    peaked at x under draft temperature 0 -- and for x >= V, where the point rule's residual is p whole, the target row under the target's
    own parameters: q == p, R == 0, and the two-row rule falls back to the plain draw from p with u_res."""
    if x < len(target):
        return peaked_row(len(target), x), (0.0, 0, 1.0)
    return target, params


DIST_MODES = ("top", "third", "outside", "cycle")


def distribution_target():
    return SS.bf16(np.random.default_rng(1000).standard_normal(SS.DIST_V) * 2.0)


def distribution_proposals(target, mode: str, n: int = SS.DIST_ROWS):
    """n proposals for the distribution property under SS.DIST_PARAMS: fixed at the most likely token, at the third most likely, at a
    token outside the kept set, or cycling through the kept set."""
    wp, _, _ = SS.weights(target, *SS.DIST_PARAMS)
    order = np.argsort(-wp, kind="stable")
    kept = np.sort(np.flatnonzero(wp > 0))
    if mode == "top":
        return [int(order[0])] * n
    if mode == "third":
        return [int(order[2])] * n
    if mode == "outside":
        return [int(np.flatnonzero(wp == 0)[0])] * n
    return [int(kept[i % kept.size]) for i in range(n)]
