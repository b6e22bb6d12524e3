"""CPU tier: speculative sampling.  The oracle (tests/spec_sample_oracle.py) has the property the whole feature rests on -- the emitted
token is distributed as the target's own sampling distribution whatever the draft -- and its edge rules; the case lists the GPU tier
uses keep the oracle's ambiguous share small; and the host loop of speculative_generate_ids(temperature > 0) keeps both caches and
its counts right, over stub engines."""

import numpy as np
import pytest
import torch

import sampling_oracle as S
import spec_sample_oracle as SS


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def _emitted(pair, proposals, rule):
    out = []
    for i, x in enumerate(proposals):
        accept, alt, _ = pair.verify(x, i, 7)
        if accept:
            out.append(x)
        elif rule == "residual":
            out.append(alt)
        else:  # the deliberately wrong rule: redraw from p itself
            out.append(SS.inverse_cdf(pair.wp, SS.uniform(i, 7, SS.RESIDUAL_TAG))[0])
    return out


@pytest.mark.parametrize("data_seed", [0, 1])
def test_oracle_emits_the_targets_distribution(data_seed):
    """G of the emitted token against p is below 3 |kept| (df = |kept| - 1: far below a wrong rule, far above chance for a right
    one); redrawing from p instead of the residual exceeds it."""
    pair, _, _, proposals = SS.distribution_case(data_seed)
    kept = int((pair.p > 0).sum())
    assert kept == 16
    g = SS.g_statistic(_emitted(pair, proposals, "residual"), pair.p)
    wrong = SS.g_statistic(_emitted(pair, proposals, "from p"), pair.p)
    print(f"G right rule {g:.1f}, wrong rule {wrong:.1f}, bound {3 * kept}")
    assert g < 3 * kept, g
    assert wrong > 3 * kept, wrong
    rejected = sum(1 for i, x in enumerate(proposals) if not pair.verify(x, i, 7)[0])
    assert 0.1 * len(proposals) < rejected < 0.9 * len(proposals)  # both branches carry weight


@pytest.mark.parametrize("V", SS.VOCABS)
def test_ambiguity_cap_of_the_gpu_case_lists(V):
    """A condition on the case lists, not a measurement of the kernel: the oracle flags at most 2 % of the rows the GPU test checks."""
    cases = SS.kernel_cases(V)
    flags = [pair.verify(x, seed, pos) for pair, *_, props in cases for x, seed, pos in props]
    share = sum(f[2] for f in flags) / len(flags)
    accepted = sum(f[0] for f in flags) / len(flags)
    print(f"V {V}: {len(flags)} rows, ambiguous {share:.4f}, accepted {accepted:.2f}")
    assert share <= 0.02, share
    assert 0.15 < accepted < 0.6, accepted  # roughly a third accepted; the rest rejected inside or outside the target's kept set


def test_ambiguity_cap_of_the_distribution_case():
    pair, _, _, proposals = SS.distribution_case(0)
    share = sum(pair.verify(x, i, 7)[2] for i, x in enumerate(proposals)) / len(proposals)
    assert share <= 0.02, share


def test_greedy_reduction():
    rng = np.random.default_rng(3)
    target = SS.bf16(rng.standard_normal(500) * 2.0)
    draft = SS.bf16(rng.standard_normal(500) * 2.0)
    g = int(np.argmax(target))
    for dp in ((0.7, 0, 1.0), (0.0, 0, 1.0), (1.0, 10, 0.9)):
        pair = SS.Pair(target, draft, (0.0, 5, 0.9), dp)
        for x in (g, (g + 1) % 500, 0, 499, 500, 10 ** 6):
            assert pair.verify(x, 11, 4) == ((1, -1, False) if x == g else (0, g, False))


def test_bonus_rows_are_the_samplers_draw():
    rng = np.random.default_rng(4)
    target = SS.bf16(rng.standard_normal(700) * 2.0)
    draft = SS.bf16(rng.standard_normal(700) * 2.0)
    for i, (T, k, p) in enumerate([(0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 50, 1.0), (0.8, 0, 0.9), (0.7, 50, 0.9)]):
        want = S.sample(target, T, k, p, 900 + i, 31 * i)
        assert SS.verify(target, draft, -1, (T, k, p), (1.0, 0, 1.0), 900 + i, 31 * i) == (0, want[0], want[1])


def test_edge_rows_are_one_hot():
    V = 300
    ok = SS.bf16(np.random.default_rng(5).standard_normal(V))
    nan, ninf = np.full(V, np.nan), np.full(V, -np.inf)
    pinf = ok.copy()
    pinf[[40, 90]] = np.inf
    params = (0.9, 20, 0.95)
    for target, hot in ((nan, 0), (ninf, 0), (pinf, 40)):
        pair = SS.Pair(target, ok, params, params)
        assert pair.hot == hot
        assert pair.verify(hot, 1, 2) == (1, -1, False)
        assert pair.verify(hot + 1, 1, 2) == (0, hot, False)
        assert pair.verify(-1, 1, 2)[:2] == (0, hot)
    # a one-hot DRAFT row: q is 1 at its id, so that proposal is accepted with probability p_x and any other proposal has q_x = 0
    pair = SS.Pair(ok, pinf, params, params)
    assert pair.q[40] == 1.0 and pair.q.sum() == 1.0
    inside = int(np.flatnonzero(pair.p > 0)[0])
    if inside != 40:
        assert pair.verify(inside, 3, 3)[:2] == (1, -1)  # u * 0 < p_x
    for target in (nan, ninf):
        w, _, hot = SS.weights(target, 1.0)
        assert hot == 0 and w[0] == 1.0 and w.sum() == 1.0


def test_residual_is_never_the_rejected_token():
    """r_x = max(p_x - q_x, 0) and a rejection needs u q_x >= p_x: the residual draw cannot return the token it replaces."""
    pair, _, _, proposals = SS.distribution_case(0)
    for i, x in enumerate(proposals[:400]):
        accept, alt, _ = pair.verify(x, i, 7)
        assert accept or (alt != x and pair.p[alt] > pair.q[alt])


# ---- the host loop over stub engines ------------------------------------------------------------------------------------------
EOS = 1
V_STUB = 64


def _rule(ctx, eos_at=None):
    if eos_at is not None and len(ctx) == eos_at:
        return EOS
    return (sum(ctx) * 31 + len(ctx) * 7) % 50 + 2


class StubEngine:
    """The surface speculative_generate_ids uses.  `rule` is what this engine proposes / emits after a context; `truth` is the target's
    rule: every context either engine is asked to extend must be the prompt followed by the target's own continuation, which is what
    the rewinds have to keep true."""

    def __init__(self, rule, truth, prompt_len):
        self.rule, self.truth, self.prompt_len = rule, truth, prompt_len
        self.vocab_size, self.device = V_STUB, "cpu"
        self.ctx, self.produced, self.pending = None, [], None
        self.calls = {"verify": 0, "verify_sampled": 0, "decode_calls": [], "set_sampling": [], "copies": 0}

    def _pure(self):
        for j in range(self.prompt_len, len(self.ctx)):
            assert self.ctx[j] == self.truth(self.ctx[:j]), ("a cache holds a token the target did not emit", j, self.ctx)

    def begin(self, slot):
        self.ctx, self.produced, self.pending = [], [], None

    def release(self, slot):
        self.ctx = None

    def set_sampling(self, slot, temperature=0.0, top_k=None, top_p=None, seed=0):
        self.calls["set_sampling"].append((temperature, top_k, top_p, seed))

    def prefill(self, slot, prompt, chunk=2048, want_logits=True):
        self.ctx += list(prompt)
        if want_logits:
            self.pending = self.rule(self.ctx)
            self.produced.append(self.pending)

    def read_tokens(self, slot, n):
        return self.produced[-n:]

    def set_token(self, slot, token):
        self._pure()
        assert token == self.truth(self.ctx), "the pending token is not the target's next token"
        self.pending = token

    def decode(self, steps, batch=None):
        self.calls["decode_calls"].append(steps)
        for _ in range(steps):
            self.ctx.append(self.pending)
            self.pending = self.rule(self.ctx)
            self.produced.append(self.pending)

    def logits_buffer(self, rows):
        return torch.zeros((rows, V_STUB), dtype=torch.bfloat16)

    def copy_logits_into(self, dst, rows=1):
        self.calls["copies"] += 1
        dst[0] = len(self.ctx)  # the context this row's proposal was drawn after (exact in bf16 at these lengths)
        dst[1] = self.pending

    def rewind(self, slot, n):
        assert 0 <= n <= len(self.ctx) - self.prompt_len, ("rewind past the prompt", n)
        del self.ctx[len(self.ctx) - n:]

    def _verify(self, tokens):
        self._pure()
        assert tokens[0] == self.truth(self.ctx)
        before = list(self.ctx)
        self.ctx += list(tokens)
        return [self.rule(before + list(tokens[:i + 1])) for i in range(len(tokens))]

    def verify(self, slot, tokens):
        self.calls["verify"] += 1
        return self._verify(tokens)

    def verify_sampled(self, slot, tokens, draft_rows, draft_sampling=(0.0, None, None)):
        self.calls["verify_sampled"] += 1
        before = len(self.ctx)
        own = self._verify(tokens)
        for i in range(len(tokens) - 1):  # row i is the row tokens[i + 1] was drawn from
            assert int(draft_rows[i, 0]) == before + i + 1 and int(draft_rows[i, 1]) == tokens[i + 1], "the wrong draft row was handed over"
        self.draft_sampling = draft_sampling
        a = 0
        while a < len(tokens) - 1 and tokens[a + 1] == own[a]:
            a += 1
        return list(tokens[1:a + 1]) + [own[a]]


def _run(temperature, draft_differs, eos_at=None, max_new=23, proposal_length=4, **kw):
    from tiny_llm_hip.engine import speculative_generate_ids

    prompt = [5, 9, 33, 2, 7]
    truth = lambda ctx: _rule(ctx, eos_at)  # noqa: E731
    draft_rule = (lambda ctx: truth(ctx) if len(ctx) % 3 else (truth(ctx) + 1) % 50 + 2) if draft_differs else truth
    target, draft = StubEngine(truth, truth, len(prompt)), StubEngine(draft_rule, truth, len(prompt))
    stats = {}
    out = speculative_generate_ids(target, draft, prompt, max_new, proposal_length=proposal_length, eos_token_id=EOS, stats=stats,
                                   temperature=temperature, **kw)
    want, ctx = [], list(prompt)
    while len(want) < max_new:
        t = truth(ctx)
        if t == EOS:
            break
        want.append(t)
        ctx.append(t)
    assert out == want
    return out, stats, target, draft


@pytest.mark.parametrize("draft_differs", [False, True])
@pytest.mark.parametrize("eos_at", [None, 14, 16])
def test_sampled_loop_rewinds_and_counts(draft_differs, eos_at):
    out, stats, target, draft = _run(0.8, draft_differs, eos_at, top_k=16, seed=5)
    _, greedy, gt, gd = _run(0.0, draft_differs, eos_at)
    assert target.calls["verify"] == 0 and target.calls["verify_sampled"] == stats["target_calls"] - 1
    assert {k: v for k, v in stats.items() if k != "resampled"} == {k: v for k, v in greedy.items() if k != "resampled"}
    assert greedy["resampled"] == 0
    assert (stats["resampled"] > 0) == draft_differs
    assert stats["resampled"] <= stats["target_calls"] - 1 and stats["accepted"] <= stats["proposed"]
    if not draft_differs and eos_at is None:
        assert stats["accepted"] == stats["proposed"]
    # both engines sample under the same parameters, from different seeds; the draft steps one step per call, each row copied
    assert target.calls["set_sampling"] == [(0.8, 16, None, 5)]
    (dt, dk, dp, dseed), = draft.calls["set_sampling"]
    assert (dt, dk, dp) == (0.8, 16, None) and dseed != 5 and 0 <= dseed < 1 << 64
    assert set(draft.calls["decode_calls"]) == {1} and sum(draft.calls["decode_calls"]) == stats["draft_steps"]
    assert draft.calls["copies"] >= stats["proposed"]
    assert target.draft_sampling == (0.8, 16, None)
    assert sum(gd.calls["decode_calls"]) == sum(draft.calls["decode_calls"])


def test_temperature_zero_is_the_greedy_function():
    out, stats, target, draft = _run(0.0, True, top_k=16, top_p=0.9, seed=3)
    assert target.calls["verify_sampled"] == 0 and target.calls["verify"] == stats["target_calls"] - 1
    assert target.calls["set_sampling"] == [] and draft.calls["set_sampling"] == [] and draft.calls["copies"] == 0
    assert stats["resampled"] == 0 and set(stats) == {"target_calls", "draft_steps", "proposed", "accepted", "resampled"}
    assert max(draft.calls["decode_calls"]) > 1  # the draft free-runs several steps per call


def test_sampled_loop_arguments():
    from tiny_llm_hip.engine import speculative_generate_ids

    truth = lambda ctx: _rule(ctx)  # noqa: E731
    target, draft = StubEngine(truth, truth, 3), StubEngine(truth, truth, 3)
    with pytest.raises(ValueError):
        speculative_generate_ids(target, draft, [1, 2, 3], 5, temperature=-1.0)
    with pytest.raises(ValueError):
        speculative_generate_ids(target, draft, [1, 2, 3], 5, temperature=0.8, top_p=1.5)
    with pytest.raises(ValueError):
        speculative_generate_ids(target, draft, [1, 2, 3], 5, temperature=0.8, slot=1)
    draft.vocab_size = 65
    with pytest.raises(ValueError):
        speculative_generate_ids(target, draft, [1, 2, 3], 5, temperature=0.8)
    # without proposals the target samples alone, one verify_sampled row per token
    draft.vocab_size = V_STUB
    out = speculative_generate_ids(target, draft, [1, 2, 3], 5, proposal_length=0, temperature=0.8)
    assert len(out) == 5 and target.calls["verify_sampled"] == 5 and draft.ctx is None
