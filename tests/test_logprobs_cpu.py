"""CPU tier: the definition of the engine's per-token log-probabilities (tests/logprob_oracle.py) against float64 log_softmax and the
sampler's order (tests/sampling_oracle.py), its edge rows, the Python argument checks, and DecodeEngine.score's chunk chaining against a
stand-in for the C library."""

import ctypes
import math

import numpy as np
import pytest
import torch

import logprob_oracle as L
import sampling_oracle as S


def test_oracle_matches_float64_log_softmax_on_untied_rows():
    rng = np.random.default_rng(1)
    for V in (7, 1024, 151936):
        l = rng.permutation(np.arange(V, dtype=np.float64)) * (8.0 / V) + rng.standard_normal() * 3
        want = torch.log_softmax(torch.from_numpy(l), 0).numpy()
        assert abs(L.lse(l) - float(torch.logsumexp(torch.from_numpy(l), 0))) < 1e-9
        for t in rng.integers(0, V, 5):
            assert abs(L.logprob(l, int(t)) - want[t]) < 1e-9
        ids, lp = L.top(l, 20)
        n = min(20, V)
        assert ids[:n].tolist() == np.argsort(-l, kind="stable")[:n].tolist()
        np.testing.assert_allclose(lp[:n], want[ids[:n]], atol=1e-9)
        assert (ids[n:] == -1).all() and np.isneginf(lp[n:]).all()


@pytest.mark.parametrize("n", [0, 1, 5, 20])
def test_top_order_is_the_samplers_kept_set(n):
    rng = np.random.default_rng(n)
    for _ in range(5):
        l = np.round(rng.standard_normal(3000) * 2.0)  # a handful of distinct values: ties everywhere
        l[rng.integers(0, 3000, 40)] = np.nan
        ids, _ = L.top(l, n)
        kept, _ = S.kept_set(l, n, 1.0) if n else (np.array([], dtype=np.int64), False)
        assert ids.tolist() == kept.tolist()


def test_ties_nan_and_short_rows():
    l = np.array([1.0, 3.0, np.nan, 3.0, -np.inf, 2.0])
    ids, lp = L.top(l, 20)
    assert ids[:5].tolist() == [1, 3, 5, 0, 4] and (ids[5:] == -1).all()  # NaN never ranked; N beyond the rankable tokens
    assert lp[0] == lp[1] and np.isneginf(lp[4]) and np.isneginf(lp[5:]).all()
    assert math.isnan(L.logprob(l, 2)) and L.logprob(l, 4) == -np.inf
    assert abs(math.exp(L.logprob(l, 1)) * 2 + math.exp(L.logprob(l, 5)) + math.exp(L.logprob(l, 0)) - 1.0) < 1e-12
    assert L.greedy(l) == 1


@pytest.mark.parametrize("row", [[np.nan] * 4, [-np.inf, np.nan, -np.inf], [1.0, np.inf, 2.0, np.inf]])
def test_rows_without_finite_maximum(row):
    l = np.array(row)
    assert math.isnan(L.lse(l))
    assert all(math.isnan(L.logprob(l, t)) for t in range(l.size))
    ids, lp = L.top(l, 3)
    assert ids.tolist() == (L.order(l).tolist() + [-1] * 3)[:3]
    assert all(math.isnan(v) for v, i in zip(lp, ids) if i >= 0)
    assert L.greedy(l) == (1 if np.isposinf(l).any() else 0)


def test_python_argument_validation():
    import tiny_llm_ext_hip as ext
    from tiny_llm_hip.engine import TokenLogprob, logprobs_arg

    assert logprobs_arg(None) == -1 and logprobs_arg(0) == 0 and logprobs_arg(20) == 20
    for bad in (-1, 21, 2.0, True, "3"):
        with pytest.raises(ValueError):
            logprobs_arg(bad)
    assert ctypes.sizeof(ext.TlTokenLogprob) == 164
    rec = ext.TlTokenLogprob()
    rec.logprob = -0.5
    for i in range(20):
        rec.top_ids[i] = i if i < 2 else -1
        rec.top_logprobs[i] = -float(i) if i < 2 else -float("inf")
    assert TokenLogprob.of(rec) == TokenLogprob(-0.5, [(0, 0.0), (1, -1.0)])
    with pytest.raises(ValueError):
        ext.logprob_rows(torch.zeros(2, 8, dtype=torch.bfloat16), None, 0)  # host tensor: the extension is GPU-only


class _FakeLib:
    """tl_engine_begin / tl_engine_score / tl_engine_release on the host: a chunk's row i scores the token after it -- the next token
    of the chunk, or next_token for the last row -- as -(token id) (NaN for next_token < 0)."""

    def __init__(self):
        self.calls = []

    def tl_engine_begin(self, h, slot):
        self.calls.append(("begin", slot))
        return 0

    def tl_engine_release(self, h, slot):
        self.calls.append(("release", slot))
        return 0

    def tl_engine_score(self, h, slot, arr, n, nxt, out, argmax):
        toks = [arr[i] for i in range(n)]
        self.calls.append(("score", slot, toks, nxt))
        follow = toks[1:] + [nxt]
        for i, t in enumerate(follow):
            out[i] = -float(t) if t >= 0 else float("nan")
        return 0


@pytest.mark.parametrize("chunk", [None, 1, 3, 4, 10])
def test_score_chains_chunks(monkeypatch, chunk):
    import tiny_llm_hip.engine as E

    fake = _FakeLib()
    monkeypatch.setattr(E, "_lib", fake)
    eng = E.DecodeEngine.__new__(E.DecodeEngine)
    eng._h, eng.max_prefill_rows = 1, 8
    tokens = list(range(1, 11))
    if chunk == 10:
        with pytest.raises(ValueError):
            eng.score(tokens, chunk=chunk)  # beyond max_prefill_rows
        return
    got = eng.score(tokens, slot=2, chunk=chunk)
    assert got == [-float(t) for t in tokens[1:]]
    size = chunk or 8
    scores = [c for c in fake.calls if c[0] == "score"]
    assert [c[2] for c in scores] == [tokens[i:i + size] for i in range(0, 10, size)]
    assert [c[3] for c in scores] == [tokens[i + size] if i + size < 10 else -1 for i in range(0, 10, size)]
    assert fake.calls[0] == ("begin", 2) and fake.calls[-1] == ("release", 2)
    assert eng.score([5], chunk=chunk) == []
    with pytest.raises(ValueError):
        eng.score([])
