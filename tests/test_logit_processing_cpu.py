"""CPU tier: the numpy restatement of the decode engine's logit processing (tests/logit_processing_oracle.py) against independent
statements of the same rules, and the argument validation of the Python layer.  No kernel is launched here."""

import math

import numpy as np
import pytest

import logit_processing_oracle as P


def _bf16_row(rng, V, sigma=2.0):
    return P.bf16_round(rng.standard_normal(V).astype(np.float32) * sigma)


def test_bf16_rounding_is_nearest_even():
    import torch

    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 50, np.float32([0.0, -0.0, 1.00390625, 1.01171875, np.inf, -np.inf, 3.3e38])])
    want = torch.from_numpy(v).bfloat16().float().numpy()
    assert np.array_equal(P.bits(P.bf16_round(v)), P.bits(want))
    assert np.isnan(P.bf16_round(np.float32([np.nan]))[0])
    assert np.array_equal(P.from_bits(P.bits(want)), want)


def test_repetition_rule_equals_transformers():
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    rng = np.random.default_rng(1)
    V = 1024
    row = _bf16_row(rng, V)
    hist = rng.integers(0, V, 40)
    proc = transformers.RepetitionPenaltyLogitsProcessor(penalty=1.3)
    want = proc(torch.from_numpy(hist)[None], torch.from_numpy(row.copy())[None])[0].numpy()
    # the oracle before its final rounding: the same float32 values, element for element
    seen = np.zeros(V, bool)
    seen[hist] = True
    with np.errstate(all="ignore"):
        got = np.where(seen, np.where(row > 0, row / np.float32(1.3), row * np.float32(1.3)), row).astype(np.float32)
    assert np.array_equal(got, want)
    # ... and the oracle itself is that, rounded; prompt tokens and produced tokens are the same to this stage
    cnt = np.zeros(V, np.int64)
    np.add.at(cnt, hist[:20], 1)
    prompt = np.zeros(V, bool)
    prompt[hist[20:]] = True
    assert np.array_equal(P.bits(P.process(row, seen, np.zeros(V, int), 1.3)), P.bits(P.bf16_round(want)))
    assert np.array_equal(P.bits(P.process(row, prompt, cnt, 1.3)), P.bits(P.bf16_round(want)))


def test_presence_and_frequency_against_float64():
    rng = np.random.default_rng(2)
    V = 4096
    row = _bf16_row(rng, V)
    cnt = rng.integers(0, 6, V) * (rng.random(V) < 0.3)
    for p, f in ((0.5, 0.0), (0.0, 0.25), (1.5, 0.7), (-0.5, -0.1)):
        got = P.process(row, np.zeros(V, bool), cnt, 1.0, p, f).astype(np.float64)
        exact = row.astype(np.float64) - cnt * float(np.float32(f)) - (cnt > 0) * float(np.float32(p))
        # at most one bf16 rounding of the result (8 significant bits: half an ulp is at most 2^-8 of the value) on top of the three
        # fp32 roundings before it (intermediates below 16 in magnitude: 3 x 16 x 2^-24 < 4e-6)
        assert np.all(np.abs(got - exact) <= np.abs(exact) * 2.0 ** -8 + 4e-6)
        assert np.array_equal(got[cnt == 0], row[cnt == 0].astype(np.float64))


def test_no_fused_multiply_add():
    """l = 1, frequency = float32(1/3), count = 3: the product rounds to exactly 1.0, so the result is +0.0; a fused multiply-add
    would give about -2.98e-8, a nonzero bf16."""
    f = np.float32(1.0) / np.float32(3.0)
    assert np.float32(f * np.float32(3.0)) == np.float32(1.0)
    assert float(np.float64(1.0) - np.float64(f) * 3.0) != 0.0  # what one rounding at the end (the fused form) would keep
    out = P.process(np.float32([1.0, 1.0]), np.zeros(2, bool), np.array([3, 0]), 1.0, 0.0, float(f))
    assert P.bits(out).tolist() == [0x0000, 0x3F80]


def test_order_of_the_stages_and_edges():
    # repetition first, then frequency, presence, bias: (4 / 2) - 0.5 * 2 - 0.25 + 1 = 1.75; a negative logit is multiplied: -4 * 2 - ... = -8.25
    out = P.process(np.float32([4.0, -4.0]), np.zeros(2, bool), np.array([2, 2]), 2.0, 0.25, 0.5, {0: 1.0, 1: 1.0})
    assert out.tolist() == [1.75, -8.25]
    # a token that is only in the prompt: repetition yes, presence / frequency no
    out = P.process(np.float32([4.0, 4.0, 4.0]), np.array([True, False, False]), np.array([0, 1, 0]), 2.0, 0.5, 0.25)
    assert out.tolist() == [2.0, 1.25, 4.0]
    # NaN stays NaN, -inf bans, -0.0 goes through v + 0.0, r < 1 and negative penalties encourage
    out = P.process(np.float32([np.nan, 3.0, -0.0, 2.0, np.inf, -np.inf]), np.zeros(6, bool), np.array([1, 1, 0, 1, 1, 1]), 0.5, -1.0, 0.0,
                    {1: -np.inf})
    assert np.isnan(out[0]) and out[1] == -np.inf and P.bits(out)[2] == 0 and out[3] == 5.0 and out[4] == np.inf and out[5] == -np.inf
    # saturation: counts beyond 32,767 act as 32,767
    a = P.process(np.float32([1.0]), np.zeros(1, bool), np.array([40000]), 1.0, 0.0, 0.001)
    b = P.process(np.float32([1.0]), np.zeros(1, bool), np.array([32767]), 1.0, 0.0, 0.001)
    assert a == b and P.pack_history([True], [40000])[0] == 0xFFFF and P.pack_history([False], [3])[0] == 3
    # neutral: bit for bit, -0.0 and NaN payloads included
    row = P.from_bits(np.uint16([0x8000, 0x7FC1, 0x3F80]))
    assert np.array_equal(P.bits(P.process(row, np.ones(3, bool), np.ones(3, int))), np.uint16([0x8000, 0x7FC1, 0x3F80]))


def test_history_follows_the_header_rule():
    h = P.History(16)
    h.consume_prompt([1, 2, 2])
    h.feed(5)
    h.feed(5)
    g = h.copy()
    g.feed(1)
    assert h.prompt.sum() == 2 and h.count[5] == 2 and h.count[1] == 0 and g.count[1] == 1


def test_penalty_args_and_request_penalties():
    from tiny_llm_hip.engine import penalty_args, request_settings, sampling_args

    assert penalty_args() == (1.0, 0.0, 0.0)
    assert penalty_args(1.3, -0.5, 2) == (1.3, -0.5, 2.0)
    for bad in (dict(repetition=0.0), dict(repetition=-1.0), dict(repetition=float("nan")), dict(repetition=float("inf")),
                dict(presence=float("inf")), dict(frequency=float("nan")), dict(presence="1"), dict(frequency=True)):
        with pytest.raises(ValueError):
            penalty_args(**bad)
    def request_penalties(sampling, n, vocab_size):
        return [(s.penalties, s.bias) for s in request_settings(sampling, n, vocab_size=vocab_size)]

    def request_sampling(sampling, n, base_seed=0):
        return [s.sampling for s in request_settings(sampling, n, base_seed, vocab_size=100)]

    assert request_penalties(None, 3, 100) == [((1.0, 0.0, 0.0), {})] * 3  # neutral: RequestSettings.apply makes no call
    got = request_penalties({"presence_penalty": 1.5, "temperature": 0.7}, 2, 100)
    assert got == [((1.0, 1.5, 0.0), {})] * 2
    got = request_penalties([{"logit_bias": {3: -math.inf}}, {}], 2, 100)
    assert got == [((1.0, 0.0, 0.0), {3: -math.inf}), ((1.0, 0.0, 0.0), {})]
    for bad in ({"presence": 1.0}, {"logit_bias": {100: 1.0}}, {"logit_bias": {1: math.nan}}, {"repetition_penalty": 0}):
        with pytest.raises(ValueError):
            request_penalties(bad, 1, 100)
    with pytest.raises(ValueError):
        request_penalties([{}], 2, 100)
    # the sampling half is what tests/test_device_sampling_cpu.py expects, with or without the new keys in the dicts
    assert sampling_args() == (0.0, 0, 1.0, 0)
    assert [g[:3] for g in request_sampling(None, 3)] == [(0.0, 0, 1.0)] * 3  # greedy
    assert [g[3] for g in request_sampling({"temperature": 1.0}, 3, base_seed=10)] == [10, 11, 12]
    assert request_sampling([{"temperature": 1.0, "seed": 5, "presence_penalty": 1.0}, {}], 2) == [(1.0, 0, 1.0, 5), (0.0, 0, 1.0, 1)]
    with pytest.raises(ValueError):
        request_sampling({"temp": 1.0}, 1)


def test_logit_bias_validation(built_libs):
    import tiny_llm_ext_hip as ext

    assert ext.TL_MAX_LOGIT_BIAS == P.MAX_LOGIT_BIAS == 1024
    assert ext.logit_bias_arg(None, 10) == ([], []) and ext.logit_bias_arg({}, 10) == ([], [])
    assert ext.logit_bias_arg({3: 1, 9: -math.inf}, 10) == ([3, 9], [1.0, -math.inf])
    assert len(ext.logit_bias_arg({i: 0.5 for i in range(1024)}, 2000)[0]) == 1024
    for bad in ({10: 1.0}, {-1: 1.0}, {1: math.nan}, {1: math.inf}, {1.0: 1.0}, {True: 1.0}, {"1": 1.0}, {1: "x"}, [(1, 1.0)],
                {i: 0.5 for i in range(1025)}):
        with pytest.raises(ValueError):
            ext.logit_bias_arg(bad, 10 if not isinstance(bad, dict) or len(bad) < 100 else 2000)


def test_header_states_the_contract():
    from pathlib import Path

    text = (Path(__file__).resolve().parent.parent / "include" / "tinyllm_engine.h").read_text()
    for needle in ("#define TL_MAX_LOGIT_BIAS 1024", "tl_engine_set_penalties", "tl_engine_set_logit_bias", "tl_process_logits", "32,767",
                   "no fused multiply-add"):
        assert needle in text, needle
