"""CPU tier: the device sampler's definition (tests/sampling_oracle.py) -- Philox4x32-10 known answers (Random123), the kept set against
a torch restatement of the reference sampler (src/tiny_llm_ref/sampler.py: top-k by partition, top-p over exp(logprobs) of the
full vocabulary, categorical over logprobs / T), the tie rules, and the argument checks of the Python layer."""

import numpy as np
import pytest
import torch

import sampling_oracle as S


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(counter, key, want):
    assert tuple(S.philox4x32_10(counter, key)) == want


def test_uniform_key_and_counter_mapping():
    seed = 0x0123456789ABCDEF
    out = S.philox4x32_10((77, 0, 0x53414D50, 0), (0x89ABCDEF, 0x01234567))
    assert S.uniform(seed, 77) == (out[0] >> 8) * 2.0 ** -24
    us = [S.uniform(5, p) for p in range(2000)]
    assert all(0.0 <= u < 1.0 for u in us) and 0.45 < np.mean(us) < 0.55


def _bf16_row(rng, V, scale=3.0):
    return torch.from_numpy(rng.standard_normal(V).astype(np.float32) * scale).bfloat16().float().numpy()


def _torch_reference_kept(l, top_k, top_p):
    """The reference sampler's masking on torch: logprobs = l - logsumexp(l); top-k keeps the k largest (argpartition); top-p keeps a
    token while the exp(logprobs) mass ranked before it is < p."""
    x = torch.from_numpy(np.asarray(l, dtype=np.float64))
    logprobs = x - torch.logsumexp(x, 0)
    keep = torch.ones_like(x, dtype=torch.bool)
    if top_k > 0:
        idx = torch.topk(logprobs, top_k).indices
        keep = torch.zeros_like(keep)
        keep[idx] = True
    if 0 < top_p < 1:
        order = torch.argsort(-logprobs, stable=True)
        p = torch.exp(logprobs[order])
        before = torch.cumsum(p, 0) - p
        kp = torch.zeros_like(keep)
        kp[order[before < top_p]] = True
        kp[order[0]] = True
        keep &= kp
    return set(torch.nonzero(keep).flatten().tolist())


@pytest.mark.parametrize("top_k,top_p", [(0, 0.9), (50, 1.0), (20, 0.8), (1, 1.0), (0, 0.5)])
def test_kept_set_matches_reference_restatement_on_untied_rows(top_k, top_p):
    rng = np.random.default_rng(3)
    for _ in range(5):
        l = rng.permutation(np.arange(4096, dtype=np.float64)) * 0.01  # distinct values: no ties
        kept, amb = S.kept_set(l, top_k, top_p)
        if amb:
            continue
        assert set(kept.tolist()) == _torch_reference_kept(l, top_k, top_p)


def test_ties_keep_exactly_k_lowest_ids_first():
    l = np.zeros(100)
    l[[5, 17, 40, 41, 90]] = 2.0
    kept, _ = S.kept_set(l, 3, 1.0)
    assert kept.tolist() == [5, 17, 40]
    kept, _ = S.kept_set(l, 7, 1.0)
    assert kept.tolist() == [5, 17, 40, 41, 90, 0, 1]
    # -0 and +0 tie
    l = np.array([0.0, -0.0, 0.0, -1.0])
    assert S.kept_set(l, 2, 1.0)[0].tolist() == [0, 1]


def test_top_p_counts_the_full_vocabulary_and_first_token_stays():
    l = np.array([1.0, 1.0, 0.0, -50.0])
    kept, _ = S.kept_set(l, 0, 0.3)
    assert kept.tolist() == [0]
    kept, _ = S.kept_set(l, 0, 0.5)  # mass before token 1 is 0.42... < 0.5
    assert kept.tolist() == [0, 1]


def test_draw_rules():
    l = _bf16_row(np.random.default_rng(1), 1000)
    assert S.sample(l, 0.0)[0] == int(np.argmax(l))
    for seed in range(20):
        assert S.sample(l, 0.7, top_k=1, seed=seed, position=seed)[0] == int(np.argmax(l))
    assert S.sample(np.full(8, np.nan), 1.0)[0] == 0
    assert S.sample(np.full(8, -np.inf), 1.0)[0] == 0
    tok, _ = S.sample(l, 1.0, top_k=10, seed=9, position=3)
    assert tok in set(S.kept_set(l, 10)[0].tolist())


def test_python_argument_validation():
    from tiny_llm_hip.engine import request_settings, sampling_args

    assert sampling_args() == (0.0, 0, 1.0, 0)
    assert sampling_args(0.7, 50, 0.9, 3) == (0.7, 50, 0.9, 3)
    for bad in [dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_k=-1),
                dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.5), dict(seed=-1), dict(seed=1 << 64)]:
        with pytest.raises(ValueError):
            sampling_args(**bad)
    def request_sampling(sampling, n, base_seed=0):
        return [s.sampling for s in request_settings(sampling, n, base_seed)]

    assert [g[:3] for g in request_sampling(None, 3)] == [(0.0, 0, 1.0)] * 3  # greedy: RequestSettings.apply makes no call
    got = request_sampling({"temperature": 1.0}, 3, base_seed=10)
    assert [g[3] for g in got] == [10, 11, 12]
    got = request_sampling([{"temperature": 1.0, "seed": 5}, {}], 2)
    assert got[0][3] == 5 and got[1] == (0.0, 0, 1.0, 1)
    with pytest.raises(ValueError):
        request_sampling([{}], 2)
    with pytest.raises(ValueError):
        request_sampling({"temp": 1.0}, 1)
