"""GPU tier: per-slot sampling on the device (tl_engine_set_sampling, tl_sample_logits, csrc/sample.h) against the numpy restatement of
its definition (tests/sampling_oracle.py).  Every id must equal the oracle's unless the oracle flags the draw ambiguous (fp32 rounding
on the device may then fall on either side)."""

import os

import numpy as np
import pytest
import torch

import sampling_oracle as S
from helpers import QWEN4B_CFG, TINY_CFG

pytestmark = pytest.mark.gpu

COMBOS = [(0, 1.0), (50, 1.0), (0, 0.9), (20, 0.8)]  # (top_k, top_p): neither, top-k, top-p, both


def _rows(V, rng):
    rand = rng.standard_normal(V).astype(np.float32) * 2.0
    peaked = rand.copy()
    peaked[rng.integers(0, V, 3)] += 12.0
    ties = np.round(rng.standard_normal(V) * 2.0).astype(np.float32)  # a handful of distinct values
    return [rand, peaked, ties]


def _check(got, want):
    assert got == want[0] or want[1], (got, want)


@pytest.mark.parametrize("V", [1024, 151936, 151941])
def test_kernel_matches_oracle(V):
    import tiny_llm_ext_hip as ext

    rng = np.random.default_rng(V)
    rows = _rows(V, rng)
    cases = [(r, T, k, p) for r in range(len(rows)) for T in (0.3, 0.7, 1.0, 2.0) for k, p in COMBOS]
    logits = torch.from_numpy(np.stack([rows[c[0]] for c in cases])).bfloat16().cuda()
    lf = logits.float().cpu().numpy()
    seeds = [1000 + i for i in range(len(cases))]
    pos = [17 * i + 3 for i in range(len(cases))]
    ids = ext.sample_logits(logits, [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], seeds, pos).cpu().tolist()
    for i, (r, T, k, p) in enumerate(cases):
        _check(ids[i], S.sample(lf[i], T, k, p, seeds[i], pos[i]))
    greedy = ext.sample_logits(logits, 0.0, 0, 1.0, 0, 0).cpu().tolist()
    assert greedy == [int(np.argmax(lf[i])) for i in range(len(cases))]
    k1 = ext.sample_logits(logits, 0.7, 1, 1.0, seeds, pos).cpu().tolist()
    assert k1 == greedy


def test_kernel_edge_rows():
    import tiny_llm_ext_hip as ext

    rows = torch.stack([torch.full((3001,), float("nan")), torch.full((3001,), float("-inf"))]).bfloat16().cuda()
    assert ext.sample_logits(rows, 1.0, 0, 0.9, 5, 5).cpu().tolist() == [0, 0]


def test_kernel_distribution():
    import tiny_llm_ext_hip as ext

    rng = np.random.default_rng(5)
    V, n = 151936, 20000
    row = torch.from_numpy(rng.standard_normal(V).astype(np.float32) * 2.0).bfloat16()
    lf = row.float().numpy().astype(np.float64)
    T, k, p = 0.7, 50, 0.9
    ids = ext.sample_logits(row.cuda()[None].expand(n, V).contiguous(), T, k, p, 12345, list(range(n))).cpu().numpy()
    kept, _ = S.kept_set(lf, k, p)
    assert set(ids.tolist()) <= set(kept.tolist())
    w = np.exp((lf[kept] - lf.max()) / T)
    expect = w / w.sum() * n
    obs = np.array([(ids == t).sum() for t in kept])
    nz = obs > 0
    g = 2.0 * np.sum(obs[nz] * np.log(obs[nz] / expect[nz]))
    assert g < 3.0 * len(kept), g  # far below a miscount (df = kept - 1)


# -- engine ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(TINY_CFG, seed=3, sigma=0.05, device="cuda")


@pytest.fixture(scope="module")
def q4b():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(dict(QWEN4B_CFG, num_hidden_layers=2), seed=11, sigma=0.02, device="cuda")


PARAMS = [(0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 50, 1.0), (0.8, 0, 0.9), (0.7, 50, 0.9)]


def _engine(model, n, route=None, **kw):
    from tiny_llm_hip.engine import DecodeEngine

    old = os.environ.pop("TL_AQL", None)
    if route == "hipgraph":
        os.environ["TL_AQL"] = "0"
    try:
        return DecodeEngine(model, page_size=16, num_pages=16 * n + 32, max_batch=n, max_prefill_rows=64, **kw)
    finally:
        os.environ.pop("TL_AQL", None)
        if old is not None:
            os.environ["TL_AQL"] = old


def _run(model, n, steps, route=None, use_graph=True, check=True, sampling=True, calls=None, **kw):
    eng = _engine(model, n, route, **kw)
    rng = np.random.default_rng(n)
    params = {}
    try:
        for i in range(n):
            eng.begin(i)
            if sampling:
                T, k, p = PARAMS[i % len(PARAMS)]
                params[i] = (T, k, p, 100 + i)
                eng.set_sampling(i, T, k or None, p if p < 1 else None, 100 + i)
            eng.prefill(i, rng.integers(0, 1000, 5 + i).tolist())
        out = [[eng.read_tokens(i, 1)[0]] for i in range(n)]
        for _ in range(steps) if calls is None else []:
            ctx = [eng.context_len(i) for i in range(n)]
            eng.decode(1, batch=n, use_graph=use_graph)
            got = eng.read_pending(n)
            if check:
                lf = eng.logits(n).float().cpu().numpy()
                for i in range(n):
                    T, k, p, seed = params.get(i, (0.0, 0, 1.0, 0))
                    _check(got[i], S.sample(lf[i], T, k, p, seed, ctx[i] + 1))
            for i in range(n):
                out[i].append(got[i])
        for c in calls or []:
            eng.decode(c, batch=n, use_graph=use_graph)
        if calls:
            out = [out[i] + eng.read_tokens(i, sum(calls)) for i in range(n)]
        return out, eng
    except Exception:
        eng.close()
        raise


@pytest.mark.parametrize("n", [1, 3, 4, 5, 17, 64])
def test_engine_draws_match_oracle(tiny, n):
    ids, eng = _run(tiny, n, 6)
    eng.close()


def test_engine_qwen4b_shapes(q4b):
    for n in (1, 5):
        ids, eng = _run(q4b, n, 3)
        eng.close()


def test_routes_agree(tiny):
    a, e1 = _run(tiny, 5, 8, check=False)
    b, e2 = _run(tiny, 5, 8, route="hipgraph", check=False)
    c, e3 = _run(tiny, 5, 8, use_graph=False, check=False)
    assert e1.replay_route() == "aql" and e2.replay_route().startswith("hipgraph")
    for e in (e1, e2, e3):
        e.close()
    assert a == b == c


def test_step_splitting(tiny):
    a, e1 = _run(tiny, 3, 0, calls=[32])
    b, e2 = _run(tiny, 3, 0, calls=[1] * 32)
    e1.close(), e2.close()
    assert a == b


def test_greedy_unchanged(tiny):
    a, e1 = _run(tiny, 5, 0, sampling=False, calls=[12])
    la = e1.logits(5).float().cpu()
    e2 = _engine(tiny, 5)
    rng = np.random.default_rng(5)
    for i in range(5):
        e2.begin(i)
        e2.set_sampling(i, 0.0, seed=7)
        e2.prefill(i, rng.integers(0, 1000, 5 + i).tolist())
    e2.decode(12, batch=5)
    b = [e2.read_tokens(i, 13) for i in range(5)]
    assert a == b
    assert torch.equal(la, e2.logits(5).float().cpu())
    # mixed batch: the greedy slots keep their ids
    m, e3 = _run(tiny, 5, 0, calls=[12])
    assert m[0] == a[0]  # slot 0 is greedy in PARAMS
    for e in (e1, e2, e3):
        e.close()


def test_top_k_one_is_greedy(tiny):
    a, e1 = _run(tiny, 2, 0, sampling=False, calls=[10])
    e2 = _engine(tiny, 2)
    rng = np.random.default_rng(2)
    for i in range(2):
        e2.begin(i)
        e2.set_sampling(i, 1.5, 1, None, 999 + i)
        e2.prefill(i, rng.integers(0, 1000, 5 + i).tolist())
    e2.decode(10, batch=2)
    assert a == [e2.read_tokens(i, 11) for i in range(2)]
    e1.close(), e2.close()


def test_first_token_and_packed_prefill(tiny):
    eng = _engine(tiny, 3)
    try:
        prompt = list(range(7, 40))
        eng.begin(0)
        eng.set_sampling(0, 1.0, seed=42)
        eng.prefill(0, prompt)
        lf = eng.logits(1).float().cpu().numpy()[0]
        _check(eng.read_tokens(0, 1)[0], S.sample(lf, 1.0, 0, 1.0, 42, len(prompt)))
        eng.begin(1)
        eng.set_sampling(1, 0.9, 40, 0.95, 43)
        eng.prefill_packed([(1, prompt[:20], True)])
        lf = eng.logits(1).float().cpu().numpy()[0]
        _check(eng.read_tokens(1, 1)[0], S.sample(lf, 0.9, 40, 0.95, 43, 20))
    finally:
        eng.close()


def test_slot_moves_fork_release_and_verify(tiny):
    eng = _engine(tiny, 4)
    try:
        eng.begin(2)
        eng.set_sampling(2, 1.0, seed=5)
        eng.prefill(2, list(range(10)))
        with pytest.raises(RuntimeError):
            eng.verify(2, [1, 2])
        eng.move(2, 0)
        eng.fork(0, 1)
        eng.set_sampling(1, 1.0, seed=6)
        ctx = eng.context_len(0)
        eng.decode(1, batch=2)
        got = eng.read_pending(2)
        lf = eng.logits(2).float().cpu().numpy()
        _check(got[0], S.sample(lf[0], 1.0, 0, 1.0, 5, ctx + 1))
        _check(got[1], S.sample(lf[1], 1.0, 0, 1.0, 6, ctx + 1))
        eng.release(0)
        eng.begin(0)
        eng.prefill(0, list(range(10)))
        eng.verify(0, [3])  # greedy again after release / begin
    finally:
        eng.close()


@pytest.mark.parametrize("n", [1, 4, 5, 64])
def test_written_once_sampled_plans(tiny, n):
    ids, eng = _run(tiny, n, 1, check=False)
    try:
        c = eng.check_step(n)
        assert c["double_writes"] == 0, c
    finally:
        eng.close()


def test_fp8_pages(tiny):
    ids, eng = _run(tiny, 3, 4, kv_format="fp8")
    eng.close()


def test_batch_generate_sampling(tiny):
    from tiny_llm_hip.engine import batch_generate_ids

    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, 1000, int(rng.integers(4, 30))).tolist() for _ in range(7)]

    def run(sampling):
        eng = _engine(tiny, 5)
        try:
            return sorted(batch_generate_ids(eng, prompts, 9, batch_size=4, prefill_step=16, sampling=sampling))
        finally:
            eng.close()

    s = {"temperature": 0.9, "top_k": 40, "top_p": 0.95}
    assert run(s) == run(s)
    assert run(None) == run([{"temperature": 0.0}] * 7)
