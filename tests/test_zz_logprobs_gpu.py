"""GPU tier: per-token log-probabilities (tl_engine_set_logprobs, tl_logprob_rows, csrc/logprob.h) and prompt scoring (tl_engine_score)
against the numpy restatement of their definition (tests/logprob_oracle.py)."""

import math
import os

import numpy as np
import pytest
import torch

import logprob_oracle as L
from helpers import QWEN4B_CFG, TINY_CFG

pytestmark = pytest.mark.gpu

TOL = 2e-4  # fp32 sum of at most 151,941 terms below 1 in a fixed order, with margin


def _rows(V, rng):
    rand = rng.standard_normal(V).astype(np.float32) * 2.0
    peaked = rand.copy()
    peaked[rng.integers(0, V, 3)] += 12.0
    ties = np.round(rng.standard_normal(V) * 2.0).astype(np.float32)
    return [rand, peaked, ties]


def _check_row(lf, lp, top_ids, top_lp, token, n):
    want = L.logprob(lf, token)
    assert (math.isnan(lp) and math.isnan(want)) or abs(lp - want) <= TOL, (lp, want)
    ids, wl = L.top(lf, n)
    assert list(top_ids[:n]) == ids.tolist()
    for g, w in zip(top_lp[:n], wl):
        assert (math.isnan(g) and math.isnan(w)) or g == w == -math.inf or abs(g - w) <= TOL, (g, w)


@pytest.mark.parametrize("V", [1024, 151936, 151941])
def test_kernel_matches_oracle(V):
    import tiny_llm_ext_hip as ext

    rng = np.random.default_rng(V)
    rows = _rows(V, rng)
    logits = torch.from_numpy(np.stack(rows)).bfloat16().cuda()
    lf = logits.float().cpu().numpy()
    ids = rng.integers(0, V, len(rows)).tolist()
    for n in (0, 1, 5, 20):
        lp, ti, tl = (t.cpu().numpy() for t in ext.logprob_rows(logits, ids, n))
        for i in range(len(rows)):
            _check_row(lf[i], lp[i], ti[i], tl[i], ids[i], n)
    lp, _, _ = ext.logprob_rows(logits, None, 0)
    for i in range(len(rows)):
        assert abs(float(lp[i]) - L.logprob(lf[i], L.greedy(lf[i]))) <= TOL


def test_kernel_edge_rows():
    import tiny_llm_ext_hip as ext

    V = 3001
    rows = torch.stack([torch.full((V,), float("nan")), torch.full((V,), float("-inf")), torch.zeros(V), torch.zeros(V)])
    rows[2, 17] = float("inf")
    rows[3, 5] = float("nan")
    rows[3, 9] = float("-inf")
    logits = rows.bfloat16().cuda()
    lf = logits.float().cpu().numpy()
    lp, ti, tl = (t.cpu().numpy() for t in ext.logprob_rows(logits, [3, 3, 17, 5], 20))
    for i, tok in enumerate([3, 3, 17, 5]):
        _check_row(lf[i], lp[i], ti[i], tl[i], tok, 20)
    assert ti[0].tolist() == [-1] * 20 and ti[2][0] == 17 and math.isnan(tl[2][0]) and math.isnan(lp[3])
    lp, _, _ = ext.logprob_rows(logits, [9, -1, 0, 9], 0)
    assert lp[0].isnan() and lp[1].isnan() and lp[3].item() == -math.inf


# -- engine ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(TINY_CFG, seed=3, sigma=0.05, device="cuda")


@pytest.fixture(scope="module")
def q4b():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(dict(QWEN4B_CFG, num_hidden_layers=2), seed=11, sigma=0.02, device="cuda")


SAMPLING = [(0.0, None, None), (1.0, None, None), (0.7, 50, 0.9)]
TOPN = [20, None, 0, 5]  # per slot, cycled: some slots off


def _engine(model, n, route=None, max_prefill_rows=64, num_pages=None, **kw):
    from tiny_llm_hip.engine import DecodeEngine

    old = os.environ.pop("TL_AQL", None)
    if route == "hipgraph":
        os.environ["TL_AQL"] = "0"
    try:
        return DecodeEngine(model, page_size=16, num_pages=num_pages or 16 * n + 64, max_batch=n, max_prefill_rows=max_prefill_rows, **kw)
    finally:
        os.environ.pop("TL_AQL", None)
        if old is not None:
            os.environ["TL_AQL"] = old


def _run(model, n, steps, route=None, use_graph=True, check=True, logprobs=True, calls=None, **kw):
    """n slots, mixed greedy / sampling, logprobs per TOPN; returns (ids per slot, records per slot, engine)."""
    eng = _engine(model, n, route, **kw)
    rng = np.random.default_rng(n)
    try:
        for i in range(n):
            eng.begin(i)
            T, k, p = SAMPLING[i % len(SAMPLING)]
            if T:
                eng.set_sampling(i, T, k, p, 100 + i)
            if logprobs and TOPN[i % len(TOPN)] is not None:
                eng.set_logprobs(i, TOPN[i % len(TOPN)])
            eng.prefill(i, rng.integers(0, 1000, 5 + i).tolist())
        on = [i for i in range(n) if logprobs and TOPN[i % len(TOPN)] is not None]
        ids = [[eng.read_tokens(i, 1)[0]] for i in range(n)]
        recs = {i: eng.read_logprobs(i, 1) for i in on}
        for _ in range(steps) if calls is None else []:
            eng.decode(1, batch=n, use_graph=use_graph)
            got = eng.read_pending(n)
            if on:
                pend = eng.read_pending_logprobs(n)
            if check and on:
                lf = eng.logits(n).float().cpu().numpy()
                for i in on:
                    r = pend[i]
                    tn = TOPN[i % len(TOPN)]
                    _check_row(lf[i], r.logprob, [t[0] for t in r.top] + [-1] * 20, [t[1] for t in r.top] + [-math.inf] * 20, got[i], tn)
                    assert len(r.top) == min(tn, L.order(lf[i]).size)
            for i in range(n):
                ids[i].append(got[i])
            for i in on:
                recs[i].append(pend[i])
        for c in calls or []:
            eng.decode(c, batch=n, use_graph=use_graph)
        if calls:
            ids = [ids[i] + eng.read_tokens(i, sum(calls)) for i in range(n)]
            recs = {i: recs[i] + eng.read_logprobs(i, sum(calls)) for i in on}
        elif on and steps:
            for i in on:  # the ring holds what the pending records said
                assert eng.read_logprobs(i, steps + 1) == recs[i]
        return ids, recs, eng
    except Exception:
        eng.close()
        raise


@pytest.mark.parametrize("n", [1, 3, 4, 5, 17, 64])
def test_engine_records_match_oracle(tiny, n):
    ids, recs, eng = _run(tiny, n, 4)
    assert eng.replay_route() == "aql"
    eng.close()
    plain, _, e2 = _run(tiny, n, 4, logprobs=False, check=False)
    e2.close()
    assert ids == plain  # recording changes no id


def test_engine_qwen4b_shapes(q4b):
    for n in (1, 5):
        ids, recs, eng = _run(q4b, n, 2)
        eng.close()


def test_routes_eager_and_step_splitting_agree(tiny):
    a, ra, e1 = _run(tiny, 5, 6, check=False)
    b, rb, e2 = _run(tiny, 5, 6, route="hipgraph", check=False)
    c, rc, e3 = _run(tiny, 5, 6, use_graph=False, check=False)
    assert e1.replay_route() == "aql" and e2.replay_route().startswith("hipgraph")
    s1 = e1.stats()
    assert s1["aql_steps"] == s1["graph_replays"] > 0  # logprob plans replay as AQL packets, none falls back
    for e in (e1, e2, e3):
        e.close()
    assert a == b == c and ra == rb == rc
    d, rd, e4 = _run(tiny, 3, 0, calls=[12])
    f, rf, e5 = _run(tiny, 3, 0, calls=[1] * 12)
    e4.close(), e5.close()
    assert d == f and rd == rf


def test_first_token_from_prefill_and_packed_prefill(tiny):
    eng = _engine(tiny, 3)
    try:
        prompt = list(range(7, 40))
        eng.begin(0)
        eng.set_logprobs(0, 20)
        eng.prefill(0, prompt)
        lf = eng.logits(1).float().cpu().numpy()[0]
        r = eng.read_logprobs(0, 1)[0]
        tok = eng.read_tokens(0, 1)[0]
        _check_row(lf, r.logprob, [t[0] for t in r.top], [t[1] for t in r.top], tok, 20)
        assert eng.read_pending_logprobs(1)[0] == r
        eng.begin(1)
        eng.set_sampling(1, 0.9, 40, 0.95, 43)
        eng.set_logprobs(1, 3)
        eng.prefill_packed([(1, prompt[:20], True)])
        lf = eng.logits(1).float().cpu().numpy()[0]
        r = eng.read_logprobs(1, 1)[0]
        _check_row(lf, r.logprob, [t[0] for t in r.top], [t[1] for t in r.top], eng.read_tokens(1, 1)[0], 3)
    finally:
        eng.close()


def test_slot_moves_fork_release_and_read_count(tiny):
    eng = _engine(tiny, 4)
    try:
        eng.begin(2)
        eng.prefill(2, list(range(10)))
        eng.set_logprobs(2, 2)  # from the next produced token on
        with pytest.raises(RuntimeError):
            eng.read_logprobs(2, 1)
        eng.decode(2, batch=3)
        first = eng.read_logprobs(2, 2)
        with pytest.raises(RuntimeError):
            eng.read_logprobs(2, 3)
        eng.move(2, 0)
        assert eng.read_pending_logprobs(1)[0] == first[-1]  # the pending record moved with the sequence
        with pytest.raises(RuntimeError):
            eng.read_logprobs(0, 1)  # the ring restarts on a move, like the token ring
        eng.fork(0, 1)
        eng.decode(1, batch=2)
        pend = eng.read_pending_logprobs(2)
        lf = eng.logits(2).float().cpu().numpy()
        got = eng.read_pending(2)
        for i in range(2):
            _check_row(lf[i], pend[i].logprob, [t[0] for t in pend[i].top], [t[1] for t in pend[i].top], got[i], 2)
            assert eng.read_logprobs(i, 1) == [pend[i]]
        eng.verify(0, [got[0]])  # records nothing
        assert eng.read_logprobs(0, 1) == [pend[0]]
        eng.release(0)
        eng.begin(0)
        eng.prefill(0, list(range(10)))
        with pytest.raises(RuntimeError):
            eng.read_logprobs(0, 1)  # begin / release switched it off
        eng.set_logprobs(1, None)
        eng.decode(1, batch=2)
        with pytest.raises(RuntimeError):
            eng.read_logprobs(1, 1)
    finally:
        eng.close()


@pytest.mark.parametrize("n", [1, 4, 5, 64])
def test_written_once_logprob_plans(tiny, n):
    ids, recs, eng = _run(tiny, n, 1, check=False)
    try:
        c = eng.check_step(n)
        assert c["double_writes"] == 0, c
        assert eng.replay_route() == "aql"
    finally:
        eng.close()


def test_fp8_pages(tiny):
    ids, recs, eng = _run(tiny, 3, 3, kv_format="fp8")
    eng.close()


def test_batch_generate_logprobs(tiny):
    from tiny_llm_hip.engine import batch_generate_ids

    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, 1000, int(rng.integers(4, 30))).tolist() for _ in range(7)]

    def run(**kw):
        eng = _engine(tiny, 5)
        try:
            return sorted(batch_generate_ids(eng, prompts, 9, batch_size=4, prefill_step=16, **kw))
        finally:
            eng.close()

    plain = run()
    with_lp = run(logprobs=3)
    assert [(i, ids) for i, ids, _ in with_lp] == plain
    for _, ids, recs in with_lp:
        assert len(recs) == len(ids) and all(len(r.top) == 3 and r.logprob <= 0.0 for r in recs)
        assert all(r.logprob == r.top[0][1] for r in recs)  # greedy: the produced token is the first of the order


# -- scoring -----------------------------------------------------------------------------------------------------------------
def _teacher_forced(eng, tokens, slot=0):
    """log_softmax of the engine's decode logits with each next token forced: row i predicts tokens[i + 1]."""
    eng.begin(slot)
    try:
        eng.prefill(slot, tokens[:1])
        rows = [eng.logits(1).float().cpu()[0]]
        for t in tokens[1:]:
            eng.set_token(slot, t)
            eng.decode(1, batch=slot + 1)
            rows.append(eng.logits(slot + 1).float().cpu()[slot])
    finally:
        eng.release(slot)
    return torch.stack(rows).double()


@pytest.mark.parametrize("which", ["tiny", "q4b"])
def test_score_matches_teacher_forced_decode(request, which):
    model = request.getfixturevalue(which)
    eng = _engine(model, 2)
    try:
        rng = np.random.default_rng(4)
        tokens = rng.integers(0, 1000, 40).tolist()
        logits = _teacher_forced(eng, tokens)
        want = torch.log_softmax(logits, -1)
        # a logprob's error is at most its logit's error plus the log-normaliser's: twice the logit tolerance, 4 bf16 ulps of the
        # largest logit magnitude (the GEMM and the GEMV round the same products differently)
        tol = 2 * 4 * 2.0 ** -8 * float(logits.abs().max())
        got = eng.score(tokens)
        assert len(got) == len(tokens) - 1
        ref = [float(want[i, tokens[i + 1]]) for i in range(len(tokens) - 1)]
        assert max(abs(g - r) for g, r in zip(got, ref)) <= tol
        chunked = eng.score(tokens, chunk=7)
        assert max(abs(a - b) for a, b in zip(got, chunked)) <= tol
        # out_argmax against verify (n <= 8)
        import ctypes

        from tiny_llm_hip.engine import _ext, _lib

        eng.begin(0)
        eng.prefill(0, tokens[:10], want_logits=False)
        arr = (ctypes.c_int32 * 6)(*tokens[10:16])
        lp = (ctypes.c_float * 6)()
        am = (ctypes.c_int32 * 6)()
        _ext.check(_lib.tl_engine_score(eng._h, 0, arr, 6, -1, lp, am))
        assert math.isnan(lp[5])
        eng.rewind(0, 6)
        assert list(am) == eng.verify(0, tokens[10:16])
        eng.release(0)
    finally:
        eng.close()


def test_score_fp8_and_long_prompt(q4b):
    eng = _engine(q4b, 2, kv_format="fp8")
    try:
        tokens = np.random.default_rng(2).integers(0, 1000, 40).tolist()
        assert all(math.isfinite(v) and v <= 0 for v in eng.score(tokens))
    finally:
        eng.close()


def test_score_4096_tokens_36_layers():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    model = synthetic_qwen3(QWEN4B_CFG, seed=5, sigma=0.02, device="cuda")
    eng = _engine(model, 1, max_prefill_rows=4096, num_pages=4096 // 16 + 8)
    try:
        tokens = np.random.default_rng(6).integers(0, 150000, 4096).tolist()
        got = eng.score(tokens)
        assert len(got) == 4095 and all(math.isfinite(v) and v <= 0 for v in got)
    finally:
        eng.close()
        del model
        torch.cuda.empty_cache()
