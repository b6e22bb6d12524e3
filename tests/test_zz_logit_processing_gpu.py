"""GPU tier: per-slot repetition / presence / frequency penalties and logit bias on the device (tl_engine_set_penalties,
tl_engine_set_logit_bias, tl_process_logits, csrc/logit_process.h) against the numpy restatement of their definition
(tests/logit_processing_oracle.py), with the choice on the processed row checked by tests/sampling_oracle.py and the records by
tests/logprob_oracle.py.  The processed row is checked bit for bit; a produced id must equal the oracle's unless the sampling oracle
flags the draw ambiguous, and at most 10 % of the draws a test checks may be flagged.

The tests keep every slot's history on the host by the header's rule: prompt tokens are marked when the slot consumes them, a produced
token is counted at the start of the decode step that feeds it back."""

import ctypes
import math
import os

import numpy as np
import pytest
import torch

import logit_processing_oracle as P
import logprob_oracle as L
import sampling_oracle as S
from helpers import QWEN4B_CFG, TINY_CFG

pytestmark = pytest.mark.gpu

NEUTRAL = (1.0, 0.0, 0.0)


# -- 1. the kernel, bit for bit ---------------------------------------------------------------------------------------------------
def _kernel_rows(V, rng):
    """(logits, prompt, count, (r, p, f), bias) per row: every stage alone and together, the edges of the header."""
    def logits(special=False):
        l = rng.standard_normal(V).astype(np.float32) * 2.0
        if special:
            at = rng.choice(V, 12, replace=False)
            l[at[:4]], l[at[4:8]], l[at[8:]] = np.nan, np.inf, -np.inf
        return P.bf16_round(l)

    def history(kind):
        prompt, count = np.zeros(V, bool), np.zeros(V, np.int64)
        if kind == "empty":
            return prompt, count
        at = rng.choice(V, min(V // 2, 600), replace=False)
        prompt[at[:200]] = True                      # prompt-only tokens
        count[at[200:300]] = 1
        count[at[300:400]] = rng.integers(2, 500, 100)
        count[at[400:420]] = 32767                   # saturated
        prompt[at[380:440]] = True                   # both
        return prompt, count

    def bias(n, banned=0):
        ids = rng.choice(V, n, replace=False)
        d = {int(i): float(np.float32(rng.standard_normal() * 3.0)) for i in ids}
        for i in ids[:banned]:
            d[int(i)] = -math.inf
        return d

    third = float(np.float32(1.0) / np.float32(3.0))
    fma_l = logits()
    fma_l[:64] = 1.0
    fma_p, fma_c = history("empty")
    fma_c[:64] = 3  # 1 - (float32(1/3) * 3) is exactly +0.0 in two operations; a fused multiply-add leaves -2.98e-8
    rows = [
        (logits(), *history("mixed"), NEUTRAL, None),                        # neutral: output == input
        (logits(True), *history("mixed"), NEUTRAL, None),
        (logits(), *history("mixed"), (1.3, 0.0, 0.0), None),                # each penalty alone
        (logits(), *history("mixed"), (1.0, 0.7, 0.0), None),
        (logits(), *history("mixed"), (1.0, 0.0, 0.3), None),
        (fma_l, fma_p, fma_c, (1.0, 0.0, third), None),
        (logits(True), *history("mixed"), (1.25, 0.5, 0.125), bias(16, 3)),  # all together, NaN / +-inf logits
        (logits(), *history("mixed"), (0.8, 0.0, 0.0), None),                # r < 1
        (logits(True), *history("mixed"), (0.9, -0.6, -0.05), bias(1)),      # negative penalties, one entry
        (logits(), *history("empty"), NEUTRAL, bias(1, 1)),                  # bias only: one banned token
        (logits(True), *history("mixed"), (1.1, 0.2, 0.01), bias(1024, 40)), # a full list
        (logits(), *history("empty"), (1.5, 1.0, 1.0), None),                # processing with an empty history: v + 0.0 only
    ]
    return rows


@pytest.mark.parametrize("V", [1024, 151936, 151941])
def test_kernel_bit_for_bit(V):
    import tiny_llm_ext_hip as ext

    rows = _kernel_rows(V, np.random.default_rng(V))
    lg = np.stack([r[0] for r in rows])
    logits = torch.from_numpy(lg).bfloat16().cuda()
    hist = np.stack([P.pack_history(r[1], r[2]) for r in rows])
    out = ext.process_logits(logits, torch.from_numpy(hist.view(np.int16)).cuda(), [r[3][0] for r in rows], [r[3][1] for r in rows],
                             [r[3][2] for r in rows], [r[4] for r in rows])
    got = out.view(torch.int16).cpu().numpy().view(np.uint16)
    raw = logits.view(torch.int16).cpu().numpy().view(np.uint16)
    for i, (l, prompt, count, (r, p, f), bias) in enumerate(rows):
        want = P.process(P.from_bits(raw[i]), prompt, count, r, p, f, bias)
        if not P.processes(r, p, f, bias):
            assert np.array_equal(got[i], raw[i]), f"row {i}: a row that does not process is copied bit for bit"
            continue
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(P.from_bits(got[i])), nan), f"row {i}: NaN positions"
        bad = np.flatnonzero((got[i] != P.bits(want)) & ~nan)
        assert bad.size == 0, (f"row {i} (r, p, f) = {(r, p, f)}: {bad.size} elements differ, first at {bad[:3]}: got "
                               f"{P.from_bits(got[i][bad[:3]])}, want {want[bad[:3]]}, logit {P.from_bits(raw[i][bad[:3]])}, "
                               f"count {count[bad[:3]]}, prompt {prompt[bad[:3]]}")
    # the case that tells two operations from a fused multiply-add: exactly +0.0
    assert (got[5][:64] == 0).all()


# -- the engine against the oracle, step by step -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(TINY_CFG, seed=3, sigma=0.05, device="cuda")


@pytest.fixture(scope="module")
def q4b():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(dict(QWEN4B_CFG, num_hidden_layers=2), seed=11, sigma=0.02, device="cuda")


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


def _cfg(pen=NEUTRAL, bias=None, smp=(0.0, 0, 1.0, 0)):
    return {"pen": pen, "bias": dict(bias or {}), "smp": smp}


def _mixed(i, V, small=True):
    """Slot i's settings: neutral greedy, neutral sampled, processing greedy, processing sampled, bias only.  The sampled slots keep the
    sampling oracle's ambiguity flag rare: top-k <= 50 (or top-k 20 + top-p 0.8) at the full vocabulary, also no truncation at 1,024."""
    rng = np.random.default_rng(1000 + i)
    bias = {int(t): float(np.float32(v)) for t, v in zip(rng.choice(V, 16, replace=False), rng.standard_normal(16) * 2.0)}
    bias[int(rng.integers(0, V))] = -math.inf
    smp = [(0.8, 50, 1.0), (0.8, 20, 0.8), (0.8, 0, 1.0) if small else (0.7, 40, 1.0)][(i // 5) % 3]
    kind = i % 5
    if kind == 0:
        return _cfg()
    if kind == 1:
        return _cfg(smp=(*smp, 100 + i))
    if kind == 2:
        return _cfg(pen=(1.3, 0.5, 0.25))
    if kind == 3:
        return _cfg(pen=(1.2, 0.4, 0.1), bias=bias, smp=(*smp, 100 + i))
    return _cfg(bias=bias)


class Sim:
    """An engine and, beside it, what the header says it holds: per slot the settings, the history and the pending token."""

    def __init__(self, model, n, route=None, **kw):
        self.eng = _engine(model, n, route, **kw)
        self.V = self.eng.vocab_size
        self.cfg, self.hist, self.pending, self.out = {}, {}, {}, {}
        self.draws = self.ambiguous = 0

    def close(self):
        self.eng.close()

    def processes(self, slot):
        c = self.cfg[slot]
        return P.processes(*c["pen"], c["bias"])

    def configure(self, slot, cfg):
        """the engine calls of a setting, in the Python layer's order; the history starts with the call that makes the slot process
        (a change that passes through a neutral state between the two calls would forget it on the device: no test makes one)"""
        was = slot in self.cfg and self.processes(slot)
        self.cfg[slot] = cfg
        if cfg["pen"] != NEUTRAL or was:
            self.eng.set_penalties(slot, *cfg["pen"])
        if cfg["bias"] or was:
            self.eng.set_logit_bias(slot, cfg["bias"])
        T, k, p, seed = cfg["smp"]
        if T > 0:
            self.eng.set_sampling(slot, T, k or None, p if p < 1 else None, seed)
        if not was or not self.processes(slot):
            self.hist[slot] = P.History(self.V)

    def expect(self, slot, raw_row, position):
        c = self.cfg[slot]
        row = P.process(raw_row, self.hist[slot].prompt, self.hist[slot].count, *c["pen"], c["bias"]) if self.processes(slot) else raw_row
        return S.sample(row, *c["smp"][:3], c["smp"][3], position), row

    def check(self, slot, got, raw_row, position):
        (want, amb), row = self.expect(slot, raw_row, position)
        self.draws += 1
        self.ambiguous += bool(amb)
        assert got == want or amb, (slot, got, want, self.cfg[slot])
        for t, v in self.cfg[slot]["bias"].items():
            assert not (v == -math.inf and got == t), f"slot {slot} produced the banned id {t}"
        return row

    def consumed(self, slot, tokens):
        if self.processes(slot):
            self.hist[slot].consume_prompt(tokens)

    def start(self, slot, cfg, prompt, chunk=None):
        self.eng.begin(slot)
        self.configure(slot, cfg)
        self.eng.prefill(slot, prompt, chunk=chunk)
        self.consumed(slot, prompt)
        self.first_token(slot)

    def first_token(self, slot, row=0, rows=1):
        got = self.eng.read_tokens(slot, 1)[0]
        raw = self.eng.logits(rows).float().cpu().numpy()[row]
        self.check(slot, got, raw, self.eng.context_len(slot))
        self.pending[slot] = got
        self.out[slot] = [got]

    def step(self, n, use_graph=True, check=True):
        live = [i for i in range(n) if i in self.cfg and self.eng.context_len(i) >= 0]
        ctx = {i: self.eng.context_len(i) for i in live}
        for i in live:  # the step's input token is counted before the step's row is processed
            if self.processes(i):
                self.hist[i].feed(self.pending[i])
        self.eng.decode(1, batch=n, use_graph=use_graph)
        got = self.eng.read_pending(n)
        raw = self.eng.logits(n).float().cpu().numpy() if check else None
        for i in live:
            if check:
                self.check(i, got[i], raw[i], ctx[i] + 1)
            self.pending[i] = got[i]
            self.out[i].append(got[i])
        return raw

    def assert_few_ambiguous(self):
        assert self.draws > 0 and self.ambiguous <= 0.1 * self.draws, f"{self.ambiguous} of {self.draws} draws flagged ambiguous"


def _mixed_run(model, n, steps, small=True, route=None, use_graph=True, check=True, **kw):
    sim = Sim(model, n, route, **kw)
    try:
        rng = np.random.default_rng(n)
        for i in range(n):
            sim.start(i, _mixed(i, sim.V, small), rng.integers(0, 1000, 5 + i % 11).tolist())
        for _ in range(steps):
            sim.step(n, use_graph=use_graph, check=check)
        return sim
    except Exception:
        sim.close()
        raise


@pytest.mark.parametrize("n", [1, 3, 4, 5, 17, 64])
def test_engine_every_step_matches_oracle(tiny, n):
    if n == 1:  # one slot: the processing sampled kind, not the neutral one
        sim = Sim(tiny, 1)
        try:
            sim.start(0, _mixed(3, sim.V), list(range(40, 49)))
            for _ in range(10):
                sim.step(1)
        except Exception:
            sim.close()
            raise
    else:
        sim = _mixed_run(tiny, n, 8)
    try:
        assert sim.eng.replay_route() == "aql"
        sim.assert_few_ambiguous()
    finally:
        sim.close()


def test_engine_qwen4b_shapes(q4b):
    for n in (1, 5):
        sim = Sim(q4b, n)
        try:
            rng = np.random.default_rng(40 + n)
            for i in range(n):
                sim.start(i, _mixed(i + (3 if n == 1 else 0), sim.V, small=False), rng.integers(0, 1000, 6 + i).tolist())
            for _ in range(8):
                sim.step(n)
            sim.assert_few_ambiguous()
        finally:
            sim.close()


# -- 3. it discriminates --------------------------------------------------------------------------------------------------------
def test_discriminates(tiny):
    prompt = list(range(100, 112))
    steps = 10

    def run(setup):
        eng = _engine(tiny, 2)
        try:
            eng.begin(0)
            setup(eng)
            eng.prefill(0, prompt)
            eng.decode(steps, batch=1)
            return eng.read_tokens(0, steps + 1), eng.logits(1).float().cpu(), eng.stats()["graph_captures"]
        finally:
            eng.close()

    plain, plain_logits, plain_captures = run(lambda eng: None)
    banned, _, _ = run(lambda eng: eng.set_logit_bias(0, {t: -math.inf for t in set(plain)}))
    assert not set(banned) & set(plain) and banned[0] != plain[0]
    target = (plain[0] + 7) % 1024
    forced, _, _ = run(lambda eng: eng.set_logit_bias(0, {target: 100.0}))
    assert forced == [target] * (steps + 1)

    def neutral(eng):
        eng.set_penalties(0, 1.0, 0.0, 0.0)
        eng.set_logit_bias(0, {})
        eng.set_logit_bias(0, None)

    same, same_logits, same_captures = run(neutral)
    assert same == plain and torch.equal(same_logits, plain_logits) and same_captures == plain_captures
    # ... also after the engine has processed before: a slot made neutral again is back on the old plan
    def on_then_off(eng):
        eng.set_penalties(0, 1.5, 1.0, 1.0)
        eng.set_penalties(0, 1.0, 0.0, 0.0)

    again, again_logits, again_captures = run(on_then_off)
    assert again == plain and torch.equal(again_logits, plain_logits) and again_captures == plain_captures


# -- 4. routes ----------------------------------------------------------------------------------------------------------------------
def test_routes_agree(tiny):
    a = _mixed_run(tiny, 5, 8, check=False)
    b = _mixed_run(tiny, 5, 8, route="hipgraph", check=False)
    c = _mixed_run(tiny, 5, 8, use_graph=False, check=False)
    try:
        assert a.eng.replay_route() == "aql" and b.eng.replay_route().startswith("hipgraph")
        # every captured step of the processing plan was replayed as AQL packets (the first step of an engine runs eagerly; a plan with a
        # kernel outside the route's code objects would fall back to hipGraphLaunch: replays without AQL steps)
        sa, sb = a.eng.stats(), b.eng.stats()
        assert sa["graph_replays"] == 7 and sa["aql_steps"] == sa["graph_replays"], sa
        assert sb["graph_replays"] == 7 and sb["aql_steps"] == 0, sb
        assert a.out == b.out == c.out
    finally:
        for s in (a, b, c):
            s.close()


@pytest.mark.parametrize("n", [1, 4, 5, 64])
def test_written_once_processing_plans(tiny, n):
    sim = Sim(tiny, n)
    try:
        for i in range(n):
            sim.start(i, _mixed(i + 2, sim.V), list(range(3 + i % 7, 12 + i % 7)))  # slot 0 processes at every n
        sim.step(n)
        c = sim.eng.check_step(n)
        assert c["double_writes"] == 0, c
        assert np.isfinite(sim.eng.logits(n).float().cpu().numpy()).all()
    finally:
        sim.close()


def test_step_splitting(tiny):
    def run(calls):
        sim = Sim(tiny, 3)
        try:
            for i in range(3):
                sim.start(i, _mixed(i + 2, sim.V), list(range(20 + i, 30 + 2 * i)))
            for c in calls:
                sim.eng.decode(c, batch=3)
            return [sim.eng.read_tokens(i, 33) for i in range(3)]
        finally:
            sim.close()

    assert run([32]) == run([1] * 32)


# -- 5. prefill paths ---------------------------------------------------------------------------------------------------------------
def test_prefill_paths(tiny):
    import tiny_llm_ext_hip as ext

    sim = Sim(tiny, 4)
    try:
        prompt = [int(t) for t in np.random.default_rng(9).integers(0, 1000, 33)]
        cfg = _cfg(pen=(1.4, 0.3, 0.2), bias={5: 1.5, 6: -math.inf})
        sim.start(0, cfg, prompt, chunk=8)  # chunked: every chunk's tokens are in the history
        # packed, two slots, one of them in two passes
        for slot in (1, 2):
            sim.eng.begin(slot)
            sim.configure(slot, _mixed(3, sim.V) if slot == 1 else cfg)
        sim.eng.prefill_packed([(1, prompt[:20], True), (2, prompt[:10], False)])
        sim.consumed(1, prompt[:20]), sim.consumed(2, prompt[:10])
        sim.first_token(1)
        sim.eng.prefill_packed([(2, prompt[10:], True)])
        sim.consumed(2, prompt[10:])
        sim.first_token(2)
        # part of the prompt consumed through score
        sim.eng.begin(3)
        sim.configure(3, cfg)
        arr = (ctypes.c_int32 * 12)(*prompt[:12])
        lp = (ctypes.c_float * 12)()
        ext.check(ext.lib().tl_engine_score(sim.eng._h, 3, arr, 12, prompt[12], lp, None))
        sim.consumed(3, prompt[:12])
        sim.eng.prefill(3, prompt[12:])
        sim.consumed(3, prompt[12:])
        sim.first_token(3)
        for _ in range(3):
            sim.step(4)
        sim.assert_few_ambiguous()
    finally:
        sim.close()


# -- 6. life cycle ------------------------------------------------------------------------------------------------------------------
def test_life_cycle(tiny):
    sim = Sim(tiny, 4)
    eng = sim.eng
    try:
        cfg = _cfg(pen=(1.5, 1.0, 0.5), bias={11: 2.0})
        sim.start(2, cfg, list(range(30, 40)))
        for _ in range(3):
            sim.step(3)
        # move mid-generation: parameters, list and history go with the sequence
        eng.move(2, 0)
        for d in (sim.cfg, sim.hist, sim.pending, sim.out):
            d[0] = d.pop(2)
        for _ in range(2):
            sim.step(1)
        # fork: the child starts from the parent's history and then keeps its own
        eng.fork(0, 1)
        sim.cfg[1], sim.hist[1], sim.pending[1], sim.out[1] = dict(sim.cfg[0]), sim.hist[0].copy(), sim.pending[0], list(sim.out[0])
        sim.configure(1, _cfg(pen=(1.5, 1.0, 0.5), bias={11: 2.0}, smp=(0.9, 30, 1.0, 77)))  # same processing: the history stays
        for _ in range(4):
            sim.step(2)
        assert sim.hist[0].count.sum() == sim.hist[1].count.sum() and sim.hist[0] is not sim.hist[1]
        # verify / rewind / set_token refuse a processing slot ...
        for call in (lambda: eng.verify(0, [1, 2]), lambda: eng.rewind(0, 1), lambda: eng.set_token(0, 5)):
            with pytest.raises(RuntimeError):
                call()
        # ... parameter errors leave the slot as it was ...
        lib = __import__("tiny_llm_ext_hip").lib()
        for bad in ((0.0, 0.0, 0.0), (float("nan"), 0.0, 0.0), (1.0, float("inf"), 0.0), (1.0, 0.0, float("nan"))):
            assert lib.tl_engine_set_penalties(eng._h, 0, *bad) != 0
        for ids, vals in (([3, 3], [1.0, 1.0]), ([1024], [1.0]), ([-1], [1.0]), ([3], [float("nan")]), ([3], [float("inf")])):
            assert lib.tl_engine_set_logit_bias(eng._h, 0, (ctypes.c_int32 * len(ids))(*ids), (ctypes.c_float * len(ids))(*vals), len(ids)) != 0
        assert lib.tl_engine_set_logit_bias(eng._h, 0, (ctypes.c_int32 * 1025)(*range(1025)), (ctypes.c_float * 1025)(), 1025) != 0
        with pytest.raises(ValueError):
            eng.set_logit_bias(0, {i: 0.0 for i in range(1025)})
        sim.step(2)
        # ... and they work again once the slot is neutral
        sim.configure(0, _cfg())
        eng.rewind(0, 1)
        eng.set_token(0, 5)
        assert len(eng.verify(0, [1, 2])) == 2
        # release + begin: the history is empty (a token penalised before is not any more)
        eng.release(1)
        del sim.cfg[1]
        sim.start(1, cfg, list(range(30, 40)))
        assert sim.hist[1].count.sum() == 0
        sim.step(2)
        # begin resets the parameters: a fresh slot is neutral
        eng.release(1)
        del sim.cfg[1]
        sim.start(1, _cfg(), list(range(30, 40)))
        sim.step(2)
        sim.assert_few_ambiguous()
    finally:
        sim.close()


# -- 7. with log-probabilities ------------------------------------------------------------------------------------------------------
def test_logprob_records_describe_the_raw_row(tiny):
    TOL = 2e-4  # tests/test_zz_logprobs_gpu.py: fp32 sum of the row's terms in a fixed order, with margin
    sim = Sim(tiny, 3)
    eng = sim.eng
    try:
        cfgs = [_cfg(pen=(1.3, 0.8, 0.4), bias={7: -math.inf}), _cfg(pen=(1.2, 0.5, 0.2), smp=(0.8, 50, 1.0, 9)), _cfg()]
        for i, c in enumerate(cfgs):
            eng.begin(i)
            sim.configure(i, c)
            eng.set_logprobs(i, 5)
            prompt = list(range(50 + i, 60 + i))
            eng.prefill(i, prompt)
            sim.consumed(i, prompt)
            sim.first_token(i)
            raw = eng.logits(1).float().cpu().numpy()[0]
            rec = eng.read_logprobs(i, 1)[0]
            assert abs(rec.logprob - L.logprob(raw, sim.pending[i])) <= TOL
            assert [t for t, _ in rec.top] == L.top(raw, 5)[0].tolist()
        for _ in range(6):
            raw = sim.step(3)
            recs = eng.read_pending_logprobs(3)
            for i in range(3):
                assert abs(recs[i].logprob - L.logprob(raw[i], sim.pending[i])) <= TOL, (i, recs[i], sim.pending[i])
                ids, lps = L.top(raw[i], 5)
                assert [t for t, _ in recs[i].top] == ids.tolist()
                assert all(abs(g - w) <= TOL for (_, g), w in zip(recs[i].top, lps))
        # the greedy processing slot chose from the processed row: not always the raw row's first maximum
        sim.assert_few_ambiguous()
    finally:
        sim.close()


# -- 8. FP8 pages and continuous batching -------------------------------------------------------------------------------------------
def test_fp8_pages(tiny):
    sim = _mixed_run(tiny, 5, 4, kv_format="fp8")
    try:
        sim.assert_few_ambiguous()
    finally:
        sim.close()


def test_batch_generate_penalties(tiny):
    from tiny_llm_hip.engine import batch_generate_ids

    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, 1000, int(rng.integers(4, 30))).tolist() for _ in range(7)]

    def run(sampling):
        eng = _engine(tiny, 5)
        try:
            return sorted(batch_generate_ids(eng, prompts, 9, batch_size=4, prefill_step=16, sampling=sampling))
        finally:
            eng.close()

    plain = run(None)
    banned = sorted({t for _, ids in plain for t in ids})[:1024]
    s = {"temperature": 0.9, "top_k": 40, "repetition_penalty": 1.3, "presence_penalty": 0.5, "frequency_penalty": 0.2,
         "logit_bias": {t: -math.inf for t in banned}}
    a = run(s)
    assert a == run(s)
    assert not {t for _, ids in a for t in ids} & set(banned)
    assert plain == run([{"repetition_penalty": 1.0, "presence_penalty": 0.0, "frequency_penalty": 0.0, "logit_bias": {}}] * 7)
    g = run({"repetition_penalty": 1.5, "presence_penalty": 1.0})
    assert g == run({"repetition_penalty": 1.5, "presence_penalty": 1.0})
