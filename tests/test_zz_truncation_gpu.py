"""GPU tier: min-p, typical-p and Mirostat v2 on the device (tl_truncate_rows, tl_mirostat_update_rows, tl_engine_set_truncation,
tl_engine_set_mirostat; csrc/truncate.h) against the numpy restatement of their definition (tests/truncation_oracle.py).  Every token the
oracle decides must come out bit for bit -- kept bits unchanged, the others -inf; the tokens it calls undecided (fp32 rounding on the
device may fall on either side) may go either way."""

import functools
import math
import os

import numpy as np
import pytest
import torch

import logprob_oracle as L
import truncation_oracle as R
from helpers import TINY_CFG

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _dev(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).cuda()


def _assert_row(got_bits, in_bits, masks, what):
    want, decided = R.filtered_bits(in_bits, masks)
    bad = np.flatnonzero(decided & (got_bits != want))
    assert bad.size == 0, (what, bad[:8].tolist(), got_bits[bad[:8]].tolist(), want[bad[:8]].tolist())
    und = ~decided
    ok = (got_bits[und] == in_bits[und]) | (got_bits[und] == R.NEG_INF_BITS)
    assert ok.all(), (what, "an undecided token is neither kept nor -inf")


@functools.lru_cache(maxsize=None)
def _rows(V):
    return R.make_rows(V)


@pytest.mark.parametrize("V", R.VOCABS)
def test_truncate_rows_match_oracle(V):
    import tiny_llm_ext_hip as ext

    bits = _rows(V)
    vals = R.bf16_values(bits)
    n = bits.shape[0]
    cases = [(i, c) for c in R.COMBOS for i in range(n)]
    params = [R.row_params(i, c) for i, c in cases]
    logits = _dev(np.stack([bits[i] for i, _ in cases]))
    out, logsum = ext.truncate_rows(logits, *[[p[k] for p in params] for k in range(4)])
    got = _bits(out)
    logsum = logsum.cpu().numpy()
    for r, ((i, c), p) in enumerate(zip(cases, params)):
        masks = R.kept(vals[i], *p)
        print(f"V={V} row {i} {c} {p}: kept {int(masks[0].sum())} undecided {int(masks[2].sum())}")
        _assert_row(got[r], bits[i], masks, (V, i, c, p))
        assert (got[r] != R.NEG_INF_BITS).any()
        if c == "mirostat":  # ln sum_kept exp(x / T) of the device's own kept set
            f = R.bf16_values(got[r]).astype(np.float64)
            a = f[f > -np.inf] / p[0]
            want = a.max() + math.log(np.exp(a - a.max()).sum())
            assert abs(logsum[r] - want) <= 1e-4, (logsum[r], want)
        else:
            assert math.isnan(logsum[r])
    # every parameter off, or temperature 0: copied bit for bit
    off, _ = ext.truncate_rows(logits[:4], [1.0, 0.0, 0.0, 0.7], [0.0, 0.3, 0.0, 0.0], [1.0, 0.5, 1.0, 0.0], [NAN, NAN, 5.0, NAN])
    assert np.array_equal(_bits(off), _bits(logits[:4]))


def test_truncate_edge_rows():
    import tiny_llm_ext_hip as ext

    V = 3001
    rng = np.random.default_rng(7)
    base = R.bf16_values(R.bf16_bits((2.0 * rng.standard_normal(V)).astype(np.float32)))
    g = int(np.argmax(base))
    rows = {
        "nan": np.full(V, np.nan, np.float32),
        "-inf": np.full(V, -np.inf, np.float32),
        "one": np.where(np.arange(V) == 1234, np.float32(1.5), np.float32(-np.inf)).astype(np.float32),
        "+inf": np.where(np.arange(V) == 77, np.float32(np.inf), base).astype(np.float32),
        "equal": np.full(V, 0.75, np.float32),
        "base": base,
        "ban": np.where(np.arange(V) == (g + 1) % V, np.float32(-np.inf), base).astype(np.float32),
        "some-nan": np.where(np.arange(V) % 97 == 5, np.float32(np.nan), base).astype(np.float32),
    }
    names = list(rows)
    bits = np.stack([R.bf16_bits(rows[k]) for k in names])
    vals = R.bf16_values(bits)
    settings = [(0.8, 0.1, 1.0, NAN), (1.0, 0.0, 0.5, NAN), (0.8, 0.05, 0.9, NAN), (1.0, 0.0, 1.0, 4.0), (1.0, 0.0, 1.0, -3.0), (1.0, 1.0, 1.0, NAN)]
    for p in settings:
        out, _ = ext.truncate_rows(_dev(bits), *p)
        torch.cuda.synchronize()
        got = _bits(out)
        for r, k in enumerate(names):
            _assert_row(got[r], bits[r], R.kept(vals[r], *p), (k, p))
    # a row of equal logits: everything ties, so everything stays; min_p = 1: only the maxima stay; mu below every surprise: the first maximum
    eq = names.index("equal")
    for p in settings[:3] + settings[5:]:
        out, _ = ext.truncate_rows(_dev(bits[eq:eq + 1]), *p)
        assert np.array_equal(_bits(out)[0], bits[eq])
    b = names.index("base")
    out, _ = ext.truncate_rows(_dev(bits[b:b + 1]), 1.0, 1.0, 1.0, NAN)
    assert np.flatnonzero(_bits(out)[0] != R.NEG_INF_BITS).tolist() == np.flatnonzero(vals[b] == vals[b].max()).tolist()
    out, _ = ext.truncate_rows(_dev(bits[eq:eq + 1]), 1.0, 0.0, 1.0, -3.0)
    assert np.flatnonzero(_bits(out)[0] != R.NEG_INF_BITS).tolist() == [0]


@pytest.mark.parametrize("V", [1024, 151941])
def test_mirostat_update_rows(V):
    import tiny_llm_ext_hip as ext

    bits = _rows(V)
    n = bits.shape[0]
    T = [R.TEMPERATURES[i % 3] for i in range(n)]
    tau = [3.0, 5.0, 8.0, 0.0][:4] * (n // 4)
    eta = [0.1, 0.5, 1.0, 0.3][:4] * (n // 4)
    mu = [2.0 * t if t > 0 else 7.0 for t in tau]
    logits = _dev(bits)
    out, logsum = ext.truncate_rows(logits, T, 0.0, 1.0, mu)
    ids = ext.sample_logits(out, T, 0, 1.0, list(range(n)), 3)
    new = ext.mirostat_update_rows(out, ids, T, logsum, tau, eta, mu).cpu().numpy()
    f = R.bf16_values(_bits(out))
    ids = ids.cpu().tolist()
    for i in range(n):
        assert f[i, ids[i]] > -np.inf
        want = R.mirostat_update(f[i], ids[i], T[i], tau[i], eta[i], mu[i]) if tau[i] > 0 else mu[i]
        print(f"V={V} row {i}: mu {mu[i]} -> {new[i]} (oracle {want})")
        assert abs(new[i] - want) <= 1e-4, (i, new[i], want)


# -- the engine against the oracle, step by step -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(TINY_CFG, seed=3, sigma=0.05, device="cuda")


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


def _cfg(T=0.0, seed=0, top_k=None, top_p=None, min_p=0.0, typ=1.0, tau=0.0, eta=0.1, pen=None, bias=None, grammar=None, lp=None):
    return dict(T=T, seed=seed, top_k=top_k, top_p=top_p, min_p=min_p, typ=typ, tau=tau, eta=eta, pen=pen, bias=bias, grammar=grammar, lp=lp)


KINDS = ("greedy", "min_p", "typical", "mirostat", "both", "greedy+min_p")


def _kind(kind, i):
    return {"greedy": _cfg(), "min_p": _cfg(0.8, 100 + i, top_k=40, min_p=0.05), "typical": _cfg(1.0, 100 + i, typ=0.9),
            "mirostat": _cfg(0.9, 100 + i, tau=5.0, eta=0.3), "both": _cfg(0.7, 100 + i, top_p=0.9, min_p=0.1, typ=0.5),
            "greedy+min_p": _cfg(min_p=0.3, typ=0.5), "sampled": _cfg(0.8, 100 + i, top_k=40)}[kind]


class Run:
    """An engine and, beside it, what the header says a truncating slot holds: its parameters and Mirostat's mu."""

    def __init__(self, model, n, kinds=KINDS, route=None, eng=None, **kw):
        """kinds = None: no slot is started (the caller starts them); eng: an engine the caller made and closes"""
        self.eng = eng if eng is not None else _engine(model, n, route, **kw)
        self.n, self.cfg, self.mu, self.out = n, {}, {}, {}
        rng = np.random.default_rng(n)
        try:
            for i in range(n if kinds else 0):
                self.start(i, _kind(kinds[i % len(kinds)], i), rng.integers(0, 1000, 5 + i % 11).tolist())
        except Exception:
            self.eng.close()
            raise

    def close(self):
        self.eng.close()

    def configure(self, i, c):
        e = self.eng
        if c["pen"]:
            e.set_penalties(i, *c["pen"])
        if c["bias"]:
            e.set_logit_bias(i, c["bias"])
        if c["grammar"] is not None:
            e.set_grammar(i, c["grammar"])
        if c["T"] > 0:
            e.set_sampling(i, c["T"], c["top_k"], c["top_p"], c["seed"])
        if c["min_p"] > 0 or c["typ"] < 1:
            e.set_truncation(i, c["min_p"], c["typ"])
        if c["tau"] > 0:
            e.set_mirostat(i, c["tau"], c["eta"])
        if c["lp"] is not None:
            e.set_logprobs(i, c["lp"])
        self.cfg[i] = c
        self.mu[i] = 2 * c["tau"] if c["tau"] > 0 else NAN

    def processes(self, i):
        c = self.cfg[i]
        return bool(c["pen"] or c["bias"] or c["grammar"] is not None)

    def truncates(self, i):
        c = self.cfg[i]
        return c["T"] > 0 and (c["min_p"] > 0 or c["typ"] < 1 or c["tau"] > 0)

    def start(self, i, c, prompt):
        self.eng.begin(i)
        self.configure(i, c)
        self.eng.prefill(i, prompt)
        tok = self.eng.read_tokens(i, 1)[0]
        self.out[i] = [tok]
        if self.truncates(i):
            self.check_row(i, 0, tok, 1)
        if c["lp"] is not None:
            self.check_record(i, self.eng.logits(1).float().cpu().numpy()[0], tok, self.eng.read_logprobs(i, 1)[0])

    def check_row(self, i, row, tok, rows):
        """the filtered row `row` of the last launch against the oracle on the row the choice would have been made from; mu follows"""
        c = self.cfg[i]
        src = self.eng.processed_logits(rows) if self.processes(i) else self.eng.logits(rows)
        in_bits, got = _bits(src)[row], _bits(self.eng.filtered_logits(rows))[row]
        masks = R.kept(R.bf16_values(in_bits), c["T"], c["min_p"], c["typ"], self.mu[i]) if self.truncates(i) else R.kept(R.bf16_values(in_bits), 0.0)
        _assert_row(got, in_bits, masks, (i, c))
        assert got[tok] != R.NEG_INF_BITS and got[tok] == in_bits[tok], (i, tok, "the produced token is not a kept token")
        if c["tau"] > 0 and c["T"] > 0:
            want = R.mirostat_update(R.bf16_values(got), tok, c["T"], c["tau"], c["eta"], self.mu[i])
            self.mu[i] = self.eng.mirostat_mu(i)
            assert abs(self.mu[i] - want) <= 1e-4, (i, self.mu[i], want)

    def check_record(self, i, raw, tok, rec):
        """the record of the produced token describes the RAW row, whatever row the token was chosen from (the comparison and
        tolerance of test_zz_logit_processing_gpu.test_logprob_records_describe_the_raw_row)"""
        TOL = 2e-4  # tests/test_zz_logprobs_gpu.py: fp32 sum of the row's terms in a fixed order, with margin
        assert abs(rec.logprob - L.logprob(raw, tok)) <= TOL, (i, rec, tok)
        ids, lps = L.top(raw, self.cfg[i]["lp"])
        assert [t for t, _ in rec.top] == ids.tolist(), (i, rec, ids)
        assert all(abs(g - w) <= TOL for (_, g), w in zip(rec.top, lps)), (i, rec, lps)

    def step(self, check=True, use_graph=True):
        self.eng.decode(1, batch=self.n, use_graph=use_graph)
        got = self.eng.read_pending(self.n)
        for i in sorted(self.cfg):
            self.out[i].append(got[i])
            if check:
                self.check_row(i, i, got[i], self.n)
        if check and any(c["lp"] is not None for c in self.cfg.values()):
            raw, recs = self.eng.logits(self.n).float().cpu().numpy(), self.eng.read_pending_logprobs(self.n)
            for i, c in self.cfg.items():
                if c["lp"] is not None:
                    self.check_record(i, raw[i], got[i], recs[i])


@pytest.mark.parametrize("n", [1, 4, 5, 64])
def test_engine_every_step_matches_oracle(tiny, n):
    kinds = ("mirostat",) if n == 1 else KINDS
    run = Run(tiny, n, kinds)
    try:
        for _ in range(4):
            run.step()
        assert run.eng.replay_route().startswith("hipgraph") and "Mirostat" in run.eng.replay_route()
        assert run.eng.stats()["aql_steps"] == 0
    finally:
        run.close()
    if n == 1:  # ... and a stateless slot, whose plan rides the AQL route
        run = Run(tiny, 1, ("both",))
        try:
            for _ in range(4):
                run.step()
            s = run.eng.stats()
            assert run.eng.replay_route() == "aql" and s["graph_replays"] == 3 and s["aql_steps"] == 3, s
        finally:
            run.close()


@pytest.mark.parametrize("n", [1, 5])
def test_step_splitting_and_routes(tiny, n):
    """decode(4) gives the tokens and mu of four decode(1) calls; the TL_AQL=0 engine and an eager engine give the same tokens."""
    kinds = ("mirostat",) if n == 1 else KINDS
    a, b, c, d = Run(tiny, n, kinds), Run(tiny, n, kinds), Run(tiny, n, kinds, route="hipgraph"), Run(tiny, n, ("min_p", "typical", "both"))
    e = Run(tiny, n, ("min_p", "typical", "both"), route="hipgraph")
    try:
        for _ in range(4):
            a.step(check=False)
            c.step(check=False)
            d.step(check=False)
            e.step(check=False)
        b.eng.decode(4, batch=n)
        toks = [b.out[i] + b.eng.read_tokens(i, 4) for i in range(n)]
        assert toks == [a.out[i] for i in range(n)] == [c.out[i] for i in range(n)]
        for i in range(n):
            ma, mb = a.eng.mirostat_mu(i), b.eng.mirostat_mu(i)
            assert ma == mb or (math.isnan(ma) and math.isnan(mb)), (i, ma, mb)
        assert d.eng.replay_route() == "aql" and d.eng.stats()["aql_steps"] == 3 and e.eng.stats()["aql_steps"] == 0
        assert d.out == e.out
    finally:
        for r in (a, b, c, d, e):
            r.close()


def test_first_token_after_prefill_and_packed_prefill_is_filtered(tiny):
    eng = _engine(tiny, 4)
    try:
        # min_p = 1: only the maxima stay, so a filtered draw is the greedy id whatever the seed
        eng.begin(0)
        eng.set_sampling(0, 1.5, seed=11)
        eng.set_truncation(0, 1.0)
        eng.prefill(0, list(range(20, 31)))
        raw = eng.logits(1).float().cpu().numpy()[0]
        f = R.bf16_values(_bits(eng.filtered_logits(1)))[0]
        assert eng.read_tokens(0, 1)[0] == int(np.argmax(raw)) and np.array_equal(np.flatnonzero(f > -np.inf), np.flatnonzero(raw == raw.max()))
        for i in (1, 2, 3):
            eng.begin(i)
            eng.set_sampling(i, 1.5, seed=20 + i)
        eng.set_truncation(1, 1.0)
        eng.set_mirostat(3, 4.0, 0.5)
        eng.prefill_packed([(1, list(range(40, 47)), True), (2, list(range(50, 59)), True), (3, list(range(60, 65)), True)])
        raw = eng.logits(3).float().cpu().numpy()
        fb = _bits(eng.filtered_logits(3))
        f = R.bf16_values(fb)
        toks = [eng.read_tokens(i, 1)[0] for i in (1, 2, 3)]
        assert toks[0] == int(np.argmax(raw[0])) and (f[0] > -np.inf).sum() == (raw[0] == raw[0].max()).sum()
        # (slot 2 does not truncate: no launch filters its row, the buffer's row is not its row)
        _assert_row(fb[2], _bits(eng.logits(3))[2], R.kept(raw[2], 1.5, mu=8.0), "packed mirostat")
        assert f[2, toks[2]] > -np.inf
        assert abs(eng.mirostat_mu(3) - R.mirostat_update(f[2], toks[2], 1.5, 4.0, 0.5, 8.0)) <= 1e-4
    finally:
        eng.close()


# the slot kinds of the whole-chain case, repeated over the batch.  "all" carries no min-p: the engine refuses min-p beside Mirostat
# (test_slot_lifecycle), so min-p rides on another row of the packed pass below.  "idle": a slot that holds no sequence during the steps
# -- begun and released without a prefill; a slot that stays begun is live, and every live slot of [0, batch) takes the step from token 0.
# Four rows hold every kind but the plain greedy one, five hold all.
CHAIN_KINDS = ("sampled", "pen+lp", "all", "idle", "greedy")
CHAIN_PEN, CHAIN_BIAS = (1.3, 0.5, 0.25), {t: -math.inf for t in range(48, 52)}


def _chain_kind(kind, i):
    return {"greedy": _cfg(), "sampled": _cfg(0.8, 100 + i, top_k=40), "pen+lp": _cfg(pen=CHAIN_PEN, bias=CHAIN_BIAS, lp=3),
            "all": _cfg(0.9, 100 + i, tau=5.0, eta=0.3, pen=CHAIN_PEN, bias=CHAIN_BIAS, lp=5),
            "min_p+pen+lp": _cfg(0.8, 100 + i, top_k=40, min_p=0.05, pen=CHAIN_PEN, bias=CHAIN_BIAS, lp=2)}[kind]


@pytest.mark.parametrize("n", [4, 5])
def test_every_launch_of_the_chain_in_one_batch(tiny, n):
    """Processing, truncation, the logprob step end and the Mirostat update in ONE step (4 rows: the GEMV step; 5: the batched-matmul
    step), beside greedy, sampled and idle rows: per step the filtered row against the oracle on the processed row, the produced token
    kept, mu, and the record of the produced token against the raw row; the idle slot's `produced` and context do not move.  Then one
    packed prefill of three prompts that all end in the pass, the processing + Mirostat + logprob slot third: its first token comes from
    row 2 of logits / processed rows / filtered rows / log-sums."""
    run = Run(tiny, n, None)
    eng = run.eng
    try:
        rng = np.random.default_rng(n)
        idle = []
        for i in range(n):
            kind, prompt = CHAIN_KINDS[i % len(CHAIN_KINDS)], rng.integers(0, 1000, 5 + i % 11).tolist()
            if kind == "idle":
                eng.begin(i)
                eng.release(i)
                idle.append(i)
            else:
                run.start(i, _chain_kind(kind, i), prompt)
        assert idle
        for _ in range(4):
            run.step()
            for i in idle:  # the device's pending-token word (the commit's first store), and the host's side of the slot
                assert eng.read_pending(n)[i] == 0 and eng.context_len(i) == -1
                with pytest.raises(RuntimeError, match="fewer ids"):  # produced == 0
                    eng.read_tokens(i, 1)
        assert all(len(run.out[i]) == 5 and eng.context_len(i) == 5 + i % 11 + 4 for i in run.cfg)
        assert "Mirostat" in eng.replay_route() and eng.stats()["graph_replays"] == 3
    finally:
        run.close()
    # the packed pass: rows 0, 1, 2 of the row buffers belong to slots 2, 0, 1
    run = Run(tiny, 4, None)
    eng = run.eng
    try:
        order = [(2, "min_p+pen+lp"), (0, "greedy"), (1, "all")]
        for slot, kind in order:
            eng.begin(slot)
            run.configure(slot, _chain_kind(kind, slot))
        eng.prefill_packed([(slot, list(range(40 + 10 * slot, 47 + 11 * slot)), True) for slot, _ in order])
        raw, recs = eng.logits(3).float().cpu().numpy(), {slot: eng.read_logprobs(slot, 1)[0] for slot in (2, 1)}
        for row, (slot, kind) in enumerate(order):
            tok = eng.read_tokens(slot, 1)[0]
            if kind == "greedy":
                assert tok == int(np.argmax(raw[row]))
                continue
            run.check_row(slot, row, tok, 3)
            run.check_record(slot, raw[row], tok, recs[slot])
    finally:
        run.close()


def test_slot_lifecycle(tiny):
    eng = _engine(tiny, 4)
    try:
        eng.begin(0)
        eng.set_sampling(0, 0.9, seed=5)
        eng.set_mirostat(0, 5.0, 0.3)
        assert eng.mirostat_mu(0) == 10.0
        eng.prefill(0, list(range(10, 22)))
        eng.decode(2, batch=1)
        mu0 = eng.mirostat_mu(0)
        assert mu0 != 10.0 and math.isfinite(mu0)
        # rewind and set_token refuse a Mirostat slot, nothing changed
        for call in (lambda: eng.rewind(0, 1), lambda: eng.set_token(0, 3)):
            with pytest.raises(RuntimeError, match="Mirostat"):
                call()
        assert eng.mirostat_mu(0) == mu0
        # exclusivity: every call that would combine Mirostat with another truncation is refused and leaves every parameter as it was
        for call in (lambda: eng.set_truncation(0, 0.05), lambda: eng.set_truncation(0, 0.0, 0.9), lambda: eng.set_sampling(0, 0.9, 40, None, 5),
                     lambda: eng.set_sampling(0, 0.9, None, 0.9, 5)):
            with pytest.raises(RuntimeError, match="excludes"):
                call()
        assert eng.mirostat_mu(0) == mu0
        # fork copies parameters and mu, move carries them
        eng.fork(0, 1)
        assert eng.mirostat_mu(1) == mu0
        eng.move(0, 2)
        assert eng.mirostat_mu(2) == mu0
        with pytest.raises(RuntimeError):
            eng.mirostat_mu(0)
        with pytest.raises(RuntimeError, match="excludes"):  # the parameters came along: slot 2 still refuses top-k
            eng.set_sampling(2, 0.9, 40, None, 5)
        eng.decode(1, batch=3)  # both go on from the mu they were given
        for i in (1, 2):
            assert eng.mirostat_mu(i) != mu0 and math.isfinite(eng.mirostat_mu(i))
        # begin / release reset
        eng.release(1)
        eng.begin(1)
        assert math.isnan(eng.mirostat_mu(1))
        eng.set_sampling(1, 0.9, 40, 0.9, 5)  # accepted: no Mirostat left
        eng.begin(0)
        assert math.isnan(eng.mirostat_mu(0))
        # a min-p slot: set_mirostat is refused (and leaves it a min-p slot), rewind and set_token are accepted
        eng.set_sampling(0, 1.5, seed=9)
        eng.set_truncation(0, 1.0, 0.9)
        with pytest.raises(RuntimeError, match="excludes"):
            eng.set_mirostat(0, 5.0)
        assert math.isnan(eng.mirostat_mu(0))
        eng.prefill(0, list(range(30, 40)))
        eng.decode(2, batch=1)
        eng.rewind(0, 1)
        eng.set_token(0, 7)
        eng.decode(1, batch=1)
        raw = eng.logits(1).float().cpu().numpy()[0]
        assert eng.read_pending(1)[0] == int(np.argmax(raw))  # still min_p = 1
        # move carries min-p / typical-p too
        eng.release(1)
        eng.move(0, 3)
        eng.decode(1, batch=4)
        raw = eng.logits(4).float().cpu().numpy()[3]
        f = R.bf16_values(_bits(eng.filtered_logits(4)))[3]
        assert eng.read_pending(4)[3] == int(np.argmax(raw)) and (f > -np.inf).sum() == (raw == raw.max()).sum()
        # bad input: TL_ERR_INVALID
        for call in (lambda: eng.set_truncation(3, 1.5), lambda: eng.set_truncation(3, -0.1), lambda: eng.set_mirostat(3, -1.0)):
            with pytest.raises((RuntimeError, ValueError)):
                call()
    finally:
        eng.close()


def test_min_p_sees_the_processed_row_and_the_text_stays_in_the_language(tiny):
    import re

    import test_zz_grammar_gpu as GG

    dev = GG.Device(1024)
    eng = _engine(tiny, 2)
    try:
        run = Run(tiny, 1, None, eng=eng)
        ban = {int(t): -math.inf for t in range(48, 52)}  # the digits 0-3
        run.start(0, _cfg(0.9, 7, top_k=40, min_p=0.2, pen=(1.3, 0.5, 0.25), bias=ban, grammar=dev.grammar(GG.NUMBER)), list(range(100, 112)))
        for _ in range(32):
            run.step()
        text, ended = GG.before_eos(run.out[0], 1024)
        assert ended and re.fullmatch(GG.NUMBER, GG.text_of(text, 1024)), GG.text_of(text, 1024)
        assert not set(run.out[0]) & set(ban)
    finally:
        eng.close()
        dev.close()


@pytest.mark.parametrize("n", [1, 5])
def test_engines_that_never_truncate_are_unchanged(tiny, n):
    """Greedy and sampling-only engines: the tokens of an engine that never calls the new API, bit for bit -- also when the new calls are
    made with neutral values, or on greedy slots (whose rows are never filtered)."""
    kinds = ("greedy", "sampled")
    plain = Run(tiny, n, kinds)
    neutral = Run(tiny, n, kinds)
    greedy_set = Run(tiny, n, ("greedy+min_p", "sampled"))
    try:
        for i in range(n):
            neutral.eng.set_truncation(i, 0.0, 1.0)
            neutral.eng.set_mirostat(i, 0.0, 0.1)
        for r in (plain, neutral, greedy_set):
            r.eng.decode(8, batch=n)
        want = [plain.eng.read_tokens(i, 9) for i in range(n)]
        assert [neutral.eng.read_tokens(i, 9) for i in range(n)] == want
        assert [greedy_set.eng.read_tokens(i, 9) for i in range(n)] == want
        sp, sn, sg = plain.eng.stats(), neutral.eng.stats(), greedy_set.eng.stats()
        assert sp["graph_captures"] == sn["graph_captures"] == sg["graph_captures"] and sp["workspace_bytes"] == sn["workspace_bytes"]
        with pytest.raises(RuntimeError):
            plain.eng.filtered_logits(n)  # nothing was allocated
    finally:
        for r in (plain, neutral, greedy_set):
            r.close()


@pytest.mark.parametrize("n", [1, 4, 5, 64])
def test_written_once_truncating_plans(tiny, n):
    run = Run(tiny, n, ("min_p", "typical", "both", "greedy"))
    try:
        run.step(check=False)
        assert run.eng.replay_route() == "aql"
        c = run.eng.check_step(n)
        assert c["double_writes"] == 0, c
        assert np.isfinite(run.eng.logits(n).float().cpu().numpy()).all()
    finally:
        run.close()


def test_fp8_pages(tiny):
    run = Run(tiny, 5, KINDS, kv_format="fp8")
    try:
        for _ in range(3):
            run.step()
    finally:
        run.close()
