"""GPU tier: batched speculative sampling (include/tinyllm_engine.h "tl_engine_verify_batch_sampled"; csrc/verify_sample.h).

Held here:
  * the rows routine (tl_verify_sample_rows) in point mode against the numpy restatement of its definition (tests/verify_sample_oracle.py):
    accept / alt of every row and the composed results equal the oracle's unless the oracle flags the row ambiguous (fp32 rounding on
    the device may then fall on either side), and at most 5 % of a vocabulary's rows may be skipped that way;
  * point mode against tl_spec_sample_rows over materialised draft rows peaked at the proposal under draft temperature 0;
  * drafted mode against tl_spec_sample_rows, bit for bit (the same ssp_row);
  * the scan on constructed patterns; edge rows; the engine call against the rows routine over the very rows it read, with greedy and
    sampling slots in one call; commit; Qwen3-4B's vocabulary; the distribution of what is emitted; the Python loop; the refusals; the CLI."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import sampling_oracle as S
import spec_sample_oracle as SS
import verify_sample_oracle as VS
from helpers import QWEN4B_CFG, TINY_CFG, to_mlx_shaped
from oracle import tiny_oracle as O
from test_zz_verify_batch_gpu import oracle_band, prompt_ids

pytestmark = pytest.mark.gpu
V_TINY = TINY_CFG["vocab_size"]


@pytest.fixture(scope="module")
def ext():
    import tiny_llm_ext_hip

    tiny_llm_ext_hip.load_library(".")
    return tiny_llm_ext_hip


def _cuda(rows):
    return torch.from_numpy(np.stack(rows).astype(np.float32)).bfloat16().cuda()


def _i32(v):
    return torch.tensor([int(t) for t in v], dtype=torch.int32, device="cuda")


# ---- 1. the rows routine, point mode ----------------------------------------------------------------------------------------------
CASES_PER_CALL = 5  # 11 rows per case: 55 of the 64 rows of a call


@functools.lru_cache(maxsize=None)
def point_calls(V):
    """The CPU tier's inputs (VS.point_cases) cut into sequences of 8, 2 and 1 rows per case and into calls of at most 64 rows: a list of
    (target rows, row0, lens, starts, tokens, params, seeds, oracle's (accept, alt, ambiguous, results)).  A case's sequences read its one
    target row.  Length 8: the six proposals and the first again, then the bonus row; length 2: the most likely token (the row mostly
    accepts: a full acceptance) -- and, every other case, a token outside the kept set (a first-row rejection); length 1: a bonus row."""
    cases = VS.point_cases(V)
    calls = []
    for c0 in range(0, len(cases), CASES_PER_CALL):
        targets, row0, lens, starts, tokens, params, seeds = [], [], [], [], [], [], []
        for ci, (target, par, props) in enumerate(cases[c0:c0 + CASES_PER_CALL]):
            xs = [x for x, _, _ in props]
            for n, chunk, pick in ((8, [7] + xs + xs[:1], 0), (2, [7, xs[2] if (c0 + ci) % 2 == 0 else xs[4]], 1), (1, [7], 2)):
                row0.append(len(tokens)), lens.append(n), starts.append(props[pick][2]), seeds.append(props[pick][1]), params.append(par)
                tokens += chunk
                targets += [target] * n
        want = VS.verify_sequences(targets, row0, lens, starts, tokens, params, seeds)
        calls.append((targets, row0, lens, starts, tokens, params, seeds, want))
    return calls


def run_point(ext, call):
    targets, row0, lens, starts, tokens, params, seeds, _ = call
    accept, alt, results = ext.verify_sample_rows(_cuda(targets), None, row0, lens, starts, _i32(tokens), [p[0] for p in params],
                                                  [p[1] for p in params], [p[2] for p in params], seeds)
    return accept.cpu().tolist(), alt.cpu().tolist(), results


@pytest.mark.parametrize("V", SS.VOCABS)
def test_point_rows_match_the_oracle(ext, V):
    rows = ambiguous = accepted = 0
    counts = {1: set(), 2: set(), 8: set()}
    for call in point_calls(V):
        targets, row0, lens, starts, tokens, params, seeds, (w_accept, w_alt, w_amb, w_results) = call
        accept, alt, results = run_point(ext, call)
        for r in range(len(tokens)):
            rows += 1
            ambiguous += bool(w_amb[r])
            accepted += accept[r]
            assert w_amb[r] or (accept[r], alt[r]) == (w_accept[r], w_alt[r]), (V, r, (accept[r], alt[r]), (w_accept[r], w_alt[r]))
            assert accept[r] in (0, 1) and (alt[r] == -1 if accept[r] else 0 <= alt[r] < V)
        for i, (r0, n) in enumerate(zip(row0, lens)):
            counts[n].add(len(results[i]))
            assert results[i] == VS.compose([r0], [n], tokens, accept, alt)[0], "the scan composes what the rows decided"
            assert any(w_amb[r0:r0 + n]) or results[i] == w_results[i], (V, i, results[i], w_results[i])
    print(f"V {V}: {rows} rows, accepted {accepted}, ambiguous {ambiguous}, counts {counts}")
    assert ambiguous <= 0.05 * rows, ambiguous
    assert counts[1] == {1} and counts[2] == {1, 2} and len(counts[8]) >= 2, "bonus rows, a first-row rejection and a full acceptance"


@pytest.mark.parametrize("V", SS.VOCABS)
def test_point_rows_equal_the_two_row_routine_over_one_hot_drafts(ext, V):
    """The same rows through tl_spec_sample_rows with materialised draft rows (VS.two_row_twin): equal on every row the oracle does not
    flag ambiguous."""
    compared = 0
    for call in point_calls(V):
        targets, row0, lens, starts, tokens, params, seeds, (_, _, w_amb, _) = call
        accept, alt, _ = run_point(ext, call)
        t_dev = _cuda(targets)
        d_dev = torch.full_like(t_dev, -4.0)
        x, tp, dp, seed, pos = [], [], [], [], []
        for i, (r0, n) in enumerate(zip(row0, lens)):
            for j in range(n):
                xi = tokens[r0 + j + 1] if j < n - 1 else -1
                dpar = (0.0, 0, 1.0)
                if 0 <= xi < V:
                    d_dev[r0 + j, xi] = 9.0
                elif xi >= V:  # the point rule's residual is p whole: the two-row rule's R == 0 fallback, q == p
                    d_dev[r0 + j] = t_dev[r0 + j]
                    dpar = params[i]
                x.append(xi), tp.append(params[i]), dp.append(dpar), seed.append(seeds[i]), pos.append(starts[i] + j + 1)
        a2, b2 = ext.spec_sample_rows(t_dev, d_dev, x, [t[0] for t in tp], [t[1] for t in tp], [t[2] for t in tp], [d[0] for d in dp],
                                      [d[1] for d in dp], [d[2] for d in dp], seed, pos)
        a2, b2 = a2.cpu().tolist(), b2.cpu().tolist()
        for r in range(len(tokens)):
            if not w_amb[r]:
                compared += 1
                assert (accept[r], alt[r]) == (a2[r], b2[r]), (V, r, x[r], tp[r], (accept[r], alt[r]), (a2[r], b2[r]))
    assert compared >= 0.95 * sum(len(c[4]) for c in point_calls(V))


# ---- 2. drafted mode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1024, 8200])
def test_drafted_rows_equal_the_two_row_routine_bit_for_bit(ext, V):
    """SS.kernel_cases(V) grouped by the draft's parameters (one triple per call): every proposal a sequence of its own -- its row and a
    bonus row -- with its own seed and position.  It is the same ssp_row: accept and alt are equal on every row."""
    groups = {}
    for case in SS.kernel_cases(V):
        groups.setdefault(case[4], []).append(case)
    rows = 0
    for dpar, cases in groups.items():
        for c0 in range(0, len(cases), 5):
            targets, drafts, row0, lens, starts, tokens, params, seeds = [], [], [], [], [], [], [], []
            for _, target, draft, tpar, _, props in cases[c0:c0 + 5]:
                for x, seed, position in props:
                    row0.append(len(tokens)), lens.append(2), starts.append(position - 1), seeds.append(seed), params.append(tpar)
                    tokens += [3, x]
                    targets += [target, target]
                    drafts += [draft, draft]
            t_dev, d_dev = _cuda(targets), _cuda(drafts)
            accept, alt, results = ext.verify_sample_rows(t_dev, d_dev, row0, lens, starts, _i32(tokens), [p[0] for p in params],
                                                          [p[1] for p in params], [p[2] for p in params], seeds, draft_sampling=dpar)
            x = [t for pair in zip(tokens[1::2], [-1] * len(row0)) for t in pair]
            per_row = lambda v: [t for t in v for _ in (0, 1)]
            pos = [s + j + 1 for s in starts for j in (0, 1)]
            a2, b2 = ext.spec_sample_rows(t_dev, d_dev, x, per_row([p[0] for p in params]), per_row([p[1] for p in params]),
                                          per_row([p[2] for p in params]), dpar[0], dpar[1], dpar[2], per_row(seeds), pos)
            assert torch.equal(accept, a2) and torch.equal(alt, b2), (V, dpar, c0)
            assert results == VS.compose(row0, lens, tokens, accept.cpu().tolist(), alt.cpu().tolist())
            rows += len(tokens)
    assert rows == 2 * sum(len(c[5]) for c in SS.kernel_cases(V)) >= 2 * 5 * len(SS.kernel_cases(V))


# ---- 3. the scan ----------------------------------------------------------------------------------------------------------------------
def test_scan_on_constructed_patterns(ext):
    """Greedy parameters make a row's decision a matter of its peak: accept iff the proposal is the peak, alt = the peak.  8 sequences of
    8 rows whose first rejection stands at every a in 0 .. 7 (proposals behind it match their peaks again and are ignored), then 64
    sequences of one row."""
    V = 256
    rng = np.random.default_rng(5)
    logits = SS.bf16(rng.standard_normal((64, V)).astype(np.float32))
    peak = [int(t) for t in rng.integers(0, V, 64)]
    for r in range(64):
        logits[r, peak[r]] = 9.0
    row0, lens = [8 * i for i in range(8)], [8] * 8
    tokens = np.zeros(64, np.int64)
    want = []
    for i, r0 in enumerate(row0):
        tokens[r0] = 5
        tokens[r0 + 1:r0 + 8] = peak[r0:r0 + 7]  # every proposal is its row's peak ...
        if i < 7:
            tokens[r0 + i + 1] = (peak[r0 + i] + 1) % V  # ... but row i's
        want.append(peak[r0:r0 + i] + [peak[r0 + i]])
    accept, alt, results = ext.verify_sample_rows(_cuda(list(logits)), None, row0, lens, [3] * 8, _i32(tokens), 0.0, 0, 1.0, 1)
    assert results == want and sorted(len(r) - 1 for r in results) == list(range(8))
    accept = accept.cpu().tolist()
    assert accept[row0[2]:row0[2] + 8] == [1, 1, 0, 1, 1, 1, 1, 0], "rows behind the first rejection decide for themselves and are ignored"
    # a sampling sequence beside greedy ones, and 64 sequences of one row each: every row is a bonus row
    accept, alt, results = ext.verify_sample_rows(_cuda(list(logits)), None, list(range(64)), [1] * 64, list(range(64)), _i32(tokens),
                                                  [0.0] * 63 + [0.9], [0] * 63 + [20], 1.0, list(range(64)))
    assert results[:63] == [[p] for p in peak[:63]] and accept.cpu().tolist() == [0] * 64
    assert results[63] == [ext.sample_logits(_cuda([logits[63]]), 0.9, 20, 1.0, 63, 64).item()]


# ---- 4. edge rows -----------------------------------------------------------------------------------------------------------------------
def test_edge_rows(ext):
    """Values in a logits row: an all-NaN row, a row of -inf, a row holding +inf, ties at the top-k boundary, x >= V."""
    V = 3001
    ok = SS.bf16(np.random.default_rng(6).standard_normal(V).astype(np.float32))
    pinf = ok.copy()
    pinf[[40, 90]] = np.inf
    ties = np.round(ok * 2.0).astype(np.float32)  # many equal logits: the boundary of top-k 20 cuts through a key
    rows = {"nan": np.full(V, np.nan, np.float32), "-inf": np.full(V, -np.inf, np.float32), "+inf": pinf, "ties": ties, "ok": ok}
    targets, row0, lens, starts, tokens, params, seeds = [], [], [], [], [], [], []
    par = (0.9, 20, 0.95)
    kept = np.flatnonzero(SS.weights(ties, *par)[0] > 0)
    proposals = {"nan": [0, 5], "-inf": [0, 5], "+inf": [40, 90, 41], "ties": [int(kept[0]), int(kept[-1]), int(kept[-1]) + 1, V, V + 7],
                 "ok": [V, 2 ** 31 - 1, int(np.argmax(ok))]}
    for name, xs in proposals.items():
        for x in xs:
            row0.append(len(tokens)), lens.append(2), starts.append(4 + len(row0)), seeds.append(90 + len(row0)), params.append(par)
            tokens += [3, x]
            targets += [rows[name]] * 2
    w_accept, w_alt, w_amb, w_results = VS.verify_sequences(targets, row0, lens, starts, tokens, params, seeds)
    accept, alt, results = ext.verify_sample_rows(_cuda(targets), None, row0, lens, starts, _i32(tokens), par[0], par[1], par[2], seeds)
    accept, alt = accept.cpu().tolist(), alt.cpu().tolist()
    assert sum(w_amb) <= 0.05 * len(tokens)
    for r in range(len(tokens)):
        assert w_amb[r] or (accept[r], alt[r]) == (w_accept[r], w_alt[r]), (r, tokens[r], (accept[r], alt[r]), (w_accept[r], w_alt[r]))
    assert [results[i] for i in range(7)] == [[0, 0], [0], [0, 0], [0], [40, 40], [40], [40]], "one-hot rows: token 0, the first +inf"
    assert all(accept[r0] == 0 for r0, x in zip(row0, tokens[1::2]) if x >= V), "x >= V is rejected"


# ---- 5. the engine call -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt():
    w = O.make_qwen3_weights(TINY_CFG, seed=3, sigma=0.05)
    return w, to_mlx_shaped(TINY_CFG, w)


def make_engine(model, **kw):
    from tiny_llm_hip.engine import DecodeEngine

    args = dict(page_size=16, num_pages=64, max_batch=4, max_prefill_rows=64)
    args.update(kw)
    return DecodeEngine(model, **args)


SLOT_PARAMS = [(0.8, 16, None, 11), (1.0, 50, 0.9, 12), (0.5, None, 0.8, 13), (0.0, None, None, 0)]  # (T, top_k, top_p, seed); slot 3 greedy
CHUNK_LENS = (1, 3, 8, 4)
PROMPT_LENS = (11, 19, 33, 24)


def engine_case(eng, arm=False):
    """Four slots prefilled, three of them sampling; the chunks: each slot's pending token, then ids taken from the slot's own prompt."""
    prompts = [prompt_ids(n, seed=400 + n) for n in PROMPT_LENS]
    chunks = []
    for s, (p, par, n) in enumerate(zip(prompts, SLOT_PARAMS, CHUNK_LENS)):
        eng.begin(s)
        if par[0] > 0:
            eng.set_sampling(s, *par)
        if arm:
            eng.set_lookup(s)
        eng.prefill(s, p)
        chunks.append((s, eng.read_tokens(s, 1) + p[2:1 + n]))
    return prompts, chunks


def rows_routine(ext, eng, chunks, starts, slot_params):
    """tl_verify_sample_rows over the rows the engine's last pass read."""
    lens = [len(c) for _, c in chunks]
    row0 = [int(v) for v in np.concatenate([[0], np.cumsum(lens)[:-1]])]
    flat = [t for _, c in chunks for t in c]
    par = [slot_params[s] for s, _ in chunks]
    return ext.verify_sample_rows(eng.verify_logits(len(flat)), None, row0, lens, starts, _i32(flat), [p[0] for p in par], [p[1] or 0 for p in par],
                                  [1.0 if p[2] is None else p[2] for p in par], [p[3] for p in par])


@pytest.mark.parametrize("kv_format", ["bf16", "fp8"])
def test_engine_call_equals_the_rows_routine(ext, ckpt, kv_format):
    _, model = ckpt
    eng, twin = make_engine(model, kv_format=kv_format), make_engine(model, kv_format=kv_format)
    try:
        prompts, chunks = engine_case(eng)
        base = eng.stats()["workspace_bytes"]
        got = eng.verify_batch_sampled(chunks)
        assert eng.stats()["workspace_bytes"] > base
        _, _, want = rows_routine(ext, eng, chunks, [len(p) for p in prompts], SLOT_PARAMS)
        assert got == want, (got, want)
        assert [eng.context_len(s) for s in range(4)] == [len(p) + n for p, n in zip(prompts, CHUNK_LENS)]
        for s, (p, (_, chunk), ids) in enumerate(zip(prompts, chunks, got)):
            assert 1 <= len(ids) <= len(chunk) and ids[:-1] == chunk[1:len(ids)] and 0 <= ids[-1] < V_TINY
        with pytest.raises(RuntimeError):
            eng.verify_logits(1, row0=16)
        assert eng.verify_logits(2, row0=14).shape == (2, V_TINY)
        # the greedy slot: exactly tl_engine_verify_batch's result for the same slot and tokens (the twin's slots are all greedy and
        # take the same chunks, so both passes run the same launches over the same rows)
        for s, p in enumerate(prompts):
            twin.begin(s)
            twin.prefill(s, p)
        assert twin.verify_batch(chunks)[3] == got[3]
    finally:
        eng.close()
        twin.close()


def test_verify_logits_before_the_first_pass(ckpt):
    eng = make_engine(ckpt[1])
    try:
        with pytest.raises(RuntimeError, match="no batched verification has run"):
            eng.verify_logits(1)
    finally:
        eng.close()


def test_commit_equals_rewind_and_set_token(ext, ckpt):
    _, model = ckpt
    a, b = make_engine(model), make_engine(model)
    try:
        prompts, chunks = engine_case(a, arm=True)
        engine_case(b, arm=True)
        got = a.verify_batch_sampled(chunks)
        for (s, chunk), ids in zip(chunks, got):
            if len(chunk) - len(ids):
                a.rewind(s, len(chunk) - len(ids))
            a.set_token(s, ids[-1])
        assert b.verify_batch_sampled(chunks, commit=True) == got
        state = lambda e: ([e.context_len(s) for s in range(4)], e.read_pending(4), [e.lookup_state(s) for s in range(4)], e.stats()["pages_in_use"])
        assert state(a) == state(b)
        assert state(a)[0] == [len(p) + len(ids) for p, ids in zip(prompts, got)] and state(a)[1] == [ids[-1] for ids in got]
        for e in (a, b):
            e.decode(1, batch=4)
        rows = a.logits(4)
        assert a.read_pending(4) == b.read_pending(4)
        for s, par in enumerate(SLOT_PARAMS):  # the sampler's id at the next position
            T, k, p = par[0], par[1] or 0, 1.0 if par[2] is None else par[2]
            want = ext.sample_logits(rows[s:s + 1], T, k, p, par[3], a.context_len(s)).item()
            assert a.read_pending(4)[s] == want, s
    finally:
        a.close()
        b.close()


def test_engine_qwen4b_shapes(ext):
    """One round at Qwen3-4B's vocabulary (151,936) on the 2-layer synthetic model, 128-token pages: lookup proposals for two sampling
    slots, one pass, the result against the rows routine over the rows it read."""
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    model = synthetic_qwen3(dict(QWEN4B_CFG, num_hidden_layers=2), seed=11, sigma=0.02, device="cuda")
    eng = DecodeEngine(model, page_size=128, num_pages=8, max_batch=2, max_prefill_rows=128)
    try:
        params = [(0.8, 50, None, 4), (1.0, 20, 0.9, 5)]
        prompts = [list(range(7, 19)) * 2, list(range(40, 47)) * 3]
        for s, (p, par) in enumerate(zip(prompts, params)):
            eng.begin(s)
            eng.set_sampling(s, *par)
            eng.set_lookup(s)
            eng.prefill(s, p)
            eng.set_token(s, p[3])  # a pending token the prompt holds: the lookup finds what followed it
        fed = eng.lookup_propose([0, 1], [5, 8], 3, 1, 7, sampled=True)
        assert [len(f) for f in fed] == [5, 8]
        chunks = list(enumerate(fed))
        got = eng.verify_batch_sampled(chunks)
        _, _, want = rows_routine(ext, eng, chunks, [len(p) for p in prompts], params)
        assert got == want
        assert [eng.context_len(s) for s in range(2)] == [len(p) + len(f) for p, f in zip(prompts, fed)]
    finally:
        eng.close()


# ---- 6. the distribution ------------------------------------------------------------------------------------------------------------------
def test_end_to_end_distribution(ckpt):
    """1,500 rounds from one prompt and one pending token, seeds 0 .. 1,499: the first emitted id against p of the row the pass read."""
    w, model = ckpt
    eng = make_engine(model, max_batch=1)
    try:
        prompt, token = [5, 17, 900, 33, 2, 41, 7, 300], 77
        T, k, p = SS.DIST_PARAMS
        row = O.OracleQwen3(TINY_CFG, w).forward(prompt + [token])[0, -1]
        wp, _, _ = SS.weights(row, T, k, p)
        prob = wp / wp.sum()
        inside = [int(t) for t in np.argsort(-prob, kind="stable") if 0.05 < prob[t] < 0.95]
        assert inside, "no kept token of the oracle's row 0 has a probability in (0.05, 0.95)"
        x = inside[0]
        eng.begin(0)
        eng.prefill(0, prompt)
        eng.set_token(0, token)
        first, accepted, p_row = [], 0, None
        for s in range(SS.DIST_ROWS):
            eng.set_sampling(0, T, k, None, s)
            ids = eng.verify_batch_sampled([(0, [token, x, 11, 12])])[0]
            if p_row is None:
                p_row = eng.verify_logits(1)[0].float().cpu().numpy()
            first.append(ids[0])
            accepted += len(ids) > 1
            assert (ids[0] == x) == (len(ids) > 1)
            eng.rewind(0, 4)
        assert eng.context_len(0) == len(prompt)
        wd, _, _ = SS.weights(p_row, T, k, p)
        g = SS.g_statistic(first, wd / wd.sum())
        kept = int((wd > 0).sum())
        print(f"G {g:.1f}, bound {3 * kept}, p_x {prob[x]:.3f}, the proposal accepted in {accepted} of {SS.DIST_ROWS} rounds")
        assert g < 3 * kept, g
        assert 0.05 * SS.DIST_ROWS < accepted < 0.95 * SS.DIST_ROWS, "both branches occur"
    finally:
        eng.close()


# ---- 7. the loop --------------------------------------------------------------------------------------------------------------------------
def repetitive(n, seed, period=7):
    rng = np.random.default_rng(seed)
    return [int(t) for t in np.resize(rng.integers(1, V_TINY, size=period), n)]


@pytest.fixture(scope="module")
def band(ckpt):
    return oracle_band(TINY_CFG, ckpt[0], [prompt_ids(n, seed=n) for n in (5, 37, 150)])


def test_lookup_generate_ids_sampled(ckpt, band):
    from tiny_llm_hip.engine import batch_generate_ids, lookup_generate_ids

    w, model = ckpt
    eng = make_engine(model, num_pages=96)
    try:
        prompts = [repetitive(23, 1), repetitive(30, 2, period=5), prompt_ids(19, seed=422)]
        # top_k = 1 keeps the first maximum alone: the greedy loop's ids.  Compared up to the first position at which the oracle's own
        # two best logits lie inside the band (behind it two greedy runs over different launches may part ways).
        stats_g, stats_s = {}, {}
        greedy = lookup_generate_ids(eng, prompts, 32, proposal_length=4, stats=stats_g)
        top1 = lookup_generate_ids(eng, prompts, 32, proposal_length=4, stats=stats_s, sampling={"temperature": 0.9, "top_k": 1}, base_seed=3)
        assert stats_s["proposed"] > 0 and stats_s["accepted"] <= stats_s["proposed"] and stats_s["rounds"] > 0
        checked = 0
        for p, g, s in zip(prompts, greedy, top1):
            rows = O.OracleQwen3(TINY_CFG, w).forward(p + g, logits_to_keep=None)[0]
            for j in range(len(g)):
                top2 = np.sort(np.asarray(rows[len(p) + j - 1], np.float64))[-2:]
                if top2[1] - top2[0] <= band:
                    break
                assert s[j] == g[j], (j, s[j], g[j])
                checked += 1
        print(f"top_k 1 against greedy: {checked} positions compared, equal throughout: {greedy == top1}; {stats_g} / {stats_s}")
        assert checked >= 16
        # real sampling: the same settings give the same ids, and the counts add up
        params = {"temperature": 0.8, "top_k": 16, "top_p": 0.95}
        runs = []
        for _ in range(2):
            stats = {}
            runs.append(lookup_generate_ids(eng, prompts, 32, proposal_length=4, stats=stats, sampling=params, base_seed=21))
            assert [len(o) for o in runs[-1]] == [32] * 3 and stats["proposed"] > 0 and 0 <= stats["accepted"] <= stats["proposed"] <= 4 * 3 * stats["rounds"]
        assert runs[0] == runs[1]
        assert runs[0] != greedy
        assert eng.stats()["pages_in_use"] == 0
        # nothing is ever proposed (no 16-gram of these prompts repeats): the loop is the plain sampler, batch_generate_ids' ids for the
        # same seeds -- up to a draw the sampler oracle flags ambiguous on the oracle's row
        plain = [prompt_ids(n, seed=500 + n) for n in (9, 14)]
        stats = {}
        spec = lookup_generate_ids(eng, plain, 12, proposal_length=4, max_ngram=16, min_ngram=16, stats=stats, sampling=params, base_seed=21)
        assert stats["rounds"] == 0 and stats["proposed"] == 0 and stats["steps"] > 0
        want = dict(batch_generate_ids(eng, plain, 12, batch_size=2, prefill_step=64, sampling=params, base_seed=21))
        for i, p in enumerate(plain):
            for j in range(12):
                if spec[i][j] != want[i][j]:
                    row = O.OracleQwen3(TINY_CFG, w).forward(p + spec[i][:j])[0, -1]
                    assert S.sample(row, 0.8, 16, 0.95, 21 + i, len(p) + j)[1], (i, j, spec[i], want[i])
                    break
    finally:
        eng.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def raw_verify(eng, chunks, commit=False, sampled=True):
    """The C entry points without the binding's own argument checks."""
    import tiny_llm_ext_hip as ext

    n = len(chunks)
    flat = [t for _, toks in chunks for t in toks]
    out = (ext.TlVerifyResult * n)()
    head = (eng._h, n, (ctypes.c_int * n)(*[s for s, _ in chunks]), (ctypes.c_int32 * len(flat))(*flat), (ctypes.c_int * n)(*[len(t) for _, t in chunks]))
    if sampled:
        return ext.lib().tl_engine_verify_batch_sampled(*head, None, 0.0, 0, 1.0, int(commit), out)
    return ext.lib().tl_engine_verify_batch(*head, int(commit), out)


@pytest.mark.parametrize("commit", [False, True])
def test_every_refusal_leaves_the_slots_as_they_were(ckpt, commit):
    import lora_oracle

    _, model = ckpt
    eng = make_engine(model, max_batch=10, num_pages=96, swap_pages=8)
    try:
        adapter = eng.load_lora(lora_oracle.to_lora_adapter(lora_oracle.make_adapter(TINY_CFG, 8, seed=0)))
        for s in range(10):
            eng.begin(s)
            eng.set_lookup(s)
            if s == 6:
                eng.set_lora(s, adapter)
            eng.prefill(s, repetitive(9 + s, 40 + s, period=3))
        eng.set_sampling(1, 0.8, None, None, 1)
        eng.set_sampling(2, 0.8, None, None, 1)
        eng.set_truncation(2, 0.1, 1.0)
        eng.set_penalties(3, 1.3)
        eng.park(4)
        eng.set_sampling(5, 0.8, None, None, 1)
        eng.set_mirostat(5, 5.0, 0.1)

        def state():
            return ([eng.context_len(s) for s in range(10)], eng.read_pending(10), [eng.lookup_state(s) for s in range(10)], eng.stats()["pages_in_use"])

        before = state()
        chunk = lambda s, n=3: (s, prompt_ids(n, seed=70 + s))
        bad = {"a processing slot": [chunk(0), chunk(3)], "a min-p slot": [chunk(0), chunk(2)], "a Mirostat slot": [chunk(0), chunk(5)],
               "an adapter slot": [chunk(0), chunk(6)], "a parked slot": [chunk(0), chunk(4)], "a duplicate": [chunk(0), chunk(1), chunk(0)],
               "nine tokens": [chunk(0), chunk(1, 9)]}
        for what, chunks in bad.items():
            assert raw_verify(eng, chunks, commit) != 0, what
            assert state() == before, what
        # 65 rows: eight chunks of 8 over distinct slots and one more token -- slots 2 .. 6 are refused for themselves, so fresh ones are used
        for s in (2, 3, 5, 6):
            eng.release(s)
            eng.begin(s)
            eng.prefill(s, repetitive(5, s))
        eng.unpark(4)
        before = state()
        rows65 = [(s, prompt_ids(8, seed=s)) for s in range(8)] + [(8, prompt_ids(1, seed=8))]
        assert sum(len(t) for _, t in rows65) == 65 and raw_verify(eng, rows65, commit) != 0 and state() == before
        with pytest.raises(ValueError, match="draft_rows must be"):
            eng.verify_batch_sampled([chunk(0), chunk(1)], commit=commit, draft_rows=torch.zeros((5, V_TINY), dtype=torch.bfloat16, device="cuda"))
        assert state() == before
        # a sampling slot is still refused by the greedy calls, and taken by the sampled ones
        assert raw_verify(eng, [chunk(0), chunk(1)], commit, sampled=False) != 0 and state() == before
        with pytest.raises(RuntimeError, match="samples"):
            eng.lookup_propose([0, 1])
        assert state() == before
        assert len(eng.lookup_propose([0, 1], sampled=True)) == 2
        got = eng.verify_batch_sampled([chunk(0), chunk(1)], commit=commit)
        assert all(1 <= len(r) <= 3 for r in got)
    finally:
        eng.close()


# ---- 9. the command line ------------------------------------------------------------------------------------------------------------------
def test_the_cli_with_top_k_one_prints_the_greedy_answers(ckpt, tmp_path, capsys):
    """lookup_main.py --sampler-temp 0.8 --sampler-top-k 1 against the greedy run, on the prompts of tests/test_zz_lookup_gpu.py's CLI
    test (the oracle keeps its two best logits at least 0.3 apart at every position either run generates)."""
    from checkpoint_fixture import write_checkpoint
    import lookup_main

    w, _ = ckpt
    words = [f"w{i}" for i in range(V_TINY - 2)]
    path = str(write_checkpoint(tmp_path / "ckpt", TINY_CFG, w, vocab_words=words))
    prompts = tmp_path / "prompts.txt"
    prompts.write_text("w194 w491 w354\nw607 w985\nw433 w670 w506 w353\n")
    common = [path, "--proposal-length", "3", "--max-ngram", "2", "--prefill-step", "16", "--max-seq-len", "12", "--raw-prompts", "--prompts-file",
              str(prompts)]
    greedy = dict(lookup_main.main(common))
    sampled = dict(lookup_main.main(common + ["--sampler-temp", "0.8", "--sampler-top-k", "1", "--sampler-seed", "5"]))
    assert sorted(sampled) == sorted(greedy) == [0, 1, 2]
    assert sampled == greedy
    assert '"rounds"' in capsys.readouterr().out
