"""GPU tier: speculative sampling on the device (tl_spec_sample_rows, tl_engine_verify_sampled, csrc/spec_sample.h) against the numpy
restatement of its definition (tests/spec_sample_oracle.py).  Every (accept, alt) must equal the oracle's unless the oracle flags the row
ambiguous (fp32 rounding on the device may then fall on either side); bonus rows equal the device sampler bit for bit; the engine's
result is the rows routine's over the same rows, exactly; and the emitted tokens are distributed as the target's own samples."""

import numpy as np
import pytest
import torch

import sampling_oracle as S
import spec_sample_oracle as SS
from helpers import QWEN4B_CFG, TINY_CFG

pytestmark = pytest.mark.gpu

C_DRAFT_SEED = 0x9E3779B97F4A7C15


def _cuda(rows):
    return torch.from_numpy(np.stack(rows).astype(np.float32)).bfloat16().cuda()


# ---- the rows routine ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SS.VOCABS)
def test_kernel_matches_oracle(V):
    import tiny_llm_ext_hip as ext

    cases = SS.kernel_cases(V)
    targets, drafts = _cuda([c[1] for c in cases]), _cuda([c[2] for c in cases])
    pair_of, x, seed, pos, tp, dp = [], [], [], [], [], []
    for i, (pair, _, _, tpar, dpar, props) in enumerate(cases):
        for xi, si, pi in props:
            pair_of.append(i), x.append(xi), seed.append(si), pos.append(pi), tp.append(tpar), dp.append(dpar)
    idx = torch.tensor(pair_of, device="cuda")
    accept, alt = ext.spec_sample_rows(targets[idx], drafts[idx], x, [t[0] for t in tp], [t[1] for t in tp], [t[2] for t in tp],
                                       [d[0] for d in dp], [d[1] for d in dp], [d[2] for d in dp], seed, pos)
    accept, alt = accept.cpu().tolist(), alt.cpu().tolist()
    ambiguous = 0
    for r in range(len(x)):
        want = cases[pair_of[r]][0].verify(x[r], seed[r], pos[r])
        ambiguous += want[2]
        assert want[2] or (accept[r], alt[r]) == want[:2], (r, x[r], tp[r], dp[r], (accept[r], alt[r]), want)
        assert accept[r] in (0, 1) and (alt[r] == -1 if accept[r] else 0 <= alt[r] < V)
    print(f"V {V}: {len(x)} rows, accepted {sum(accept)}, ambiguous {ambiguous}")
    assert ambiguous <= 0.02 * len(x), ambiguous
    assert 0.15 * len(x) < sum(accept) < 0.6 * len(x)


@pytest.mark.parametrize("V", [8200, 151941])
def test_kernel_bonus_greedy_and_out_of_range_rows(V):
    import tiny_llm_ext_hip as ext

    rng = np.random.default_rng(V + 1)
    base = SS.rows(V, rng)
    kinds = list(base)
    targets = _cuda([base[k] for k in kinds])
    drafts = _cuda([SS.bf16(base[k] + rng.standard_normal(V).astype(np.float32)) for k in kinds])
    # bonus rows (x = -1): bit for bit the device sampler's ids, greedy rows included
    params = [(r, T, k, p) for r in range(len(kinds)) for T in (0.0, 0.3, 1.0, 2.0) for k, p in SS.COMBOS]
    idx = torch.tensor([c[0] for c in params], device="cuda")
    T, K, P = [c[1] for c in params], [c[2] for c in params], [c[3] for c in params]
    seeds, pos = [700 + i for i in range(len(params))], [11 * i + 1 for i in range(len(params))]
    accept, alt = ext.spec_sample_rows(targets[idx], drafts[idx], -1, T, K, P, 1.0, 0, 1.0, seeds, pos)
    assert accept.cpu().tolist() == [0] * len(params)
    assert torch.equal(alt, ext.sample_logits(targets[idx], T, K, P, seeds, pos))
    # T_p = 0: accept iff the proposal is the first maximum, alt = the first maximum
    lf = targets.float().cpu().numpy()
    greedy = [int(np.argmax(lf[r])) for r in range(len(kinds))]
    xs = [g + d for g in greedy for d in (0, 1)]
    idx = torch.tensor([r for r in range(len(kinds)) for _ in (0, 1)], device="cuda")
    accept, alt = ext.spec_sample_rows(targets[idx], drafts[idx], [min(v, V - 1) for v in xs], 0.0, 40, 0.9, 0.8, 0, 1.0, 3, 9)
    want = [(1, -1) if min(v, V - 1) == g else (0, g) for v, g in zip(xs, [g for g in greedy for _ in (0, 1)])]
    assert list(zip(accept.cpu().tolist(), alt.cpu().tolist())) == want
    # x >= V is rejected without a read at it; alt follows the oracle (p_x = 0: the residual is drawn as for any rejection)
    big = [V, V + 1, 2 ** 31 - 1]
    idx = torch.tensor([0] * len(big), device="cuda")
    accept, alt = ext.spec_sample_rows(targets[idx], drafts[idx], big, 0.7, 20, 1.0, 0.7, 20, 1.0, [1, 2, 3], 5)
    assert accept.cpu().tolist() == [0, 0, 0]
    pair = SS.Pair(lf[0], drafts[0].float().cpu().numpy(), (0.7, 20, 1.0), (0.7, 20, 1.0))
    for i, v in enumerate(big):
        want = pair.verify(v, i + 1, 5)
        assert want[2] or alt[i].item() == want[1]


def test_kernel_edge_rows():
    import tiny_llm_ext_hip as ext

    V = 3001
    ok = torch.from_numpy(np.random.default_rng(6).standard_normal(V).astype(np.float32)).bfloat16()
    pinf = ok.clone()
    pinf[[40, 90]] = float("inf")
    targets = torch.stack([torch.full((V,), float("nan")).bfloat16(), torch.full((V,), float("-inf")).bfloat16(), pinf, ok]).cuda()
    drafts = torch.stack([ok, ok, ok, pinf]).cuda()
    hot = [0, 0, 40]
    for x in (0, 40, 41):
        accept, alt = ext.spec_sample_rows(targets[:3], drafts[:3], x, 0.9, 20, 0.95, 0.9, 20, 0.95, 5, 5)
        assert list(zip(accept.cpu().tolist(), alt.cpu().tolist())) == [(1, -1) if x == h else (0, h) for h in hot]
    # a one-hot draft row: every other proposal has q_x = 0 and is accepted where the target keeps it
    pair = SS.Pair(ok.float().numpy(), pinf.float().numpy(), (0.9, 20, 0.95), (0.9, 20, 0.95))
    inside = int(np.flatnonzero(pair.p > 0)[0])
    for x in (inside, 40):
        accept, alt = ext.spec_sample_rows(targets[3:], drafts[3:], x, 0.9, 20, 0.95, 0.9, 20, 0.95, 5, 5)
        want = pair.verify(x, 5, 5)
        assert want[2] or (accept.item(), alt.item()) == want[:2]


def test_kernel_distribution():
    """The CPU tier's property through the device: the emitted token (x if accepted, else alt) against p, G < 3 |kept|."""
    import tiny_llm_ext_hip as ext

    pair, target, draft, proposals = SS.distribution_case(0)
    n = len(proposals)
    t = _cuda([target]).expand(n, SS.DIST_V).contiguous()
    d = _cuda([draft]).expand(n, SS.DIST_V).contiguous()
    T, k, p = SS.DIST_PARAMS
    accept, alt = ext.spec_sample_rows(t, d, proposals, T, k, p, T, k, p, list(range(n)), 7)
    accept, alt = accept.cpu().numpy(), alt.cpu().numpy()
    emitted = np.where(accept == 1, np.asarray(proposals), alt)
    kept = int((pair.p > 0).sum())
    g = SS.g_statistic(emitted, pair.p)
    print(f"G {g:.1f}, bound {3 * kept}, accepted {int(accept.sum())} of {n}")
    assert g < 3 * kept, g


# ---- the engine ---------------------------------------------------------------------------------------------------------------
def _tiny_model(seed):
    from oracle import tiny_oracle as O
    from helpers import to_mlx_shaped

    return to_mlx_shaped(TINY_CFG, O.make_qwen3_weights(TINY_CFG, seed=seed, sigma=0.05))


@pytest.fixture(scope="module")
def tiny_pair():
    return _tiny_model(3), _tiny_model(11)


@pytest.fixture(scope="module")
def q4b_pair():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    cfg = dict(QWEN4B_CFG, num_hidden_layers=2)
    return synthetic_qwen3(cfg, seed=11, sigma=0.02, device="cuda"), synthetic_qwen3(cfg, seed=12, sigma=0.02, device="cuda")


def _engines(models, **kw):
    from tiny_llm_hip.engine import DecodeEngine

    args = dict(page_size=16, num_pages=64, max_batch=8, max_prefill_rows=64)
    args.update(kw)
    return DecodeEngine(models[0], **args), DecodeEngine(models[1], **args)


def _draft_round(draft, rows, token, k):
    """k draft steps from the pending `token`, one per call, each row copied; the proposals."""
    draft.set_token(0, token)
    for i in range(k):
        draft.decode(1, batch=1)
        draft.copy_logits_into(rows[i], 1)
    return draft.read_tokens(0, k)


def _compose(accept, alt, fed):
    a = 0
    while a < len(fed) - 1 and accept[a]:
        a += 1
    return fed[1:a + 1] + [alt[a]]


def _one_round(models, prompt, k, tpar, dpar, seed, **kw):
    """One round by hand; checks the engine's result against the rows routine over the very rows it used, then the bookkeeping."""
    import tiny_llm_ext_hip as ext

    target, draft = _engines(models, **kw)
    try:
        for e in (target, draft):
            e.begin(0)
        target.set_sampling(0, *tpar, seed)
        draft.set_sampling(0, *dpar, seed ^ C_DRAFT_SEED)
        target.prefill(0, prompt)
        draft.prefill(0, prompt, want_logits=False)
        token = target.read_tokens(0, 1)[0]
        rows = draft.logits_buffer(7)
        proposals = _draft_round(draft, rows, token, k)
        fed = [token] + proposals
        ctx = target.context_len(0)
        assert ctx == len(prompt)
        emitted = target.verify_sampled(0, fed, rows if k else None, dpar)
        assert target.context_len(0) == ctx + len(fed)
        n = len(fed)
        t_rows = target.logits(n)
        d_rows = torch.cat([rows[:k], rows[:1]]) if k else t_rows  # (the bonus row's draft row is never read)
        T, K, P = tpar[0], tpar[1] or 0, tpar[2] or 1.0
        accept, alt = ext.spec_sample_rows(t_rows, d_rows.contiguous(), proposals + [-1], T, K, P, dpar[0], dpar[1] or 0, dpar[2] or 1.0, seed,
                                           [ctx + i + 1 for i in range(n)])
        accept, alt = accept.cpu().tolist(), alt.cpu().tolist()
        assert emitted == _compose(accept, alt, fed), (emitted, accept, alt, fed)
        # the last row alone is the sampler's draw at its position
        want_last = ext.sample_logits(t_rows[n - 1:], T, K, P, seed, ctx + n).item()
        assert alt[n - 1] == want_last
        if n == 1:
            assert emitted == [want_last]
        # the caller's bookkeeping, as after verify: rewind the rejected suffix, set the next token, decode on
        a = len(emitted) - 1
        target.rewind(0, n - 1 - a)
        assert target.context_len(0) == ctx + a + 1
        if k and a < k:
            draft.rewind(0, k - a - 1)
            assert draft.context_len(0) == ctx + a + 1
        target.set_token(0, emitted[a])
        target.decode(1, batch=1)
        nxt = target.read_tokens(0, 1)[0]
        lf = target.logits(1).float().cpu().numpy()[0]
        want = S.sample(lf, T, K, P, seed, ctx + a + 2)
        assert nxt == want[0] or want[1]
        return emitted, accept
    finally:
        target.close()
        draft.close()


@pytest.mark.parametrize("k", [0, 3, 7])
def test_engine_matches_rows_routine(tiny_pair, k):
    for seed in (1, 2, 3):
        _one_round(tiny_pair, [5, 17, 900, 33, 2, 41, 7], k, (0.8, 16, None), (0.8, 16, None), seed)
    _one_round(tiny_pair, [5, 17, 900, 33, 2], k, (1.0, 50, 0.9), (0.7, None, None), 9)


def test_engine_greedy_slot_verifies_greedily(tiny_pair):
    target, draft = _engines(tiny_pair)
    try:
        target.begin(0)
        target.prefill(0, [5, 17, 900, 33, 2])
        token = target.read_tokens(0, 1)[0]
        fed = [token, 3, 4, 5]
        want = target.verify(0, fed)
        target.rewind(0, len(fed))
        rows = target.logits_buffer(7)
        rows.zero_()
        torch.cuda.synchronize()
        got = target.verify_sampled(0, fed, rows, (0.8, None, None))
        cut = next((i for i in range(3) if want[i] != fed[i + 1]), 3)
        assert got == fed[1:cut + 1] + [want[cut]]
    finally:
        target.close()
        draft.close()


def test_engine_qwen4b_shapes(q4b_pair):
    _one_round(q4b_pair, list(range(7, 30)), 7, (0.8, 50, None), (0.8, 50, None), 4, page_size=128, num_pages=8, max_prefill_rows=128)


@pytest.mark.parametrize("draft_kind", ["other model", "same model, hotter"])
def test_end_to_end_distribution(tiny_pair, draft_kind):
    """1,500 rounds from one prompt and one pending token, seeds 0 .. 1,499: the first emitted token against the target's p of row 0.
    Fails when the draft rows handed over are not the rows the proposals were drawn from.  (The two synthetic models' 16-token kept
    sets hardly meet, so nearly every round of "other model" is a residual draw; the target's own weights under a hotter draft
    sampler give a q that overlaps p, and both branches carry weight.)"""
    other = draft_kind == "other model"
    Tq = SS.DIST_PARAMS[0] if other else 1.5
    target, draft = _engines(tiny_pair if other else (tiny_pair[0], tiny_pair[0]))
    try:
        prompt = [5, 17, 900, 33, 2, 41, 7, 300]
        T, k, p = SS.DIST_PARAMS
        for e in (target, draft):
            e.begin(0)
        target.prefill(0, prompt)
        draft.prefill(0, prompt, want_logits=False)
        token = target.read_tokens(0, 1)[0]
        rows = draft.logits_buffer(7)
        first, accepted = [], 0
        p_row = None
        for s in range(SS.DIST_ROWS):
            target.set_sampling(0, T, k, None, s)
            draft.set_sampling(0, Tq, k, None, s ^ C_DRAFT_SEED)
            fed = [token] + _draft_round(draft, rows, token, 3)
            emitted = target.verify_sampled(0, fed, rows, (Tq, k, None))
            if p_row is None:
                p_row = target.logits(4)[0].float().cpu().numpy()
            first.append(emitted[0])
            accepted += len(emitted) > 1
            target.rewind(0, 4)
            draft.rewind(0, 3)
            assert target.context_len(0) == draft.context_len(0) == len(prompt)
        w, _, _ = SS.weights(p_row, T, k, p)
        g = SS.g_statistic(first, w / w.sum())
        kept = int((w > 0).sum())
        print(f"G {g:.1f}, bound {3 * kept}, first proposal accepted in {accepted} of {SS.DIST_ROWS} rounds")
        assert g < 3 * kept, g
        if not other:
            assert 0.05 * SS.DIST_ROWS < accepted < 0.95 * SS.DIST_ROWS  # both branches carry weight
    finally:
        target.close()
        draft.close()


def test_speculative_generate_ids_sampled(tiny_pair):
    from tiny_llm_hip.engine import speculative_generate_ids

    prompt = [7, 19, 402, 5, 101, 33]
    for models, same in (((tiny_pair[0], tiny_pair[0]), True), (tiny_pair, False)):
        target, draft = _engines(models, max_batch=1)
        try:
            runs = []
            for _ in range(2):
                stats = {}
                runs.append((speculative_generate_ids(target, draft, prompt, 40, proposal_length=4, temperature=0.8, top_k=16, seed=21,
                                                      stats=stats), stats))
            assert runs[0] == runs[1]
            out, stats = runs[0]
            assert len(out) == 40 and all(0 <= t < TINY_CFG["vocab_size"] for t in out)
            other = speculative_generate_ids(target, draft, prompt, 40, proposal_length=4, temperature=0.8, top_k=16, seed=22)
            assert other != out
            rate = stats["accepted"] / max(stats["proposed"], 1)
            print(f"same draft {same}: accepted {stats['accepted']} of {stats['proposed']}, resampled {stats['resampled']}")
            if same:  # p and q differ by kernel-route rounding only
                assert rate >= 0.9, rate
            assert target.stats()["pages_in_use"] == 0 and draft.stats()["pages_in_use"] == 0
        finally:
            target.close()
            draft.close()


def test_refusals(tiny_pair):
    target, draft = _engines(tiny_pair)
    try:
        rows = target.logits_buffer(7)
        target.begin(0)
        target.set_sampling(0, 0.8, 16, None, 3)
        target.prefill(0, [5, 17, 900])
        with pytest.raises(RuntimeError):
            target.verify(0, [1, 2])  # tl_engine_verify still refuses a sampling slot
        with pytest.raises(ValueError):
            target.verify_sampled(0, [1, 2], None)
        with pytest.raises(ValueError):
            target.verify_sampled(0, list(range(9)), rows)
        with pytest.raises(ValueError):
            target.verify_sampled(0, [1, 2], rows[:, :100])
        ctx = target.context_len(0)
        target.set_truncation(0, min_p=0.05)
        with pytest.raises(RuntimeError):
            target.verify_sampled(0, [1, 2], rows)
        target.set_truncation(0, min_p=0.0, typical_p=0.9)
        with pytest.raises(RuntimeError):
            target.verify_sampled(0, [1, 2], rows)
        target.set_truncation(0)
        target.set_penalties(0, repetition=1.3)
        with pytest.raises(RuntimeError):
            target.verify_sampled(0, [1, 2], rows)
        target.set_penalties(0)
        target.set_sampling(0, 0.8, None, None, 3)
        target.set_mirostat(0, 5.0, 0.1)
        with pytest.raises(RuntimeError):
            target.verify_sampled(0, [1, 2], rows)
        target.set_mirostat(0, 0.0)
        assert target.context_len(0) == ctx  # a refused call appends nothing
        with pytest.raises(RuntimeError):
            target.verify_sampled(1, [1, 2], rows)  # a slot that is not live
        assert len(target.verify_sampled(0, [1], None)) == 1
    finally:
        target.close()
        draft.close()


def test_cli_speculative_sampling(tmp_path, capsys):
    """main.py --draft-model ... --sampler-temp 0.8 --sampler-seed 1 on a written checkpoint: it runs and prints text."""
    from checkpoint_fixture import write_checkpoint
    from oracle import tiny_oracle as O
    import main as cli

    w = O.make_qwen3_weights(TINY_CFG, seed=3, sigma=0.05)
    words = [f"w{i}" for i in range(TINY_CFG["vocab_size"] - 2)]
    path = str(write_checkpoint(tmp_path / "ckpt", TINY_CFG, w, vocab_words=words))
    base = ["--model", path, "--prompt", "w5 w17 w400 w3", "--raw-prompt", "--max-new-tokens", "12", "--draft-model", path,
            "--proposal-length", "3", "--sampler-temp", "0.8", "--sampler-top-k", "20"]
    a = cli.main(base + ["--sampler-seed", "1"])
    assert isinstance(a, str) and 0 < len(a.split()) <= 12
    assert a in capsys.readouterr().out
    assert cli.main(base + ["--sampler-seed", "1"]) == a
    cli.main(base)
    assert "seed 0" in capsys.readouterr().out
