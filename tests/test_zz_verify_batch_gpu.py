"""GPU tier: batched speculative verification (include/tinyllm_engine.h "tl_engine_verify_batch"; csrc/verify_attn.h).

Up to 8 tokens for each of several slots in ONE pass over the decode route, acceptance decided on the device.  Held here:
  * the attention stage over caller pools (tl_verify_attention_rows) against the numpy oracle's q/k-norm + RoPE + paged attention per
    sequence, with the per-element tolerance tests/test_ops_gpu.py applies to tl_paged_attention at L <= 8 (one bf16 ulp of the oracle's
    value + ACC_FLOOR * 4 |v|max), and the pools afterwards: the appended rows the oracle's, every other row of every page untouched;
  * the same over FP8 pages: the FP8 launch against the bf16 launch over the dequantised pages by the rule of
    tests/test_zz_kv_fp8_gpu.py (a zero k-norm weight and chunk V rows on the E4M3 grid make the quantisation of the appended rows the
    identity, so both launches see the same values: at most 0.2 % of the elements differ, each by at most one bf16 step); and, in the
    general case, codes and scales of the appended rows are kv8's of the rows the bf16 launch appends, the output held to the oracle;
  * the acceptance stage (tl_verify_accept_rows) against a numpy restatement;
  * the engine call against the oracle (bands derived as in tests/test_engine_gpu.py), against tl_engine_verify, its all-or-nothing
    refusals, its commit through a prefix-cache page, MoE layers, and batch_speculative_generate_ids over two engines.
TINY_CFG, 16-token pages: the smallest shapes at which the row arithmetic can go wrong (a chunk that crosses a page, one that starts
on a page, a context that is split)."""

import ctypes

import numpy as np
import pytest
import torch

from helpers import TINY_CFG, assert_bf16_close, assert_rounded_close, bf16_ulp, check_against_truth, to_mlx_shaped
from oracle import kv_fp8
from oracle import tiny_oracle as O
from test_ops_gpu import ACC_FLOOR  # the accumulation floor of the paged-attention operator tests: named, not re-invented

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, PAGE = 128, 16
EPS, THETA = 1e-6, 1e6
V = TINY_CFG["vocab_size"]


@pytest.fixture(scope="module")
def ext():
    import tiny_llm_ext_hip

    tiny_llm_ext_hip.load_library(".")
    return tiny_llm_ext_hip


def _t(a, dtype=torch.bfloat16):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _host(t):
    return t.float().cpu().numpy()


# ---- 1 / 2: the attention stage over caller pools ---------------------------------------------------------------------------------------
LENS = (1, 8, 3, 5)
# a fresh sequence; rows that cross a page boundary inside the chunk; a chunk that starts exactly on a new page; and the smallest final
# context that the split rule of tl_paged_attention cuts in two (max_ctx / 64 >= 2): 123 + 5 = 128
STARTS = (0, 15, 16, 123)
SLOTS = (2, 0, 4, 1)  # block-table rows, out of order and with a row nobody uses


def attention_case(hq, hkv, seed, k_norm_zero=False):
    """k_norm_zero (the construction of tests/test_zz_kv_fp8_gpu.py, _decode_case): the appended K rows are all zeros and the chunk's V
    rows lie on the E4M3 grid, so quantising what a launch appends changes nothing."""
    rng = np.random.default_rng(seed)
    need = [(s + n + PAGE - 1) // PAGE for s, n in zip(STARTS, LENS)]
    P = sum(need) + 3
    ids = list(rng.permutation(P))
    table = -np.ones((5, max(need) + 1), dtype=np.int32)
    for slot, pages in zip(SLOTS, need):
        for j in range(pages):
            table[slot, j] = ids.pop()
    kp = O.bf16(rng.standard_normal((P, hkv, PAGE, D), dtype=np.float32))  # (random rows: the context, and the sentinel of every row nobody may touch)
    vp = O.bf16(rng.standard_normal((P, hkv, PAGE, D), dtype=np.float32))
    qkv = O.bf16(rng.standard_normal((sum(LENS), (hq + 2 * hkv) * D), dtype=np.float32))
    qn = O.bf16(1.0 + 0.1 * rng.standard_normal((D,), dtype=np.float32))
    kn = O.bf16(1.0 + 0.1 * rng.standard_normal((D,), dtype=np.float32))
    if k_norm_zero:
        kn = np.zeros((D,), np.float32)
        rows = qkv.reshape(sum(LENS), hq + 2 * hkv, D)
        rows[:, hq + hkv:] = kv_fp8.round_trip(rows[:, hq + hkv:])
        qkv = rows.reshape(sum(LENS), -1)
    return kp, vp, table, qkv, qn, kn


def attention_oracle(case, hq, hkv, round_trip=None):
    """Reference op order per sequence (qwen3_week3.py:63-86): q/k RMSNorm -> RoPE at the chunk's offset -> paged_cache_update -> causal
    paged_attention over start + len tokens.  round_trip: what a row becomes on its way into the pages (FP8: oracle/kv_fp8.py)."""
    kp, vp, table, qkv, qn, kn = case
    kp, vp = kp.copy(), vp.copy()
    out = np.zeros((sum(LENS), hq * D), np.float32)
    touched = np.zeros(kp.shape[:3], dtype=bool)
    row0 = 0
    for slot, start, n in zip(SLOTS, STARTS, LENS):
        rows = qkv[row0:row0 + n].reshape(n, hq + 2 * hkv, D)
        q = O.rope(O.rms_norm_fast(rows[:, :hq], qn, EPS)[None], [start], D, THETA, False, "bf16")        # [1, n, Hq, D]
        k = O.rope(O.rms_norm_fast(rows[:, hq:hq + hkv], kn, EPS)[None], [start], D, THETA, False, "bf16")
        v = rows[:, hq + hkv:][None]
        if round_trip is not None:
            k, v = round_trip(k), round_trip(v)
        for j in range(n):
            pid, r = int(table[slot, (start + j) // PAGE]), (start + j) % PAGE
            kp[pid, :, r], vp[pid, :, r] = k[0, j], v[0, j]
            touched[pid, :, r] = True
        att = O.paged_attention(q[0].transpose(1, 0, 2), kp, vp, table[slot:slot + 1], np.asarray([start + n], np.int32), D ** -0.5, True, hkv, hq)
        out[row0:row0 + n] = att.transpose(1, 0, 2).reshape(n, hq * D)
        row0 += n
    return out, kp, vp, touched


def run_attention(ext, case, hq, hkv):
    kp, vp, table, qkv, qn, kn = case
    kpd, vpd = _t(kp), _t(vp)
    out, info = ext.verify_attention_rows(_t(qkv), _t(qn), _t(kn), kpd, vpd, _t(table, torch.int32), SLOTS, STARTS, LENS, num_heads=hq,
                                          num_kv_heads=hkv, rope_theta=THETA, eps=EPS)
    return _host(out), _host(kpd), _host(vpd), info


@pytest.fixture(scope="module", params=[(4, 2), (8, 2)], ids=["hq4_hkv2", "hq8_hkv2"])
def attention_run(ext, request):
    """One launch and one oracle evaluation per head shape, shared by the tests below (neither is modified)."""
    hq, hkv = request.param
    case = attention_case(hq, hkv, seed=100 * hq + hkv)
    return case, attention_oracle(case, hq, hkv), run_attention(ext, case, hq, hkv)


def test_attention_rows_match_the_oracle(attention_run):
    case, (want, _, _, _), (got, _, _, info) = attention_run
    assert info["n_splits"] > 1, f"the 128-token context was meant to be split: {info}"
    assert_rounded_close(got, want, "bf16", ulps=1.0, floor=ACC_FLOOR * 4 * float(np.abs(case[1]).max()), what=f"verify attention rows {info}")


def test_attention_rows_leave_the_oracle_s_pools(attention_run):
    """Whole pools: the appended K/V rows equal the oracle's bit for bit, every other row of every page keeps its sentinel."""
    case, (_, kp_want, vp_want, touched), (_, kp_after, vp_after, _) = attention_run
    assert touched.sum() == sum(LENS) * case[0].shape[1]
    np.testing.assert_array_equal(vp_after, vp_want, err_msg="value pages")
    np.testing.assert_array_equal(kp_after[~touched], case[0][~touched], err_msg="key pages outside the appended rows")
    np.testing.assert_array_equal(kp_after, kp_want, err_msg="key pages (appended rows: norm + RoPE)")


@pytest.mark.parametrize("hq,hkv", [(4, 2), (8, 2)])
def test_attention_rows_over_fp8_pages(ext, hq, hkv):
    case = attention_case(hq, hkv, seed=7 + hq)
    kp, vp, table, qkv, qn, kn = case
    kc, ks = kv_fp8.quantize_rows(kp)
    vc, vs = kv_fp8.quantize_rows(vp)
    pools = [_t(kc, torch.uint8), _t(ks, torch.float32), _t(vc, torch.uint8), _t(vs, torch.float32)]
    out, info = ext.verify_attention_rows(_t(qkv), _t(qn), _t(kn), pools[0], pools[2], _t(table, torch.int32), SLOTS, STARTS, LENS, num_heads=hq,
                                          num_kv_heads=hkv, rope_theta=THETA, eps=EPS, key_scales=pools[1], value_scales=pools[3])
    assert info["n_splits"] > 1
    kc2, ks2, vc2, vs2 = (p.cpu().numpy() for p in pools)
    # the rows the bf16 launch appends over the dequantised pools, quantised by the oracle's codec: the FP8 launch's codes and scales
    kd, vd = kv_fp8.dequantize_rows(kc, ks), kv_fp8.dequantize_rows(vc, vs)
    twin = run_attention(ext, (kd, vd, table, qkv, qn, kn), hq, hkv)
    _, _, _, touched = attention_oracle((kd, vd, table, qkv, qn, kn), hq, hkv)
    for name, codes, scales, before_c, before_s, rows in (("key", kc2, ks2, kc, ks, twin[1]), ("value", vc2, vs2, vc, vs, twin[2])):
        want_c, want_s = kv_fp8.quantize_rows(rows[touched])
        np.testing.assert_array_equal(codes[touched], want_c, err_msg=f"{name} codes of the appended rows")
        np.testing.assert_array_equal(scales[touched].view(np.uint32), want_s.view(np.uint32), err_msg=f"{name} scales of the appended rows")
        np.testing.assert_array_equal(codes[~touched], before_c[~touched], err_msg=f"{name} codes outside the appended rows")
        np.testing.assert_array_equal(scales[~touched], before_s[~touched], err_msg=f"{name} scales outside the appended rows")
    # ... and the output against the oracle over the dequantised pages with the round trip of the new rows in place: the bar of
    # test_decode_attention_fp8_quantises_the_token_being_decoded (tests/test_zz_kv_fp8_gpu.py)
    want, _, _, _ = attention_oracle((kd, vd, table, qkv, qn, kn), hq, hkv, round_trip=kv_fp8.round_trip)
    assert_bf16_close(_host(out), want, ulps=1.0, abs_floor=1.5e-3, what=f"verify attention rows over FP8 pages {info}")


@pytest.mark.parametrize("hq,hkv", [(4, 2), (8, 2)])
def test_attention_rows_over_fp8_pages_equal_the_bf16_launch_over_the_dequantised_pages(ext, hq, hkv):
    """The rule of test_decode_walks_over_fp8_pages_equal_the_bf16_walks_bit_for_bit (tests/test_zz_kv_fp8_gpu.py) for a walk on the
    VALU: with appended rows that quantisation leaves as they are, the FP8 launch and the bf16 launch over the dequantised pages see the
    same values; hipcc may contract `acc * f + p * v` differently per instantiation, so at most 0.2 % of the elements may differ, each
    by at most one bf16 step (no absolute floor).  The pools afterwards hold the same values."""
    kp, vp, table, qkv, qn, kn = attention_case(hq, hkv, seed=31 + hq, k_norm_zero=True)
    kc, ks = kv_fp8.quantize_rows(kp)
    vc, vs = kv_fp8.quantize_rows(vp)
    pools = [_t(kc, torch.uint8), _t(ks, torch.float32), _t(vc, torch.uint8), _t(vs, torch.float32)]
    out, info = ext.verify_attention_rows(_t(qkv), _t(qn), _t(kn), pools[0], pools[2], _t(table, torch.int32), SLOTS, STARTS, LENS, num_heads=hq,
                                          num_kv_heads=hkv, rope_theta=THETA, eps=EPS, key_scales=pools[1], value_scales=pools[3])
    got = _host(out)
    kd, vd = kv_fp8.dequantize_rows(kc, ks), kv_fp8.dequantize_rows(vc, vs)
    twin, kd_after, vd_after, info2 = run_attention(ext, (kd, vd, table, qkv, qn, kn), hq, hkv)
    assert info == info2 and info["n_splits"] > 1
    diff = got != twin
    assert diff.mean() <= 2e-3, f"{info}: {int(diff.sum())} of {diff.size} elements differ"
    assert_bf16_close(got, twin, ulps=1.0, abs_floor=0.0, what=f"FP8 launch against the bf16 launch over the dequantised pages {info}")
    kc2, ks2, vc2, vs2 = (p.cpu().numpy() for p in pools)
    np.testing.assert_array_equal(kv_fp8.dequantize_rows(kc2, ks2), kd_after)
    np.testing.assert_array_equal(kv_fp8.dequantize_rows(vc2, vs2), vd_after)


def test_attention_rows_refuse_bad_input(ext):
    case = attention_case(4, 2, seed=1)
    kp, vp, table, qkv, qn, kn = case
    args = (_t(qkv), _t(qn), _t(kn), _t(kp), _t(vp), _t(table, torch.int32))
    kw = dict(num_heads=4, num_kv_heads=2, rope_theta=THETA, eps=EPS)
    with pytest.raises(RuntimeError, match="a slot appears twice"):
        ext.verify_attention_rows(*args, (2, 0, 2, 1), STARTS, LENS, **kw)
    with pytest.raises(RuntimeError, match="outside its block-table row"):
        ext.verify_attention_rows(*args, SLOTS, (0, 15, 16, 140), LENS, **kw)
    with pytest.raises(RuntimeError, match="between 1 and 8 rows"):
        ext.verify_attention_rows(_t(qkv[:9]), *args[1:], (0,), (0,), (9,), **kw)


# ---- 3: the acceptance stage ---------------------------------------------------------------------------------------------------------
def accept_numpy(logits, row0, lens, tokens):
    """a = the first j < n - 1 whose greedy id (first maximum, NaN never) differs from the next token fed; ids g[0 .. a]."""
    out = []
    for r0, n in zip(row0, lens):
        g = [int(np.argmax(np.where(np.isnan(logits[r0 + j]), -np.inf, logits[r0 + j]))) for j in range(n)]
        a = next((j for j in range(n - 1) if g[j] != int(tokens[r0 + j + 1])), n - 1)
        out.append(g[:a + 1])
    return out


def test_accept_rows_on_constructed_logits(ext):
    rng = np.random.default_rng(12)
    vocab = 1024
    lens = [4, 5, 6, 1, 3, 3, 5]
    row0 = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    R = sum(lens)
    logits = O.bf16(rng.standard_normal((R, vocab), dtype=np.float32))
    best = [int(t) for t in rng.integers(0, vocab, R)]
    for r in range(R):
        logits[r, best[r]] = 8.0
    tokens = np.zeros(R, np.int32)
    for s, (r0, n) in enumerate(zip(row0, lens)):
        tokens[r0] = 5 + s
        tokens[r0 + 1:r0 + n] = best[r0:r0 + n - 1]  # every proposal agrees ...
    tokens[row0[1] + 1] = (best[row0[1]] + 1) % vocab                     # ... but: the first proposal rejected
    tokens[row0[2] + 3] = (best[row0[2] + 2] + 1) % vocab                 # a rejection in the middle
    r = row0[4]                                                           # a tie on a deciding row: the lower id wins (and is the proposal)
    lo, hi = sorted((best[r], (best[r] + 77) % vocab))
    logits[r, lo] = logits[r, hi] = 8.0
    tokens[r + 1] = lo
    r = row0[5]                                                           # a NaN beside the maximum is never chosen
    logits[r, (best[r] + 1) % vocab] = np.nan
    logits[r + 1, 0] = np.nan
    tokens[row0[6] + 2] = (best[row0[6] + 1] + 1) % vocab                 # proposals that agree again behind a mismatch do not count
    want = accept_numpy(logits, row0, lens, tokens)
    assert [len(w) for w in want] == [4, 1, 3, 1, 3, 3, 2]
    got = ext.verify_accept_rows(_t(logits), row0, lens, _t(tokens, torch.int32))
    assert got == want
    with pytest.raises(RuntimeError, match="between 1 and 8 rows"):
        ext.verify_accept_rows(_t(logits), [0], [9], _t(tokens, torch.int32))


# ---- 4 .. 7, 9, 10: the engine call ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt():
    w = O.make_qwen3_weights(TINY_CFG, seed=3, sigma=0.05)
    return w, to_mlx_shaped(TINY_CFG, w)


def prompt_ids(n, seed=0):
    rng = np.random.default_rng(seed)
    return [int(t) for t in rng.integers(1, V, size=n)]


def oracle_band(cfg, w, prompts, forced_moe=False):
    """The band of tests/test_engine_gpu.py (fixture `err`), computed the same way: E = the bf16 oracle's largest distance from the float64
    truth over a few prompts and decode steps; HIP vs oracle 2.5 E + one bf16 ulp of the largest logit."""
    worst, top = 0.0, 0.0
    for prompt in prompts:
        truth, orc = O.TruthQwen3(cfg, w), O.OracleQwen3(cfg, w)
        lo = orc.forward(prompt)[0, -1]
        if forced_moe:
            truth.forced_moe_ids = orc.moe_ids
        lt = truth.forward(prompt)[0, -1]
        for _ in range(4):
            tok = [int(np.argmax(lo))]
            lo = orc.forward(tok)[0, -1]
            lt = truth.forward(tok)[0, -1]
            worst = max(worst, float(np.abs(lo - lt).max()))
            top = max(top, float(np.abs(lt).max()))
    return 2.5 * worst + float(bf16_ulp(top))


@pytest.fixture(scope="module")
def band(ckpt):
    return oracle_band(TINY_CFG, ckpt[0], [prompt_ids(n, seed=n) for n in (5, 37, 150)])


def assert_near_greedy(logits_row, token, band, what):
    row = np.asarray(logits_row, dtype=np.float64)
    gap = float(row.max() - row[token])
    assert gap <= band, f"{what}: token {token} is {gap:.4f} below the best logit (band {band:.4f})"


# seeds at which the oracle alone puts every deciding row's margin (0.36 .. 0.86) well outside the band (~0.10): checked on the CPU when
# this was written, so that the comparison with tl_engine_verify below skips no position
PROMPT_SEEDS = {11: 411, 19: 422, 33: 433}


def verify_case(w):
    """Three slots prefilled with 11, 19 and 33 tokens and their chunks of 5, 8 and 1 tokens: the pending token, then the oracle's own
    greedy continuation as proposals -- slot 0's third proposal replaced by another id, slot 1's all kept.  Also the oracle's logits rows
    of prompt + chunk (row len(prompt) + j follows chunk token j)."""
    prompts = [prompt_ids(n, seed=s) for n, s in PROMPT_SEEDS.items()]
    chunks, rows = [], []
    for i, (p, n) in enumerate(zip(prompts, (5, 8, 1))):
        model = O.OracleQwen3(TINY_CFG, w)
        chunk = [int(np.argmax(model.forward(p)[0, -1]))]
        while len(chunk) < n:
            chunk.append(int(np.argmax(model.forward([chunk[-1]])[0, -1])))
        if i == 0:
            chunk[3] = (chunk[3] + 1) % V
        chunks.append(chunk)
        rows.append(O.OracleQwen3(TINY_CFG, w).forward(p + chunk, logits_to_keep=None)[0])
    return prompts, chunks, rows


@pytest.fixture(scope="module")
def case(ckpt):
    return verify_case(ckpt[0])


def make_engine(model, **kw):
    from tiny_llm_hip.engine import DecodeEngine

    args = dict(page_size=PAGE, num_pages=64, max_batch=3, max_prefill_rows=64)
    args.update(kw)
    return DecodeEngine(model, **args)


def prefilled(eng, prompts):
    for slot, p in enumerate(prompts):
        eng.begin(slot)
        eng.prefill(slot, p)


def check_result(prompt, chunk, ids, rows, band, what):
    """ids = the greedy ids of rows 0 .. a, a = the first row whose id is not the next proposal; each the oracle's argmax or a provable
    near-tie with it."""
    assert 1 <= len(ids) <= len(chunk)
    for j, tok in enumerate(ids):
        assert_near_greedy(rows[len(prompt) + j], tok, band, f"{what}, row {j}")
    assert ids[:-1] == chunk[1:len(ids)], f"{what}: the ids ahead of the last are the accepted proposals"
    if len(ids) < len(chunk):
        assert ids[-1] != chunk[len(ids)], f"{what}: the call stopped at a proposal it could have accepted"


@pytest.mark.parametrize("kv_format", ["bf16", "fp8"])
def test_engine_call_matches_the_oracle(ckpt, case, band, kv_format):
    w, model = ckpt
    prompts, chunks, rows = case
    if kv_format == "fp8":  # the oracle with the E4M3 round trip on every row that enters the cache
        rows = [O.OracleQwen3(TINY_CFG, w, kv_format="fp8").forward(p + c, logits_to_keep=None)[0] for p, c in zip(prompts, chunks)]
    eng = make_engine(model, kv_format=kv_format)
    try:
        prefilled(eng, prompts)
        base = eng.stats()["workspace_bytes"]
        got = eng.verify_batch(list(enumerate(chunks)))
        assert eng.stats()["workspace_bytes"] > base, "the scratch of the first call is counted"
        for s in range(3):
            check_result(prompts[s], chunks[s], got[s], rows[s], band, f"slot {s}")
            assert eng.context_len(s) == len(prompts[s]) + len(chunks[s])
            eng.release(s)
        # the same with commit: the slots hold the accepted prefix and the next input, and decode on from there
        prefilled(eng, prompts)
        got = eng.verify_batch(list(enumerate(chunks)), commit=True)
        for s in range(3):
            check_result(prompts[s], chunks[s], got[s], rows[s], band, f"slot {s} (commit)")
            assert eng.context_len(s) == len(prompts[s]) + len(got[s])
        assert eng.read_pending(3) == [g[-1] for g in got]
        eng.decode(1, batch=3)
        after = eng.logits(3).float().cpu().numpy()
        for s in range(3):
            seq = prompts[s] + chunks[s][:len(got[s])] + [got[s][-1]]
            ref = O.OracleQwen3(TINY_CFG, w, kv_format=kv_format).forward(seq)[0, -1]
            truth = O.TruthQwen3(TINY_CFG, w).forward(seq)[0, -1]
            if kv_format == "bf16":
                check_against_truth(after[s][None], ref[None], truth[None], what=f"decode after verify_batch + commit, slot {s}")
            else:  # (the truth has no quantised cache: the FP8 engine is held to the quantised oracle's choice)
                assert_near_greedy(ref, int(np.argmax(after[s])), band, f"decode after verify_batch + commit over FP8 pages, slot {s}")
            eng.release(s)
        assert eng.stats()["pages_in_use"] == 0
    finally:
        eng.close()


def test_engine_call_agrees_with_verify_one_slot_at_a_time(ckpt, case, band):
    """The same slots and tokens through tl_engine_verify on a second engine: equal ids wherever the oracle's own margin between its two
    best logits exceeds the band; a position inside the band may differ, and at most 1 position in 20 may be skipped that way."""
    _, model = ckpt
    prompts, chunks, rows = case
    a, b = make_engine(model), make_engine(model)
    try:
        prefilled(a, prompts)
        prefilled(b, prompts)
        got = a.verify_batch(list(enumerate(chunks)))
        solo = [b.verify(s, chunks[s]) for s in range(3)]
        total = skipped = 0
        for s in range(3):
            for j, tok in enumerate(got[s]):
                top2 = np.sort(np.asarray(rows[s][len(prompts[s]) + j], np.float64))[-2:]
                total += 1
                if top2[1] - top2[0] <= band:
                    skipped += 1
                    continue
                assert tok == solo[s][j], f"slot {s}, row {j}: {tok} (batch) vs {solo[s][j]} (one slot)"
        assert total >= 10 and skipped * 20 <= total, f"{skipped} of {total} positions inside the band"
    finally:
        a.close()
        b.close()


def raw_verify_batch(eng, chunks, commit=False):
    """The C entry point without the binding's own argument checks."""
    import tiny_llm_ext_hip as ext

    n = len(chunks)
    flat = [t for _, toks in chunks for t in toks]
    out = (ext.TlVerifyResult * n)()
    return ext.lib().tl_engine_verify_batch(eng._h, n, (ctypes.c_int * n)(*[s for s, _ in chunks]), (ctypes.c_int32 * len(flat))(*flat),
                                            (ctypes.c_int * n)(*[len(t) for _, t in chunks]), int(commit), out)


@pytest.mark.parametrize("failure", ["pool", "sampling", "duplicate", "nine_tokens", "rows_65"])
@pytest.mark.parametrize("commit", [False, True])
def test_engine_call_is_all_or_nothing(ckpt, failure, commit):
    """A failure in the LAST sequence leaves every slot's context length, the page count and the pending tokens as they were."""
    _, model = ckpt
    n_slots = 9 if failure == "rows_65" else 3
    lengths = [11, 19, 32] + [3] * (n_slots - 3)
    prompts = [prompt_ids(n, seed=900 + n + i) for i, n in enumerate(lengths)]
    # pool: 1 + 2 + 2 pages are all there is, and the last chunk needs a third page for its slot
    eng = make_engine(model, max_batch=n_slots, num_pages=5 if failure == "pool" else 64)
    try:
        prefilled(eng, prompts)
        chunks = [(s, prompt_ids(8 if failure == "rows_65" else 4, seed=70 + s)) for s in range(n_slots)]
        if failure == "sampling":
            eng.set_sampling(n_slots - 1, 0.8, None, None, 1)
        elif failure == "duplicate":
            chunks[-1] = (0, chunks[-1][1])
        elif failure == "nine_tokens":
            chunks[-1] = (n_slots - 1, prompt_ids(9, seed=5))
        elif failure == "rows_65":
            chunks[-1] = (n_slots - 1, prompt_ids(1, seed=5))
            assert sum(len(t) for _, t in chunks) == 65
        before = ([eng.context_len(s) for s in range(n_slots)], eng.stats()["pages_in_use"], eng.read_pending(n_slots))
        assert raw_verify_batch(eng, chunks, commit) != 0
        assert ([eng.context_len(s) for s in range(n_slots)], eng.stats()["pages_in_use"], eng.read_pending(n_slots)) == before
        # ... and the call goes through once the cause is gone (the pool case: without the slot that needs the page)
        if failure == "sampling":
            eng.set_sampling(n_slots - 1, 0.0, None, None, 0)
        good = [(s, prompt_ids(4, seed=70 + s)) for s in range(2 if failure == "pool" else 3)]
        assert all(1 <= len(r) <= 4 for r in eng.verify_batch(good, commit=commit))
    finally:
        eng.close()


def test_commit_rewinds_into_a_page_the_prefix_index_holds(ckpt, band):
    """The publisher leaves three full pages (48 tokens).  Slot 1 attaches the first 40 of them (two pages shared, 8 rows of the third
    copied), then a chunk of 8 fills its third page, which enters the index; the rejection lands inside that page, so the commit's rewind
    gives the slot a private copy.  What the index holds keeps its bytes: a later request over the publisher's prefix still equals a cold
    engine bit for bit (the pattern of tests/test_zz_prefix_cache_gpu.py)."""
    w, model = ckpt
    rng = np.random.default_rng(442)  # (the oracle's margins at the three rows that can be accepted: 0.64 and more)
    S = [int(t) for t in rng.integers(1, V, 40)]
    T2 = [int(t) for t in rng.integers(1, V, 9)]
    orc = O.OracleQwen3(TINY_CFG, w)
    chunk = [int(np.argmax(orc.forward(S)[0, -1]))]
    while len(chunk) < 8:
        chunk.append(int(np.argmax(orc.forward([chunk[-1]])[0, -1])))
    chunk[3] = (chunk[3] + 1) % V  # rows 0 .. 2 can be accepted: the context ends at 41 .. 43, inside the page of tokens 32 .. 47
    rows = O.OracleQwen3(TINY_CFG, w).forward(S + chunk, logits_to_keep=None)[0]
    PUB = S + [(t + 1) % V for t in chunk]  # the publisher's own tokens 40 .. 47: none of them the chunk's

    def continuation(eng, slot):
        out = [eng.logits(1)[0].clone()]
        for _ in range(3):
            eng.decode(1, batch=slot + 1)
            out.append(eng.logits(slot + 1)[slot].clone())
        return out, eng.read_tokens(slot, 4)

    eng, cold = make_engine(model, num_pages=16, prefix_cache=True), make_engine(model, num_pages=16)
    try:
        eng.begin(0)
        eng.prefill(0, PUB, chunk=64)
        eng.release(0)
        assert eng.prefix_stats()["pages_retained"] == 3
        eng.begin(1)
        assert eng.prefix_attach(1, S + chunk) == 40
        before = eng.stats()
        got = eng.verify_batch([(1, chunk)], commit=True)[0]
        check_result(S, chunk, got, rows, band, "attached slot")
        assert len(got) <= 3 and eng.context_len(1) == 40 + len(got)
        after = eng.stats()
        assert after["page_allocations"] == before["page_allocations"] + 1, "the rewind into the indexed page copies it"
        assert eng.prefix_stats()["pages_retained"] >= 1, "the index keeps the page the slot left"
        eng.decode(1, batch=2)
        seq = S + chunk[:len(got)] + [got[-1]]
        check_against_truth(eng.logits(2)[1].float().cpu().numpy()[None], O.OracleQwen3(TINY_CFG, w).forward(seq)[0, -1][None],
                            O.TruthQwen3(TINY_CFG, w).forward(seq)[0, -1][None], what="decode after a commit through an indexed page")
        eng.release(1)
        # the publisher's prefix, hit again, against a cold engine (cache off, same slot, same chunks)
        eng.begin(0)
        assert eng.prefix_attach(0, S[:32] + T2) == 32
        eng.prefill(0, T2, chunk=len(T2))
        hit = continuation(eng, 0)
        cold.begin(0)
        cold.prefill(0, PUB, chunk=64, want_logits=False)
        cold.rewind(0, 16)
        cold.prefill(0, T2, chunk=len(T2))
        want = continuation(cold, 0)
        assert hit[1] == want[1]
        for i, (g, x) in enumerate(zip(hit[0], want[0])):
            assert torch.equal(g, x), f"logits row {i} of the later hit differs from the cold run"
    finally:
        eng.close()
        cold.close()


def test_more_rows_than_the_engine_was_created_for(ckpt, band):
    """An engine created for 16 rows (max_batch 5, max_prefill_rows 16) verifies 40: the pass runs on its scratch's own activations and
    on the matmul workspace a 40-row M needs, which tl_engine_create did not size, with the router's pointers swapped for the pass
    and back.  Ids against the oracle; the engine decodes on afterwards as before."""
    w, model = ckpt
    prompts = [prompt_ids(n, seed=700 + n) for n in (9, 17, 21, 30, 5)]
    chunks, rows = [], []
    for p in prompts:
        orc = O.OracleQwen3(TINY_CFG, w)
        chunk = [int(np.argmax(orc.forward(p)[0, -1]))]
        while len(chunk) < 8:
            chunk.append(int(np.argmax(orc.forward([chunk[-1]])[0, -1])))
        chunks.append(chunk)
        rows.append(O.OracleQwen3(TINY_CFG, w).forward(p + chunk, logits_to_keep=None)[0])
    eng = make_engine(model, max_batch=5, max_prefill_rows=16)
    try:
        prefilled(eng, prompts)
        got = eng.verify_batch(list(enumerate(chunks)), commit=True)
        assert sum(len(c) for c in chunks) == 40
        for s in range(5):
            check_result(prompts[s], chunks[s], got[s], rows[s], band, f"slot {s} of 40 rows on a 16-row engine")
            assert eng.context_len(s) == len(prompts[s]) + len(got[s])
        eng.decode(1, batch=5)  # the engine's own buffers and workspace are back in place
        after = eng.logits(5).float().cpu().numpy()
        for s in (0, 4):
            seq = prompts[s] + chunks[s][:len(got[s])] + [got[s][-1]]
            check_against_truth(after[s][None], O.OracleQwen3(TINY_CFG, w).forward(seq)[0, -1][None],
                                O.TruthQwen3(TINY_CFG, w).forward(seq)[0, -1][None], what=f"decode after a 40-row pass on a 16-row engine, slot {s}")
    finally:
        eng.close()


def test_nothing_is_allocated_before_the_first_call(ckpt):
    _, model = ckpt
    eng = make_engine(model)
    try:
        base = eng.stats()["workspace_bytes"]
        prefilled(eng, [prompt_ids(5, seed=1), prompt_ids(9, seed=2)])
        eng.decode(2, batch=2)
        assert eng.verify(0, prompt_ids(3, seed=3)) and eng.stats()["workspace_bytes"] == base
        eng.verify_batch([(0, prompt_ids(2, seed=4)), (1, prompt_ids(3, seed=5))])
        grown = eng.stats()["workspace_bytes"]
        assert grown > base
        eng.verify_batch([(1, prompt_ids(2, seed=6))])
        assert eng.stats()["workspace_bytes"] == grown, "the scratch is allocated once"
    finally:
        eng.close()


# ---- 8: MoE layers ---------------------------------------------------------------------------------------------------------------------
def test_moe_layers(tmp_path):
    """The tiny MoE configuration of tests/test_engine_moe_gpu.py, two slots x 3 tokens: ids near-greedy against that file's oracle
    (OracleQwen3 with moe_block layers), band derived as above with the truth on the oracle's expert choice."""
    from checkpoint_fixture import MOE_CFG_OVERRIDES, make_moe_weights, write_checkpoint
    from tiny_llm_hip import load

    cfg = dict(TINY_CFG, **MOE_CFG_OVERRIDES)
    w = make_moe_weights(cfg, seed=21)
    path = write_checkpoint(tmp_path / "ckpt", cfg, w, vocab_words=[f"w{i}" for i in range(cfg["vocab_size"] - 2)])
    model, _ = load(str(path))
    rng = np.random.default_rng(8)
    prompts = [[int(t) for t in rng.integers(2, cfg["vocab_size"], size=n)] for n in (9, 21)]
    moe_band = oracle_band(cfg, w, prompts, forced_moe=True)
    chunks, rows = [], []
    for p in prompts:
        orc = O.OracleQwen3(cfg, w)
        chunk = [int(np.argmax(orc.forward(p)[0, -1]))]
        while len(chunk) < 3:
            chunk.append(int(np.argmax(orc.forward([chunk[-1]])[0, -1])))
        chunks.append(chunk)
        rows.append(O.OracleQwen3(cfg, w).forward(p + chunk, logits_to_keep=None)[0])
    eng = make_engine(model, num_pages=32, max_batch=2)
    try:
        prefilled(eng, prompts)
        got = eng.verify_batch(list(enumerate(chunks)), commit=True)
        for s in range(2):
            check_result(prompts[s], chunks[s], got[s], rows[s], moe_band, f"MoE slot {s}")
            assert eng.context_len(s) == len(prompts[s]) + len(got[s])
    finally:
        eng.close()


def test_batch_cli_with_a_draft_model(ckpt, tmp_path, capsys):
    """batch_main.py --draft-model on a written checkpoint (the model as its own draft) generates the ids of the run without it.  The
    two runs are greedy over the same weights through different kernels (the batched decode step against the verification pass), so
    the prompts are three at which the oracle alone keeps its two best logits at least 0.3 apart -- three times the band -- at every
    position either run generates (12-token sequences; checked on the CPU when this was written): both runs must then emit the
    oracle's ids, and the answers are equal."""
    from checkpoint_fixture import write_checkpoint
    import batch_main

    w, _ = ckpt
    words = [f"w{i}" for i in range(V - 2)]
    path = str(write_checkpoint(tmp_path / "ckpt", TINY_CFG, w, vocab_words=words))
    prompts = tmp_path / "prompts.txt"
    prompts.write_text("w194 w491 w354\nw607 w985\nw433 w670 w506 w353\n")
    base = ["--model", path, "--batch-size", "2", "--prefill-step", "16", "--max-seq-len", "12", "--raw-prompts", "--prompts-file", str(prompts)]
    plain = dict(batch_main.main(base))
    spec = dict(batch_main.main(base + ["--draft-model", path, "--proposal-length", "3"]))
    assert sorted(spec) == sorted(plain) == [0, 1, 2]
    assert all(len(plain[i].split()) >= 8 for i in plain), f"the answers were meant to run to their limit: {plain}"
    assert spec == plain
    capsys.readouterr()


# ---- 9: the generation loop over two engines ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same_draft", [True, False])
def test_batch_speculative_generation_over_two_engines(ckpt, band, same_draft):
    from tiny_llm_hip.engine import batch_speculative_generate_ids

    w, model = ckpt
    draft_model = model if same_draft else to_mlx_shaped(TINY_CFG, O.make_qwen3_weights(TINY_CFG, seed=11, sigma=0.05))
    target, draft = make_engine(model, max_batch=4), make_engine(draft_model, max_batch=4)
    try:
        prompts = [prompt_ids(n, seed=300 + n) for n in (7, 19, 33, 12)]
        stats = {}
        outs = batch_speculative_generate_ids(target, draft, prompts, 24, proposal_length=3, stats=stats)
        checked = 0
        for p, spec in zip(prompts, outs):
            assert len(spec) == 24
            rows = O.OracleQwen3(TINY_CFG, w).forward(p + spec, logits_to_keep=None)[0]
            for j, tok in enumerate(spec):
                row = rows[len(p) - 1 + j]
                assert_near_greedy(row, tok, band, f"prompt of {len(p)} tokens, generated position {j}")
                checked += int(tok == int(np.argmax(row)))
        assert checked > 80, "most positions should simply be the oracle's argmax"
        rate = stats["accepted"] / max(stats["proposed"], 1)
        assert (rate > 0.8) if same_draft else (rate < 0.5), f"acceptance rate {rate:.2f}"
        assert stats["target_calls"] == len(prompts) + stats["rounds"] and stats["rounds"] < 24
        assert target.stats()["pages_in_use"] == 0 and draft.stats()["pages_in_use"] == 0
    finally:
        target.close()
        draft.close()
