"""GPU parity of the fused decode engine (include/tinyllm_engine.h) against
  (a) the numpy oracle's Qwen3 forward (oracle.OracleQwen3: readable restatement of Qwen3ModelWeek2/3), and
  (b) the op-by-op product model (tiny_llm_hip.Qwen3ModelWeek3 on the same HIP operators),
on a seeded 2-layer Qwen3-shaped W4 checkpoint, mirroring the reference's model-level checks
(tests_refsol/test_week_3_day_3.py:386-402: Week3 vs Week2 log-probs, rtol=atol=1e-3 on a fake model;
tests_refsol/test_week_2_day_6.py:92-109: full-model log-probs vs mlx_lm, rtol 0.1 / atol 2.0).

Tolerances are DERIVED, not chosen: the bf16 oracle and the HIP engine both round activations to bfloat16 at every
reference op boundary, in different fp32 summation orders, so neither is "right" -- both approximate the real-valued
function that oracle.TruthQwen3 evaluates in float64 with no intermediate rounding.  Wherever a truth is available a
test asserts  max|HIP - truth| <= 1.5 * max|oracle - truth| + 1 bf16 ulp  on the raw logits (helpers.check_against_truth;
the measured numbers go to gpurun_out/parity_numbers.jsonl).  Comparisons between two rounded paths use bands that follow
from that by the triangle inequality, with E = the oracle's measured distance from the truth on this checkpoint (fixture
`err`): HIP vs oracle 2.5 E, HIP vs HIP (solo vs batch, chunked vs one-shot) 3 E.  A greedy token may differ from a
reference path's only where the reference's own margin to that token is inside the band (a provable near-tie).
North-star "1e-3" is the reference's tolerance between two MLX paths on a FAKE tiny model (test_week_3_day_3.py:386-402);
on this checkpoint the bf16 oracle itself sits E ~ 2e-2 from the truth, so no bf16 pipeline can meet 1e-3 against another.
"""

import numpy as np
import pytest
import torch

from oracle import tiny_oracle as O
from helpers import TINY_CFG, bf16_ulp, check_against_truth, log_parity, to_mlx_shaped

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ckpt():
    w = O.make_qwen3_weights(TINY_CFG, seed=3, sigma=0.05)
    return w, to_mlx_shaped(TINY_CFG, w)


@pytest.fixture()
def engine(ckpt):
    from tiny_llm_hip.engine import DecodeEngine

    eng = DecodeEngine(ckpt[1], page_size=16, num_pages=64, max_batch=2, max_prefill_rows=64)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def err(ckpt):
    """E: the bf16 oracle's distance (max abs logit error) from the float64 truth on this checkpoint, measured over the
    prompts the tests use; and the bands derived from it.  CPU only."""
    w, _ = ckpt
    worst, worst_gemm, top = 0.0, 0.0, 0.0
    for n in (5, 37, 150):
        prompt = prompt_ids(n, seed=n)
        truth, orc, gemm = O.TruthQwen3(TINY_CFG, w), O.OracleQwen3(TINY_CFG, w), O.OracleQwen3(TINY_CFG, w, gemm_rows_threshold=0)
        lt, lo, lg = truth.forward(prompt)[0, -1], orc.forward(prompt)[0, -1], gemm.forward(prompt)[0, -1]
        for _ in range(4):
            tok = [int(np.argmax(lo))]
            lt, lo, lg = truth.forward(tok)[0, -1], orc.forward(tok)[0, -1], gemm.forward(tok)[0, -1]
            worst = max(worst, float(np.abs(lo - lt).max()))
            worst_gemm = max(worst_gemm, float(np.abs(lg - lt).max()))
            top = max(top, float(np.abs(lt).max()))
    ulp = float(bf16_ulp(top))
    out = {"E": worst, "E_gemm": worst_gemm, "ulp": ulp, "hip_vs_oracle": 2.5 * worst + ulp, "hip_vs_hip": 3.0 * worst + ulp,
           "gemv_vs_gemm": 1.5 * (worst + worst_gemm) + ulp}
    log_parity({"what": "engine test bands (TINY checkpoint)", **out})
    return out


def assert_near_greedy(logits_row, token, band, what):
    """`token` must be the argmax of `logits_row`, or so close to it that the two paths' rounding can explain the choice."""
    row = np.asarray(logits_row, dtype=np.float64)
    gap = float(row.max() - row[token])
    assert gap <= band, f"{what}: token {token} is {gap:.4f} below the best logit (band {band:.4f})"


def prompt_ids(n, seed=0):
    rng = np.random.default_rng(seed)
    return [int(t) for t in rng.integers(1, TINY_CFG["vocab_size"], size=n)]


def oracle_run(w, prompt, steps, cfg=TINY_CFG):
    """Greedy decode with the bf16 oracle, and the float64 truth teacher-forced on the same ids; returns per-step logits
    (first from prefill) of both, and the oracle's ids."""
    model, truth = O.OracleQwen3(cfg, w), O.TruthQwen3(cfg, w)
    logits, exact = [model.forward(prompt)[0, -1]], [truth.forward(prompt)[0, -1]]
    ids = [int(np.argmax(logits[-1]))]
    for _ in range(steps):
        logits.append(model.forward([ids[-1]])[0, -1])
        exact.append(truth.forward([ids[-1]])[0, -1])
        ids.append(int(np.argmax(logits[-1])))
    return np.stack(logits), ids, np.stack(exact)


@pytest.mark.parametrize("n_prompt", [1, 5, 20, 37, 90, 150, 300])
def test_engine_matches_oracle(ckpt, engine, err, n_prompt):
    """prefill (GEMV path for <=8 rows, MFMA GEMM + paged FlashAttention above) then 12 fused decode steps,
    crossing page boundaries (page_size 16); the decode attention window grows 64 -> 512 tokens in one workgroup, beyond
    that it is split and merged by a second launch.  HIP must sit as close to the float64 truth as the bf16 oracle does."""
    w, _ = ckpt
    prompt = prompt_ids(n_prompt, seed=n_prompt)
    steps = 12
    want_logits, want_ids, truth_logits = oracle_run(w, prompt, steps)
    engine.begin(0)
    engine.prefill(0, prompt, chunk=64)
    got = [engine.logits(1)[0].float().cpu().numpy()]
    ids = engine.read_tokens(0, 1)
    for s in range(steps):
        # teacher-force the oracle's token so both sides see the same history even after a near-tie
        engine.set_token(0, want_ids[s])
        engine.decode(1, batch=1)
        got.append(engine.logits(1)[0].float().cpu().numpy())
        ids.append(engine.read_tokens(0, 1)[0])
    engine.release(0)
    got = np.stack(got)
    # prompts above 8 rows prefill through the tile GEMM (weights rounded to bf16 first, reference quantize.py:54-65), as the
    # oracle does; the decode steps are GEMV on both sides
    check_against_truth(got, want_logits, truth_logits, what=f"engine vs oracle vs truth, TINY, prompt {n_prompt}")
    for s in range(steps + 1):
        assert_near_greedy(want_logits[s], ids[s], err["hip_vs_oracle"], f"greedy token at step {s}")


def test_engine_graph_equals_eager_and_free_running(ckpt, engine):
    """A replayed hipGraph step must be bit-identical to eager launches; free-running greedy decode (device
    feeds its own argmax back) must reproduce itself."""
    prompt = prompt_ids(9, seed=1)
    runs = []
    for use_graph in (False, True, True):
        engine.begin(0)
        engine.prefill(0, prompt)
        engine.decode(20, batch=1, use_graph=use_graph)
        runs.append((engine.read_tokens(0, 21), engine.logits(1).clone()))
        engine.release(0)
    assert runs[0][0] == runs[1][0] == runs[2][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[1][1], runs[2][1])
    st = engine.stats()
    assert st["graph_captures"] >= 1 and st["graph_replays"] >= 30
    assert st["pages_in_use"] == 0 and st["pages_free"] == 64


def test_engine_matches_op_by_op_model(ckpt, engine, err):
    """Same checkpoint through tiny_llm_hip.Qwen3ModelWeek3 (one HIP operator per reference op)."""
    from tiny_llm_hip import Qwen3ModelWeek3

    _, mlx_model = ckpt
    model = Qwen3ModelWeek3(mlx_model, page_size=16)
    prompt = prompt_ids(23, seed=5)
    cache = model.create_kv_cache()
    try:
        toks = torch.tensor([prompt], dtype=torch.int32, device="cuda")
        ref = [model(toks, 0, cache, logits_to_keep=1)[0, -1].float().cpu().numpy()]
        offset = len(prompt)
        ids = [int(np.argmax(ref[-1]))]
        for _ in range(8):
            t = torch.tensor([[ids[-1]]], dtype=torch.int32, device="cuda")
            ref.append(model(t, offset, cache, logits_to_keep=1)[0, -1].float().cpu().numpy())
            ids.append(int(np.argmax(ref[-1])))
            offset += 1
    finally:
        for c in cache:
            c.release()
    engine.begin(0)
    engine.prefill(0, prompt, chunk=64)
    got = [engine.logits(1)[0].float().cpu().numpy()]
    for s in range(8):
        engine.set_token(0, ids[s])
        engine.decode(1, batch=1)
        got.append(engine.logits(1)[0].float().cpu().numpy())
    engine.release(0)
    # two HIP paths (fused engine vs one operator per reference op), each within 1.5 E of the truth
    assert float(np.abs(np.stack(got) - np.stack(ref)).max()) <= err["hip_vs_hip"]


def test_engine_batch_slots_are_independent(ckpt, engine):
    """Two live slots decoded together (M=2 GEMV rows, batched attention) == each decoded alone; an idle
    slot (reference: context_len 0 row, kv_cache.py:210-224) does not disturb its neighbour."""
    pa, pb = prompt_ids(11, seed=2), prompt_ids(30, seed=4)
    solo = []
    for p in (pa, pb):
        engine.begin(0)
        engine.prefill(0, p)
        engine.decode(10, batch=1)
        solo.append(engine.read_tokens(0, 11))
        engine.release(0)
    engine.begin(0)
    engine.begin(1)
    engine.prefill(0, pa)
    engine.prefill(1, pb)
    engine.decode(10, batch=2)
    both = [engine.read_tokens(0, 11), engine.read_tokens(1, 11)]
    engine.release(0)
    # slot 1 keeps going with slot 0 idle
    engine.decode(3, batch=2)
    tail = engine.read_tokens(1, 14)
    engine.release(1)
    assert both[0] == solo[0] and both[1] == solo[1]
    assert tail[:11] == solo[1]


def test_engine_rewind_and_chunked_prefill(ckpt, engine, err):
    """rewind(n) then re-decoding reproduces the same ids (reference rewind, paged_kv_cache.py:414-434);
    chunked prefill (chunks of 8 -> GEMV/decode-attention path, 16 -> MFMA path) matches one-shot prefill
    within the band of two HIP paths of which one runs the tile GEMM (weights rounded to bf16 first)."""
    prompt = prompt_ids(40, seed=9)
    engine.begin(0)
    engine.prefill(0, prompt)
    first = engine.read_tokens(0, 1)[0]
    engine.decode(6, batch=1)
    a = engine.read_tokens(0, 7)
    engine.rewind(0, 6)
    assert engine.context_len(0) == 40
    engine.set_token(0, first)
    engine.decode(6, batch=1)
    b = engine.read_tokens(0, 6)
    one_shot = engine.logits(1)[0].float().cpu().numpy()
    engine.release(0)
    assert a[1:] == b
    for chunk in (8, 16):
        engine.begin(0)
        engine.prefill(0, prompt, chunk=chunk)
        for t in a[:6]:
            engine.set_token(0, t)
            engine.decode(1, batch=1)
        got = engine.logits(1)[0].float().cpu().numpy()
        engine.release(0)
        assert float(np.abs(got - one_shot).max()) <= err["gemv_vs_gemm"], f"chunk {chunk}"


def test_engine_errors(ckpt, engine):
    with pytest.raises(RuntimeError, match="slot holds no sequence"):
        engine.prefill(0, [1, 2, 3])
    engine.begin(0)
    with pytest.raises(RuntimeError, match="already holds"):
        engine.begin(0)
    with pytest.raises(RuntimeError, match="out of range"):
        engine.prefill(0, [TINY_CFG["vocab_size"]])
    with pytest.raises(RuntimeError, match="pool exhausted|max_pages_per_seq"):
        engine.reserve(0, 16 * 64 + 1)
    assert engine.stats()["pages_in_use"] == 0  # the failed reserve left nothing behind
    with pytest.raises(RuntimeError, match="max_prefill_rows"):
        engine.prefill(0, list(range(1, 66)), chunk=65)
    engine.release(0)


def _solo_rows(eng, prompt, ids, chunk):
    """Logits row that chose ids[j], for every j, when the request is served ALONE and fed exactly `ids`."""
    eng.begin(0)
    try:
        eng.prefill(0, prompt, chunk=chunk)
        rows = [eng.logits(1)[0].float().cpu().numpy()]
        for tok in ids[:-1]:
            eng.set_token(0, tok)
            eng.decode(1, batch=1)
            rows.append(eng.logits(1)[0].float().cpu().numpy())
    finally:
        eng.release(0)
    return rows


def test_continuous_batching_matches_solo_generation(ckpt, err):
    """batch_generate_ids (reference batch.py:136-285 schedule: one prefill chunk + one batched decode step per turn,
    staging slot -> decode slot hand-over).  EVERY id of EVERY request is checked: served alone and fed the same history,
    the engine must rank that id first, or within the band two HIP paths can differ by (rows of a batch see another
    attention window split and another RMSNorm grouping than a solo row, so a provable near-tie may go the other way --
    nothing else is accepted).  All pages come back."""
    from tiny_llm_hip.engine import DecodeEngine, batch_generate_ids

    eng = DecodeEngine(ckpt[1], page_size=16, num_pages=96, max_batch=4, max_prefill_rows=64)
    try:
        prompts = [prompt_ids(n, seed=100 + n) for n in (5, 23, 9, 40, 17, 3)]
        limits = [26, 29, 24, 27, 1, 28]
        active_counts = []
        got = batch_generate_ids(eng, prompts, limits, batch_size=3, prefill_step=16, on_step=active_counts.append)
        assert sorted(i for i, _ in got) == list(range(len(prompts)))
        total, first_choice = 0, 0
        for idx, ids in got:
            assert len(ids) == limits[idx], f"request {idx}"
            rows = _solo_rows(eng, prompts[idx], ids, chunk=16)
            for j, tok in enumerate(ids):
                assert_near_greedy(rows[j], tok, err["hip_vs_hip"], f"request {idx}, generated position {j}")
                first_choice += int(tok == int(np.argmax(rows[j])))
                total += 1
        assert first_choice >= 0.95 * total, f"only {first_choice} of {total} ids are the solo path's first choice"
        assert max(active_counts) == 3, "the decode batch should fill up"
        st = eng.stats()
        assert st["pages_in_use"] == 0 and st["pages_free"] == 96
    finally:
        eng.close()


def _solo_vs_batch(model, n_seq, steps=3, page_size=16, env_pages=None, return_ids=False):
    """Logits of every sequence decoded alone (slot 0, fused GEMV) and decoded together (one batch of n_seq rows).  The batch
    is teacher-forced on the ids of the solo runs, so both paths see the same history even where a near-tie would let their
    greedy choices differ."""
    from tiny_llm_hip.engine import DecodeEngine

    vocab = model.args.vocab_size if hasattr(model, "args") else TINY_CFG["vocab_size"]
    eng = DecodeEngine(model, page_size=page_size, num_pages=env_pages or (8 * n_seq + 8), max_batch=n_seq,
                       max_prefill_rows=64)
    try:
        rng = np.random.default_rng(77)
        prompts = [[int(t) for t in rng.integers(1, vocab, size=4 + (3 * i) % 23)] for i in range(n_seq)]
        solo, fed = [], []
        for p in prompts:
            eng.begin(0)
            eng.prefill(0, p)
            eng.decode(steps, batch=1)
            solo.append(eng.logits(1)[0].float().cpu().numpy())
            fed.append(eng.read_tokens(0, steps + 1)[:-1])  # the token each decode step consumed
            eng.release(0)
        for i, p in enumerate(prompts):
            eng.begin(i)
            eng.prefill(i, p)
        for k in range(steps):
            for i in range(n_seq):
                eng.set_token(i, fed[i][k])
            eng.decode(1, batch=n_seq)
        got = eng.logits(n_seq).float().cpu().numpy()
        for i in range(n_seq):
            eng.release(i)
        assert eng.stats()["pages_in_use"] == 0
        if return_ids:
            return got, np.stack(solo), prompts, fed
        return got, np.stack(solo)
    finally:
        eng.close()


@pytest.mark.parametrize("n_seq", [9, 12, 24, 40, 64])
def test_batched_decode_skinny_matmul_matches_solo(ckpt, err, monkeypatch, n_seq):
    """9..64 decode rows run the K-sliced skinny MFMA matmul (csrc/qmm3.h): the GEMV's algebraic form (reference
    quantized_matmul.metal:510-521) with the slices summed in fp32, so a sequence must decode to (nearly) the same
    logits alone and in a batch -- the band of two HIP paths that share every rounding point."""
    monkeypatch.delenv("TL_ENGINE_OPTIONS", raising=False)
    got, solo = _solo_vs_batch(ckpt[1], n_seq)
    assert float(np.abs(got - solo).max()) <= err["hip_vs_hip"]


def test_batched_decode_reference_gemm_path(ckpt, err, monkeypatch):
    """Engine option "qmm3" = 0: more than 8 decode rows go through RMSNorm + W4 MFMA GEMM + SwiGLU/residual kernels (reference
    quantize.py:54-65 sends rows > 8 to the matmul path, whose weights are rounded to bf16 first): logits within
    1.5 x (E of the GEMV oracle + E of the all-GEMM oracle) of solo decoding, both E measured against the float64 truth."""
    monkeypatch.setenv("TL_ENGINE_OPTIONS", "qmm3=0")  # (tl_engine_set_option through the host mirror)
    got, solo = _solo_vs_batch(ckpt[1], 12)
    assert float(np.abs(got - solo).max()) <= err["gemv_vs_gemm"]


WIDE_CFG = dict(hidden_size=1280, num_hidden_layers=1, num_attention_heads=10, num_key_value_heads=2, head_dim=128,
                intermediate_size=2560, vocab_size=4096, rope_theta=1000000, rms_norm_eps=1e-6,
                max_position_embeddings=4096, tie_word_embeddings=True)


@pytest.mark.parametrize("n_seq", [16, 32, 64])
def test_skinny_matmul_wide_shapes(n_seq):
    """Reduction dims of 10 / 20 quantisation groups (hidden 1280, intermediate 2560) reach the 10-, 8- and 5-group slice
    variants and several slices per row.  Batch rows vs the same rows decoded alone (3 E), and two rows of the batch against
    the bf16 oracle and the float64 truth fed the same tokens (HIP error <= 1.5 x oracle error)."""
    w = O.make_qwen3_weights(WIDE_CFG, seed=5, sigma=0.03)
    model = to_mlx_shaped(WIDE_CFG, w)
    got, solo, prompts, fed = _solo_vs_batch(model, n_seq, steps=2, page_size=16, return_ids=True)
    worst = 0.0
    for row in (0, n_seq - 1):
        orc, truth = O.OracleQwen3(WIDE_CFG, w), O.TruthQwen3(WIDE_CFG, w)
        lo, lt = orc.forward(prompts[row])[0, -1], truth.forward(prompts[row])[0, -1]
        for tok in fed[row]:
            lo, lt = orc.forward([tok])[0, -1], truth.forward([tok])[0, -1]
        rec = check_against_truth(got[row][None], lo[None], lt[None], what=f"WIDE batch of {n_seq}, row {row} (skinny matmul)")
        worst = max(worst, rec["max_abs_oracle_vs_truth"])
    band = 3.0 * worst + float(bf16_ulp(np.abs(solo).max()))
    assert float(np.abs(got - solo).max()) <= band, "batch rows vs the same rows decoded alone"


def _prefill_logits(model, prompt, rows):
    from tiny_llm_hip.engine import DecodeEngine

    eng = DecodeEngine(model, page_size=16, num_pages=64, max_batch=1, max_prefill_rows=rows)
    try:
        eng.begin(0)
        eng.prefill(0, prompt, chunk=rows)
        out = eng.logits(1)[0].float().cpu().numpy()
        eng.release(0)
        return out
    finally:
        eng.close()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n_prompt,rows", [(100, 128), (200, 256), (300, 128), (77, 80)])
def test_prefill_long_chunks(ckpt, wide, n_prompt, rows):
    """Chunks of 80 .. 256 rows: W4 MFMA GEMM (row tiles of 32 / 64 / 128, split-K where the tiles alone cannot fill the
    chip), paged FlashAttention with ragged last query blocks and -- for the later chunks of the 300-token prompt -- a
    non-empty cached context.  HIP must sit as close to the float64 truth as the bf16 oracle (tile-GEMM semantics) does."""
    if wide:
        cfg, w = WIDE_CFG, O.make_qwen3_weights(WIDE_CFG, seed=5, sigma=0.03)
        model = to_mlx_shaped(WIDE_CFG, w)
    else:
        cfg, (w, model) = TINY_CFG, ckpt
    prompt = [int(t) for t in np.random.default_rng(n_prompt).integers(1, cfg["vocab_size"], size=n_prompt)]
    got = _prefill_logits(model, prompt, rows)
    want = O.OracleQwen3(cfg, w).forward(prompt)[0, -1]
    truth = O.TruthQwen3(cfg, w).forward(prompt)[0, -1]
    check_against_truth(got[None], want[None], truth[None], what=f"prefill {'WIDE' if wide else 'TINY'} {n_prompt} tokens, chunks of {rows}")


def test_engine_verify_matches_oracle_rows(ckpt, engine, err):
    """tl_engine_verify: rows of one multi-token call (L <= 8 through the paged decode kernel) give the oracle's greedy
    continuation at every position, and rewinding the rejected suffix restores the cache for normal decoding."""
    w, _ = ckpt
    prompt = prompt_ids(11, seed=5)
    extra = prompt_ids(5, seed=6)
    model = O.OracleQwen3(TINY_CFG, w)
    want = model.forward(prompt + extra, logits_to_keep=None)[0]  # logits of every position
    engine.begin(0)
    engine.prefill(0, prompt)
    got = engine.verify(0, extra)
    assert engine.context_len(0) == len(prompt) + len(extra)
    for i in range(len(extra)):  # every row's greedy id: the oracle's argmax, or a provable near-tie with it
        assert_near_greedy(want[len(prompt) + i], got[i], err["hip_vs_oracle"], f"verify row {i}")
    # drop the last 3 verified tokens again and decode on: same result as a sequence that never saw them
    engine.rewind(0, 3)
    engine.set_token(0, extra[2])
    engine.decode(1, batch=1)
    after = engine.logits(1)[0].float().cpu().numpy()
    engine.release(0)
    ref = O.OracleQwen3(TINY_CFG, w).forward(prompt + extra[:3])[0, -1]
    truth = O.TruthQwen3(TINY_CFG, w).forward(prompt + extra[:3])[0, -1]
    check_against_truth(after[None], ref[None], truth[None], what="decode after verify + rewind, TINY")


@pytest.mark.parametrize("same_draft", [True, False])
def test_speculative_decoding_over_two_engines(ckpt, err, same_draft):
    """speculative_generate_ids: the result is a greedy continuation of the TARGET whatever the draft proposes, checked id
    by id against the oracle forward of the emitted sequence; an identical draft is accepted almost always, a different one
    rarely."""
    from tiny_llm_hip.engine import DecodeEngine, speculative_generate_ids

    w, model = ckpt
    draft_model = model if same_draft else to_mlx_shaped(TINY_CFG, O.make_qwen3_weights(TINY_CFG, seed=11, sigma=0.05))
    target = DecodeEngine(model, page_size=16, num_pages=64, max_batch=1, max_prefill_rows=64)
    draft = DecodeEngine(draft_model, page_size=16, num_pages=64, max_batch=1, max_prefill_rows=64)
    try:
        prompts = [prompt_ids(n, seed=300 + n) for n in (7, 19, 33, 12)]
        accepted, proposed, checked = 0, 0, 0
        for p in prompts:
            stats = {}
            spec = speculative_generate_ids(target, draft, p, 28, proposal_length=4, stats=stats)
            assert len(spec) == 28 and stats["target_calls"] <= 29
            accepted += stats["accepted"]
            proposed += stats["proposed"]
            # every emitted id must be the oracle's greedy choice given the ids emitted before it, or a provable near-tie
            # with it (the oracle's own margin to that id inside the HIP-vs-oracle band)
            rows = O.OracleQwen3(TINY_CFG, w).forward(p + spec, logits_to_keep=None)[0]
            for j, tok in enumerate(spec):
                row = rows[len(p) - 1 + j]
                assert_near_greedy(row, tok, err["hip_vs_oracle"], f"prompt of {len(p)} tokens, generated position {j}")
                checked += int(tok == int(np.argmax(row)))
        assert checked > 100, "most positions should simply be the oracle's argmax"
        rate = accepted / max(proposed, 1)
        assert (rate > 0.8) if same_draft else (rate < 0.5), f"acceptance rate {rate:.2f}"
        assert target.stats()["pages_in_use"] == 0 and draft.stats()["pages_in_use"] == 0
    finally:
        target.close()
        draft.close()


def test_engine_from_a_loaded_checkpoint_directory(ckpt, tmp_path):
    """tiny_llm_hip.load (the mlx_lm.load replacement) -> DecodeEngine: an MLX-format 4-bit checkpoint written to disk decodes
    bit-identically to the same weights handed over in memory, and the loaded tokenizer drives the id-level loop."""
    from checkpoint_fixture import write_checkpoint
    from tiny_llm_hip import load
    from tiny_llm_hip.engine import DecodeEngine

    w, in_memory = ckpt
    words = [f"w{i}" for i in range(TINY_CFG["vocab_size"] - 2)]
    model, tok = load(str(write_checkpoint(tmp_path / "ckpt", TINY_CFG, w, shards=2, vocab_words=words)))
    prompt = tok.encode("w5 w17 w400 w3 w99", add_special_tokens=False)
    assert prompt == [7, 19, 402, 5, 101]
    outs = []
    for m in (model, in_memory):
        eng = DecodeEngine(m, page_size=16, num_pages=16, max_batch=1, max_prefill_rows=64)
        try:
            ids = eng.generate(prompt, 12)
            outs.append((ids, eng.logits(1).clone()))
        finally:
            eng.close()
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])
    assert isinstance(tok.decode(outs[0][0]), str)


def test_cli_entry_points_on_a_written_checkpoint(ckpt, tmp_path, capsys):
    """main.py (greedy, sampled, speculative; engine and op-by-op solutions) and batch_main.py on a checkpoint directory."""
    from checkpoint_fixture import write_checkpoint
    import batch_main
    import main as cli

    w, _ = ckpt
    words = [f"w{i}" for i in range(TINY_CFG["vocab_size"] - 2)]
    path = str(write_checkpoint(tmp_path / "ckpt", TINY_CFG, w, vocab_words=words))
    base = ["--model", path, "--prompt", "w5 w17 w400 w3", "--raw-prompt", "--max-new-tokens", "10"]
    greedy = cli.main(base)
    assert isinstance(greedy, str) and len(greedy.split()) <= 10
    spec = cli.main(base + ["--draft-model", path, "--proposal-length", "3"])
    assert spec.split()[:3] == greedy.split()[:3]
    sampled = cli.main(base + ["--sampler-temp", "0.8", "--sampler-top-k", "20", "--sampler-top-p", "0.9"])
    assert isinstance(sampled, str)
    ops = cli.main(base + ["--solution", "ops"])
    assert ops.split()[:3] == greedy.split()[:3]
    chat = cli.main(["--model", path, "--prompt", "w5 w6", "--max-new-tokens", "4"])  # through the chat template
    assert isinstance(chat, str)
    prompts = tmp_path / "prompts.txt"
    prompts.write_text("w5 w6 w7\nw8 w9\nw10 w11 w12 w13\n")
    done = batch_main.main(["--model", path, "--batch-size", "2", "--prefill-step", "16", "--max-seq-len", "24",
                            "--raw-prompts", "--prompts-file", str(prompts)])
    assert sorted(i for i, _ in done) == [0, 1, 2]
    capsys.readouterr()


def test_fork_shares_prefix_pages_and_branches_decode_independently(ckpt, err):
    """tl_engine_fork: a forked slot continues exactly like its source (same logits), full pages are shared and a partial
    tail page is copied (page accounting), the two branches then take different tokens without disturbing each other
    (each checked against a sequence that was prefilled from scratch), rewinding into a shared page copies it first, and
    releasing in either order returns every page."""
    from tiny_llm_hip.engine import DecodeEngine

    w, model = ckpt
    eng = DecodeEngine(model, page_size=16, num_pages=32, max_batch=3, max_prefill_rows=64)
    try:
        prompt = prompt_ids(37, seed=41)          # 2 full pages + 5 tokens
        eng.begin(0)
        eng.prefill(0, prompt)
        base_pages = eng.stats()["pages_in_use"]
        assert base_pages == 3
        eng.fork(0, 1)
        assert eng.stats()["pages_in_use"] == base_pages + 1 and eng.context_len(1) == len(prompt)
        eng.decode(1, batch=2)                    # both consume the same pending token
        both = eng.logits(2)
        assert torch.equal(both[0], both[1])
        first = eng.read_tokens(0, 2)             # [token after the prompt, token after that]
        # branch: slot 0 keeps its own continuation, slot 1 is forced onto another token
        other = (first[1] + 17) % TINY_CFG["vocab_size"]
        eng.set_token(1, other)
        eng.decode(4, batch=2)
        branch0, branch1 = eng.read_tokens(0, 4), eng.read_tokens(1, 4)
        fresh = DecodeEngine(model, page_size=16, num_pages=32, max_batch=1, max_prefill_rows=64)
        try:
            # all 4 ids of both branches: an unshared sequence with the same history must make the same choice (or hold a
            # provable near-tie with it: the forked batch of 2 rows runs another GEMV instantiation than the solo row)
            for history, got in ((prompt + first, branch0), (prompt + [first[0], other], branch1)):
                fresh.begin(0)
                fresh.prefill(0, history[:-1], want_logits=False)
                fed = [history[-1]] + got[:-1]
                for j, tok in enumerate(got):
                    fresh.set_token(0, fed[j])
                    fresh.decode(1, batch=1)
                    row = fresh.logits(1)[0].float().cpu().numpy()
                    assert_near_greedy(row, tok, err["hip_vs_hip"], f"branch id {j} vs an unshared sequence")
                fresh.release(0)
        finally:
            fresh.close()
        # rewind slot 1 back into the shared second page: it must get a private copy before it appends again
        ctx1 = eng.context_len(1)
        eng.rewind(1, ctx1 - 20)
        shared_before = eng.stats()["pages_in_use"]
        eng.set_token(1, prompt[20])
        eng.decode(1, batch=2)
        solo = DecodeEngine(model, page_size=16, num_pages=32, max_batch=1, max_prefill_rows=64)
        try:
            solo.begin(0)
            solo.prefill(0, prompt[:21])
            # the copied page must hold the same K/V as a from-scratch prefill: two HIP paths (decode step in a batch of 2
            # vs the last row of a prefill), band 3 E
            delta = np.abs(solo.logits(1)[0].float().cpu().numpy() - eng.logits(2)[1].float().cpu().numpy()).max()
            assert float(delta) <= err["gemv_vs_gemm"], f"logits after the copy-on-write rewind differ by {delta}"
            solo.release(0)
        finally:
            solo.close()
        assert eng.stats()["pages_in_use"] <= shared_before + 1
        # slot 0 still decodes as before the rewind of slot 1 (its pages were not touched)
        eng.release(1)
        eng.fork(0, 2)
        eng.release(0)                            # the source goes first: shared pages must survive for slot 2
        eng.decode(2, batch=3)
        assert eng.context_len(2) > len(prompt)
        eng.release(2)
        st = eng.stats()
        assert st["pages_in_use"] == 0 and st["pages_free"] == 32
    finally:
        eng.close()


def test_packed_prefill_of_several_slots(ckpt, err):
    """tl_engine_prefill_packed: several slots' chunks through ONE multi-token pass (projections over the concatenated rows,
    RoPE / KV append / paged FlashAttention per sequence).  Every prompt's last-row logits are held against the oracle and
    the float64 truth exactly like a solo prefill's; prompts split over two packed calls with different partners (a cached
    context plus a fresh prompt in the same pass) and a following batched decode step must agree with the same requests
    served alone; all-or-nothing argument checks."""
    from tiny_llm_hip.engine import DecodeEngine

    w, model = ckpt
    prompts = [prompt_ids(n, seed=700 + n) for n in (100, 37, 200, 9)]
    oracle_rows = [O.OracleQwen3(TINY_CFG, w).forward(p)[0, -1] for p in prompts]
    truth_rows = [O.TruthQwen3(TINY_CFG, w).forward(p)[0, -1] for p in prompts]
    eng = DecodeEngine(model, page_size=16, num_pages=128, max_batch=4, max_prefill_rows=512)
    try:
        # 1. four whole prompts in one pass
        for s in range(4):
            eng.begin(s)
        eng.prefill_packed([(s, prompts[s], True) for s in range(4)])
        got = eng.logits(4).float().cpu().numpy()
        for s in range(4):
            check_against_truth(got[s][None], oracle_rows[s][None], truth_rows[s][None], what=f"packed prefill, prompt {s} ({len(prompts[s])} tokens)")
        assert [eng.context_len(s) for s in range(4)] == [len(p) for p in prompts]
        first = eng.read_pending(4)
        for s in range(4):
            assert_near_greedy(got[s], first[s], err["hip_vs_oracle"], f"packed prefill first token of prompt {s}")
        eng.decode(1, batch=4)
        batch_rows = eng.logits(4).float().cpu().numpy()
        for s in range(4):
            eng.release(s)
        # 2. the same requests alone (sequential prefill, same first token fed)
        for s in range(4):
            eng.begin(0)
            eng.prefill(0, prompts[s], chunk=512)
            eng.set_token(0, first[s])
            eng.decode(1, batch=1)
            solo = eng.logits(1)[0].float().cpu().numpy()
            eng.release(0)
            assert float(np.abs(solo - batch_rows[s]).max()) <= err["hip_vs_hip"], f"decode step after a packed prefill, prompt {s}"
        # 3. prompts split over two passes with different partners
        for s in range(3):
            eng.begin(s)
        eng.prefill_packed([(0, prompts[0][:60], False), (1, prompts[1], True)])
        eng.prefill_packed([(2, prompts[2], True), (0, prompts[0][60:], True)])  # slot 0 continues behind a fresh prompt
        got2 = eng.logits(2).float().cpu().numpy()  # rows in chunk order: prompt 2, prompt 0
        check_against_truth(got2[0][None], oracle_rows[2][None], truth_rows[2][None], what="packed prefill, second pass, fresh prompt")
        check_against_truth(got2[1][None], oracle_rows[0][None], truth_rows[0][None], what="packed prefill, prompt continued in a second pass")
        # 4. argument checks leave everything as it was
        ctx_before = [eng.context_len(s) for s in range(3)]
        free_before = eng.stats()["pages_free"]
        for bad in ([(0, [1, 2], True), (0, [3], True)], [(3, [1], True)], [(0, list(range(1, 400)), True), (1, list(range(1, 200)), True)]):
            with pytest.raises(RuntimeError):
                eng.prefill_packed(bad)
        assert [eng.context_len(s) for s in range(3)] == ctx_before and eng.stats()["pages_free"] == free_before
        for s in range(3):
            eng.release(s)
        assert eng.stats()["pages_in_use"] == 0
    finally:
        eng.close()


@pytest.mark.parametrize("n_prompt", [5, 37, 200])
def test_one_sequence_packed_prefill_equals_solo_prefill(ckpt, n_prompt):
    """A packed prefill of one sequence runs the same layer pass as a solo prefill: the last-row logits, the pending token and
    the logits of the following decode step must be bit-identical on the same engine."""
    from tiny_llm_hip.engine import DecodeEngine

    prompt = prompt_ids(n_prompt, seed=900 + n_prompt)
    eng = DecodeEngine(ckpt[1], page_size=16, num_pages=64, max_batch=1, max_prefill_rows=256)
    try:
        runs = []
        for packed in (False, True):
            eng.begin(0)
            if packed:
                eng.prefill_packed([(0, prompt, True)])
            else:
                eng.prefill(0, prompt)
            first, pending = eng.logits(1), eng.read_pending(1)
            eng.decode(1, batch=1, use_graph=False)
            runs.append((first, pending, eng.logits(1)))
            eng.release(0)
        (solo_first, solo_pending, solo_next), (packed_first, packed_pending, packed_next) = runs
        assert torch.equal(solo_first, packed_first), "last-row logits of the prefill"
        assert solo_pending == packed_pending, "pending token after the prefill"
        assert torch.equal(solo_next, packed_next), "logits of the decode step after the prefill"
    finally:
        eng.close()


NORM_CFG = dict(hidden_size=2560, num_hidden_layers=3, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=1024,
                vocab_size=2048, rope_theta=1000000, rms_norm_eps=1e-6, max_position_embeddings=4096, tie_word_embeddings=True)


@pytest.mark.parametrize("cfg_name", ["wide", "2304", "2560", "4096"])
@pytest.mark.parametrize("n_prompt,rows", [(300, 128), (77, 80), (40, 64), (600, 256), (130, 128)])
def test_prefill_reduce_norm_fusion_is_bit_identical(ckpt, monkeypatch, n_prompt, rows, cfg_name):
    """The split-K residual reduction that also writes the RMSNorm of the rows it completes (csrc/qmm.hip splitk_reduce_residual_norm_kernel: wo -> post-attention
    norm, w_down -> the NEXT layer's input norm) against the two launches it replaces (engine option "prefill_reduce_norm" = 0): the same expressions on the same
    values in the same order, so every logit must be IDENTICAL -- hidden sizes of 2,304 / 2,560 / 4,096 (the range the fusion takes: tl_rms_norm's 256-thread
    kernel, whose threads 0 .. dim / 8 - 257 add a second chunk), 1,280 (not fused: the control), three layers so that a fused input norm feeds a layer,
    chunks that leave ragged last passes."""
    cfg = WIDE_CFG if cfg_name == "wide" else dict(NORM_CFG, hidden_size=int(cfg_name))
    model = to_mlx_shaped(cfg, O.make_qwen3_weights(cfg, seed=5, sigma=0.03))
    prompt = [int(t) for t in np.random.default_rng(n_prompt).integers(1, cfg["vocab_size"], size=n_prompt)]
    monkeypatch.setenv("TL_ENGINE_OPTIONS", "prefill_reduce_norm=0")
    separate = _prefill_logits(model, prompt, rows)
    monkeypatch.setenv("TL_ENGINE_OPTIONS", "prefill_reduce_norm=1")
    fused = _prefill_logits(model, prompt, rows)
    assert np.array_equal(separate, fused), f"{int((separate != fused).sum())} logits differ, max {np.abs(separate - fused).max()}"


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n_prompt,rows", [(300, 512), (77, 80), (40, 64), (600, 256)])
def test_prefill_gemm_fused_epilogue_is_bit_identical(ckpt, monkeypatch, n_prompt, rows, wide):
    """Residual add / SwiGLU folded into the prefill GEMM's store (unsplit reduction) or into its split-K reduction
    (csrc/qmm.hip qmm_bf16_epilogue) against the separate elementwise launches (engine option "gemm_fused_epilogue" = 0): the epilogue is
    applied to the same bf16-rounded matmul result with the same expressions, so every logit must be IDENTICAL -- over chunk
    lengths that exercise row tiles of 32 / 64 / 128 and both the split and the unsplit reduction."""
    if wide:
        cfg, model = WIDE_CFG, to_mlx_shaped(WIDE_CFG, O.make_qwen3_weights(WIDE_CFG, seed=5, sigma=0.03))
    else:
        cfg, model = TINY_CFG, ckpt[1]
    prompt = [int(t) for t in np.random.default_rng(n_prompt).integers(1, cfg["vocab_size"], size=n_prompt)]
    monkeypatch.setenv("TL_ENGINE_OPTIONS", "gemm_fused_epilogue=0")
    separate = _prefill_logits(model, prompt, rows)
    monkeypatch.setenv("TL_ENGINE_OPTIONS", "gemm_fused_epilogue=1")
    fused = _prefill_logits(model, prompt, rows)
    assert np.array_equal(separate, fused), f"{int((separate != fused).sum())} logits differ, max {np.abs(separate - fused).max()}"
