"""GPU tier: Qwen3-MoE layers inside the fused engine (tl_engine_set_moe_layer; reference: the Week-3 model builds a Moe block for
every sparse layer, src/tiny_llm_ref/qwen3_week3.py:209-214, 258-272; the block is moe.py:39-89).

A 3-layer checkpoint whose layers 1 and 2 are sparse (4 experts, top 2, renormalised scores; layer 0 dense through mlp_only_layers)
is written to disk in the mlx_lm layout, loaded by tiny_llm_hip.load, and run two ways on the same weights: op by op through the
host mirror (Qwen3ModelWeek3 with tiny_llm_hip.Moe blocks -- held against the numpy oracle's moe_block by tests/test_ops_gpu.py and
against the reference's own classes through the facade by tests/test_loader_cpu.py) and through the fused engine, whose MoE layers
run the same op sequence inside the captured step.  Teacher-forced, so both sides see the same history: the logits must agree
within a few bf16 steps at every position, prefill by GEMV rows (<= 8), by GEMM rows, and chunked; decode by graph replay."""

import numpy as np
import pytest
import torch

from helpers import TINY_CFG

pytestmark = pytest.mark.gpu


def _moe_checkpoint(tmp_path_factory, name, seed, **overrides):
    from checkpoint_fixture import MOE_CFG_OVERRIDES, make_moe_weights, write_checkpoint
    from tiny_llm_hip import load

    cfg = dict(TINY_CFG, **MOE_CFG_OVERRIDES)
    cfg.update(overrides)
    w = make_moe_weights(cfg, seed=seed)
    words = [f"w{i}" for i in range(cfg["vocab_size"] - 2)]
    path = write_checkpoint(tmp_path_factory.mktemp(name) / "ckpt", cfg, w, vocab_words=words)
    model, _ = load(str(path))
    model._oracle_weights = w  # the numpy weight dict the checkpoint was written from (oracle / truth side of the tests below)
    return cfg, model


@pytest.fixture(scope="module")
def moe_model(tmp_path_factory):
    return _moe_checkpoint(tmp_path_factory, "moe", 21)


# The expert counts the MoE kernels were written for (the layers stay 256 wide, the experts 128: what is new is the router's width, eight
# expert rows per token, the tie rule at 128 bf16 probabilities): Qwen3-MoE's 128 experts, top 8, renormalised ...
REAL_COUNTS = {"128x8": dict(num_experts=128, num_experts_per_tok=8, moe_intermediate_size=128, norm_topk_prob=True),
               # ... and Qwen1.5/2-MoE's 60 experts, top 4, the probabilities as they are
               "60x4": dict(num_experts=60, num_experts_per_tok=4, moe_intermediate_size=128, norm_topk_prob=False)}


@pytest.fixture(scope="module")
def moe_model_128(tmp_path_factory):
    return _moe_checkpoint(tmp_path_factory, "moe128", 22, **REAL_COUNTS["128x8"])


@pytest.fixture(scope="module")
def moe_model_60(tmp_path_factory):
    return _moe_checkpoint(tmp_path_factory, "moe60", 23, **REAL_COUNTS["60x4"])


def mirror_logits(model, prompt, forced):
    from tiny_llm_hip import Moe, Qwen3ModelWeek3

    week3 = Qwen3ModelWeek3(model, page_size=16)
    assert [type(layer.mlp).__name__ for layer in week3.layers_inner] == ["Qwen3MLP", "Moe", "Moe"]
    assert isinstance(week3.layers_inner[1].mlp, Moe)
    cache = week3.create_kv_cache()
    try:
        toks = torch.tensor([prompt], dtype=torch.int32, device="cuda")
        out = [week3(toks, 0, cache, logits_to_keep=1)[0, -1].float().cpu().numpy()]
        offset = len(prompt)
        for tok in forced:
            t = torch.tensor([[tok]], dtype=torch.int32, device="cuda")
            out.append(week3(t, offset, cache, logits_to_keep=1)[0, -1].float().cpu().numpy())
            offset += 1
        return np.stack(out)
    finally:
        for c in cache:
            c.release()


def engine_logits(model, prompt, forced, chunk, batch_slot=0):
    from tiny_llm_hip.engine import DecodeEngine

    eng = DecodeEngine(model, page_size=16, num_pages=32, max_batch=2, max_prefill_rows=64)
    try:
        eng.begin(batch_slot)
        eng.prefill(batch_slot, prompt, chunk=chunk)
        got = [eng.logits(1)[0].float().cpu().numpy()]
        for tok in forced:
            eng.set_token(batch_slot, tok)
            eng.decode(1, batch=1)
            got.append(eng.logits(1)[0].float().cpu().numpy())
        stats = eng.stats()
        eng.release(batch_slot)
        return np.stack(got), stats
    finally:
        eng.close()


@pytest.mark.parametrize("n_prompt,chunk", [(5, 64), (23, 64), (50, 16)])
def test_fused_engine_with_moe_layers_matches_the_op_by_op_model(moe_model, n_prompt, chunk):
    cfg, model = moe_model
    rng = np.random.default_rng(n_prompt)
    prompt = [int(t) for t in rng.integers(2, cfg["vocab_size"], size=n_prompt)]
    forced = [int(t) for t in rng.integers(2, cfg["vocab_size"], size=6)]
    want = mirror_logits(model, prompt, forced)
    got, stats = engine_logits(model, prompt, forced, chunk)
    assert stats["graph_replays"] + stats["graph_captures"] >= len(forced), "the decode steps did not go through captured graphs"
    assert np.isfinite(got).all()
    step = 2.0 ** -7 * max(1.0, float(np.abs(want).max()))  # one bf16 step of the largest logit
    worst = float(np.abs(got - want).max())
    # the two paths share every expert kernel; they differ where the dense paths differ (fused GEMV against op-by-op launches,
    # the fused attention) and in the softmax / accumulation order of the routing arithmetic
    assert worst <= 4 * step, f"logits {worst / step:.1f} bf16 steps apart (prompt {n_prompt}, chunk {chunk})"
    assert (np.argmax(got, -1) == np.argmax(want, -1)).mean() >= 0.8, "greedy ids mostly differ"


def test_moe_layers_must_be_attached_before_the_first_step(moe_model):
    """tl_engine_set_moe_layer after a prefill is refused (captured graphs and workspaces are fixed by then)."""
    from tiny_llm_hip.engine import DecodeEngine

    cfg, model = moe_model
    eng = DecodeEngine(model, page_size=16, num_pages=8, max_batch=1, max_prefill_rows=16)
    try:
        eng.begin(0)
        eng.prefill(0, [5, 6, 7])
        with pytest.raises(RuntimeError, match="before the first prefill"):
            eng._attach_moe(1, model.model.layers[1].mlp, model.args)
    finally:
        eng.close()


def two_sequences_together_and_alone(cfg, model):
    from tiny_llm_hip.engine import DecodeEngine

    rng = np.random.default_rng(5)
    prompts = [[int(t) for t in rng.integers(2, cfg["vocab_size"], size=n)] for n in (9, 30)]
    forced = [[int(t) for t in rng.integers(2, cfg["vocab_size"], size=5)] for _ in prompts]
    alone = [engine_logits(model, p, f, 64)[0] for p, f in zip(prompts, forced)]
    eng = DecodeEngine(model, page_size=16, num_pages=32, max_batch=2, max_prefill_rows=64)
    try:
        for slot, p in enumerate(prompts):
            eng.begin(slot)
            eng.prefill(slot, p, chunk=64)
        got = [[], []]
        for s in range(5):
            for slot in range(2):
                eng.set_token(slot, forced[slot][s])
            eng.decode(1, batch=2)
            lg = eng.logits(2).float().cpu().numpy()
            for slot in range(2):
                got[slot].append(lg[slot])
        for slot in range(2):
            eng.release(slot)
    finally:
        eng.close()
    for slot in range(2):
        want = alone[slot][1:]
        have = np.stack(got[slot])
        step = 2.0 ** -7 * max(1.0, float(np.abs(want).max()))
        assert float(np.abs(have - want).max()) <= 2 * step, f"sequence {slot}: batched and single-sequence logits differ"


def test_two_sequences_decode_together_as_they_do_alone(moe_model):
    """Batched decode over MoE layers: rows x top_k expert rows in one grouped launch; each sequence's logits stay within two bf16
    steps of its own single-sequence run (the dense projections take the two-row GEMV plan) and free-running greedy ids repeat."""
    two_sequences_together_and_alone(*moe_model)


def test_two_sequences_decode_together_as_they_do_alone_at_128_experts(moe_model_128):
    """The same at 128 experts, eight per token: sixteen expert rows in each grouped launch of a step."""
    two_sequences_together_and_alone(*moe_model_128)


@pytest.mark.parametrize("n_prompt,chunk", [(5, 64), (7, 64), (23, 64)])
def test_fused_engine_with_moe_layers_against_the_oracle_and_the_float64_truth(moe_model, n_prompt, chunk):
    """The comparand of the first test is the HIP op-by-op model (the same expert kernels on both sides).  Here it is the CPU side: the
    numpy oracle with Qwen3-MoE layers (oracle.OracleQwen3 + moe_block: src/tiny_llm_ref/moe.py:39-89 inside qwen3_week3.py:55-121)
    and the float64 truth (oracle.TruthQwen3, pinned to transformers' Qwen3MoeForCausalLM by tests/test_truth_vs_transformers_cpu.py),
    teacher-forced on the same tokens.  The top-k choice is the model's one discontinuity: the truth is evaluated on the ORACLE's
    choice, and a position counts only where the truth's own choice is the same set of experts (a toss-up between the k-th and the
    (k+1)-th expert is not an error of either side); at least two thirds of the positions must count.  Bar: the engine sits as close to
    the truth as the bf16 oracle does (helpers.check_against_truth); 5 and 7 prompt tokens prefill by GEMV rows, 23 by the tile GEMM."""
    oracle_and_truth_case(*moe_model, n_prompt, chunk, seed=100 + n_prompt)


def reference_side(cfg, w, prompt, forced):
    """(bf16 oracle logits, float64 truth logits on the oracle's expert choice, which positions count) -- nothing here runs on a device.
    A position counts where (1) the truth's own choice is the oracle's set of experts in every sparse layer and (2) the oracle's k-th and
    (k+1)-th bf16 probabilities stand more than one bf16 step apart there: the engine's float32 softmax may round either of them one
    step the other way and select differently without being wrong."""
    from helpers import bf16_ulp
    from oracle import tiny_oracle as O

    oracle, truth = O.OracleQwen3(cfg, w), O.TruthQwen3(cfg, w)
    want = [oracle.forward(prompt)[0, -1]] + [oracle.forward([t])[0, -1] for t in forced]
    truth.forced_moe_ids = oracle.moe_ids
    exact = [truth.forward(prompt)[0, -1]] + [truth.forward([t])[0, -1] for t in forced]
    k = int(cfg["num_experts_per_tok"])

    def clear_of_a_tie(c):
        for calls in oracle.moe_probs.values():
            srt = np.sort(calls[c][-1])[::-1]
            if len(srt) > k and srt[k - 1] - srt[k] <= bf16_ulp(srt[k - 1]):
                return False
        return True

    # call c of a sparse layer = position c of the teacher-forced sequence (call 0: the prompt, its last token is the row compared)
    counted = [all(bool(calls[c]["same_choice"][-1]) for calls in truth.moe_margins.values()) and clear_of_a_tie(c) for c in range(len(forced) + 1)]
    return np.stack(want), np.stack(exact), counted


def prompt_and_forced(cfg, n_prompt, seed):
    rng = np.random.default_rng(seed)
    prompt = [int(t) for t in rng.integers(2, cfg["vocab_size"], size=n_prompt)]
    return prompt, [int(t) for t in rng.integers(2, cfg["vocab_size"], size=6)]


def oracle_and_truth_case(cfg, model, n_prompt, chunk, seed):
    from helpers import check_against_truth

    prompt, forced = prompt_and_forced(cfg, n_prompt, seed)
    got, stats = engine_logits(model, prompt, forced, chunk)
    assert stats["graph_replays"] + stats["graph_captures"] >= len(forced)
    want, exact, counted = reference_side(cfg, model._oracle_weights, prompt, forced)
    assert sum(counted) >= 2 * len(counted) // 3 + 1, f"too many toss-up selections to compare: {counted}"
    keep = np.asarray(counted)
    check_against_truth(np.asarray(got)[keep], want[keep], exact[keep],
                        what=f"fused engine with 2 MoE layers ({cfg['num_experts']} experts, top {cfg['num_experts_per_tok']}), prompt {n_prompt} "
                             f"(chunk {chunk}), {int(keep.sum())} of {len(keep)} positions")


# Prompt seeds for which the reference side ALONE (reference_side on the CPU, no device) counts at least 6 of the 7 positions: the
# two-thirds floor above stays a condition the comparison must meet, not a tolerance.  (All four count 7 of 7 there; of the seeds
# tried before them 128 experts counted 4 to 6.)
REAL_COUNT_SEEDS = {("128x8", 5): 355, ("128x8", 23): 573, ("60x4", 5): 305, ("60x4", 23): 323}


@pytest.mark.parametrize("n_prompt", [5, 23])
@pytest.mark.parametrize("which", ["128x8", "60x4"])
def test_fused_engine_at_real_expert_counts_against_the_oracle_and_the_float64_truth(moe_model_128, moe_model_60, which, n_prompt):
    """The oracle-and-truth test above at 128 experts top 8 (renormalised) and 60 experts top 4 (not): the router's 256-thread arg-max
    across waves, eight or four expert rows per token through the grouped GEMVs, the weighted sum over more than two terms (where a sum
    rounded after every add would be another operation).  5 prompt tokens prefill by GEMV rows, 23 by the tile GEMM."""
    cfg, model = moe_model_128 if which == "128x8" else moe_model_60
    assert (cfg["num_experts"], cfg["num_experts_per_tok"]) == tuple(int(v) for v in which.split("x"))
    oracle_and_truth_case(cfg, model, n_prompt, 64, seed=REAL_COUNT_SEEDS[which, n_prompt])
