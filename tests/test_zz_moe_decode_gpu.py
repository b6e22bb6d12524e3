"""GPU tier: the decode-shaped route of a MoE MLP's experts (tl_moe_experts_rows_decode, csrc/moe_decode.h; in the engine
tl_engine_set_moe_decode / DecodeEngine(moe_decode_rows=...)): gate | up and down -- one read of an expert for all rows that name it,
MFMA products in the GEMV's arithmetic -- against the oracle's GEMV and the float64 chain, stage by stage on the device's own input
to each stage, and the engine's graph-replayed decode steps on the route against the oracle and the float64 truth."""

import functools

import numpy as np
import pytest
import torch

import moe_oracle as MO
from helpers import assert_rounded_close, check_against_truth
from oracle import tiny_oracle as O
from test_engine_moe_gpu import REAL_COUNT_SEEDS, REAL_COUNTS, _moe_checkpoint, prompt_and_forced, reference_side
from test_zz_moe_gpu import expert_stack, gemv_stage, host, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
STAGE_CASES = [(*shape, rows) for shape in [(16, 16, 256, 128), (8, 4, 1664, 384), (128, 8, 256, 128), (32, 8, 2048, 768)]
               for rows in (1, 2, 17, 64) if shape != (32, 8, 2048, 768) or rows in (1, 17)]


def own_ids(rng, rows, E, k):
    """Raw ids [rows, k].  Row 0 names expert 1 k times; the other slots, shuffled, hold as far as they reach: expert 0, one id past the
    range (E + 5, clamped to E - 1), E - 1 itself, expert 2 exactly 16 times, expert 3 17 times, at 64 rows expert 4 64 times, then
    experts of a pool of at most 11 outside {2, 3, 4, 5}: expert 5 gets no row."""
    wanted = [0, E + 5, E - 1] + [2] * 16 + [3] * 17 + [4] * (64 if rows == 64 else 0)
    free = (rows - 1) * k
    pool = np.array([e for e in range(E) if e not in (2, 3, 4, 5)][:10] + [E - 1])
    rest = np.concatenate([wanted[:free], pool[rng.integers(0, len(pool), size=max(0, free - len(wanted)))]]).astype(np.int32)
    return np.concatenate([np.full(k, 1, dtype=np.int32), rng.permutation(rest)]).reshape(rows, k)


@pytest.mark.parametrize("E,k,D,I,rows", STAGE_CASES)
def test_decode_experts_stage_by_stage_and_against_the_truth(E, k, D, I, rows):
    """act: as close to the float64 chain as the bf16 oracle chain (oracle.quantized_matmul of gate and up, moe_oracle.silu_mul) is
    (helpers.check_against_truth).  y: the oracle's GEMV of the device's own act, one bf16 ulp + ACC_FLOOR * sum |a| |w| (the GEMV
    route's allowance).  out: bit-equal to moe_oracle.combine of the device's y.  The block: check_against_truth.  A second call: the
    same bytes."""
    import tiny_llm_ext_hip as ext

    stack = expert_stack(E, D, I)
    rng = np.random.default_rng(E * 1000 + k * 100 + rows)
    ids = own_ids(rng, rows, E, k)
    flat = np.clip(ids, 0, E - 1).reshape(-1)
    counts = np.bincount(flat, minlength=E)
    assert (ids[0] == 1).all() and (rows == 1 or ((ids > E - 1).any() and counts[0] > 0 and counts[E - 1] > 1 and counts[5] == 0))
    assert rows < 17 or (counts[2] == 16 and counts[3] == 17 and counts[4] == (64 if rows == 64 else 0))
    scores = MO.renormalise(O.bf16(rng.uniform(0.02, 0.3, size=(rows, k)).astype(np.float32)))
    xn = O.bf16(rng.standard_normal((rows, D)).astype(np.float32))
    h = O.bf16(rng.standard_normal((rows, D)).astype(np.float32) * np.float32(0.25))
    args = (to_dev(xn), to_dev(h), torch.from_numpy(ids).to(DEV), to_dev(scores), stack.dev["gate"], stack.dev["up"], stack.dev["down"])
    out_t, stages = ext.moe_experts_rows_decode(*args)
    torch.cuda.synchronize()
    got, out = {name: host(t) for name, t in stages.items()}, host(out_t)
    what = f"decode experts E={E} k={k} hidden={D} I={I} rows={rows}"

    a = np.repeat(xn, k, axis=0)  # expert row r reads activation row r // k
    (want_gate, gate64, _), (want_up, up64, _) = (gemv_stage(stack, name, a, flat) for name in ("gate", "up"))
    act_o = MO.silu_mul(want_gate, want_up)
    act64 = gate64 / (1.0 + np.exp(-gate64)) * up64
    check_against_truth(got["act"], act_o, act64, what=what + ": act")

    want_y, _, floor = gemv_stage(stack, "down", got["act"], flat)
    assert_rounded_close(got["y"], want_y, "bf16", ulps=1.0, floor=floor, what=what + ": down")

    want_out = MO.combine(got["y"].reshape(rows, k, D), scores, h)
    assert np.array_equal(O.bf16_bits(out), O.bf16_bits(want_out)), f"{what}: combine {int((out != want_out).sum())} elements differ"

    y_o, _, _ = gemv_stage(stack, "down", act_o, flat)
    oracle_out = MO.combine(y_o.reshape(rows, k, D), scores, h)
    y64 = np.zeros((rows * k, D))
    for e in np.unique(flat):
        y64[flat == e] = act64[flat == e] @ stack.dense64("down", int(e)).T
    truth = h.astype(np.float64) + (y64.reshape(rows, k, D) * scores.astype(np.float64)[..., None]).sum(axis=1)
    check_against_truth(out, oracle_out, truth, what=what)

    out2, stages2 = ext.moe_experts_rows_decode(*args)
    torch.cuda.synchronize()
    assert torch.equal(out2, out_t) and all(torch.equal(stages2[name], stages[name]) for name in stages), what + ": a second call differs"


@pytest.fixture(scope="module")
def reference_case(tmp_path_factory):
    """which -> (cfg, model, prompt, forced, the CPU side: test_engine_moe_gpu.reference_side), computed once per checkpoint."""
    @functools.lru_cache(maxsize=None)
    def case(which):
        cfg, model = _moe_checkpoint(tmp_path_factory, "decode" + which, {"128x8": 22, "60x4": 23}[which], **REAL_COUNTS[which])
        prompt, forced = prompt_and_forced(cfg, 23, REAL_COUNT_SEEDS[which, 23])
        return cfg, model, prompt, forced, reference_side(cfg, model._oracle_weights, prompt, forced)

    return case


def engine_run(model, seqs, decode_rows):
    """seqs: [(prompt, forced)], decoded together.  -> (per sequence the logits after each forced token, the first one's prefill logits,
    the route's state, the engine's stats)."""
    from tiny_llm_hip.engine import DecodeEngine

    eng = DecodeEngine(model, page_size=16, num_pages=32, max_batch=2, max_prefill_rows=64, moe_decode_rows=decode_rows)
    try:
        for slot, (prompt, _) in enumerate(seqs):
            eng.begin(slot)
            eng.prefill(slot, prompt, chunk=64)
            first = eng.logits(1)[0].float().cpu().numpy() if slot == 0 else first
        got = [[] for _ in seqs]
        for s in range(len(seqs[0][1])):
            for slot, (_, forced) in enumerate(seqs):
                eng.set_token(slot, forced[s])
            eng.decode(1, batch=len(seqs))
            for slot, lg in enumerate(eng.logits(len(seqs)).float().cpu().numpy()):
                got[slot].append(lg)
        return [np.stack(g) for g in got], first, eng.moe_decode_state(), eng.stats()
    finally:
        eng.close()


@pytest.mark.parametrize("decode_rows,calls", [(1, 12), (0, 0)])
@pytest.mark.parametrize("which", ["128x8", "60x4"])
def test_engine_decode_steps_on_the_route_against_the_oracle_and_the_float64_truth(reference_case, which, decode_rows, calls):
    """23 prompt tokens, six teacher-forced decode steps through graph replay, the bar of test_engine_moe_gpu.oracle_and_truth_case.
    calls: six steps x two sparse layers with the route on from one row, none with it off."""
    _, model, prompt, forced, (want, exact, counted) = reference_case(which)
    (steps,), first, state, stats = engine_run(model, [(prompt, forced)], decode_rows)
    assert state == {"min_rows": decode_rows, "calls": calls}
    assert stats["graph_replays"] + stats["graph_captures"] >= len(forced), "the decode steps did not go through captured graphs"
    assert sum(counted) >= 2 * len(counted) // 3 + 1, f"too many toss-up selections to compare: {counted}"
    keep = np.asarray(counted)
    check_against_truth(np.concatenate([first[None], steps])[keep], want[keep], exact[keep], what=f"engine, decode route from {decode_rows} rows, {which}")


@pytest.mark.parametrize("which", ["128x8", "60x4"])
def test_two_sequences_on_the_route_decode_together_as_they_do_alone(reference_case, which):
    """Each sequence of a two-row step stays within two bf16 steps of its single-sequence run on the same route."""
    cfg, model = reference_case(which)[:2]
    rng = np.random.default_rng(5)
    seqs = [([int(t) for t in rng.integers(2, cfg["vocab_size"], size=n)], [int(t) for t in rng.integers(2, cfg["vocab_size"], size=5)]) for n in (9, 30)]
    together, _, state, _ = engine_run(model, seqs, 1)
    assert state["calls"] == 5 * 2
    for slot, seq in enumerate(seqs):
        want = engine_run(model, [seq], 1)[0][0]
        step = 2.0 ** -7 * max(1.0, float(np.abs(want).max()))
        assert float(np.abs(together[slot] - want).max()) <= 2 * step, f"{which}, sequence {slot}: batched and single-sequence logits differ"
