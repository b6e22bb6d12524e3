"""GPU tier: the grouped-expert route of a MoE MLP's experts (tl_moe_experts_rows_grouped, csrc/moe_grouped.h; in the engine
tl_engine_set_moe_grouped / DecodeEngine(moe_grouped_rows=...)): the device's stable sort by expert held to numpy's, gate | up and
down -- MFMA tile GEMMs over rows that share an expert -- to the tile oracle (oracle.quantized_matmul_tile) and the float64 chain,
stage by stage on the device's own input to each stage, and the engine with the route on to the oracle and the float64 truth."""

import functools

import numpy as np
import pytest
import torch

import moe_oracle as MO
from helpers import assert_rounded_close, check_against_truth, w4_abs_dot
from oracle import tiny_oracle as O
from test_engine_moe_gpu import REAL_COUNT_SEEDS, REAL_COUNTS, _moe_checkpoint, prompt_and_forced, reference_side
from test_ops_gpu import ACC_FLOOR
from test_zz_moe_gpu import expert_stack, host, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    import tiny_llm_ext_hip as ext

    return ext


# rows as (multiple of the library's tile height TM, plus): 1, 9, TM + 1, 3 TM; the real widths run 9 and TM + 1 only
STAGE_CASES = [(*shape, rows) for shape in [(16, 16, 256, 128), (8, 4, 1664, 384), (128, 8, 256, 128), (32, 8, 2048, 768)]
               for rows in [(0, 1), (0, 9), (1, 1), (3, 0)] if shape != (32, 8, 2048, 768) or rows in [(0, 9), (1, 1)]]


def own_ids(rng, rows, E, k, TM):
    """Raw ids [rows, k].  Row 0 names expert 1 k times; the other slots, shuffled, hold as far as they reach: expert 0, one id past
    the range (E + 5, clamped to E - 1), expert 4 once, expert 2 exactly TM times, expert 3 TM + 1 times, then a few experts outside
    {2, 3, 4, 5}: expert 5 gets no row."""
    wanted = [0, E + 5, 4] + [2] * TM + [3] * (TM + 1)
    free = (rows - 1) * k
    pool = np.array([e for e in range(E) if e not in (2, 3, 4, 5)][:10] + [E - 1])
    rest = np.concatenate([wanted[:free], pool[rng.integers(0, len(pool), size=max(0, free - len(wanted)))]]).astype(np.int32)
    return np.concatenate([np.full(k, 1, dtype=np.int32), rng.permutation(rest)]).reshape(rows, k)


def tile_stage(stack, name, a, flat):
    """(oracle.quantized_matmul_tile of rows `a` each against its own expert, the allowance's floor ACC_FLOOR * sum |a| |w|)."""
    out_dim = stack.dev[name][0].shape[1]
    want, floor = np.zeros((len(flat), out_dim), dtype=np.float32), np.zeros((len(flat), out_dim))
    for e in np.unique(flat):
        sel = np.flatnonzero(flat == e)
        packed, s, z = stack.host_w4(name, int(e))
        want[sel] = O.quantized_matmul_tile(s, z, a[sel], packed)
        floor[sel] = ACC_FLOOR * w4_abs_dot(a[sel], packed, s, z, "bf16")
    return want, floor


def dense64_stage(stack, name, a64, flat):
    out = np.zeros((len(flat), stack.dev[name][0].shape[1]))
    for e in np.unique(flat):
        sel = np.flatnonzero(flat == e)
        out[sel] = a64[sel] @ stack.dense64(name, int(e)).T
    return out


@pytest.mark.parametrize("E,k,D,I,rows", STAGE_CASES)
def test_grouped_experts_stage_by_stage_and_against_the_truth(ext, E, k, D, I, rows):
    """perm / offsets: numpy's stable sort of the clamped ids and the cumulative counts, exact.  act: as close to the float64 chain
    as the bf16 tile-oracle chain (tile GEMMs of gate and up, then moe_oracle.silu_mul) is (helpers.check_against_truth, TRUTH_FACTOR).
    y: the tile oracle of the device's own act, one bf16 ulp + ACC_FLOOR * sum |a| |w| (the tile GEMM's allowance in test_ops_gpu).
    out: bit-equal to moe_oracle.combine of the device's y.  The block: check_against_truth.  A second call: the same bytes."""
    TM = ext.lib().tl_moe_grouped_tile_rows()
    rows = rows[0] * TM + rows[1]
    stack = expert_stack(E, D, I)
    rng = np.random.default_rng(E * 1000 + k * 100 + rows)
    ids = own_ids(rng, rows, E, k, TM)
    flat = np.clip(ids, 0, E - 1).reshape(-1)
    counts = np.bincount(flat, minlength=E)
    assert (ids[0] == 1).all() and (rows == 1 or ((ids > E - 1).any() and counts[0] > 0 and counts[E - 1] > 0 and counts[5] == 0))
    assert rows * k < 2 * TM + 4 + k or (counts[2] == TM and counts[3] == TM + 1 and counts[4] == 1)
    scores = MO.renormalise(O.bf16(rng.uniform(0.02, 0.3, size=(rows, k)).astype(np.float32)))
    xn = O.bf16(rng.standard_normal((rows, D)).astype(np.float32))
    h = O.bf16(rng.standard_normal((rows, D)).astype(np.float32) * np.float32(0.25))
    args = (to_dev(xn), to_dev(h), torch.from_numpy(ids).to(DEV), to_dev(scores), stack.dev["gate"], stack.dev["up"], stack.dev["down"])
    out_t, stages = ext.moe_experts_rows_grouped(*args)
    torch.cuda.synchronize()
    got = {name: t.cpu().numpy() if t.dtype == torch.int32 else host(t) for name, t in stages.items()}
    out = host(out_t)
    what = f"grouped experts E={E} k={k} hidden={D} I={I} rows={rows}"

    assert np.array_equal(got["perm"], np.argsort(flat, kind="stable")), what + ": perm is not the stable sort by expert"
    assert np.array_equal(got["offsets"], np.concatenate([[0], np.cumsum(counts)])), what + ": offsets"

    a = np.repeat(xn, k, axis=0)  # expert row r reads activation row r // k
    want_gate, _ = tile_stage(stack, "gate", a, flat)
    want_up, _ = tile_stage(stack, "up", a, flat)
    act_o = MO.silu_mul(want_gate, want_up)
    gate64, up64 = (dense64_stage(stack, name, a.astype(np.float64), flat) for name in ("gate", "up"))
    act64 = gate64 / (1.0 + np.exp(-gate64)) * up64
    check_against_truth(got["act"], act_o, act64, what=what + ": act")

    want_y, floor = tile_stage(stack, "down", got["act"], flat)
    assert_rounded_close(got["y"], want_y, "bf16", ulps=1.0, floor=floor, what=what + ": down")

    want_out = MO.combine(got["y"].reshape(rows, k, D), scores, h)
    assert np.array_equal(O.bf16_bits(out), O.bf16_bits(want_out)), f"{what}: combine {int((out != want_out).sum())} elements differ"

    y_o, _ = tile_stage(stack, "down", act_o, flat)
    oracle_out = MO.combine(y_o.reshape(rows, k, D), scores, h)
    y64 = dense64_stage(stack, "down", act64, flat)
    truth = h.astype(np.float64) + (y64.reshape(rows, k, D) * scores.astype(np.float64)[..., None]).sum(axis=1)
    check_against_truth(out, oracle_out, truth, what=what)

    out2, stages2 = ext.moe_experts_rows_grouped(*args)
    torch.cuda.synchronize()
    assert torch.equal(out2, out_t) and all(torch.equal(stages2[name], stages[name]) for name in stages), what + ": a second call differs"


@pytest.fixture(scope="module")
def reference_case(tmp_path_factory):
    """which -> (model, prompt, forced, the CPU side: test_engine_moe_gpu.reference_side), computed once for a checkpoint's three cases."""
    @functools.lru_cache(maxsize=None)
    def case(which):
        cfg, model = _moe_checkpoint(tmp_path_factory, "grouped" + which, {"128x8": 22, "60x4": 23}[which], **REAL_COUNTS[which])
        prompt, forced = prompt_and_forced(cfg, 23, REAL_COUNT_SEEDS[which, 23])
        return model, prompt, forced, reference_side(cfg, model._oracle_weights, prompt, forced)

    return case


def engine_run(model, prompt, forced, chunk, grouped_rows):
    from tiny_llm_hip.engine import DecodeEngine

    eng = DecodeEngine(model, page_size=16, num_pages=32, max_batch=2, max_prefill_rows=64, moe_grouped_rows=grouped_rows)
    try:
        eng.begin(0)
        eng.prefill(0, prompt, chunk=chunk)
        got = [eng.logits(1)[0].float().cpu().numpy()]
        after_prefill = eng.moe_grouped_state()["grouped_calls"]
        for tok in forced:
            eng.set_token(0, tok)
            eng.decode(1, batch=1)
            got.append(eng.logits(1)[0].float().cpu().numpy())
        state = eng.moe_grouped_state()
        eng.release(0)
        return np.stack(got), after_prefill, state
    finally:
        eng.close()


@pytest.mark.parametrize("chunk,grouped_rows,calls", [(64, 8, 2), (16, 8, 2), (64, 0, 0)])
@pytest.mark.parametrize("which", ["128x8", "60x4"])
def test_engine_with_the_grouped_route_against_the_oracle_and_the_float64_truth(reference_case, which, chunk, grouped_rows, calls):
    """23 prompt tokens, six teacher-forced decode steps, the bar of test_engine_moe_gpu.oracle_and_truth_case.  chunk 64: one 23-row
    pass on the grouped route; chunk 16: a 16-row grouped pass, then a 7-row pass on the GEMV route; 2 sparse layers each.  The decode
    steps add no grouped call; with the route off (0) there is none."""
    model, prompt, forced, (want, exact, counted) = reference_case(which)
    got, after_prefill, state = engine_run(model, prompt, forced, chunk, grouped_rows)
    assert state == {"min_rows": grouped_rows, "grouped_calls": calls} and after_prefill == calls
    assert sum(counted) >= 2 * len(counted) // 3 + 1, f"too many toss-up selections to compare: {counted}"
    keep = np.asarray(counted)
    check_against_truth(got[keep], want[keep], exact[keep], what=f"engine, grouped route from {grouped_rows} rows, {which}, chunk {chunk}")


def test_a_real_engine_refuses_a_negative_row_count_and_keeps_its_setting(reference_case):
    from tiny_llm_hip.engine import DecodeEngine, _ext, _lib

    eng = DecodeEngine(reference_case("60x4")[0], page_size=16, num_pages=8, max_batch=1, max_prefill_rows=16, moe_grouped_rows=8)
    try:
        with pytest.raises(RuntimeError, match="min_rows must be >= 0"):
            _ext.check(_lib.tl_engine_set_moe_grouped(eng._h, -1))
        assert eng.moe_grouped_state() == {"min_rows": 8, "grouped_calls": 0}
    finally:
        eng.close()
