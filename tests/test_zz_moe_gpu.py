"""GPU tier: the engine's MoE kernels over caller rows (tl_moe_route_rows, tl_moe_experts_rows; csrc/engine_kernels.h) against the float64
restatement of their definitions (tests/moe_oracle.py), at the expert counts they were written for -- 128 experts top 8 (Qwen3-MoE),
60 experts top 4 without renormalisation (Qwen1.5/2-MoE), the 256-expert stride, 1,024 experts top 16 -- and, for the experts, at the
Qwen3-30B-A3B layer shape (hidden 2,048, expert width 768, eight experts per token).

Router
* exact tier: rows whose float64 probabilities all stand clear of a bf16 rounding boundary (moe_oracle.robust_rows) leave a float32
  softmax no freedom: ids equal the oracle's stable top-k in order, scores bit for bit.  No row of this tier is excused.
* crafted ties: few distinct logit values, plateaus across the k-th place, a wave boundary and the 256 stride: lower index first.
* validity tier: every random row, robust or not: a selection no float32 softmax rounded to bf16 could not have made.
* NaN / Inf logits: top_k distinct ids in range, nothing more (the kernel documents nothing more).
Experts: every stage read back from the caller's workspace and judged on the DEVICE's own input to that stage; the whole block against
the float64 truth (helpers.check_against_truth)."""

import functools

import numpy as np
import pytest
import torch

import moe_oracle as MO
from helpers import bf16_ulp, check_against_truth, w4_abs_dot, assert_rounded_close
from oracle import tiny_oracle as O
from test_ops_gpu import ACC_FLOOR  # the accumulation floor of the grouped GEMV's own test: named, not re-invented

pytestmark = pytest.mark.gpu
DEV = "cuda"

ROUTER_CASES = [(4, 2), (8, 8), (60, 4), (64, 1), (128, 8), (257, 16), (320, 16), (1024, 16)]
ROW_COUNTS = (1, 3, 64)


@pytest.fixture(scope="module")
def ext():
    import tiny_llm_ext_hip as ext

    return ext


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV, torch.bfloat16)


def host(t):
    return t.float().cpu().numpy()


def bits_to_dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def candidate_rows(E, sigma):
    """bf16 N(0, sigma) router logits, generated on the CPU in batches until 64 robust rows exist: (all rows generated, the first 64
    robust ones).  The rows are picked by the float64 reference alone."""
    rng = np.random.default_rng(1000 * E + int(sigma * 100))
    rows, robust = [], []
    while sum(len(r) for r in robust) < max(ROW_COUNTS):
        batch = O.bf16(rng.standard_normal((256, E)).astype(np.float32) * np.float32(sigma))
        rows.append(batch)
        robust.append(batch[MO.robust_rows(MO.probs64(batch))])
        assert len(rows) <= 16, "robust rows are rarer than the float64 reference said (12 % at 1,024 experts)"
    return np.concatenate(rows), np.concatenate(robust)[:max(ROW_COUNTS)]


def device_route(ext, logits, k, norm):
    ids, scores = ext.moe_route_rows(to_dev(logits), k, bool(norm))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), host(scores)


@pytest.mark.parametrize("sigma", [0.25, 1.0])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("E,k", ROUTER_CASES)
def test_router_rows_the_reference_decides_are_exact(ext, E, k, norm, sigma):
    """The device's softmax is float32.  Against the float64 one its relative error is bounded by the kernel's operation count: the
    argument x - max is exact or half a float32 step of a value below 8 (2^-22 absolute = relative in exp); expf is within 2 float32
    steps (2^-22); a lane adds at most 4 terms, the wave 6 shuffle levels, the workgroup 2 more adds: 12 adds of positive terms, 2^-24
    each; one divide, 2^-24.  Numerator 2^-21, denominator 2^-21 + 12 x 2^-24, divide 2^-24: below 1.9 x 2^-20.  A row is ROBUST when
    every float64 probability rounds to the same bf16 under a relative error of 2^-17 either way -- four times that bound -- so on such
    a row the device's bf16 probabilities are the oracle's, natural ties included, and everything after them is exact arithmetic on
    bf16 values: ids in the oracle's order (stable: lower index first), scores bit for bit; with renormalisation
    bf16(q_j / bf16(float32 sum in selection order)) in numpy float32 (no fast-math in the build: the division is correctly rounded)."""
    _, robust = candidate_rows(E, sigma)
    for rows in ROW_COUNTS:
        logits = robust[:rows]
        want_ids, want_scores, _, _ = MO.route(logits, k, norm)
        ids, scores = device_route(ext, logits, k, norm)
        assert ids.shape == (rows, k) and scores.shape == (rows, k)
        bad = np.flatnonzero((ids != want_ids).any(axis=-1))
        assert bad.size == 0, f"E={E} k={k} rows={rows}: ids differ in rows {bad[:5].tolist()}: got {ids[bad[0]].tolist()}, want {want_ids[bad[0]].tolist()}"
        assert np.array_equal(O.bf16_bits(scores), O.bf16_bits(want_scores)), (
            f"E={E} k={k} norm={norm} rows={rows}: {int((scores != want_scores).sum())} scores differ, "
            f"worst {float(np.abs(scores - want_scores).max()):.3g}")


def crafted_rows(E, k):
    """Rows of few distinct logit values, 1/32 apart and more (3 % in probability: four bf16 steps), with what the selection must be."""
    rng = np.random.default_rng(E * 31 + k)
    rows, want = [], []

    def leaders_and_plateau(plateau, n_plateau_taken):
        # k - n_plateau_taken leaders (values in equal pairs above 1: ties INSIDE the selection too) + a plateau at 1.0 across the k-th place
        n_lead = k - n_plateau_taken
        free = np.setdiff1d(np.arange(E), plateau)
        lead = rng.choice(free, size=n_lead, replace=False) if n_lead else np.zeros(0, dtype=np.int64)
        x = np.zeros(E, dtype=np.float32)
        x[plateau] = 1.0
        x[lead] = 1.0 + (1 + np.arange(n_lead) // 2) / 32.0
        order = sorted(lead.tolist(), key=lambda i: (-x[i], i)) + sorted(plateau.tolist())[:n_plateau_taken]
        rows.append(x), want.append(order)

    rows.append(np.zeros(E, dtype=np.float32)), want.append(list(range(k)))                    # all equal
    rows.append(np.full(E, -3.5, dtype=np.float32)), want.append(list(range(k)))
    if E > k:
        top = np.arange(E - min(5, E - 1), E)                                                   # a plateau at the highest indices
        for taken in range(1, min(k, len(top) - 1) + 1):
            leaders_and_plateau(top, taken)
    if E >= 128:
        leaders_and_plateau(np.arange(60, 71), 1)                                               # across the wave boundary at 64
        leaders_and_plateau(np.arange(60, 71), min(k, 6))
    if E >= 320:
        leaders_and_plateau(np.arange(250, 261), 1)                                             # across the 256 stride
        leaders_and_plateau(np.arange(250, 261), min(k, 8))
        leaders_and_plateau(np.concatenate([np.arange(60, 66), np.arange(254, 259), np.arange(E - 3, E)]), min(k, 13))
    return np.stack(rows), np.asarray(want)


@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("E,k", ROUTER_CASES)
def test_router_ties_go_to_the_lower_index(ext, E, k, norm):
    logits, want = crafted_rows(E, k)
    assert np.array_equal(O.bf16(logits), logits)
    oracle_ids, oracle_scores, _, _ = MO.route(logits, k, norm)
    assert np.array_equal(oracle_ids, want), "the oracle's stable top-k is not the order the rows were built for"
    ids, scores = device_route(ext, logits, k, norm)
    bad = np.flatnonzero((ids != want).any(axis=-1))
    assert bad.size == 0, f"E={E} k={k}: row {bad[0]}: got {ids[bad[0]].tolist()}, want {want[bad[0]].tolist()}"
    if not norm:  # equal logits give equal probabilities on the device too; their bf16 rounding may fall either way
        assert np.all(np.abs(scores - oracle_scores) <= bf16_ulp(oracle_scores))
        same = oracle_scores[:, 1:] == oracle_scores[:, :-1]
        assert np.array_equal(scores[:, 1:] == scores[:, :-1], same)


@pytest.mark.parametrize("sigma", [0.25, 1.0])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("E,k", ROUTER_CASES)
def test_router_selection_is_valid_on_every_row(ext, E, k, norm, sigma):
    """Unfiltered rows.  Each device probability is bf16 (half a step: a relative 2^-8) of a float32 value within 2^-20 of the float64
    one, so an unchosen expert can stand above a chosen one by at most (1 + 2^-8) / (1 - 2^-8) x (1 + 2^-19) < 1 + 2^-7 + 2^-12 in
    float64 probability.  Without renormalisation the scores are the bf16 probabilities themselves: non-increasing, ids ascending
    inside a run of equal scores, each within one bf16 step of bf16(p64)."""
    logits = candidate_rows(E, sigma)[0][:64]
    p64 = MO.probs64(logits)
    oracle_ids = MO.route(logits, k, norm)[0]
    bound = 1 + 2.0 ** -7 + 2.0 ** -12
    assert MO.selection_ratio(p64, oracle_ids).max() <= bound  # the oracle's own selection (bf16 of the float64 probabilities) obeys it too
    ids, scores = device_route(ext, logits, k, norm)
    assert ids.min() >= 0 and ids.max() < E
    assert all(len(set(r)) == k for r in ids.tolist()), "an expert was selected twice"
    ratio = MO.selection_ratio(p64, ids)
    assert ratio.max() <= bound, f"E={E} k={k}: row {int(ratio.argmax())} skips an expert {ratio.max():.5f} x above a chosen one"
    if not norm:
        assert np.all(scores[:, 1:] <= scores[:, :-1]), "scores increase"
        tied = scores[:, 1:] == scores[:, :-1]
        assert np.all(ids[:, 1:][tied] > ids[:, :-1][tied]), "equal scores: the higher expert index came first"
        want = O.bf16(np.take_along_axis(p64, ids, axis=-1))
        assert np.all(np.abs(scores - want) <= bf16_ulp(want))


@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("E,k", [(4, 2), (8, 8), (128, 8), (320, 16), (1024, 16)])
def test_router_with_non_finite_logits_still_names_distinct_experts(ext, E, k, norm):
    """What the kernel documents for NaN / Inf logits: top_k distinct ids in [0, E) (the grouped GEMVs index expert weights with them).
    The scores are unspecified, and these ids go nowhere else."""
    rng = np.random.default_rng(E + k)
    base = O.bf16_bits(rng.standard_normal((6, E)).astype(np.float32))
    base[0, E // 2] = 0x7FC0   # a NaN
    base[1, E - 1] = 0x7F80    # +Inf
    base[2, :] = 0xFF80        # all -Inf
    base[3, 0] = 0xFFFF        # the NaN whose bf16 pattern the kernel uses as its "picked" mark
    base[4, :] = 0xFFFF
    base[5, 1] = 0xFFC0        # a negative NaN
    ids, _ = ext.moe_route_rows(bits_to_dev(base), k, bool(norm))
    torch.cuda.synchronize()
    ids = ids.cpu().numpy()
    assert ids.shape == (6, k) and ids.min() >= 0 and ids.max() < E
    assert [len(set(r)) for r in ids.tolist()] == [k] * 6, ids.tolist()


def test_op_level_router_orders_equal_probabilities_lower_index_first(ext):
    """tiny_llm_hip.moe.route_topk (the op-by-op block the engine tests compare with): experts with identical router rows have equal
    logits, hence equal probabilities -- a stable descending sort names them in ascending index order, as the engine and the oracle do."""
    from tiny_llm_hip import QuantizedWeights, route_topk
    from tiny_llm_hip.synthetic import quantize

    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    E, D, k = 16, 256, 6
    w = torch.randn((E, D), generator=gen, device=DEV) * 0.3
    w[[2, 5, 9, 14]] = w[7].clone()  # five experts share a row
    packed, scales, biases = quantize(w.to(torch.bfloat16))
    x = torch.randn((1, 12, D), generator=gen, device=DEV).to(torch.bfloat16)
    probs, ids, scores = route_topk(x, QuantizedWeights(scales, biases, 128, 4, packed), k, False)
    probs, ids = host(probs).reshape(-1, E), ids.reshape(-1, k).cpu().numpy()
    assert np.array_equal(probs[:, [2, 5, 9, 14]], probs[:, [7, 7, 7, 7]])
    assert np.array_equal(ids, MO.stable_topk(probs, k))
    assert any(len(set(r) & {2, 5, 7, 9, 14}) >= 2 for r in ids.tolist()), "no row selects two of the tied experts: the case shows nothing"


# ---- the experts ---------------------------------------------------------------------------------------------------------------------------------
# The grouped GEMV's plans (csrc/linear_plan.h, qmv_plan(1, N = columns reduced, K = output rows); no entry point exports them, so the
# arithmetic stands here): J = ceil(N / 512) chunks; K / 8 < 768 for every K below, so the planner asks for WN = 4 waves along the
# reduction and keeps min(WN, J >= 2 ? 2 : 1) when J < 4.
#   (32, 8, 2048, 768)  gate / up N = 2048: J = 4 -> WN = 4;  down N = 768 = 512 + 256: J = 2 -> WN = 2 over a ragged last chunk
#   (8, 4, 1664, 384)   gate / up N = 1664 = 3 x 512 + 128: J = 4 -> WN = 4 with a ragged last chunk;  down N = 384: J = 1 -> WN = 1
#   (16, 16, 256, 128)  J = 1 both ways -> WN = 1; a_rows_div = 16
EXPERT_SHAPES = [(32, 8, 2048, 768), (8, 4, 1664, 384), (16, 16, 256, 128)]


class ExpertStack:
    """W4 experts built on the GPU (tiny_llm_hip.synthetic.quantize); an expert's tensors come back to the host when the oracle asks."""

    def __init__(self, E, D, I):
        from tiny_llm_hip.synthetic import quantize

        gen = torch.Generator(device=DEV)
        gen.manual_seed(E * 7 + D + I)
        self.E, self.D, self.I = E, D, I
        self.dev = {}
        for name, (out_dim, in_dim) in (("gate", (I, D)), ("up", (I, D)), ("down", (D, I))):
            parts = [quantize((torch.randn((out_dim, in_dim), generator=gen, device=DEV) * 0.03).to(torch.bfloat16)) for _ in range(E)]
            self.dev[name] = tuple(torch.stack([p[j] for p in parts]).contiguous() for j in range(3))
        self._host = {}

    def host_w4(self, name, e):
        """(packed uint32, scales, biases as float32) of one expert."""
        if (name, e) not in self._host:
            packed, scales, biases = self.dev[name]
            self._host[name, e] = (packed[e].cpu().numpy().view(np.uint32), host(scales[e]), host(biases[e]))
        return self._host[name, e]

    def dense64(self, name, e):
        packed, s, z = self.host_w4(name, e)
        q = O.unpack_codes(packed).astype(np.float64)
        return q * np.repeat(s.astype(np.float64), 128, axis=-1) + np.repeat(z.astype(np.float64), 128, axis=-1)


@functools.lru_cache(maxsize=None)
def expert_stack(E, D, I):
    return ExpertStack(E, D, I)


def own_ids(rng, rows, E, k):
    """The test's own selection: row 0 names ONE expert k times (E - 1 when it is the only row); row 1 names experts E - 1 and 0 among
    distinct ones; every other row k distinct experts of a pool of at most 12 (what the oracle has to fetch and dequantise)."""
    pool = np.concatenate([[0, E - 1], 1 + rng.permutation(E - 2)[:max(k, min(E, 12)) - 2]]) if E > 2 else np.arange(E)
    ids = np.stack([rng.permutation(pool)[:k] for _ in range(rows)]).astype(np.int32)
    ids[0, :] = E - 1 if rows == 1 else pool[2 % len(pool)]
    if rows > 1:
        rest = [e for e in ids[1].tolist() if e not in (0, E - 1)]
        ids[1] = ([E - 1, 0] + rest)[:k] if k >= 2 else [E - 1]
    return ids


def gemv_stage(stack, name, a, flat_ids):
    """(the oracle's GEMV of rows `a` each against its own expert -- float64 accumulation, one bf16 rounding --, the unrounded float64
    sums, the allowance's floor ACC_FLOOR * sum |a| |w|), an expert dequantised once for all its rows."""
    out_dim = stack.dev[name][0].shape[1]
    want, raw, floor = (np.zeros((len(flat_ids), out_dim)) for _ in range(3))
    for e in np.unique(flat_ids):
        sel = np.flatnonzero(flat_ids == e)
        packed, s, z = stack.host_w4(name, int(e))
        raw[sel] = O.quantized_matmul(s, z, a[sel], packed, raw=True)
        want[sel] = O.bf16(raw[sel].astype(np.float32))
        floor[sel] = ACC_FLOOR * w4_abs_dot(a[sel], packed, s, z, "bf16")
    return want, raw, floor


@pytest.mark.parametrize("rows", [1, 2, 9, "router"])
@pytest.mark.parametrize("E,k,D,I", EXPERT_SHAPES)
def test_experts_stage_by_stage_and_against_the_truth(ext, E, k, D, I, rows):
    """tl_moe_experts_rows with the caller's ids and scores ("router": two rows whose ids and scores are the device router's over random
    logits, renormalised).  Per stage, on the device's own input to it:
      gate, up   the oracle's GEMV of xn: one bf16 ulp + ACC_FLOOR * sum |a| |w| (the allowance of test_gather_quantized_matvec)
      act        bf16(bf16(silu(gate)) * up) of the device's gate and up in numpy float32: one bf16 ulp (expf against numpy's exp); bit for
                 bit wherever the float64 silu stands clear of a bf16 boundary (the product of two bf16 values is exact in float32)
      y          the oracle's GEMV of the device's act, same allowance
      out        bit-equal to the float32 restatement of the combine over the device's y and scores
    and the whole block as close to its float64 truth as the bf16 oracle's chain is (helpers.check_against_truth)."""
    stack = expert_stack(E, D, I)
    rng = np.random.default_rng(E * 100 + k * 10 + (rows if rows != "router" else 7))
    if rows == "router":
        rows = 2
        logits = O.bf16(rng.standard_normal((rows, E)).astype(np.float32))
        ids_t, scores_t = ext.moe_route_rows(to_dev(logits), k, True)
        ids, scores = ids_t.cpu().numpy(), host(scores_t)
        assert ids.min() >= 0 and ids.max() < E
    else:
        ids = own_ids(rng, rows, E, k)
        scores = MO.renormalise(O.bf16(rng.uniform(0.02, 0.3, size=(rows, k)).astype(np.float32)))
        ids_t, scores_t = torch.from_numpy(ids).to(DEV), to_dev(scores)
        assert (ids[0] == ids[0, 0]).all() and (ids == E - 1).any()
    xn = O.bf16(rng.standard_normal((rows, D)).astype(np.float32))
    h = O.bf16(rng.standard_normal((rows, D)).astype(np.float32) * np.float32(0.25))
    out_t, stages = ext.moe_experts_rows(to_dev(xn), to_dev(h), ids_t, scores_t, stack.dev["gate"], stack.dev["up"], stack.dev["down"])
    torch.cuda.synchronize()
    got = {name: host(t) for name, t in stages.items()}
    out = host(out_t)
    flat = ids.reshape(-1)
    what = f"experts E={E} k={k} hidden={D} I={I} rows={rows}"

    a = np.repeat(xn, k, axis=0)  # expert row r reads activation row r // k
    want_gate, gate64, floor = gemv_stage(stack, "gate", a, flat)
    assert_rounded_close(got["gate"], want_gate, "bf16", ulps=1.0, floor=floor, what=what + ": gate")
    want_up, up64, floor = gemv_stage(stack, "up", a, flat)
    assert_rounded_close(got["up"], want_up, "bf16", ulps=1.0, floor=floor, what=what + ": up")

    want_act = MO.silu_mul(got["gate"], got["up"])
    off = np.abs(got["act"] - want_act)
    assert np.all(off <= bf16_ulp(want_act)), f"{what}: act {int((off > bf16_ulp(want_act)).sum())} elements beyond one bf16 ulp"
    lo, hi = MO.silu_candidates(got["gate"])
    decided = lo == hi
    assert decided.mean() > 0.99
    assert np.array_equal(got["act"][decided], O.bf16(lo * got["up"])[decided]), f"{what}: act differs where the rounding of silu is decided"

    want_y, _, floor = gemv_stage(stack, "down", got["act"], flat)
    assert_rounded_close(got["y"], want_y, "bf16", ulps=1.0, floor=floor, what=what + ": down")

    want_out = MO.combine(got["y"].reshape(rows, k, D), scores, h)
    assert np.array_equal(O.bf16_bits(out), O.bf16_bits(want_out)), f"{what}: combine {int((out != want_out).sum())} elements differ from the float32 restatement"

    # end to end: the bf16 oracle's own chain and the float64 truth, both on the same ids and scores
    act_o = O.bf16(O.bf16(O.silu(want_gate)) * want_up)
    y_o, _, _ = gemv_stage(stack, "down", act_o, flat)
    oracle_out = MO.combine(y_o.reshape(rows, k, D), scores, h)
    act64 = gate64 / (1.0 + np.exp(-gate64)) * up64
    y64 = np.zeros((rows * k, D))
    for e in np.unique(flat):
        sel = np.flatnonzero(flat == e)
        y64[sel] = act64[sel] @ stack.dense64("down", int(e)).T
    truth = h.astype(np.float64) + (y64.reshape(rows, k, D) * scores.astype(np.float64)[..., None]).sum(axis=1)
    check_against_truth(out, oracle_out, truth, what=what)
