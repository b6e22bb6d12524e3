"""CPU tier: the test-only MoE oracle (tests/moe_oracle.py) against the two statements the engine is judged by -- oracle.moe_block (bf16,
one rounding per reference op) and oracle.TruthQwen3._moe (float64) -- on small blocks; the definition of the weighted sum (float32 in
expert order, rounded once: the same operation as a sum rounded after every add for top_k <= 2, another one from three experts on);
the tie order; the row classifier of the GPU router test on hand-made rows; and the bad-argument returns of tl_moe_route_rows /
tl_moe_experts_rows through the built library (decided on the host: no device is touched)."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import moe_oracle as MO
from oracle import tiny_oracle as O

ROOT = Path(__file__).resolve().parent.parent
TL_ERR_INVALID = -1


def small_block(seed, E, D, I, sigma=0.05, router_sigma=0.5):
    rng = np.random.default_rng(seed)

    def stack(out_dim, in_dim):
        parts = [O.quantize_affine(O.bf16(rng.standard_normal((out_dim, in_dim), dtype=np.float32) * sigma)) for _ in range(E)]
        return tuple(np.stack([p[j] for p in parts]) for j in range(3))

    router = O.quantize_affine(O.bf16(rng.standard_normal((E, D), dtype=np.float32) * router_sigma))
    return rng, router, stack(I, D), stack(I, D), stack(D, I)


@pytest.mark.parametrize("E,k,norm", [(8, 2, True), (8, 3, False), (12, 8, True), (5, 5, False)])
def test_the_oracle_restates_moe_block(E, k, norm):
    D, I, T = 128, 128, 6
    rng, router, gate, up, down = small_block(E * 10 + k, E, D, I)
    x = O.bf16(rng.standard_normal((T, D), dtype=np.float32))
    want, want_ids, want_scores = O.moe_block(x, router, gate, up, down, k, norm)
    logits = O.quantized_matmul(router[1], router[2], x, router[0])
    ids, scores, pb, p64 = MO.route(logits, k, norm)
    assert np.array_equal(ids, want_ids)
    assert np.array_equal(scores, want_scores)  # (the selected probabilities span few binades: their float32 sum is exact in any order)
    assert np.array_equal(pb, O.bf16(O.softmax(logits)))
    rows, flat = np.repeat(x, k, axis=0), ids.reshape(-1)
    g = O.gather_quantized_matvec(gate[1], gate[2], rows, gate[0], flat)
    u = O.gather_quantized_matvec(up[1], up[2], rows, up[0], flat)
    act_block = O.bf16(O.bf16(O.silu(g)) * u)  # moe_block's: x * sigmoid(x), the kernel's: x / (1 + exp(-x)) -- one float32 step apart at most
    act = MO.silu_mul(g, u)
    assert np.all(np.abs(act - act_block) <= 2.0 ** (np.floor(np.log2(np.maximum(np.abs(act_block), 2.0 ** -126))) - 7))
    lo, hi = MO.silu_candidates(g)
    decided = lo == hi
    assert decided.mean() > 0.99 and np.array_equal(act[decided], O.bf16(lo * u)[decided])
    y = O.gather_quantized_matvec(down[1], down[2], act_block, down[0], flat).reshape(T, k, D)
    assert np.array_equal(MO.weighted_sum(y, scores), want)
    h = O.bf16(rng.standard_normal((T, D), dtype=np.float32))
    assert np.array_equal(MO.combine(y, scores, h), O.bf16(h + want))


@pytest.mark.parametrize("k,norm", [(2, True), (4, False)])
def test_the_oracle_against_the_float64_truth(k, norm):
    """TruthQwen3._moe on the oracle's selection: the same experts wherever the truth's own k-th probability stands clear of the
    (k+1)-th, and an output one bf16 rounding chain away from moe_block's."""
    E, D, I, T = 8, 128, 128, 6
    rng, router, gate, up, down = small_block(77 + k, E, D, I)
    x = O.bf16(rng.standard_normal((T, D), dtype=np.float32))
    m = dict(router=router, gate_proj=gate, up_proj=up, down_proj=down)
    cfg = dict(num_hidden_layers=1, num_experts_per_tok=k, norm_topk_prob=norm)
    logits = O.quantized_matmul(router[1], router[2], x, router[0])
    ids, scores, _, p64 = MO.route(logits, k, norm)
    truth = O.TruthQwen3(cfg, dict(layers=[dict(moe=m)]))
    truth.forced_moe_ids = {0: [ids]}
    exact = truth._moe(0, x.astype(np.float64), m)
    rec = truth.moe_margins[0][0]
    # the router logits are bf16-rounded on the oracle's side only (|logit| < 32: up to 2^-4 each, a factor e^(2^-3) between two
    # probabilities): a k-th probability less than 2^-2 of itself above the next may flip
    clear = rec["margin"] > 2.0 ** -2 * np.sort(p64, axis=-1)[:, -k]
    assert np.abs(logits).max() < 32
    assert clear.any() and rec["same_choice"][clear].all()
    want, _, _ = O.moe_block(x, router, gate, up, down, k, norm, ids=ids)
    scale = float(np.abs(exact).max())
    assert np.abs(want - exact).max() <= 2.0 ** -6 * scale  # a handful of bf16 roundings (2^-9 each) of values up to `scale`
    # the float64 probabilities of the test oracle are the truth's, up to the bf16 rounding of the logits
    t_logits = x.astype(np.float64) @ truth._stacked(router).T
    assert np.abs(MO.probs64(t_logits) - p64).max() <= 2.0 ** -7


def test_the_two_forms_of_the_sum_coincide_up_to_two_experts_and_differ_at_eight():
    rng = np.random.default_rng(3)
    T, D = 16, 256
    for k in (1, 2):
        y = O.bf16(rng.standard_normal((T, k, D), dtype=np.float32))
        sc = O.bf16(rng.uniform(0.05, 0.6, size=(T, k)).astype(np.float32))
        assert np.array_equal(MO.weighted_sum(y, sc), MO.weighted_sum(y, sc, per_add=True)), k
    y = O.bf16(rng.standard_normal((T, 8, D), dtype=np.float32))
    sc = MO.renormalise(O.bf16(rng.uniform(0.02, 0.2, size=(T, 8)).astype(np.float32)))
    once, per_add = MO.weighted_sum(y, sc), MO.weighted_sum(y, sc, per_add=True)
    exact = (O.bf16(y * sc[..., None]).astype(np.float64)).sum(axis=1)
    differ = once != per_add
    assert differ.mean() > 0.1, "the sum rounded after every add is another operation at eight experts"
    # ... and the worse one: the single rounding is the correctly rounded sum wherever float32 held it exactly
    assert np.abs(once - exact).max() <= np.abs(per_add - exact).max()
    assert np.abs(once - exact).mean() < np.abs(per_add - exact).mean()


def test_equal_probabilities_go_lower_index_first():
    pb = np.array([[0.125, 0.25, 0.125, 0.25, 0.125, 0.125]], dtype=np.float32)
    assert MO.stable_topk(pb, 4).tolist() == [[1, 3, 0, 2]]
    ids, scores, pb, _ = MO.route(np.zeros((2, 6), dtype=np.float32), 3, False)
    assert ids.tolist() == [[0, 1, 2]] * 2 and np.array_equal(scores, O.bf16(np.full((2, 3), 1 / 6)))
    ids, scores, _, _ = MO.route(np.array([[0.0, 1.0, 0.0, 1.0]], dtype=np.float32), 3, True)
    assert ids.tolist() == [[1, 3, 0]]
    q = np.take_along_axis(O.bf16(MO.probs64(np.array([[0.0, 1.0, 0.0, 1.0]]))), ids, axis=-1)
    den = O.bf16(np.float32(np.float32(q[0, 0] + q[0, 1]) + q[0, 2]))
    assert np.array_equal(scores, O.bf16(q / den))


def test_the_row_classifier_on_hand_made_rows():
    """A row is robust when no probability sits within a relative 2^-17 of a bf16 rounding boundary (the midpoint of two neighbours)."""
    mid = 0.5 + 2.0 ** -9  # halfway between the bf16 neighbours 0.5 and 0.5 + 2^-8
    rows = np.array([[0.5, 0.5],                              # exactly representable
                     [mid, 1 - mid],                          # on a boundary
                     [mid + 2.0 ** -20, 1 - mid - 2.0 ** -20],  # 2^-19 relative above it: inside the margin
                     [mid + 2.0 ** -14, 1 - mid - 2.0 ** -14],  # 2^-13 relative above it: clear
                     [mid - 2.0 ** -14, 1 - mid + 2.0 ** -14]])
    assert MO.robust_rows(rows).tolist() == [True, False, False, True, True]
    assert MO.robust_rows(rows, margin=2.0 ** -22).tolist() == [True, False, True, True, True]
    # one expert near a boundary spoils the row, wherever it stands
    p = np.full((1, 64), 2.0 ** -6)
    assert MO.robust_rows(p).all()
    p[0, 63] = 2.0 ** -6 * (1 + 2.0 ** -8 + 2.0 ** -21)
    assert not MO.robust_rows(p).any()
    # the selection ratio: an exact top-k stays at or below 1, a selection that skips a larger probability does not
    p = np.array([[0.4, 0.3, 0.2, 0.1]])
    assert MO.selection_ratio(p, [[0, 1]])[0] == pytest.approx(2 / 3) and MO.selection_ratio(p, [[0, 2]])[0] == pytest.approx(1.5)
    assert MO.selection_ratio(p, [[3, 2, 1, 0]])[0] == 0.0


def test_the_symbols_are_declared_exported_and_bound(built_libs):
    import tiny_llm_ext_hip as ext

    header = (ROOT / "include" / "tinyllm_engine.h").read_text()
    for name in ("tl_moe_route_rows", "tl_moe_experts_workspace_bytes", "tl_moe_experts_rows"):
        assert re.search(r"\b%s\(" % name, header), name
        assert getattr(ext.lib(), name).argtypes is not None and name in ext._SIGNATURES, name
    assert callable(ext.moe_route_rows) and callable(ext.moe_experts_rows)


def test_bad_arguments_are_invalid(built_libs):
    """Every refusal below is decided on the host before anything is launched: the addresses are never read."""
    import tiny_llm_ext_hip as ext

    lib = ext.lib()
    # logits, rows, experts, top_k, norm, ids, scores
    good = (4096, 3, 128, 8, 1, 8192, 12288)
    bad = [(None,) + good[1:], good[:5] + (None,) + good[6:], good[:6] + (None,), good[:1] + (0,) + good[2:], good[:2] + (0,) + good[3:],
           good[:2] + (1025,) + good[3:], good[:3] + (0,) + good[4:], good[:3] + (17,) + good[4:], good[:2] + (4, 5) + good[4:]]
    for args in bad:
        assert lib.tl_moe_route_rows(*args, None) == TL_ERR_INVALID, args
    assert b"moe_route_rows" in lib.tl_last_error()

    ws = lib.tl_moe_experts_workspace_bytes
    assert ws(2, 8, 2048, 768) == 2 * 8 * (3 * 768 + 2048) * 2
    assert ws(0, 8, 2048, 768) == 0 and ws(2, 0, 2048, 768) == 0 and ws(2, 8, 0, 768) == 0 and ws(2, 8, 2048, -128) == 0

    def weights(**kw):
        w = ext.TlMoeWeights(ext.TlW4(), *[4096 * (i + 1) for i in range(9)], 128, 8, 768, 1)
        for name, value in kw.items():
            setattr(w, name, value)
        return w

    rows, hidden = 2, 2048
    need = ws(rows, 8, hidden, 768)
    # xn, h, ids, scores, weights, rows, hidden, out, workspace, workspace bytes
    good = dict(xn=1 << 20, h=2 << 20, ids=3 << 20, scores=4 << 20, w=weights(), rows=rows, hidden=hidden, out=5 << 20, ws=6 << 20, ws_bytes=need)

    def call(**kw):
        a = {**good, **kw}
        w = a["w"]
        return lib.tl_moe_experts_rows(a["xn"], a["h"], a["ids"], a["scores"], ctypes.byref(w) if w is not None else None, a["rows"], a["hidden"],
                                       a["out"], a["ws"], a["ws_bytes"], None)

    refused = [dict(xn=None), dict(h=None), dict(ids=None), dict(scores=None), dict(w=None), dict(out=None), dict(ws=None),
               dict(w=weights(gate_dev=None)), dict(w=weights(down_biases_dev=None)), dict(w=weights(up_scales_dev=None)),
               dict(w=weights(num_experts=0)), dict(w=weights(num_experts=1025)), dict(w=weights(experts_per_token=0)),
               dict(w=weights(experts_per_token=17)), dict(w=weights(num_experts=4, experts_per_token=5)),
               dict(w=weights(intermediate_size=0)), dict(w=weights(intermediate_size=192)), dict(w=weights(intermediate_size=-128)),
               dict(hidden=0), dict(hidden=2000), dict(rows=0), dict(rows=-1), dict(rows=8192), dict(ws_bytes=need - 1), dict(ws_bytes=0),
               dict(rows=3),  # (the workspace is one row short)
               dict(xn=(1 << 20) + 2), dict(ws=(6 << 20) + 8)]
    for kw in refused:
        assert call(**kw) == TL_ERR_INVALID, kw
        assert b"moe_experts_rows" in lib.tl_last_error()
    # 8,191 rows x 8 experts = 65,528 expert rows is the last size one grouped launch takes; 8,192 x 8 is refused above whatever the workspace
    assert call(rows=8192, ws_bytes=ws(8192, 8, hidden, 768)) == TL_ERR_INVALID
