"""GPU parity of the FP8-activation (W4A8) prefill GEMM (csrc/gemm_fp8.h, engine option "prefill_fp8"; the reference has no counterpart).

  * the row quantiser against oracle.kv_fp8.quantize_rows per 128-column group: codes and scales BIT-identical; the group sums S against the
    float64 sum of the dequantised group within 11 fp32 roundings of sum |a^| (the kernel adds 8 values in a lane, then 4 butterfly levels);
  * the weight copy: its first rows * cols bytes, row-major, decode to exactly the checkpoint's nibbles less 8 (the kernel's centred form);
  * the product against float64 over a^ (the oracle codec) and the exact q s + beta: one bf16 step of the reference + 2^-20 of sum |a^||w|
    (the bf16 GEMM test's accumulation floor), residual / SwiGLU bands formed as tests/test_zz_prefill_bf16_gemm_gpu.py forms them, at the
    smallest shapes that reach every edge of the 128 x 256 tile and of the three-stage ring;
  * the engine on the peaked checkpoint: the option changes the first-token logits (the route ran), the greedy ids stay the truth's; the
    distance from the float64 truth is logged for both runs, not bounded (a cost to report: profiles/prefill_fp8.json).

Why the kernel splits the activation codes into exponent bands: with ONE matrix instruction per group 32 of the 54 product cases missed their band,
by up to 57 x, on rows with an outlier group (one value 2^15 above the other 127) where the output nearly cancels -- v_mfma_scale_f32_16x16x128_f8f6f4
adds its products in blocks of 8 inside a window of about 14 bits below the block's largest (a code of 288 beside 127 codes of 2^-9 .. 2^-6, all
weights 1: the sum comes back short by EXACTLY the 7 block neighbours of the 288).  With four bands all cases are inside the band (worst: one bf16 step).
"""

import numpy as np
import pytest
import torch

from oracle import kv_fp8 as KV
from oracle import tiny_oracle as O
from helpers import TINY_CFG, assert_within, bf16_ulp, check_against_truth, log_parity, oracle_weights_from_model, ulp_of, w4_abs_dot

pytestmark = pytest.mark.gpu

DEV = "cuda"
BM, BN = 128, 256  # the kernel's tile (gemm_fp8.h)


@pytest.fixture(scope="module")
def ext(built_libs):
    import tiny_llm_ext_hip as e

    return e


def _dev_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV, torch.bfloat16)


def _host(t):
    return O.from_bf16_bits(t.view(torch.int16).cpu().numpy().view(np.uint16))


def _rows(M, K, seed):
    """bf16 rows whose groups (counted over the flattened [M, K / 128]) cycle through: E4M3 ties under scale 1 (448 pins it), all zero, one
    large outlier over small values, plain normal."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M * (K // 128), 128)).astype(np.float32)
    x[0::4] *= 0.01
    x[0::4, :8] = [448.0, 17.0, 19.0, 1.0625, 2.0 ** -10, 3 * 2.0 ** -10, -21.0, -1.1875]
    x[1::4] = 0.0
    x[2::4] *= 0.01
    x[2::4, 77] = -300.0
    return O.bf16(x.reshape(M, K))


def _weights(N, K, seed, beta_dominates=False):
    rng = np.random.default_rng(seed)
    packed = rng.integers(0, 2 ** 32, size=(N, K // 8), dtype=np.uint64).astype(np.uint32)
    s = O.bf16((0.002 + 0.004 * rng.random((N, K // 128))).astype(np.float32) * (2.0 ** -12 if beta_dominates else 1.0))
    b = O.bf16(rng.standard_normal((N, K // 128)).astype(np.float32) if beta_dominates else -7.5 * s * (1 + 0.1 * rng.standard_normal(s.shape).astype(np.float32)))
    q = ((packed[:, :, None] >> (4 * np.arange(8, dtype=np.uint32))) & 15).reshape(N, K).astype(np.float64)
    w = q * np.repeat(s.astype(np.float64), 128, axis=1) + np.repeat(b.astype(np.float64), 128, axis=1)
    return packed, s, b, q, w


@pytest.mark.parametrize("K", [128, 1152])
@pytest.mark.parametrize("M", [1, 17])
def test_quantiser_is_the_oracles_row_codec_per_group(ext, M, K):
    x = _rows(M, K, seed=M + K)
    codes, scales, sums = (t.cpu().numpy() for t in ext.prefill_quantize_rows_fp8(_dev_bf16(x)))
    want_codes, want_scales = KV.quantize_rows(x.reshape(M, K // 128, 128))
    assert np.array_equal(codes.reshape(want_codes.shape), want_codes)
    assert np.array_equal(scales.view(np.uint32), want_scales.view(np.uint32))
    deq = KV.dequantize_rows(want_codes, want_scales).astype(np.float64)
    assert_within(sums, deq.sum(-1), 11 * 2.0 ** -24 * np.abs(deq).sum(-1), what=f"group sums M={M} K={K}")


def test_weight_copy_decodes_to_the_nibbles_less_eight(ext):
    N, K = 272, 384
    packed, s, b, q, _ = _weights(N, K, seed=1)
    wf = ext.prefill_weights_fp8(torch.from_numpy(packed.view(np.int32)).to(DEV), _dev_bf16(s), _dev_bf16(b))
    assert np.array_equal(KV.decode_e4m3(wf[: N * K].cpu().numpy().reshape(N, K)) + 8, q.astype(np.float32))  # (gemm_fp8.h: codes of q - 8)


def _product_case(ext, M, N, K, epi, beta_dominates=False):
    packed, s, b, _, w = _weights(N, K, seed=N + K, beta_dominates=beta_dominates)
    x = _rows(M, K, seed=3 * M + K)
    a_hat = KV.round_trip(x.reshape(M, K // 128, 128)).reshape(M, K)  # the dequantised activations, exactly bf16 values
    rng = np.random.default_rng(M * N)
    res = O.bf16(rng.standard_normal((M, N)).astype(np.float32))
    wf = ext.prefill_weights_fp8(torch.from_numpy(packed.view(np.int32)).to(DEV), _dev_bf16(s), _dev_bf16(b))
    qr = ext.prefill_quantize_rows_fp8(_dev_bf16(x))
    got = _host(ext.prefill_matmul_fp8(*qr, wf, N, epilogue=epi, residual=_dev_bf16(res) if epi == 1 else None))
    want_plain = O.bf16(a_hat.astype(np.float64) @ w.T)
    floor = 2.0 ** -20 * w4_abs_dot(a_hat, packed, s, b, "bf16")
    what = f"gemm_fp8 M={M} N={N} K={K} epi={epi}"
    if epi == 0:
        want, allowed = want_plain, ulp_of(want_plain, "bf16") + floor
    elif epi == 1:
        want = O.bf16(res + want_plain)
        allowed = ulp_of(want_plain, "bf16") + floor + bf16_ulp(want)
    else:
        g, u = want_plain[:, 0::2].astype(np.float64), want_plain[:, 1::2].astype(np.float64)
        want = O.swiglu(want_plain[:, 0::2], want_plain[:, 1::2])
        allowed = 1.1 * (bf16_ulp(g) + floor[:, 0::2]) * np.abs(u) + (bf16_ulp(u) + floor[:, 1::2]) * np.abs(g / (1 + np.exp(-g))) + bf16_ulp(want)
    err = np.abs(got.astype(np.float64) - want)
    print(what, "max err", float(err.max()), "max err / allowed", float((err / allowed).max()))
    assert_within(got, want, allowed, what=what)


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("K", [128, 384, 1152])
@pytest.mark.parametrize("N", [BN - 16, BN + 32])
@pytest.mark.parametrize("M", [1, BM - 1, BM + 3])
def test_product_against_float64_over_the_dequantised_operands(ext, M, N, K, epi):
    _product_case(ext, M, N, K, epi)  # (_rows puts an all-zero activation group into every case with more than one group)


def test_product_where_the_bias_term_dominates(ext):
    _product_case(ext, BM + 3, BN + 32, 384, 0, beta_dominates=True)  # s 2^-12 of the usual, beta of order 1: the output is the K-extension's beta . S


def test_engine_prefill_takes_the_fp8_route_and_keeps_the_truths_greedy_ids():
    from oracle import c_oracle
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert c_oracle.available(), "oracle/libqwen3_oracle.so missing (run __graft_entry__.build())"
    model = synthetic_qwen3(TINY_CFG, seed=21, sigma=0.05, device="cuda", embed_sigma=0.5, residual_gain=0.5, head_permutation=(5, 11))
    weights, cfg = oracle_weights_from_model(model), dict(TINY_CFG, tie_word_embeddings=False)
    prompt = [int(t) for t in np.random.default_rng(9).integers(1, TINY_CFG["vocab_size"], size=300)]
    steps = 4
    want = {}
    for name, cls in (("port", c_oracle.COracleQwen3), ("truth", c_oracle.CTruthQwen3)):
        m = cls(cfg, weights, max_ctx=len(prompt) + steps + 2)
        try:
            for t in prompt:
                tid, logits = m.step(t)
            first, ids = np.asarray(logits, dtype=np.float64).copy(), []
            for _ in range(steps):
                ids.append(int(tid))
                tid, logits = m.step(tid)
        finally:
            m.close()
        want[name] = (first, ids)
    runs = {}
    for flag in (0, 128):  # 128: the smallest row threshold the option takes -- the 300-row chunk crosses it
        eng = DecodeEngine(model, page_size=128, num_pages=6, max_batch=1, max_prefill_rows=512, options={"prefill_fp8": flag})
        try:
            eng.begin(0)
            eng.prefill(0, prompt, chunk=512)
            first = eng.logits(1)[0].float().cpu().numpy()
            eng.decode(steps - 1, batch=1)
            runs[flag] = (first, eng.read_tokens(0, steps))
            eng.release(0)
        finally:
            eng.close()
    assert not np.array_equal(runs[0][0], runs[128][0]), "the option changed nothing: the FP8 route did not run"
    check_against_truth(runs[0][0][None], want["port"][0][None], want["truth"][0][None], what="prefill_fp8 engine test: option off")
    rec = check_against_truth(runs[128][0][None], want["port"][0][None], want["truth"][0][None], what="prefill_fp8 engine test: option on", factor=float("inf"))
    log_parity({"what": "prefill_fp8_engine_vs_truth", **rec})
    assert runs[128][1] == want["truth"][1], f"greedy ids with FP8 prefill {runs[128][1]} differ from the truth's {want['truth'][1]}"
