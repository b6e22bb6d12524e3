"""The device quantiser (csrc/quantize_w4.h, ext.quantize_w4) against oracle.tiny_oracle.quantize_affine, BIT FOR BIT: every step of
the rule is one correctly rounded fp32 operation on both sides, so there is no tolerance.  Shapes: (1, 128) one group = one DPP row,
three rows of the wave idle; (3, 384) nine groups, no multiple of a wave's four; (5, 2560) more than one workgroup iteration per row;
(2, 4, 256) a stack of experts."""
import numpy as np
import pytest
import torch

import tiny_llm_ext_hip as ext
from oracle import tiny_oracle as O

pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def _weights(shape, dtype, seed=0):
    """Seeded normals that `dtype` represents exactly; groups 0 .. 4 (modulo the group count) overwritten to hit each branch of the
    rule: all zero, constant, largest magnitude positive / negative, and values exactly halfway between two codes."""
    rng = np.random.default_rng(seed)
    w = torch.from_numpy(rng.standard_normal(shape, dtype=np.float32) * 0.05).to(dtype).float().numpy()
    g = w.reshape(-1, 128)  # a view
    n = len(g)
    g[0] = 0.0
    g[1 % n] = 0.75
    g[2 % n, 5] = 3.0
    g[3 % n, 7] = -3.0
    g[4 % n, :2] = (-8.0, 7.0)
    _, s, b = O.quantize_affine(g[4 % n][None])  # the oracle's own scale and bias of that group: 1 and -8
    g[4 % n, 9:11] = (b[0, 0] + 8.5 * s[0, 0], b[0, 0] + 9.5 * s[0, 0])
    assert (s[0, 0], b[0, 0]) == (1.0, -8.0) and np.array_equal(torch.from_numpy(w).to(dtype).float().numpy(), w)
    return w


@pytest.mark.parametrize("shape", [(1, 128), (3, 384), (5, 2560), (2, 4, 256)])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_the_kernel_is_quantize_affine_bit_for_bit(dtype, shape):
    w = _weights(shape, DTYPES[dtype])
    want = [x.reshape(*shape[:-1], -1) for x in O.quantize_affine(w.reshape(-1, shape[-1]))]
    packed, scales, biases = ext.quantize_w4(torch.from_numpy(w).to("cuda", DTYPES[dtype]))
    assert packed.dtype == torch.int32 and scales.dtype == biases.dtype == torch.bfloat16
    np.testing.assert_array_equal(packed.cpu().numpy().view(np.uint32), want[0])
    np.testing.assert_array_equal(O.bf16_bits(scales.float().cpu().numpy()), O.bf16_bits(want[1]))
    np.testing.assert_array_equal(O.bf16_bits(biases.float().cpu().numpy()), O.bf16_bits(want[2]))


def test_quantized_matmul_reads_what_the_kernel_wrote():
    w = _weights((384, 256), torch.bfloat16, seed=1)
    a = torch.from_numpy(np.random.default_rng(2).standard_normal((8, 256), dtype=np.float32)).to("cuda", torch.bfloat16)
    p, s, b = O.quantize_affine(w)
    want = (torch.from_numpy(p.view(np.int32)).cuda(), torch.from_numpy(s).to("cuda", torch.bfloat16), torch.from_numpy(b).to("cuda", torch.bfloat16))
    got = ext.quantize_w4(torch.from_numpy(w).to("cuda", torch.bfloat16))
    out = [ext.quantized_matmul(s, b, 128, 4, a, p, True) for p, s, b in (got, want)]
    assert out[0].shape == (8, 384) and torch.equal(out[0], out[1])


@pytest.mark.parametrize("case", ["cols=64", "null pointer", "cpu tensor"])
def test_refusals(case):
    if case == "null pointer":
        assert ext.lib().tl_quantize_w4(None, 2, 128, ext.TL_BF16, None, None, None, None) == -1 and b"null pointer" in ext.lib().tl_last_error()
        return
    w = torch.zeros(2, 64 if case == "cols=64" else 128, dtype=torch.bfloat16, device="cpu" if case == "cpu tensor" else "cuda")
    with pytest.raises(RuntimeError, match="GPU-only" if case == "cpu tensor" else "multiple of the group size 128"):
        ext.quantize_w4(w)
