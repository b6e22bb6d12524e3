// MLX affine W4 (group 128) quantiser for gfx950: unquantised weights -> the packed words, bf16 scales and bf16 biases every matmul,
// gather and embedding kernel of this library reads.  No reference kernel is replaced (the reference gets its weights quantised from
// mlx_lm); the rule is the project's restatement of mx.quantize, oracle/tiny_oracle.py::quantize_affine, and the result is that
// function's bit for bit.
//
// Work split.  cols % 128 == 0 and the rows are contiguous, so a matrix [rows, cols] (or a stack [E, rows, cols]) is a flat list of
// rows * cols / 128 groups: group g is elements [128 g, 128 g + 128), its words are packed[16 g .. 16 g + 16), its scale and bias have
// index g.  One lane owns 8 consecutive elements = one 16-byte load of a 16-bit source (two of fp32) = exactly one output word; 16
// lanes own one group, so a group IS a DPP row: its min and max are four v_min / v_max with row rotations each, every lane of the row
// ends up with both, and all 16 compute the group's scale and bias redundantly (the SIMD would idle otherwise).  No LDS, no
// cross-row traffic, no atomics: what a lane writes depends on its own group alone, so the result does not depend on the grid.  A wave
// takes 4 groups per iteration, a 256-thread workgroup 16 (2,048 contiguous elements); workgroups walk the groups grid-stride.
//
// Stores.  Every lane stores its word (a wave writes 256 contiguous bytes); lane 0 of a row stores the group's scale and lane 1 its
// bias with ONE store instruction whose base pointer is selected per lane.
//
// Bit identity.  Every line of quantize_rule / quantize_codes below is ONE IEEE-754 single-precision operation, in the order of the
// oracle's lines: correctly rounded subtraction and division (HIP's default for `/`; the object is built with
// -fhip-fp32-correctly-rounded-divide-sqrt and -ffp-contract=off on top of the pragmas here, csrc/Makefile), rintf = v_rndne_f32 =
// np.rint (ties to even), BF16::from_float = round to nearest even = the oracle's bf16().  min / max are exact in any order.  There
// is no reciprocal-multiply and no fused multiply-add anywhere on the path.
#pragma once
#include "common.h"

namespace tl {

constexpr int QW4_GROUP = 128;            // elements per scale / bias
constexpr int QW4_LANE_ELEMS = 8;         // elements per lane = codes per word
constexpr int QW4_THREADS = 256;
constexpr int QW4_GROUPS_PER_BLOCK = QW4_THREADS / 16;

__device__ __forceinline__ float group16_min_self(float v) {
    v = fminf(v, dpp_row_ror_self<8>(v));
    v = fminf(v, dpp_row_ror_self<4>(v));
    v = fminf(v, dpp_row_ror_self<2>(v));
    v = fminf(v, dpp_row_ror_self<1>(v));
    return v;
}

// a lane's 8 consecutive source elements as fp32 (exact for all three source types)
template <typename TT>
__device__ __forceinline__ void quantize_load8(const typename TT::storage *__restrict__ p, float (&x)[8]) {
    if constexpr (sizeof(typename TT::storage) == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p);
        const f32x4 b = *reinterpret_cast<const f32x4 *>(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[i] = a[i];
            x[4 + i] = b[i];
        }
    } else {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = TT::to_float((uint16_t)(v[i] & 0xffffu));
            x[2 * i + 1] = TT::to_float((uint16_t)(v[i] >> 16));
        }
    }
}

// quantize_affine's lines `scale = ...` to `bias = cast(bias)`: the group's min and max -> its bf16 scale and bias
__device__ __forceinline__ void quantize_rule(float lo, float hi, uint16_t &scale_bits, uint16_t &bias_bits) {
#pragma clang fp contract(off)
    const float range = hi - lo;
    float scale = range / 15.0f;
    scale = fmaxf(scale, 1e-7f);
    const bool side = fabsf(lo) > fabsf(hi);
    scale = side ? scale : -scale;
    const float edge = side ? lo : hi;
    const float q0 = rintf(edge / scale);
    const bool nz = q0 != 0.f;
    const float snapped = edge / (nz ? q0 : 1.0f);
    scale = nz ? snapped : scale;
    const float bias = nz ? edge : 0.f;
    scale_bits = BF16::from_float(scale);
    bias_bits = BF16::from_float(bias);
}

// quantize_affine's lines `safe = ...` and `q = clip(rint((g - bias) / safe), 0, 15)` for a lane's 8 elements, packed: element i in
// bits [4i, 4i + 4)
__device__ __forceinline__ uint32_t quantize_codes(const float (&x)[8], uint16_t scale_bits, uint16_t bias_bits) {
#pragma clang fp contract(off)
    const float scale = BF16::to_float(scale_bits);
    const float bias = BF16::to_float(bias_bits);
    const float safe = scale == 0.f ? 1.0f : scale;
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float centred = x[i] - bias;
        float q = centred / safe;
        q = rintf(q);
        q = fminf(fmaxf(q, 0.f), 15.f);
        word |= (uint32_t)q << (4 * i);
    }
    return word;
}

template <typename TT>
__global__ __launch_bounds__(QW4_THREADS) void quantize_w4_kernel(const typename TT::storage *__restrict__ w, long groups,
                                                                   uint32_t *__restrict__ packed, uint16_t *__restrict__ scales,
                                                                   uint16_t *__restrict__ biases) {
    const int sub = threadIdx.x & 15;  // lane within its DPP row = word within the group
    const long stride = (long)gridDim.x * QW4_GROUPS_PER_BLOCK;
    // g is uniform over a DPP row: a row leaves the loop as a whole, and the rotations below never leave the row
    for (long g = (long)blockIdx.x * QW4_GROUPS_PER_BLOCK + (threadIdx.x >> 4); g < groups; g += stride) {
        float x[8];
        quantize_load8<TT>(w + g * QW4_GROUP + sub * QW4_LANE_ELEMS, x);
        float lo = fminf(fminf(fminf(x[0], x[1]), fminf(x[2], x[3])), fminf(fminf(x[4], x[5]), fminf(x[6], x[7])));
        float hi = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
        lo = group16_min_self(lo);
        hi = group16_max(hi);
        uint16_t scale_bits, bias_bits;
        quantize_rule(lo, hi, scale_bits, bias_bits);
        packed[g * 16 + sub] = quantize_codes(x, scale_bits, bias_bits);
        if (sub < 2) (sub ? biases : scales)[g] = sub ? bias_bits : scale_bits;
    }
}

}  // namespace tl
