// The W4 x 16-bit MFMA fragment pieces the tile GEMMs share (qmm.hip: qmm_mfma_kernel; moe_grouped.h): the 32x32x16 matrix
// instruction per 16-bit type and the dequantisation of one packed word into a lane's B fragment.
#pragma once
#include "common.h"

namespace tl {

template <typename TT>
struct Mfma;
template <>
struct Mfma<BF16> {
    __device__ __forceinline__ static f32x16 mma(const u32x4 &a, const u32x4 &b, const f32x16 &c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b),
                                                       c, 0, 0, 0);
    }
};
template <>
struct Mfma<F16> {
    __device__ __forceinline__ static f32x16 mma(const u32x4 &a, const u32x4 &b, const f32x16 &c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b),
                                                      c, 0, 0, 0);
    }
};

template <typename TT>
__device__ __forceinline__ u32x4 dequant_word(uint32_t w, float s, float beta) {
    // even nibbles as the bytes of one word, odd nibbles as the bytes of another: each of the 8 conversions is then a single
    // v_cvt_f32_ubyteN (3 mask / shift instructions per word instead of 2 per nibble; the counters showed 11 VALU per MFMA)
    uint32_t even = w & 0x0f0f0f0fu, odd = (w >> 4) & 0x0f0f0f0fu;
    asm volatile("" : "+v"(even), "+v"(odd));  // or the optimiser folds the masks back into per-nibble shift + and
    u32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float lo = (float)((even >> (8 * e)) & 0xffu) * s + beta;
        const float hi = (float)((odd >> (8 * e)) & 0xffu) * s + beta;
        r[e] = TT::pack2(lo, hi);
    }
    return r;
}

}  // namespace tl
