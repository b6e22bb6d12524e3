// tl_quantize_w4: checks and launch of the affine W4 quantiser (quantize_w4.h).
#include "quantize_w4.h"

#include <algorithm>

using namespace tl;

namespace {

// enough workgroups for 8 waves on every SIMD of a 256-CU part (the kernel needs few registers, so they are all resident): each wave
// keeps 1 KB of loads in flight, and the grid-stride loop covers whatever is left
constexpr long QW4_MAX_BLOCKS = 256 * 8;

template <typename TT>
void launch_quantize_w4(const void *w, long groups, uint32_t *packed, void *scales, void *biases, hipStream_t st) {
    const int blocks = (int)std::min<long>((groups + QW4_GROUPS_PER_BLOCK - 1) / QW4_GROUPS_PER_BLOCK, QW4_MAX_BLOCKS);
    hipLaunchKernelGGL((quantize_w4_kernel<TT>), dim3(blocks), dim3(QW4_THREADS), 0, st, (const typename TT::storage *)w, groups,
                       packed, (uint16_t *)scales, (uint16_t *)biases);
}

}  // namespace

extern "C" int tl_quantize_w4(const void *w, long rows, int cols, tl_dtype src_dtype, uint32_t *packed, void *scales, void *biases,
                              void *stream) {
    TL_REQUIRE(cols > 0 && cols % QW4_GROUP == 0, "quantize_w4: cols must be a positive multiple of the group size 128");
    TL_REQUIRE(rows >= 0, "quantize_w4: rows must not be negative");
    if (rows == 0) return TL_OK;  // (an empty tensor's pointers may be null: nothing is read or written)
    TL_REQUIRE(w && packed && scales && biases, "quantize_w4: null pointer");
    TL_REQUIRE((uintptr_t)w % 16 == 0 && (uintptr_t)packed % 16 == 0, "quantize_w4: the input and the packed output must be 16-byte aligned");
    TL_REQUIRE((uintptr_t)scales % 2 == 0 && (uintptr_t)biases % 2 == 0, "quantize_w4: scales and biases must be 2-byte aligned");
    const long groups = rows * (long)(cols / QW4_GROUP);
    hipStream_t st = (hipStream_t)stream;
    switch (src_dtype) {
        case TL_F32: launch_quantize_w4<F32>(w, groups, packed, scales, biases, st); break;
        case TL_F16: launch_quantize_w4<F16>(w, groups, packed, scales, biases, st); break;
        case TL_BF16: launch_quantize_w4<BF16>(w, groups, packed, scales, biases, st); break;
        default: return fail(TL_ERR_INVALID, "quantize_w4: expected float32, float16, or bfloat16");
    }
    TL_CHECK_LAUNCH("quantize_w4");
    return TL_OK;
}
