// Launcher of the decode attention on the matrix cores (attn_mfma.h).
#include "attn_mfma.h"

namespace tl {

void launch_attn_decode_mfma(const AttnDecodeArgs &a, const AttnPlan &plan, hipStream_t st) {
    const dim3 grid(plan.grid[0], plan.grid[1], plan.grid[2]);
#define ATTN_CASE(QP, KV8) \
    if (plan.qp == QP && plan.kv8 == KV8) hipLaunchKernelGGL((attn_decode_mfma_kernel<QP, KV8>), grid, dim3(256), plan.lds_bytes, st, a);
    ATTN_MFMA_TABLE(ATTN_CASE)
#undef ATTN_CASE
}

}  // namespace tl
