// The launch of the decode attention (host only; included by engine.hip, same translation unit): what an engine -- or an operator entry
// point, on its stack -- owns for it (AttnCtx), one layer's call (AttnCall), and the one function that turns a plan (attn_plan.h) into
// the attention launch and, where the plan has one, the merge launch behind it.
#pragma once

#include "attn_mfma.h"      // launch_attn_decode_mfma; with it engine_kernels.h and attn_plan.h
#include "decode_linear.h"  // KeptPartials, ProfCtx

namespace tl {

struct AttnCtx {
    AttnGeometry geometry;
    AttnKnobs knobs;
    float eps = 0.f, rope_theta = 0.f;
    hipStream_t stream = nullptr;
    const int32_t *block_table = nullptr, *context_lens = nullptr;
    const float2 *rope_cur = nullptr;
    size_t ws_bytes = 0;  // what AttnCall::ws holds at least (an engine: the arena's piece, which the prefill operators share)
    AttnPlan plan(int batch, int max_ctx, bool kv8) const { return plan_decode_attention(geometry, knobs, batch, max_ctx, kv8); }
};

// One layer's decode attention: qkv [batch, (Hq + 2 Hkv) D] -> out [batch, Hq D] over slots [0, batch), split partials in ws.
struct AttnCall {
    const uint16_t *qkv = nullptr;
    const void *q_norm = nullptr, *k_norm = nullptr;
    uint16_t *key_pages = nullptr, *value_pages = nullptr;
    float *key_scales = nullptr, *value_scales = nullptr;  // FP8 pages (kv8.h)
    uint16_t *out = nullptr;
    float *ws = nullptr;
    KeptPartials qkv_parts;  // where the qkv projection left its slice planes: the kernel adds them itself
};

// q/k-norm + RoPE + KV append + decode attention of one layer, and the plan's merge launch (plan.launches() in all; a plan whose windows
// the wo GEMV merges leaves `out` unwritten)
static int launch_decode_attention(const AttnCtx &ctx, const AttnPlan &plan, const AttnCall &t, int batch, ProfCtx *pc) {
    const AttnGeometry &g = ctx.geometry;
    const int D = g.head_dim;
    prof_t *pb = pc ? pc->buf : nullptr;
    TL_REQUIRE(t.key_scales == nullptr || D == 128, "engine: FP8 pages need head_dim 128");
    TL_REQUIRE(plan.kv8 == (t.key_scales != nullptr) && plan.qp == (t.qkv_parts.partial != nullptr && !plan.refuses_qkv_partials) &&
                   plan.grid[2] == (unsigned)batch, "engine: the decode-attention plan was made for another call");
    TL_REQUIRE(!plan.refuses_qkv_partials, "engine: this decode-attention plan does not read qkv slice partials");
    AttnDecodeArgs a{};
    a.qkv = t.qkv, a.q_norm_w = (const uint16_t *)t.q_norm, a.k_norm_w = (const uint16_t *)t.k_norm;
    a.key_pages = t.key_pages, a.value_pages = t.value_pages, a.key_scales = t.key_scales, a.value_scales = t.value_scales;
    a.block_table = ctx.block_table, a.context_lens = ctx.context_lens, a.rope_cur = ctx.rope_cur, a.out = t.out, a.ws = t.ws, a.prof = pb;
    a.page_size = g.page_size, a.max_pages = g.max_pages, a.num_heads = g.num_heads, a.num_kv_heads = g.num_kv_heads;
    a.scale = 1.0f / sqrtf((float)D), a.eps = ctx.eps, a.rope_base = ctx.rope_theta;
    a.n_splits = plan.n_splits, a.n_row_chunks = plan.row_chunks, a.tokens_per_split = plan.tokens_per_split;
    a.split_shift = plan.split_shift, a.rep = plan.rep, a.page_shift = plan.page_shift;
    if (plan.qp) a.qkv_partial = t.qkv_parts.partial, a.qkv_slices = t.qkv_parts.slices, a.qkv_plane = t.qkv_parts.plane;
    TL_REQUIRE(plan.partials_bytes(batch) <= ctx.ws_bytes || plan.n_splits == 1, "engine: attention workspace too small for this split plan");
    if (!attn_plan_has_variant(plan)) return fail(TL_ERR_UNSUPPORTED, "engine: head_dim must be 32, 64 or 128");
    const dim3 grid(plan.grid[0], plan.grid[1], plan.grid[2]);
    if (plan.walk == AttnWalk::MATRIX_CORE) {
        launch_attn_decode_mfma(a, plan, ctx.stream);
    } else {
        const bool sp = plan.walk == AttnWalk::SINGLE_PAGE, ip = plan.walk == AttnWalk::STAGE_PAGE;
#define ATTN_CASE(VD, RQ, SP, IP, QP, KV8)                                                                              \
    if (D == 16 * VD && plan.rq == RQ && sp == SP && ip == IP && plan.qp == QP && plan.kv8 == KV8)                      \
        hipLaunchKernelGGL((attn_decode_fused_kernel<VD, 4, RQ, SP, IP, QP, KV8>), grid, dim3(256), plan.lds_bytes, ctx.stream, a);
        ATTN_FUSED_TABLE(ATTN_CASE)
#undef ATTN_CASE
    }
    if (pc) prof_after(pc, 5, (int)(grid.x * grid.y * grid.z));
    const dim3 mg(batch * g.num_heads), mb(128);
    switch (plan.merge) {
        case AttnMerge::NONE: break;
        case AttnMerge::M2: hipLaunchKernelGGL(attn_merge_kernel<2>, mg, mb, 0, ctx.stream, t.ws, t.out, D, pb); break;
        case AttnMerge::M4: hipLaunchKernelGGL(attn_merge_kernel<4>, mg, mb, 0, ctx.stream, t.ws, t.out, D, pb); break;
        case AttnMerge::M8: hipLaunchKernelGGL(attn_merge_kernel<8>, mg, mb, 0, ctx.stream, t.ws, t.out, D, pb); break;
        case AttnMerge::COLUMNS:  // 16 and more splits: a row's partials spread over D / 32 workgroups x 8 split groups
            hipLaunchKernelGGL(attn_merge_cols_kernel, dim3(mg.x, (D + 31) / 32), dim3(256), 0, ctx.stream, t.ws, t.out, D, plan.n_splits, pb);
            break;
    }
    if (pc && plan.merge != AttnMerge::NONE) prof_after(pc, 6, (int)mg.x * (plan.merge == AttnMerge::COLUMNS ? (D + 31) / 32 : 1));
    TL_CHECK_LAUNCH("engine attention");
    return TL_OK;
}

}  // namespace tl
