// The projection router of the decode path (host only; included by engine.hip, same translation unit): which kernel takes one
// projection of `M` activation rows (Proj) given what an engine -- or an entry point, on its stack -- owns for it (LinearCtx; the decisions
// themselves are host-only code over its LinearKnobs, linear_plan.h: the planners, the routing predicates, the route of a layer), and the
// kernel-level entry points tl_decode_linear[_ex] that run the same functions on caller-owned buffers.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tinyllm_engine.h"
#include "common.h"
#include "device_block.h"
#include "engine_kernels.h"
#include "qmv.h"
#include "qmv3.h"
#include "qmm3.h"
#include "qmm6.h"
#include "qmm7.h"
#include "gemm8.h"

namespace tl {

#define TL_TRY(expr)                  \
    do {                              \
        const int rc__ = (expr);      \
        if (rc__ != TL_OK) return rc__; \
    } while (0)

// ---- profile step bookkeeping -------------------------------------------------------------------------
// tl_engine_check_step (test-only): the hand-over regions -- [0] the shared activations of the arena, [1] the per-layer buffers -- with
// a shadow copy and one "written this step" byte per 2-byte element each, alive only inside the call
struct WrittenOnceCheck {
    char *region[2] = {nullptr, nullptr};
    size_t bytes[2] = {0, 0};
    uint32_t *shadow[2] = {nullptr, nullptr};
    uint8_t *written[2] = {nullptr, nullptr};
    unsigned long long *report = nullptr;
};

// kinds: 0..4 GEMV (qkv, o, gate_up, down, lm_head), 5 attention, 6 merge, 7 step end
struct ProfCtx {
    hipStream_t stream = nullptr;             // the stream of the stamped launches
    const WrittenOnceCheck *check = nullptr;  // tl_engine_check_step: the checker runs behind every stamped launch
    DeviceBlock buf_mem, pairs_mem;
    prof_t *buf = nullptr;    // per-workgroup (start, end) pairs of the launch in flight
    prof_t *pairs = nullptr;  // [n][2] reduced (start, end) per launch
    std::vector<int> kinds;
    int cap = 0;
    // room for one eagerly launched step over `batch` rows (tl_engine_profile_step, tl_engine_check_step): the largest grid of the
    // step -- the lm_head GEMV (4 rows per workgroup at worst) or the attention grid -- and up to 11 launches per layer at 5 .. 64 rows
    // (four skinny matmuls + reductions, attention, merge, norms); the stamps start zeroed, stream-ordered
    bool alloc(const tl_engine_config &c, int batch, hipStream_t st) {
        stream = st;
        const size_t buf_bytes = (size_t)(std::max(c.vocab_size / 4 + 64, 64 * 4 * c.num_kv_heads * batch) + 1024) * 2 * sizeof(prof_t);
        cap = c.num_layers * 12 + 8;
        if (buf_mem.alloc(buf_bytes, "hipMalloc(stamps) failed") != TL_OK || pairs_mem.alloc((size_t)cap * 2 * sizeof(prof_t), "hipMalloc(stamp pairs) failed") != TL_OK)
            return false;
        buf = buf_mem.at<prof_t>(), pairs = pairs_mem.at<prof_t>();
        return hipMemsetAsync(buf, 0, buf_bytes, stream) == hipSuccess;
    }
};

static void prof_after(ProfCtx *pc, int kind, int n_wg) {
    const int idx = (int)pc->kinds.size();
    if (idx >= pc->cap) return;
    hipLaunchKernelGGL(prof_reduce_kernel, dim3(1), dim3(1024), 0, pc->stream, pc->buf, n_wg, pc->pairs + 2 * (size_t)idx);
    pc->kinds.push_back(kind);
    if (pc->check)  // what this launch (and any unstamped one ahead of it) stored, against "written once per step"
        for (int rg = 0; rg < 2; ++rg)
            if (pc->check->bytes[rg])
                hipLaunchKernelGGL(written_once_check_kernel, dim3(1024), dim3(256), 0, pc->stream, (const uint32_t *)pc->check->region[rg],
                                   pc->check->shadow[rg], pc->check->written[rg], pc->check->bytes[rg] / 4, idx, rg, pc->check->report);
}

// ---- what the router reads ------------------------------------------------------------------------------
// a W4 matrix in the tiled MFMA layout (qmv3.h)
struct TiledW4 {
    uint32_t *wt = nullptr, *sbt = nullptr;
};
// ... and the owner of its two allocations
struct TiledW4Mem {
    DeviceBlock wt, sbt;
};
// the tiled copy of `w` (rows a multiple of 16, columns of 128) into fresh allocations, repacked on `st`; all or nothing
static int tiled_w4_make(const tl_w4 &w, hipStream_t st, TiledW4Mem &mem, TiledW4 &t, const char *alloc_failed, const char *repack_failed) {
    const size_t wbytes = (size_t)w.rows * w.cols / 2, sbytes = (size_t)w.rows * (w.cols / 128) * 4;
    TiledW4Mem m;
    TL_TRY(m.wt.alloc(wbytes + 16384, alloc_failed));  // + slack: fixed-length wave slices
    TL_TRY(m.sbt.alloc(sbytes + 1024, alloc_failed));
    if (repack_w4_tiled(w.weight_dev, (const uint16_t *)w.scales_dev, (const uint16_t *)w.biases_dev, m.wt.at<uint32_t>(), m.sbt.at<uint32_t>(), w.rows,
                        w.cols, st) != 0)
        return fail(TL_ERR_HIP, repack_failed);
    t.wt = m.wt.at<uint32_t>(), t.sbt = m.sbt.at<uint32_t>();
    mem = std::move(m);
    return TL_OK;
}

// the router's scratch: the buffers a caller may stand its own in for the duration of a pass (the batched verification's 64 rows)
struct LinearScratch {
    uint16_t *xn = nullptr;  // rows of an RMSNorm that runs as its own launch
    uint16_t *gu = nullptr, *tmp = nullptr;  // GEMM path with separate epilogue launches: gate|up rows ahead of SwiGLU, the product ahead of the residual add
    // split-K partials of the GEMM and slice planes of the skinny matmul (a call may bring planes of its own: Proj::planes)
    void *splitk_ws = nullptr;
    size_t splitk_ws_bytes = 0;
};
struct LinearCtx : LinearScratch, LinearKnobs {
    hipStream_t stream = nullptr;
    float rms_norm_eps = 0.f;
    // decode-path copy of every W4 matrix in the tiled MFMA layout (qmv3.h); keyed by the checkpoint pointer
    std::map<const uint32_t *, TiledW4> tiled;
    // Prefill chunks of GEMM8_MIN_ROWS (1,792) rows and more (an engine created with max_prefill_rows that large): the layer matrices once more as
    // bf16 -- bf16(q * s + beta), the B operand the reference's tile GEMM forms in threadgroup memory (quantized_matmul.metal:96-249) -- for
    // the plain bf16 GEMM of gemm8.h (256 x 256 tiles by LDS-DMA, no dequantisation in the loop).  7.3 GB at Qwen3-4B, of 288.
    std::map<const uint32_t *, uint16_t *> bf16w;
    bool use_gemm8 = true;  // tl_engine_set_option "gemm8" = 0: every chunk through the W4 GEMM (qmm.hip), the twin
    bool fuse_reduce_norm = true;  // "prefill_reduce_norm" = 0: the split-K residual reduction and the RMSNorm behind it as two launches, the twin
    bool gemm_fused_epilogue = true;    // tl_engine_set_option "gemm_fused_epilogue" = 0: residual / SwiGLU of the prefill GEMM as separate launches
    tl_linear_info *linfo = nullptr;    // kernel-level entry points: which kernel a projection ran
    // what the routing (linear_plan.h) sees of a matrix, of a layer
    ProjShape shape(const tl_w4 &w) const { return ProjShape{w.rows, w.cols, tiled.count(w.weight_dev) != 0}; }
    LayerShapes shapes(const tl_layer_weights &w) const { return LayerShapes{shape(w.wqkv), shape(w.wo), shape(w.wgu), shape(w.wdown), w.wgu.weight_dev != nullptr}; }
};

// ---- one projection, by name ------------------------------------------------------------------------------
struct KeptPartials {
    const float *partial = nullptr;
    int slices = 0;
    long plane = 0;  // elements between slices (= rows * output columns)
};

// out = epilogue(prologue(a) @ w^T) over M rows.  One record for engine_qmv / engine_qmm6 / engine_linear / engine_gemm; a field the
// route that runs does not take is an error there (their TL_REQUIREs), never ignored silently.
struct Proj {
    const tl_w4 *w = nullptr;
    const uint16_t *a = nullptr;  // [M, cols]; PRO_ATTN_MERGE reads merge_ws instead
    uint16_t *out = nullptr;      // [M, rows] ([M, rows / 2] behind EPI_SWIGLU)
    int M = 0;
    int pro = PRO_NONE, epi = EPI_STORE;
    const void *norm_w = nullptr;        // PRO_RMSNORM: its weight
    const uint16_t *residual = nullptr;  // EPI_RESIDUAL: its rows
    int kind = 0;                        // the profile kind of the launches (ProfCtx)
    // partial sums of squares of the rows of `a` ([M][ss_in_n]) where its producer left them: the skinny matmul reads exactly QM3_SS per
    // row (what the embedding kernels and its own reduction leave), the GEMV any number, qmm6 takes them with WEIGHTED rows in `a`
    const float *ss_in = nullptr;
    int ss_in_n = QM3_SS;
    float *ss_out = nullptr;  // EPI_RESIDUAL: where to leave those of `out`; ProjResult::ss_n says how many per row were written
    // EPI_RESIDUAL: also leave out * norm_out in out_w for a consumer of weighted rows (engine_gemm: the RMSNorm behind the projection,
    // out_w its rows, where the split-K reduction can take it along)
    const void *norm_out = nullptr;
    uint16_t *out_w = nullptr;
    // the weighted rows on either side (`a` with ss_in, `out_w`) lie in fragment order (qmm6.h) -- the engine's own hand-over;
    // out_w_frag >= 0 decides for out_w alone (the kernel-level entry point)
    bool frag = false;
    int out_w_frag = -1;
    // EPI_STORE on the skinny matmul: the caller's consumer adds the slices itself -- the reduction launch is skipped, ProjResult::kept
    // says where the fp32 planes are and `out` is NOT written (kept.partial stays null when another kernel took the projection)
    bool keep = false;
    // the skinny matmul's fp32 slice planes when they are not the context's workspace (a step on the per-layer buffers)
    float *planes = nullptr;
    size_t planes_bytes = 0;
    // PRO_ATTN_MERGE (the wo GEMV of ONE row, h = x + merge(attention partials) @ wo^T): the decode-attention split partials
    const float *merge_ws = nullptr;
    int n_splits = 0;
    f32x2 *tile_max = nullptr;  // a single-pass EPI_STORE GEMV leaves its per-16-row (max, lowest index) pairs here (qmv3.h tile_max)
};
static Proj proj(const tl_w4 &w, const uint16_t *a, uint16_t *out, int M) { return Proj{&w, a, out, M}; }

struct ProjResult {
    int ss_n = 0;           // partials per row left in ss_out: QM3_SS by the slice reduction, rows / 16 by a GEMV or qmm6, 0 = none
    KeptPartials kept;      // Proj::keep
    int maxima_rows = 0;    // rows whose pairs were left in Proj::tile_max (0 = none)
};

static int check_w4(const tl_w4 &w, int rows, int cols, const char *name) {
    if (!w.weight_dev || !w.scales_dev || !w.biases_dev)
        return fail(TL_ERR_INVALID, std::string("engine: null weight pointer in ") + name);
    if (w.rows != rows || w.cols != cols)
        return fail(TL_ERR_INVALID, std::string("engine: unexpected shape for ") + name + " (got " +
                                        std::to_string(w.rows) + "x" + std::to_string(w.cols) + ", want " +
                                        std::to_string(rows) + "x" + std::to_string(cols) + ")");
    if ((uintptr_t)w.weight_dev % 16 != 0)
        return fail(TL_ERR_INVALID, std::string("engine: weight not 16-byte aligned: ") + name);
    return TL_OK;
}

// tl_linear_info of the kernel-level entry points: the kernel that ran (the packed-dot fallback, 3, sticks once a pass took it), its
// launches, the rows per pass and the plan
static void report_launch(const LinearCtx &ctx, int kernel, int launches, int rows_per_pass, std::initializer_list<int> plan = {}) {
    if (!ctx.linfo) return;
    tl_linear_info &li = *ctx.linfo;
    li.kernel = kernel == 1 && li.kernel == 3 ? 3 : kernel;
    li.launches += launches;
    li.rows_per_pass = rows_per_pass;
    std::copy(plan.begin(), plan.end(), li.p);
}

// GEMV with fused prologue/epilogue over M <= 8 rows; splits the rows when the activation tile exceeds LDS.
static int engine_qmv(LinearCtx &ctx, const Proj &p, ProfCtx *pc = nullptr, ProjResult *res = nullptr) {
    // norm_out / out_w (EPI_RESIDUAL): the caller has checked (weighted_rows_apply) that the MFMA GEMV takes all rows in one pass --
    // anything else is an error, not a silent fallback
    ProjResult none, &r = res ? *res : none;
    r = ProjResult{};
    const tl_w4 &w = *p.w;
    const int M = p.M;
    const bool merge = p.pro == PRO_ATTN_MERGE;  // qmv3.hip, launch_qmv3_attn_merge_bf16: the instantiated plans (wo_merge_applicable)
    bool all_emitted = p.ss_out != nullptr && p.epi == EPI_RESIDUAL && ctx.gemv_producer_ss;
    int step = std::min(M, 8);  // both GEMV kernels hold at most 8 activation rows (MR <= 8): more rows go in passes of 8
    const auto tiled = ctx.tiled.find(w.weight_dev);
    const bool has_tiled = tiled != ctx.tiled.end();
    auto fits = [&](int rows) {
        return (has_tiled && qmv3_plan(rows, w.cols, w.rows).ok) || qmv_plan(rows, w.cols, w.rows).lds <= 150 * 1024;
    };
    while (!fits(step) && step > 1) step = (step + 1) / 2;
    const int out_cols = p.epi == EPI_SWIGLU ? w.rows / 2 : w.rows;
    for (int m0 = 0; m0 < M; m0 += step) {
        QmvArgs args{};
        args.scales = (const uint16_t *)w.scales_dev;
        args.biases = (const uint16_t *)w.biases_dev;
        args.b = w.weight_dev;
        args.a = p.a + (size_t)m0 * w.cols;
        args.out = p.out + (size_t)m0 * out_cols;
        args.norm_w = (const uint16_t *)p.norm_w;
        args.residual = p.residual ? p.residual + (size_t)m0 * w.rows : nullptr;
        args.eps = ctx.rms_norm_eps;
        args.M = std::min(step, M - m0);
        args.N = w.cols;
        args.K = w.rows;
        args.prof = pc ? pc->buf : nullptr;
        const Qmv3Plan p3 = qmv3_plan(args.M, args.N, args.K);
        if (has_tiled && (p3.ok || merge)) {
            Qmv3Args a3{};
            a3.wt = tiled->second.wt;
            a3.sbt = tiled->second.sbt;
            a3.a = merge ? nullptr : args.a;
            a3.merge_ws = merge ? const_cast<float *>(p.merge_ws) : nullptr;
            a3.out = args.out;
            a3.norm_w = args.norm_w;
            a3.residual = args.residual;
            a3.eps = args.eps;
            a3.M = args.M;
            a3.N = args.N;
            a3.K = args.K;
            a3.prof = args.prof;
            if (ctx.gemv_producer_ss) {
                if ((p.pro == PRO_RMSNORM || p.pro == PRO_RMS_WEIGHTED) && p.ss_in && p.ss_in_n > 0)
                    a3.ss_in = p.ss_in + (size_t)m0 * p.ss_in_n, a3.ss_n = p.ss_in_n;
                if (p.epi == EPI_RESIDUAL && p.ss_out) a3.ss_out = p.ss_out + (size_t)m0 * (w.rows / 16);
            }
            if (p.tile_max && p.epi == EPI_STORE && step == M && w.rows % 16 == 0) {
                a3.tile_max = p.tile_max;
                r.maxima_rows = M;
            }
            if (p.out_w) {
                TL_REQUIRE(p.epi == EPI_RESIDUAL && p.norm_out && step == M, "engine: weighted rows need the residual epilogue and one pass");
                a3.norm_out = (const uint16_t *)p.norm_out;
                a3.out_w = p.out_w;
            }
            if ((merge ? launch_qmv3_attn_merge_bf16(a3, p3, p.n_splits, ctx.stream) : launch_qmv3_bf16(a3, p3, p.pro, p.epi, ctx.stream)) != 0)
                return fail(TL_ERR_UNSUPPORTED, merge ? "engine: no wo GEMV that merges the attention partials for this shape" : "engine: MFMA GEMV launch failed");
            if (pc) prof_after(pc, p.kind, p3.blocks);
            report_launch(ctx, 1, 1, step, {p3.MR, p3.KS, p3.CW, p3.LM, p3.blocks});
            continue;
        }
        all_emitted = false;  // the packed-dot fallback leaves no partials
        TL_REQUIRE(p.out_w == nullptr && p.pro != PRO_RMS_WEIGHTED && !merge, "engine: weighted rows are a route of the MFMA GEMV only");
        if (launch_qmv_fused_bf16(args, p.pro, p.epi, ctx.stream) != 0)
            return fail(TL_ERR_UNSUPPORTED, "engine: no GEMV configuration for this shape");
        if (pc) prof_after(pc, p.kind, qmv_plan(args.M, args.N, args.K).blocks);
        report_launch(ctx, 3, 1, step);
    }
    TL_CHECK_LAUNCH(merge ? "engine wo gemv with merge" : "engine gemv");
    if (all_emitted && w.rows % 16 == 0) r.ss_n = w.rows / 16;
    return TL_OK;
}

// The split-K / skinny-matmul workspace is sized ONCE in tl_engine_create for every shape the engine can launch
// (instantiated graphs hold its address, and a capture cannot synchronise or allocate): a request beyond it is an error.
static int ensure_splitk(const LinearCtx &ctx, size_t bytes) {
    if (bytes <= ctx.splitk_ws_bytes) return TL_OK;
    return fail(TL_ERR_INVALID, "engine: matmul workspace too small for this shape (sized at tl_engine_create: " +
                                    std::to_string(ctx.splitk_ws_bytes) + " bytes, need " + std::to_string(bytes) + ")");
}

// Reference-semantics GEMM over the checkpoint layout (weights rounded to bf16 first): tl_quantized_matmul.
static int engine_qmm(LinearCtx &ctx, const tl_w4 &w, const uint16_t *a, uint16_t *out, int M) {
    const size_t need = tl_quantized_matmul_workspace_bytes(M, w.cols, w.rows, TL_BF16, 1, 1);
    TL_TRY(ensure_splitk(ctx, need));
    return tl_quantized_matmul(w.scales_dev, w.biases_dev, a, w.weight_dev, out, M, w.cols, w.rows, 128, 4, TL_BF16, 1, 1,
                               ctx.splitk_ws, ctx.splitk_ws_bytes, ctx.stream);
}

// out = epilogue(a @ W^T) for any number of rows (chunked prefill, batches above 64): the reference's own op sequence --
// W4 MFMA GEMM over the checkpoint layout (quantize.py:54-65 routes rows > 8 to the matmul path, whose tile kernel rounds
// the dequantised weights to bf16 first), then SwiGLU / residual as separate launches.
// From this many rows a chunk's projections run on the plain bf16 GEMM (gemm8.h).  In the lab (back-to-back launches on one weight matrix, which then sits in the
// 256-MB Infinity Cache) gemm8 wins from ~1,500 rows; in the ENGINE every layer streams its own 202 MB of bf16 weights from HBM and the grid counts in
// whole 256-row bands, measured at the end of round 6 (chunked prefill of 6,144 / 8,192 tokens, gemm8 / W4 GEMM, tokens/s): 1,536-row chunks 63.0k / 71.7k,
// 2,048 83.8k / 75.6k, 3,072 77.7k / 78.0k, 4,096 100.5k / 75.9k -- so from 7 bands (until then the constant was 1,536: 12 % slower at exactly that size).
constexpr int GEMM8_MIN_ROWS = 1792;
static bool gemm8_wins(int M) { return M >= GEMM8_MIN_ROWS; }
// p.norm_out / p.out_w / norm_done: the RMSNorm that follows an EPI_RESIDUAL projection (its weight, its rows), taken along by its split-K reduction
// pass where there is one (small chunks on the W4 GEMM); *norm_done says whether out_w was written -- the caller launches tl_rms_norm otherwise
static int engine_gemm(LinearCtx &ctx, const Proj &p, bool *norm_done = nullptr) {
    const tl_w4 &w = *p.w;
    const int M = p.M;
    if (norm_done) *norm_done = false;
    if (ctx.use_gemm8 && gemm8_wins(M)) {
        const auto wb = ctx.bf16w.find(w.weight_dev);
        if (wb != ctx.bf16w.end() && gemm8_applicable(M, w.rows, w.cols)) {
            Gemm8Args g{};
            g.a = p.a, g.w = wb->second, g.out = p.out, g.residual = p.residual, g.M = M, g.N = w.rows, g.K = w.cols;
            if (launch_gemm8_bf16(g, p.epi, ctx.stream) != 0) return fail(TL_ERR_UNSUPPORTED, "engine: bf16 GEMM launch failed");
            TL_CHECK_LAUNCH("engine bf16 matmul");
            return TL_OK;
        }
    }
    if (p.epi != EPI_STORE && M > 8 && ctx.gemm_fused_epilogue) {  // residual / SwiGLU inside the GEMM store or its split-K reduction
        const size_t need = tl_quantized_matmul_workspace_bytes(M, w.cols, w.rows, TL_BF16, 1, 1);
        TL_TRY(ensure_splitk(ctx, need));
        TL_TRY(qmm_bf16_epilogue(w.scales_dev, w.biases_dev, p.a, w.weight_dev, p.out, M, w.cols, w.rows, p.epi, p.residual, ctx.splitk_ws,
                                 ctx.splitk_ws_bytes, ctx.stream, ctx.fuse_reduce_norm ? (const uint16_t *)p.norm_out : nullptr, p.out_w,
                                 ctx.rms_norm_eps, norm_done));
        TL_CHECK_LAUNCH("engine matmul");
        return TL_OK;
    }
    uint16_t *plain = p.epi == EPI_STORE ? p.out : (p.epi == EPI_SWIGLU ? ctx.gu : ctx.tmp);
    TL_TRY(engine_qmm(ctx, w, p.a, plain, M));
    if (p.epi == EPI_SWIGLU) {
        const long n4 = (long)M * (w.rows / 2) / 4;
        hipLaunchKernelGGL(swiglu_interleaved_kernel, dim3(ceil_div(n4, 256)), dim3(256), 0, ctx.stream, plain, p.out, n4);
    } else if (p.epi == EPI_RESIDUAL) {
        const long n8 = (long)M * w.rows / 8;
        hipLaunchKernelGGL(residual_add_kernel, dim3(ceil_div(n8, 256)), dim3(256), 0, ctx.stream, p.residual, plain, p.out, n8);
    }
    TL_CHECK_LAUNCH("engine matmul");
    return TL_OK;
}

// One projection through qmm6: `a` plain rows, or (ss_in given) WEIGHTED rows whose 1 / rms scales the result.  EPI_RESIDUAL: ss_out
// receives rows / 16 partial sums of squares per row, out_w the rows weighted for the next RMSNorm (norm_out).
static int engine_qmm6(LinearCtx &ctx, const Proj &p, ProfCtx *pc = nullptr, ProjResult *res = nullptr) {
    ProjResult none, &r = res ? *res : none;
    r = ProjResult{};
    const tl_w4 &w = *p.w;
    const int M = p.M;
    const auto tiled = ctx.tiled.find(w.weight_dev);
    TL_REQUIRE(tiled != ctx.tiled.end(), "engine: the register-resident matmul needs the tiled weights");
    const bool a_frag = p.frag && p.ss_in != nullptr && p.epi != EPI_RESIDUAL;
    const Qmm7Plan p7 = (ctx.use_qmm7 || ctx.force_qmm7) && a_frag && p.out_w == nullptr ? qmm7_plan(M, w.cols, w.rows, ctx.ncu) : Qmm7Plan{};
    TL_REQUIRE(p7.ok || !ctx.force_qmm7, "engine: the row-streaming matmul takes weighted rows in fragment order (store / SwiGLU) at the shapes of qmm7_plan");
    const Qmm6Plan pl = qmm6_plan(M, w.cols, w.rows, a_frag, ctx.ncu);
    TL_REQUIRE(p7.ok || pl.ok, "engine: the register-resident matmul does not cover this shape");
    Qmm6Args q{};
    q.wt = tiled->second.wt;
    q.sbt = tiled->second.sbt;
    q.a = p.a;
    q.out = p.out;
    q.residual = p.residual;
    q.norm_out = (const uint16_t *)p.norm_out;
    q.out_w = p.out_w;
    q.ss = p.ss_in;
    q.ss_n = p.ss_in ? p.ss_in_n : 0;
    q.ss_out = p.epi == EPI_RESIDUAL ? p.ss_out : nullptr;
    q.eps = ctx.rms_norm_eps;
    q.M = M;
    q.N = w.cols;
    q.K = w.rows;
    q.prof = pc ? pc->buf : nullptr;
    q.a_frag = a_frag;
    q.out_w_frag = (p.out_w_frag >= 0 ? p.out_w_frag != 0 : p.frag) && p.out_w != nullptr;
    if (p7.ok) {
        if (launch_qmm7_bf16(q, p7, p.epi, ctx.stream) != 0) return fail(TL_ERR_UNSUPPORTED, "engine: row-streaming matmul launch failed");
        if (pc) prof_after(pc, p.kind, p7.wgs);
        report_launch(ctx, 6, 1, p7.MB * 16, {p7.MB, p7.GPW, p7.T, p7.row_blocks, p7.wgs});
        TL_CHECK_LAUNCH("engine row-streaming matmul");
        return TL_OK;
    }
    if (launch_qmm6_bf16(q, pl, p.epi, ctx.stream) != 0) return fail(TL_ERR_UNSUPPORTED, "engine: register-resident matmul launch failed");
    if (pc) prof_after(pc, p.kind, pl.wgs * pl.row_blocks);
    if (q.ss_out) r.ss_n = w.rows / 16;
    report_launch(ctx, 5, 1, pl.MB * 16, {pl.MB, pl.GPW, pl.NSETS, pl.row_blocks, pl.wgs * pl.row_blocks});
    TL_CHECK_LAUNCH("engine register-resident matmul");
    return TL_OK;
}

// One projection of the decode step over `M` activation rows.  Up to 4 rows: the fused MFMA GEMV (weights streamed once,
// RMSNorm / residual / SwiGLU inside).  5 .. 64 rows: the skinny matmul (qmm3.h) for every projection -- at 8 rows the GEMV
// re-stages all rows in every workgroup (qkv 10.3 us against 4.8 + reduction; profiles/r02_labs/batched_rows_routing.log).  More rows, or option "qmm3" = 0: the
// reference's own op sequence -- RMSNorm kernel, W4 MFMA GEMM (quantize.py:54-65 routes rows > 8 to the matmul path),
// then SwiGLU / residual kernels.
static int engine_linear(LinearCtx &ctx, const Proj &p, ProfCtx *pc = nullptr, ProjResult *res = nullptr) {
    ProjResult none, &r = res ? *res : none;
    r = ProjResult{};
    const tl_w4 &w = *p.w;
    const int M = p.M;
    if (gemv_takes_rows(ctx, M)) return engine_qmv(ctx, p, pc, &r);
    TL_REQUIRE(p.pro != PRO_ATTN_MERGE, "engine: merged attention partials are a route of the fused GEMV only");
    TL_REQUIRE(p.pro != PRO_RMS_WEIGHTED && (p.out_w == nullptr || (p.epi == EPI_RESIDUAL && p.norm_out != nullptr)),
               "engine: the skinny matmul leaves weighted rows behind a residual epilogue only, and takes none");
    const float *ss_in = qmm3_takes_ss(p.ss_in_n) ? p.ss_in : nullptr;
    const uint16_t *in = p.a;
    // qmm3_min_rows .. 64 rows (batched decode): K-sliced skinny MFMA matmul over the tiled weights, then the slice
    // reduction with the epilogue.  RMSNorm runs as its own launch (a slice does not see the whole row).
    const Qmm3Plan p3 = skinny_matmul_plan(ctx, ctx.shape(w), M);
    if (p3.ok) {
        const auto tiled = ctx.tiled.find(w.weight_dev);
        const bool fused_norm = p.pro == PRO_RMSNORM && ss_in != nullptr && ctx.fuse_norm;
        if (p.pro == PRO_RMSNORM && !fused_norm) {
            TL_TRY(tl_rms_norm(p.a, p.norm_w, ctx.xn, M, w.cols, ctx.rms_norm_eps, TL_BF16, ctx.stream));
            in = ctx.xn;
        }
        if (p.planes) TL_REQUIRE(p3.partial_bytes <= p.planes_bytes, "engine: per-layer slice planes too small for this shape");
        else TL_TRY(ensure_splitk(ctx, p3.partial_bytes));
        Qmm3Args q{};
        q.wt = tiled->second.wt;
        q.sbt = tiled->second.sbt;
        q.a = in;
        q.partial = p.planes ? p.planes : (float *)ctx.splitk_ws;
        q.M = M;
        q.N = w.cols;
        q.K = w.rows;
        q.prof = pc ? pc->buf : nullptr;
        q.norm_w = (const uint16_t *)p.norm_w;
        q.ss = ss_in;
        q.ss_n = p.ss_in_n;
        q.eps = ctx.rms_norm_eps;
        if (launch_qmm3_bf16(q, p3, ctx.stream, fused_norm ? PRO_RMSNORM : PRO_NONE) != 0)
            return fail(TL_ERR_UNSUPPORTED, "engine: skinny matmul launch failed");
        if (pc) prof_after(pc, p.kind, p3.persistent ? p3.grid_x : p3.grid_x * p3.slices);
        float *ss_dst = (p.ss_out && ctx.fuse_norm && qmm3_reduce_can_emit_ss(p.epi, w.rows)) ? p.ss_out : nullptr;
        const bool kept = p.keep && p.epi == EPI_STORE && ss_dst == nullptr;
        if (kept) {
            r.kept.partial = q.partial;
            r.kept.slices = p3.slices;
            r.kept.plane = (long)M * w.rows;
        } else {
            int reduce_wg = 0;
            if (launch_qmm3_reduce_bf16(q.partial, p3.slices, M, w.rows, p.epi, p.residual, p.out, q.prof, ctx.stream, ss_dst, &reduce_wg,
                                        p.out_w ? (const uint16_t *)p.norm_out : nullptr, p.out_w, p.frag ? 1 : 0) != 0)
                return fail(TL_ERR_UNSUPPORTED, "engine: skinny matmul reduction launch failed");
            if (pc) prof_after(pc, p.kind, reduce_wg);
        }
        r.ss_n = ss_dst != nullptr ? QM3_SS : 0;
        TL_CHECK_LAUNCH("engine skinny matmul");
        report_launch(ctx, 2, (kept ? 1 : 2) + (p.pro == PRO_RMSNORM && !fused_norm ? 1 : 0), M,
                      {p3.MB, p3.persistent ? 0 : p3.TW, p3.LM, p3.slices, p3.persistent ? p3.grid_x : p3.grid_x * p3.slices});
        return TL_OK;
    }
    if (ctx.force_linear == 2) return fail(TL_ERR_UNSUPPORTED, "engine: the skinny matmul does not cover this shape");
    TL_REQUIRE(p.out_w == nullptr, "engine: no kernel leaves weighted rows for this shape");
    if (M <= 8) return engine_qmv(ctx, p, pc, &r);
    Proj g = p;
    if (p.pro == PRO_RMSNORM) {
        TL_TRY(tl_rms_norm(p.a, p.norm_w, ctx.xn, M, w.cols, ctx.rms_norm_eps, TL_BF16, ctx.stream));
        g.a = ctx.xn;
    }
    if (ctx.linfo) ctx.linfo->kernel = 4;
    g.norm_out = nullptr;
    return engine_gemm(ctx, g);
}

}  // namespace tl

// ================================================================================================
// Kernel-level entry points of the decode path (include/tinyllm_engine.h, last section): the SAME launch code the engine
// runs per projection, on caller-owned buffers.  Used by the operator microbenches and by the parity tests at
// the real Qwen3-4B shapes.
struct tl_tiled_w4 {
    tl_w4 w{};
    tl::TiledW4 t{};
    tl::TiledW4Mem mem;
};

extern "C" int tl_tiled_w4_create(const tl_w4 *w, void *stream, tl_tiled_w4 **out) {
    using namespace tl;
    TL_REQUIRE(w && out, "tiled_w4_create: null argument");
    TL_TRY(check_w4(*w, w->rows, w->cols, "tiled_w4_create"));
    TL_REQUIRE(w->rows > 0 && w->rows % 16 == 0 && w->cols > 0 && w->cols % 128 == 0,
               "tiled_w4_create: rows must be a multiple of 16 and cols a multiple of 128");
    auto t = std::make_unique<tl_tiled_w4>();
    t->w = *w;
    TL_TRY(tiled_w4_make(*w, (hipStream_t)stream, t->mem, t->t, "tiled_w4_create: hipMalloc failed", "tiled_w4_create: repack launch failed"));
    *out = t.release();
    return TL_OK;
}

extern "C" void tl_tiled_w4_destroy(tl_tiled_w4 *t) { delete t; }

extern "C" size_t tl_decode_linear_workspace_bytes(int M, int rows, int cols) {
    using namespace tl;
    if (M <= 0 || rows <= 0 || cols <= 0) return 0;
    size_t need = align_up((size_t)((M + 15) / 16 * 16) * cols * 2, 256);  // RMSNorm output ahead of the skinny matmul / rows in fragment order (kernel 5)
    size_t partial = 0;
    for (int mode = 0; mode < 2; ++mode) {  // either grid of the skinny matmul (kernel 3 / 4 pin one)
        const Qmm3Plan p3 = qmm3_plan(std::min(M, 64), cols, rows, mode, qmm3_num_cus());
        if (p3.ok) partial = std::max(partial, p3.partial_bytes);
    }
    return need + partial;
}

// validate, fill a LinearCtx and a Proj, call the function the engine calls for that kernel number (which reports into *info)
static int decode_linear_impl(const tl_tiled_w4 *w, const void *a_dev, void *out_dev, int M, int prologue, int epilogue,
                              const void *norm_w_dev, const void *residual_dev, float eps, int kernel, void *workspace_dev,
                              size_t workspace_bytes, void *stream, const tl_linear_ex *ex, tl_linear_info *info) {
    using namespace tl;
    TL_REQUIRE(w && out_dev, "decode_linear: null argument");
    TL_REQUIRE(M >= 1 && M <= 64, "decode_linear: between 1 and 64 activation rows");
    TL_REQUIRE(prologue == PRO_NONE || prologue == PRO_RMSNORM || (ex && (prologue == PRO_ATTN_MERGE || prologue == PRO_RMS_WEIGHTED)),
               "decode_linear: prologue is 0 (none) or 1 (RMSNorm); tl_decode_linear_ex also takes 2 (merge of attention partials) and 3 (weighted rows)");
    TL_REQUIRE(epilogue == EPI_STORE || epilogue == EPI_RESIDUAL || epilogue == EPI_SWIGLU,
               "decode_linear: epilogue is 0 (store), 1 (residual add) or 2 (SwiGLU over interleaved rows)");
    TL_REQUIRE(prologue == PRO_ATTN_MERGE || a_dev, "decode_linear: null activation rows");
    TL_REQUIRE(prologue != PRO_RMSNORM || norm_w_dev, "decode_linear: the RMSNorm prologue needs its weight");
    TL_REQUIRE(epilogue != EPI_RESIDUAL || residual_dev, "decode_linear: the residual epilogue needs the residual rows");
    TL_REQUIRE(kernel >= 0 && kernel <= 6,
               "decode_linear: kernel is 0 (engine routing), 1 (fused GEMV), 2 (skinny matmul), 3 / 4 (its one-shot / persistent grid), 5 (register-resident matmul), 6 (row-streaming matmul)");
    TL_REQUIRE(epilogue != EPI_SWIGLU || w->w.rows % 2 == 0, "decode_linear: SwiGLU needs an even number of weight rows");
    // the engine's own fused variants: RMSNorm+store (qkv, lm_head), residual (wo, w_down), RMSNorm+SwiGLU (gate|up), plain;
    // through tl_decode_linear_ex also: merged attention partials + residual (wo of one row), weighted rows + SwiGLU (gate|up)
    TL_REQUIRE((prologue == PRO_NONE && epilogue != EPI_SWIGLU) || (prologue == PRO_RMSNORM && epilogue != EPI_RESIDUAL) ||
                   (prologue == PRO_ATTN_MERGE && epilogue == EPI_RESIDUAL) || (prologue == PRO_RMS_WEIGHTED && epilogue == EPI_SWIGLU) ||
                   ((kernel == 5 || kernel == 6) && prologue == PRO_RMS_WEIGHTED && epilogue == EPI_STORE),
               "decode_linear: no fused variant for this prologue / epilogue pair");
    const size_t need = tl_decode_linear_workspace_bytes(M, w->w.rows, w->w.cols);
    TL_REQUIRE(workspace_dev && workspace_bytes >= need, "decode_linear: workspace is missing or too small");
    if (info) *info = tl_linear_info{};
    LinearCtx ctx;
    ctx.rms_norm_eps = eps;
    ctx.stream = (hipStream_t)stream;
    ctx.tiled[w->w.weight_dev] = w->t;
    ctx.xn = (uint16_t *)workspace_dev;
    const size_t xn_bytes = align_up((size_t)((M + 15) / 16 * 16) * w->w.cols * 2, 256);
    ctx.splitk_ws = (char *)workspace_dev + xn_bytes;
    ctx.splitk_ws_bytes = workspace_bytes - xn_bytes;
    ctx.force_linear = kernel >= 2 && kernel <= 4 ? 2 : (kernel >= 5 ? 0 : kernel);
    ctx.use_qmm7 = false, ctx.force_qmm7 = kernel == 6;  // 5 and 6 name their kernel
    ctx.qmm3_mode = kernel == 3 ? 0 : (kernel == 4 ? 1 : -1);
    ctx.linfo = info;
    ctx.ncu = qmm3_num_cus();
    ctx.read_env();
    Proj p = proj(w->w, (const uint16_t *)a_dev, (uint16_t *)out_dev, M);
    p.pro = prologue, p.epi = epilogue, p.norm_w = norm_w_dev, p.residual = (const uint16_t *)residual_dev;
    if (ex) {
        p.ss_out = ex->ss_out_dev;
        p.norm_out = ex->norm_out_dev, p.out_w = (uint16_t *)ex->out_w_dev;
    }
    if (kernel == 6 && (prologue != PRO_RMS_WEIGHTED || epilogue == EPI_RESIDUAL))
        return fail(TL_ERR_INVALID, "decode_linear: the row-streaming matmul takes weighted rows with ss_in (prologue 3) and stores or applies SwiGLU (epilogue 0 / 2)");
    if (kernel == 5 || kernel == 6) {  // qmm6.h / qmm7.h: plain rows (qmm6 only), or weighted rows with their partial sums of squares
        const bool weighted = prologue == PRO_RMS_WEIGHTED;
        if (prologue == PRO_RMSNORM || prologue == PRO_ATTN_MERGE)
            return fail(TL_ERR_INVALID, "decode_linear: the register-resident matmul takes plain rows (prologue 0) or weighted rows with ss_in (prologue 3)");
        if (weighted && (!ex || !ex->ss_in_dev || !qmm3_takes_ss(ex->ss_in_n)))
            return fail(TL_ERR_INVALID, "decode_linear_ex: weighted rows need ss_in (a multiple of 4, at most 256 partials per row)");
        if (ex && ((ex->out_w_dev != nullptr) != (ex->norm_out_dev != nullptr) || ((ex->out_w_dev || ex->ss_out_dev) && epilogue != EPI_RESIDUAL)))
            return fail(TL_ERR_INVALID, "decode_linear_ex: ss_out / (norm_out, out_w) belong to the residual epilogue; norm_out and out_w come together");
        if (kernel == 5 && !qmm6_plan(M, w->w.cols, w->w.rows, false, ctx.ncu).ok)
            return fail(TL_ERR_UNSUPPORTED, "decode_linear: the register-resident matmul does not cover this shape");
        if (kernel == 6 && !qmm7_plan(M, w->w.cols, w->w.rows, ctx.ncu).ok)
            return fail(TL_ERR_UNSUPPORTED, "decode_linear: the row-streaming matmul does not cover this shape");
        // weighted rows enter the kernel in fragment order (qmm6.h): as the caller left them (ex->fragment_order), or re-ordered here
        if (weighted && !ex->fragment_order) {
            const long n8 = (long)M * w->w.cols / 8;
            hipLaunchKernelGGL(weight_rows_kernel, dim3(ceil_div(n8, 256)), dim3(256), 0, ctx.stream, p.a, (const uint16_t *)nullptr, ctx.xn, n8, w->w.cols / 8, 1);
            p.a = ctx.xn;
        }
        if (weighted) p.ss_in = ex->ss_in_dev, p.ss_in_n = ex->ss_in_n;
        p.frag = weighted;
        p.out_w_frag = ex && ex->fragment_order ? 1 : 0;
        return engine_qmm6(ctx, p);
    }
    if (!ex) return engine_linear(ctx, p);
    // ---- the routes only the engine could reach before round 4 (qmv3.h: PRO_ATTN_MERGE, PRO_RMS_WEIGHTED, ss_in / ss_out, out_w)
    const bool skinny_forced = kernel >= 2 && kernel <= 4;  // its slice reduction also leaves weighted rows (not the GEMV's 16-row sums of squares)
    const bool gemv_only = prologue == PRO_ATTN_MERGE || prologue == PRO_RMS_WEIGHTED || ex->ss_out_dev || (ex->out_w_dev && !skinny_forced);
    if (gemv_only && !(kernel == 1 || (kernel == 0 && M < ctx.qmm3_min_rows)))
        return fail(TL_ERR_INVALID, "decode_linear_ex: merged partials, weighted rows, ss_out and out_w are routes of the fused GEMV (kernel 1, or 0 with fewer than 5 rows)");
    if ((ex->out_w_dev != nullptr) != (ex->norm_out_dev != nullptr) || (ex->out_w_dev && epilogue != EPI_RESIDUAL) ||
        (ex->ss_out_dev && epilogue != EPI_RESIDUAL))
        return fail(TL_ERR_INVALID, "decode_linear_ex: ss_out / (norm_out, out_w) belong to the residual epilogue; norm_out and out_w come together");
    if (ex->ss_in_dev && (ex->ss_in_n <= 0 || !(prologue == PRO_RMSNORM || prologue == PRO_RMS_WEIGHTED)))
        return fail(TL_ERR_INVALID, "decode_linear_ex: ss_in needs ss_in_n > 0 and a normalising prologue (1 or 3)");
    if (prologue == PRO_ATTN_MERGE) {
        if (M != 1 || !ex->merge_ws_dev) return fail(TL_ERR_INVALID, "decode_linear_ex: the merging prologue takes ONE row and the split partials (merge_ws_dev)");
        p.merge_ws = ex->merge_ws_dev, p.n_splits = ex->n_splits;
    }
    if (prologue == PRO_RMS_WEIGHTED) {
        const Qmv3Plan pl = qmv3_plan(std::min(M, 8), w->w.cols, w->w.rows);
        if (!ex->ss_in_dev || M > 8 || !qmv3_takes_weighted_rows(pl, w->w.cols, ex->ss_in_n))
            return fail(TL_ERR_INVALID, "decode_linear_ex: weighted rows need ss_in (a multiple of 4, at most 256 partials per row), at most 8 rows and a row that fits the staging registers");
    }
    p.ss_in = ex->ss_in_dev, p.ss_in_n = ex->ss_in_n;
    if (gemv_only || kernel == 1 || (kernel == 0 && M < ctx.qmm3_min_rows)) {
        if (M > 8) return fail(TL_ERR_INVALID, "decode_linear_ex: the fused GEMV takes at most 8 rows");
        ProjResult r;
        TL_TRY(engine_qmv(ctx, p, nullptr, &r));
        if (ex->ss_out_dev && r.ss_n != w->w.rows / 16)
            return fail(TL_ERR_UNSUPPORTED, "decode_linear_ex: the GEMV that ran left no sums of squares (packed-dot fallback or several passes)");
        return TL_OK;
    }
    // skinny matmul with its fused RMSNorm (any multiple of 4 up to 256 partials per row)
    if (ex->ss_in_dev && !qmm3_takes_ss(ex->ss_in_n))
        return fail(TL_ERR_INVALID, "decode_linear_ex: the skinny matmul reads a multiple of 4, at most 256, partial sums of squares per row");
    if (!ex->ss_in_dev) p.ss_in_n = 0;
    p.frag = ex->fragment_order != 0;
    return engine_linear(ctx, p);
}

extern "C" int tl_decode_linear(const tl_tiled_w4 *w, const void *a_dev, void *out_dev, int M, int prologue, int epilogue,
                                const void *norm_w_dev, const void *residual_dev, float eps, int kernel, void *workspace_dev,
                                size_t workspace_bytes, void *stream, tl_linear_info *info) {
    return decode_linear_impl(w, a_dev, out_dev, M, prologue, epilogue, norm_w_dev, residual_dev, eps, kernel, workspace_dev,
                              workspace_bytes, stream, nullptr, info);
}

extern "C" int tl_decode_linear_ex(const tl_tiled_w4 *w, const void *a_dev, void *out_dev, int M, int prologue, int epilogue,
                                   const void *norm_w_dev, const void *residual_dev, float eps, int kernel, void *workspace_dev,
                                   size_t workspace_bytes, void *stream, const tl_linear_ex *ex, tl_linear_info *info) {
    TL_REQUIRE(ex, "decode_linear_ex: null extension block (use tl_decode_linear)");
    return decode_linear_impl(w, a_dev, out_dev, M, prologue, epilogue, norm_w_dev, residual_dev, eps, kernel, workspace_dev,
                              workspace_bytes, stream, ex, info);
}
