// Multi-LoRA: low-rank adapters added to the frozen projections, a different adapter per row (include/tinyllm_engine.h "LoRA adapters",
// DESIGN.md section 4; tl_lora_rows, tl_engine_lora_load, tl_engine_set_lora).  For a projection with base weight W and an adapter
// (A [r, in], B [out, r], scale), all bf16, row-major, the PEFT orientation:
//     y = W x + scale * B (A x)           A x and B t accumulate in fp32, scale multiplies in fp32, bf16 only where a value is stored.
//
// FUSED LAYOUTS, the ones the base weights use.  A projection group (qkv, wo, gate|up, w_down) has ONE fused A of rtot rows -- the A of
// its present targets stacked -- and one B [out, rank]; output column o belongs to a SEGMENT s(o) and reads t[t_off[s] .. t_off[s] + rank):
//     LORA_SEG_PLAIN         one segment (wo, w_down)
//     LORA_SEG_BLOCKS        s = (o >= end0) + (o >= end1): q | k | v rows of wqkv
//     LORA_SEG_INTERLEAVED   s = o & 1: row 2i = gate_proj row i, row 2i + 1 = up_proj row i of wgu
// A target the adapter lacks is a segment with t_off < 0: its A rows do not exist and its output columns are skipped, not multiplied by zeros.
//
// TWO LAUNCHES per group, over tiles of up to 16 rows (lora_tiles.h):
//   shrink   grid (tiles, ceil(in / 512)), one wave each: t_partial[tile][slice][j][row] = sum over the slice of A[j][c] x[row][c] through
//            v_mfma_f32_16x16x32_bf16 (x the A operand, the adapter's rows the B operand: products of two bf16 are exact, sums fp32).  The
//            adapter's fragment is loaded once per tile and 32 columns and serves all its rows.  RMSNorm prologue (decode: the normalised
//            row is never materialised): the norm is linear, so the dot runs over x * w -- an fp32 product split into a bf16 head and tail,
//            two MFMAs, 2^-17 relative -- the slice's sum of squares of x goes out beside the partials, and the expand launch applies
//            rsqrt(mean + eps) to the reduced t.  A tile whose rows carry several adapters (a decode step) takes one pass per distinct
//            adapter, ascending by first row, and keeps from each pass the rows that carry it.  A tile without adapters exits at once.
//   expand   grid (tiles, ceil(out / 512)), 256 threads, two output columns each: the slices are added in ascending order into t [16][rtot]
//            in LDS (every workgroup of the tile does so for itself: 19 slices x 3 KB at w_down / rank 16, from L2), then
//            d[row][o] = scale * sum_j B[o][j] t[row][j] in fp32 on the VALU, j ascending -- t stays fp32, which a bf16 MFMA operand could
//            not hold -- B's 8-wide chunks loaded once per tile and adapter.  Epilogues:
//                ADD           out = bf16(out + d), in place (qkv)
//                RESIDUAL_PRE  tmp = bf16(residual + d): the base projection's EPI_RESIDUAL takes tmp as its residual (wo, w_down)
//                SWIGLU        over the interleaved gate|up rows of an EPI_STORE base projection:
//                              g' = bf16(g + dg), u' = bf16(u + du), act = bf16(silu(g') u') -- the arithmetic of swiglu_interleaved_kernel
//            A row without an adapter, a skipped column and an element whose d is zero keep the base value BIT FOR BIT (ADD: not written;
//            RESIDUAL_PRE: the residual's bits; SWIGLU: the base SwiGLU).
// No atomics, one summation order: a row's result depends on its values and its adapter alone -- not on its position, its tile, its
// neighbours or their adapters (a row of D of an MFMA depends on that row of the A operand only).
//
// The device table: LoraDesc per (adapter, layer, group); the kernels read entry table[adapter * stride + index].  rank 0 = not adapted
// (an unloaded id, or a group none of whose targets the adapter has): such rows count as rows without an adapter.  Loading, unloading and
// assigning therefore change device words only and never a captured plan.
#pragma once

#include "common.h"
#include "lora_tiles.h"
#include "../../include/tinyllm_engine.h"

namespace tl {

enum { LORA_SEG_PLAIN = 0, LORA_SEG_BLOCKS = 1, LORA_SEG_INTERLEAVED = 2 };
constexpr int LORA_EXPAND_THREADS = 256;
constexpr int LORA_EXPAND_COLS = 2 * LORA_EXPAND_THREADS;

struct LoraDesc {
    const uint16_t *a;  // [rtot, in]
    const uint16_t *b;  // [out, rank]
    float scale;
    int rank, rtot;     // rtot = rank * present segments
    int t_off[3];       // per segment: first row of its A inside the fused A, < 0 = target missing
};

struct LoraArgs {
    const LoraDesc *table;
    int stride, index, n_adapters;
    const int32_t *row_adapter;  // [rows] for tiles of LORA_ROW_LOOKUP (may be null when no tile looks up)
    const LoraTile *tiles;
    const uint16_t *x;           // [total_rows, in]
    int total_rows;              // a tile's rows end here at the latest (a decode step's fixed tiles serve every batch)
    int in, out, slices;
    const uint16_t *norm_w;      // RMSNorm prologue: its weight [in]; null = none
    float eps;
    float *partial;              // [tiles][slices][LORA_MAX_RTOT][16]
    float *ss;                   // [tiles][slices][16]
    int seg_mode, seg_end0, seg_end1, mode;
    const uint16_t *base;        // RESIDUAL_PRE: the residual [rows, out]; SWIGLU: the interleaved gate|up rows [rows, out]
    uint16_t *dst;               // ADD / RESIDUAL_PRE [rows, out]; SWIGLU [rows, out / 2]
};

// the adapter of row r of a tile, or LORA_NONE: out of the tile, no adapter, an id outside the table, a group the adapter does not adapt
__device__ __forceinline__ int lora_row_adapter(const LoraArgs &q, const LoraTile &tile, int r) {
    if (r >= tile.rows || tile.adapter == LORA_NONE) return LORA_NONE;
    const int a = tile.adapter == LORA_ROW_LOOKUP ? q.row_adapter[tile.row0 + r] : tile.adapter;
    if (a < 0 || a >= q.n_adapters) return LORA_NONE;
    return q.table[(size_t)a * q.stride + q.index].rank > 0 ? a : LORA_NONE;
}

// grid = (tiles, slices), block = 64
static __global__ __launch_bounds__(WAVE) void lora_shrink_kernel(const LoraArgs q) {
    LoraTile tile = q.tiles[blockIdx.x];
    tile.rows = min(tile.rows, q.total_rows - tile.row0);
    const int lane = threadIdx.x, r = lane & 15, c = lane >> 4;
    const int mine = lora_row_adapter(q, tile, r);
    unsigned todo = (unsigned)(__ballot(mine >= 0) & 0xffffull);
    if (todo == 0) return;
    const int k0 = blockIdx.y * LORA_KS, k1 = min(q.in, k0 + LORA_KS);
    const size_t unit = (size_t)blockIdx.x * q.slices + blockIdx.y;
    const bool row_in = r < tile.rows;
    const uint16_t *xrow = q.x + (size_t)(tile.row0 + (row_in ? r : 0)) * q.in + 8 * c;
    const bool norm = q.norm_w != nullptr;
    if (norm) {  // the slice's sum of squares of every row: lane (r, c) adds its columns ascending, then the four c of a row
        float ss = 0.f;
        if (row_in) {
            for (int k = k0; k < k1; k += 32) {
                const u32x4 xv = *reinterpret_cast<const u32x4 *>(xrow + k);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float lo = __uint_as_float(xv[e] << 16), hi = __uint_as_float(xv[e] & 0xffff0000u);
                    ss += lo * lo;
                    ss += hi * hi;
                }
            }
        }
        ss += lane_xor16(ss, lane);
        ss += lane_xor32(ss, lane);
        if (c == 0) q.ss[unit * LORA_TILE + r] = ss;
    }
    float *part = q.partial + unit * LORA_MAX_RTOT * LORA_TILE;
    while (todo) {
        const int lead = __ffs(todo) - 1;
        const int a = __shfl(mine, lead);
        const unsigned same = (unsigned)(__ballot(mine == a) & 0xffffull);
        todo &= ~same;
        const LoraDesc d = q.table[(size_t)a * q.stride + q.index];
        const int blocks = (d.rtot + 15) / 16;
        for (int rb0 = 0; rb0 < blocks; rb0 += 4) {
            f32x4 acc[4];
            const uint16_t *arow[4];
            bool live[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                const int j = (rb0 + i) * 16 + r;
                live[i] = j < d.rtot;
                arow[i] = d.a + (size_t)(live[i] ? j : 0) * q.in + 8 * c;
            }
            for (int k = k0; k < k1; k += 32) {
                u32x4 xh = {0u, 0u, 0u, 0u}, xl = {0u, 0u, 0u, 0u};
                if (row_in) {
                    xh = *reinterpret_cast<const u32x4 *>(xrow + k);
                    if (norm) {
                        const u32x4 wv = *reinterpret_cast<const u32x4 *>(q.norm_w + k + 8 * c);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float p0 = __uint_as_float(xh[e] << 16) * __uint_as_float(wv[e] << 16);
                            const float p1 = __uint_as_float(xh[e] & 0xffff0000u) * __uint_as_float(wv[e] & 0xffff0000u);
                            const uint16_t h0 = BF16::from_float(p0), h1 = BF16::from_float(p1);
                            xl[e] = BF16::pack2(p0 - BF16::to_float(h0), p1 - BF16::to_float(h1));
                            xh[e] = (uint32_t)h0 | ((uint32_t)h1 << 16);
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (rb0 + i >= blocks) continue;
                    u32x4 av = {0u, 0u, 0u, 0u};
                    if (live[i]) av = *reinterpret_cast<const u32x4 *>(arow[i] + k);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, xh), __builtin_bit_cast(bf16x8_t, av), acc[i], 0, 0, 0);
                    if (norm) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, xl), __builtin_bit_cast(bf16x8_t, av), acc[i], 0, 0, 0);
                }
            }
            // D: lane (r, c) holds column j = 16 block + r of rows 4 c .. 4 c + 3; only the rows that carry this adapter are kept
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (rb0 + i >= blocks || !live[i]) continue;
                float *dst = part + (size_t)((rb0 + i) * 16 + r) * LORA_TILE + 4 * c;
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if ((same >> (4 * c + m)) & 1u) dst[m] = acc[i][m];
            }
        }
    }
}

__device__ __forceinline__ int lora_segment(const LoraArgs &q, int o) {
    if (q.seg_mode == LORA_SEG_BLOCKS) return (o >= q.seg_end0 ? 1 : 0) + (o >= q.seg_end1 ? 1 : 0);
    return q.seg_mode == LORA_SEG_INTERLEAVED ? (o & 1) : 0;
}
// base + d as it is stored: the base's own bits where nothing is added
__device__ __forceinline__ uint16_t lora_add(uint16_t base, float d) { return d != 0.f ? BF16::from_float(BF16::to_float(base) + d) : base; }

// grid = (tiles, ceil(out / 512)), block = 256
static __global__ __launch_bounds__(LORA_EXPAND_THREADS) void lora_expand_kernel(const LoraArgs q) {
    __shared__ float t_s[LORA_TILE][LORA_MAX_RTOT];
    __shared__ int ad_s[LORA_TILE], rtot_s[LORA_TILE];
    __shared__ float rs_s[LORA_TILE];
    LoraTile tile = q.tiles[blockIdx.x];
    tile.rows = min(tile.rows, q.total_rows - tile.row0);
    const int tid = threadIdx.x;
    const size_t unit0 = (size_t)blockIdx.x * q.slices;
    if (tid < LORA_TILE) {
        const int a = lora_row_adapter(q, tile, tid);
        ad_s[tid] = a;
        rtot_s[tid] = a >= 0 ? q.table[(size_t)a * q.stride + q.index].rtot : 0;
        float rs = 1.f;
        if (a >= 0 && q.norm_w != nullptr) {
            float ss = 0.f;
            for (int s = 0; s < q.slices; ++s) ss += q.ss[(unit0 + s) * LORA_TILE + tid];
            rs = rsqrtf(ss / (float)q.in + q.eps);
        }
        rs_s[tid] = rs;
    }
    __syncthreads();
    for (int idx = tid; idx < LORA_TILE * LORA_MAX_RTOT; idx += LORA_EXPAND_THREADS) {
        const int j = idx >> 4, row = idx & 15;
        if (j >= rtot_s[row]) continue;
        float t = 0.f;
        for (int s = 0; s < q.slices; ++s) t += q.partial[((unit0 + s) * LORA_MAX_RTOT + j) * LORA_TILE + row];
        t_s[row][j] = t * rs_s[row];
    }
    __syncthreads();
    const int o0 = blockIdx.y * LORA_EXPAND_COLS + 2 * tid;
    if (o0 >= q.out) return;  // (out is even: o0 + 1 < out)
    float d[LORA_TILE][2];
#pragma unroll
    for (int row = 0; row < LORA_TILE; ++row) d[row][0] = d[row][1] = 0.f;
    unsigned todo = 0;
#pragma unroll
    for (int row = 0; row < LORA_TILE; ++row) todo |= ad_s[row] >= 0 ? 1u << row : 0u;
    while (todo) {
        const int a = ad_s[__ffs(todo) - 1];
        unsigned same = 0;
#pragma unroll
        for (int row = 0; row < LORA_TILE; ++row) same |= ad_s[row] == a ? 1u << row : 0u;
        todo &= ~same;
        const LoraDesc ds = q.table[(size_t)a * q.stride + q.index];
#pragma unroll
        for (int col = 0; col < 2; ++col) {
            const int seg = lora_segment(q, o0 + col);
            const int off = seg == 0 ? ds.t_off[0] : (seg == 1 ? ds.t_off[1] : ds.t_off[2]);  // (no indexed read: the descriptor stays in registers)
            if (off < 0) continue;
            const uint16_t *brow = ds.b + (size_t)(o0 + col) * ds.rank;
            for (int j0 = 0; j0 < ds.rank; j0 += 8) {
                const u32x4 bv = *reinterpret_cast<const u32x4 *>(brow + j0);
                float bw[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) bw[2 * e] = __uint_as_float(bv[e] << 16), bw[2 * e + 1] = __uint_as_float(bv[e] & 0xffff0000u);
#pragma unroll
                for (int row = 0; row < LORA_TILE; ++row) {
                    if (!((same >> row) & 1u)) continue;
                    float s = d[row][col];
#pragma unroll
                    for (int e = 0; e < 8; ++e) s = fmaf(t_s[row][off + j0 + e], bw[e], s);
                    d[row][col] = s;
                }
            }
#pragma unroll
            for (int row = 0; row < LORA_TILE; ++row)
                if ((same >> row) & 1u) d[row][col] *= ds.scale;
        }
    }
#pragma unroll
    for (int row = 0; row < LORA_TILE; ++row) {
        if (row >= tile.rows) continue;
        const size_t at = (size_t)(tile.row0 + row) * q.out + o0;
        if (q.mode == TL_LORA_ADD) {
            if (ad_s[row] < 0) continue;
            const uint32_t two = *reinterpret_cast<const uint32_t *>(q.dst + at);
            const uint32_t res = (uint32_t)lora_add((uint16_t)(two & 0xffffu), d[row][0]) | ((uint32_t)lora_add((uint16_t)(two >> 16), d[row][1]) << 16);
            if (res != two) *reinterpret_cast<uint32_t *>(q.dst + at) = res;
        } else if (q.mode == TL_LORA_RESIDUAL_PRE) {
            const uint32_t two = *reinterpret_cast<const uint32_t *>(q.base + at);
            *reinterpret_cast<uint32_t *>(q.dst + at) =
                (uint32_t)lora_add((uint16_t)(two & 0xffffu), d[row][0]) | ((uint32_t)lora_add((uint16_t)(two >> 16), d[row][1]) << 16);
        } else {
            const uint32_t two = *reinterpret_cast<const uint32_t *>(q.base + at);
            const float gt = BF16::to_float(lora_add((uint16_t)(two & 0xffffu), d[row][0]));
            const float up = BF16::to_float(lora_add((uint16_t)(two >> 16), d[row][1]));
            q.dst[(size_t)(tile.row0 + row) * (q.out / 2) + o0 / 2] = BF16::from_float((gt / (1.0f + expf(-gt))) * up);
        }
    }
}

// One adapted projection group over the tiles of `tiles_dev`: the shrink and the expand launch, stream ordered.  The caller vouches for
// the rows behind the tiles and for a workspace of lora_partial_floats / lora_ss_floats(n_tiles, in) words.
struct LoraCall {
    const LoraDesc *table = nullptr;
    int stride = 1, index = 0, n_adapters = 0;
    const int32_t *row_adapter = nullptr;
    const LoraTile *tiles_dev = nullptr;
    int n_tiles = 0;
    const uint16_t *x = nullptr;
    int total_rows = 0;
    int in = 0, out = 0;
    const uint16_t *norm_w = nullptr;
    float eps = 0.f;
    float *partial = nullptr, *ss = nullptr;
    int seg_mode = LORA_SEG_PLAIN, seg_end0 = 0, seg_end1 = 0;
    int mode = TL_LORA_ADD;
    const uint16_t *base = nullptr;
    uint16_t *dst = nullptr;
};
static inline int lora_apply(const LoraCall &c, hipStream_t stream) {
    TL_REQUIRE(c.table && c.tiles_dev && c.x && c.dst && c.partial && c.ss, "lora: null argument");
    TL_REQUIRE(c.n_tiles >= 1 && c.n_tiles <= 65535, "lora: between 1 and 65,535 tiles per launch");
    TL_REQUIRE(c.total_rows >= 1, "lora: no rows");
    TL_REQUIRE(c.in >= 32 && c.in % 32 == 0 && c.in <= LORA_KS * LORA_MAX_SLICES, "lora: in must be a multiple of 32 up to 32,768");
    TL_REQUIRE(c.out >= 2 && c.out % 2 == 0, "lora: out must be even");
    TL_REQUIRE(c.mode == TL_LORA_ADD || c.mode == TL_LORA_RESIDUAL_PRE || c.mode == TL_LORA_SWIGLU, "lora: unknown epilogue");
    TL_REQUIRE(c.mode == TL_LORA_ADD || c.base, "lora: this epilogue reads base rows");
    TL_REQUIRE(c.seg_mode >= LORA_SEG_PLAIN && c.seg_mode <= LORA_SEG_INTERLEAVED, "lora: unknown segment layout");
    TL_REQUIRE((uintptr_t)c.x % 16 == 0 && (uintptr_t)c.dst % 4 == 0 && (uintptr_t)c.base % 4 == 0 && (uintptr_t)c.norm_w % 16 == 0,
               "lora: rows must be 16-byte aligned");
    LoraArgs q{};
    q.table = c.table, q.stride = c.stride, q.index = c.index, q.n_adapters = c.n_adapters, q.row_adapter = c.row_adapter, q.tiles = c.tiles_dev;
    q.x = c.x, q.total_rows = c.total_rows, q.in = c.in, q.out = c.out, q.slices = lora_slices(c.in), q.norm_w = c.norm_w, q.eps = c.eps, q.partial = c.partial, q.ss = c.ss;
    q.seg_mode = c.seg_mode, q.seg_end0 = c.seg_end0, q.seg_end1 = c.seg_end1, q.mode = c.mode, q.base = c.base, q.dst = c.dst;
    hipLaunchKernelGGL(lora_shrink_kernel, dim3(c.n_tiles, q.slices), dim3(WAVE), 0, stream, q);
    hipLaunchKernelGGL(lora_expand_kernel, dim3(c.n_tiles, ceil_div(c.out, LORA_EXPAND_COLS)), dim3(LORA_EXPAND_THREADS), 0, stream, q);
    TL_CHECK_LAUNCH("lora shrink / expand");
    return TL_OK;
}

}  // namespace tl
