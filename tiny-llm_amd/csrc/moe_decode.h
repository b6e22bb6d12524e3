// Decode-shaped route of a MoE MLP's experts stage (tl_moe_experts_rows_decode; engine_moe_mlp in decode steps from
// tl_engine_set_moe_decode's row count upward): 1 .. 64 activation rows, so at most 1,024 expert rows, few per expert, many experts,
// memory bound.  Rows that name the same expert share ONE read of its gate, up and down weights, and the products run on
// v_mfma_f32_16x16x32_bf16 with up to 16 of the expert's activation rows as the A operand; weights come straight from the checkpoint
// layout.  Two launches, followed by the GEMV route's moe_combine_kernel over the same token-major y:
//   moe_decode_gate_up_kernel  act[m] = bf16(bf16(silu(bf16(xn[m / k] . gate_e))) * bf16(xn[m / k] . up_e))   e = ids[m]
//   moe_decode_down_kernel     y[m] = bf16(act[m] . down_e)
// There is no sort launch: every workgroup reads the (at most 1,024) ids itself, marks the experts named, takes the blockIdx.y-th
// of them in ascending order and collects that expert's rows in ascending order.  The grid's second dimension is the host's bound
// min(rows * k, E); workgroups past the number of distinct experts return.  Nothing is read back and no grid depends on device data.
// The arithmetic is the GEMV's (oracle.quantized_matmul): per group of 128 columns acc += s * (q . x) + beta * sum(x) in fp32, the
// nibbles unpacked with shifts and masks into bf16 operands with no per-weight multiply.
//
// The host side (the planner, sizes, the launch) is declared for every includer; the kernels and the launch body are compiled by
// moe_decode.hip alone (TL_MOE_DECODE_KERNELS).
#pragma once
#include "moe_decode_plan.h"
#include "common.h"
#include "../../include/tinyllm_engine.h"

namespace tl {

inline bool moe_decode_takes(int rows, int k, int D, int I) {
    return rows >= 1 && rows <= MOE_DEC_MAX_ROWS && k >= 1 && k <= MOE_DEC_MAX_K && D > 0 && D % 128 == 0 && I > 0 && I % 128 == 0;
}
// act [rows * k, I] bf16, then y [rows * k, D] bf16, both token-major (expert row m = token * k + j)
inline size_t moe_decode_rows_bytes(int rows, int k, int D, int I) { return (size_t)rows * k * ((size_t)I + D) * 2; }

// gate | up + down (moe_decode.hip): two launches on `st`, no host read, no synchronisation.  The caller has checked the limits
// (moe_decode_takes, E <= 1,024, 16-byte aligned expert words) and follows with moe_combine_kernel over y.
int moe_decode_launch(const tl_moe_weights &m, const uint16_t *xn, const int32_t *ids, uint16_t *act, uint16_t *y, int rows, int D, int cus,
                      hipStream_t st);

}  // namespace tl

#ifdef TL_MOE_DECODE_KERNELS

namespace tl {

// This file's device code is built without the packed fp32 VALU forms (the Makefile's rule for moe_decode.o).

struct MoeDecodeArgs {
    const uint16_t *a;            // [*, N]; expert row m reads row m / a_div
    const uint32_t *b[2];         // [E, K, N / 8]
    const uint16_t *s[2], *z[2];  // [E, K, N / 128]
    uint16_t *out;                // [n, K], row m
    const int32_t *ids;           // [n]
    int n, E, N, K, a_div, features, wk, per;
};

// 8 nibbles of a checkpoint word (nibble i = column i) -> four bf16 pairs (1 + q_i / 16, 1 + q_{i+4} / 16): the nibble shifted into the
// TOP four mantissa bits, (w >> (4 i - 3)) & 0x00780078 | 0x3f803f80 (qmv3.h's unpack, plain C for the reason given there, over the
// checkpoint's nibble order and with the code in the high mantissa bits: in units of a code the constant carried along is 16, not the
// 128 of the low bits, and it is what an output that nearly cancels is rounded against -- with 128 three of 69,632 down outputs of the
// 16-expert test shape missed the GEMV route's allowance).  The A fragment is permuted to match.
__device__ __forceinline__ u32x4 moe_dec_unpack(uint32_t w, uint32_t mask_s, uint32_t magic_v) {
    return u32x4{((w << 3) & mask_s) | magic_v, ((w >> 1) & mask_s) | magic_v, ((w >> 5) & mask_s) | magic_v, ((w >> 9) & mask_s) | magic_v};
}
// columns (0 1, 2 3, 4 5, 6 7) -> (0 4, 1 5, 2 6, 3 7)
__device__ __forceinline__ u32x4 moe_dec_permute(const u32x4 &v) {
    return u32x4{(v[0] & 0xffffu) | (v[2] << 16), (v[0] >> 16) | (v[2] & 0xffff0000u), (v[1] & 0xffffu) | (v[3] << 16),
                 (v[1] >> 16) | (v[3] & 0xffff0000u)};
}

// One workgroup per (named expert, p.features output features): wave w = (feature block w / wk, reduction slice w % wk).  A lane is
// (r = lane & 15, c = lane >> 4): as a B lane it holds feature r's words 4 c .. 4 c + 3 of a group (one 16-byte request per group and
// matrix, MFMA t takes word t: columns 32 c + 8 t ..), as an A lane row r of the current 16-row block over the same columns (four
// 16-byte requests per group, straight from the activation rows: with one feature block per workgroup -- every gate | up launch of
// the real shapes -- no two waves want the same columns, so a staging pass through LDS would only add a barrier in front of the weight
// stream; absent rows repeat the expert's last row and are never stored: a D row depends on its own A row alone).  As a D lane it
// holds feature r of rows 4 c .. 4 c + 3.  Per step a wave puts the block's activations, then MOE_DEC_LM groups of weights, scales
// and biases in flight before the first use; the row sums of a group come from one more MFMA against ones.  An expert with more than
// 16 rows runs further 16-row blocks against the same weight registers (kept packed: 8 VALU per word to unpack again, a quarter of the
// registers) whenever a wave's slice is one step -- up to 2,048 reduced columns; a longer slice requests its steps again per block.
// NB = 2: gate and up of the same features, SwiGLU in registers; NB = 1: down.
template <int NB>
__device__ __forceinline__ void moe_decode_body(const MoeDecodeArgs &p) {
    constexpr int LM = MOE_DEC_LM;
    __shared__ uint16_t sid[MOE_DEC_MAX_ROWS * MOE_DEC_MAX_K];      // the clamped ids
    __shared__ uint16_t rowlist[MOE_DEC_MAX_ROWS * MOE_DEC_MAX_K];  // this expert's rows, ascending
    __shared__ uint32_t named[MOE_DEC_MAX_E / 32];
    __shared__ int cnt_s;
    __shared__ float red[MOE_DEC_WAVES][NB][4][64];
    const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, c = lane >> 4;
    if (tid < MOE_DEC_MAX_E / 32) named[tid] = 0;
    __syncthreads();
    for (int i = tid; i < p.n; i += nt) {
        const int e = min(max(p.ids[i], 0), p.E - 1);
        sid[i] = (uint16_t)e;
        atomicOr(&named[e >> 5], 1u << (e & 31));
    }
    __syncthreads();
    int expert = -1, skip = blockIdx.y;
    for (int w = 0; w < MOE_DEC_MAX_E / 32; ++w) {
        uint32_t m = named[w];
        const int have = __popc(m);
        if (skip < have) {
            for (; skip > 0; --skip) m &= m - 1;
            expert = w * 32 + __ffs(m) - 1;
            break;
        }
        skip -= have;
    }
    if (expert < 0) return;  // (uniform: the grid is the host's bound on the experts named)
    if (wave == 0) {
        int at = 0;
        for (int base = 0; base < p.n; base += 64) {
            const int i = base + lane;
            const bool hit = i < p.n && sid[i] == expert;
            const unsigned long long votes = __ballot(hit);
            if (hit) rowlist[at + __popcll(votes & ((1ull << lane) - 1ull))] = (uint16_t)i;
            at += __popcll(votes);
        }
        if (lane == 0) cnt_s = at;
    }
    __syncthreads();
    const int cnt = cnt_s;  // >= 1: the expert is named

    const int N = p.N, K = p.K, G = N >> 7, words = N >> 3, wk = p.wk, ks = wave % wk;
    int f0, g0, g1;
    moe_decode_wave_at(p.features, wk, p.per, G, blockIdx.x, wave, &f0, &g0, &g1);
    const int f = f0 + r;
    const size_t wat = (size_t)expert * K + f;
    const uint32_t *wsrc[NB];
    const uint16_t *ssrc[NB], *zsrc[NB];
#pragma unroll
    for (int gm = 0; gm < NB; ++gm) wsrc[gm] = p.b[gm] + wat * words + 4 * c, ssrc[gm] = p.s[gm] + wat * G, zsrc[gm] = p.z[gm] + wat * G;

    uint32_t nib_mask = 0x00780078u, magic = 0x3f803f80u;
    asm volatile("" : "+s"(nib_mask));  // opaque constants (qmv3.h): the mask in an SGPR, the magic in a VGPR, one v_and_or_b32 per pair
    const u32x4 ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
    const bool one_step = g1 - g0 <= LM;
    u32x4 wq[NB][LM];
    uint32_t sq[NB][LM], zq[NB][LM];

#pragma unroll 1
    for (int blk = 0; blk * 16 < cnt; ++blk) {
        // (per block: the unpacked words are not carried from block to block, which would take four times the registers)
        asm volatile("" : "+v"(magic));
        float acc[NB][4];
#pragma unroll
        for (int gm = 0; gm < NB; ++gm)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[gm][j] = 0.f;
        const int arow = rowlist[min(blk * 16 + r, cnt - 1)] / p.a_div;
        const uint16_t *asrc = p.a + (size_t)arow * N + 32 * c;

#pragma unroll 1
        for (int gs = g0; gs < g1; gs += LM) {
            u32x4 areg[LM][4];  // ahead of the weights: requests retire in order and these are needed first
#pragma unroll
            for (int i = 0; i < LM; ++i)
#pragma unroll
                for (int t = 0; t < 4; ++t) areg[i][t] = *reinterpret_cast<const u32x4 *>(asrc + (size_t)min(gs + i, G - 1) * 128 + 8 * t);
            if (blk == 0 || !one_step) {
#pragma unroll
                for (int gm = 0; gm < NB; ++gm)
#pragma unroll
                    for (int i = 0; i < LM; ++i) {
                        const int g = min(gs + i, G - 1);  // (a surplus group of the fixed-length body repeats the last one, unscaled)
                        wq[gm][i] = *reinterpret_cast<const u32x4 *>(wsrc[gm] + (size_t)g * 16);
                        sq[gm][i] = ssrc[gm][g], zq[gm][i] = zsrc[gm][g];
                    }
            }
#pragma unroll
            for (int i = 0; i < LM; ++i) {
                f32x4 d[NB], sm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int gm = 0; gm < NB; ++gm) d[gm] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const u32x4 ax = moe_dec_permute(areg[i][t]);
#pragma unroll
                    for (int gm = 0; gm < NB; ++gm) {
                        const u32x4 bq = moe_dec_unpack(wq[gm][i][t], nib_mask, magic);
                        d[gm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ax), __builtin_bit_cast(bf16x8_t, bq), d[gm], 0, 0, 0);
                    }
                    sm = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ax), __builtin_bit_cast(bf16x8_t, ones), sm, 0, 0, 0);
                }
                const bool live = gs + i < g1;
#pragma unroll
                for (int gm = 0; gm < NB; ++gm) {
                    const float sc = live ? 16.0f * __uint_as_float(sq[gm][i] << 16) : 0.f;       // d = sum (1 + q / 16) x = sm + (q . x) / 16:
                    const float be = live ? __uint_as_float(zq[gm][i] << 16) - sc : 0.f;          // s (q . x) + beta sm = 16 s d + (beta - 16 s) sm
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[gm][j] += sc * d[gm][j] + be * sm[j];
                }
            }
        }

        // the slices of a feature block meet in LDS and are added in slice order; slice 0 stores rows 4 c .. 4 c + 3 of feature f
        if (wk > 1) {  // (uniform over the workgroup, as cnt is: every wave meets the same barriers)
#pragma unroll
            for (int gm = 0; gm < NB; ++gm)
#pragma unroll
                for (int j = 0; j < 4; ++j) red[wave][gm][j][lane] = acc[gm][j];
            __syncthreads();
            if (ks == 0)
                for (int k2 = 1; k2 < wk; ++k2)
#pragma unroll
                    for (int gm = 0; gm < NB; ++gm)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[gm][j] += red[wave + k2][gm][j][lane];
        }
        if (ks == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int at = blk * 16 + 4 * c + j;
                if (at < cnt) {
                    uint16_t v;
                    if constexpr (NB == 2) {  // the two roundings of moe_silu_mul_kernel on the bf16-rounded gate and up
                        const float gt = bf16_round(acc[0][j]);
                        v = BF16::from_float(bf16_round(gt / (1.0f + expf(-gt))) * bf16_round(acc[1][j]));
                    } else {
                        v = BF16::from_float(acc[0][j]);
                    }
                    p.out[(size_t)rowlist[at] * K + f] = v;
                }
            }
        }
        if (wk > 1) __syncthreads();  // red is written again by the next block
    }
}

static __global__ __launch_bounds__(64 * MOE_DEC_WAVES, 2) void moe_decode_gate_up_kernel(const MoeDecodeArgs p) { moe_decode_body<2>(p); }
static __global__ __launch_bounds__(64 * MOE_DEC_WAVES, 2) void moe_decode_down_kernel(const MoeDecodeArgs p) { moe_decode_body<1>(p); }

int moe_decode_launch(const tl_moe_weights &m, const uint16_t *xn, const int32_t *ids, uint16_t *act, uint16_t *y, int rows, int D, int cus,
                      hipStream_t st) {
    const int E = m.num_experts, k = m.experts_per_token, I = m.intermediate_size;
    const MoeDecodePlan plan = moe_decode_split(rows, k, E, D, I, cus);
    const MoeDecodeStage &gs = plan.gate_up, &ds = plan.down;
    MoeDecodeArgs gu{xn, {m.gate_dev, m.up_dev}, {(const uint16_t *)m.gate_scales_dev, (const uint16_t *)m.up_scales_dev},
                     {(const uint16_t *)m.gate_biases_dev, (const uint16_t *)m.up_biases_dev}, act, ids, rows * k, E, D, I, k, gs.features, gs.wk, gs.per};
    hipLaunchKernelGGL(moe_decode_gate_up_kernel, dim3(gs.grid_x, gs.grid_y), dim3(gs.threads), 0, st, gu);
    MoeDecodeArgs dn{act, {m.down_dev, nullptr}, {(const uint16_t *)m.down_scales_dev, nullptr}, {(const uint16_t *)m.down_biases_dev, nullptr},
                     y, ids, rows * k, E, I, D, 1, ds.features, ds.wk, ds.per};
    hipLaunchKernelGGL(moe_decode_down_kernel, dim3(ds.grid_x, ds.grid_y), dim3(ds.threads), 0, st, dn);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(TL_ERR_HIP, std::string("moe decode experts: ") + hipGetErrorString(err));
    return TL_OK;
}

}  // namespace tl
#endif  // TL_MOE_DECODE_KERNELS
