// FP8-activation (W4A8) GEMM for prefill chunks on the block-scaled matrix instruction of gfx950, v_mfma_scale_f32_16x16x128_f8f6f4
// (opt-in: engine option "prefill_fp8"; the reference has no counterpart -- an extension in the sense of the FP8 KV pages, kv8.h).
//
// Arithmetic.  w[n,k] = q[n,k] s[n,g] + beta[n,g], g = k / 128.  Every 128-column group of every activation row is
// quantised as oracle/kv_fp8.py quantises a row: 128 E4M3 codes + one power-of-two fp32 scale alpha[m,g]; a^[m,k] = decode(code) alpha[m,g]
// (exactly a bf16 value), S[m,g] = sum_{k in g} a^[m,k] in fp32.  Then
//     out[m,n] = epilogue( sum_g ( s[n,g] sum_{k in g} a^[m,k] q[n,k]  +  beta[n,g] S[m,g] ) ),   fp32 accumulation, ONE rounding to bf16.
// The kernel works on the CENTRED form of the same weights, w = (q - 8) s + beta' with beta' = beta + 8 s: the two terms of q s + beta cancel
// (beta is near -7.5 s in a checkpoint: a weight near zero is the difference of two numbers of size 7.5 s), and the error of the matrix
// instruction's own sum then scales with sum |a^| (q s + |beta|) instead of sum |a^| |w|; centred, both terms are of the size of |w|.
// The codes -8 .. 7 are exact in E4M3, so the only approximation against the bf16 GEMM is the rounding of the activations.
//
// The weight copy (gemm_fp8_weight_bytes, made once by expand_w4_to_fp8) is one block of three pieces:
//   [0, N K)                    E4M3 codes of q - 8, ROW-MAJOR [N][K] -- decoding byte n K + k and adding 8 gives nibble k of checkpoint row n (no
//                               tiling to undo);
//   [off_s, + 4 G Np)           s as fp32, GROUP-major [G][Np]: a lane reads the four scales of its four output columns as one 16-byte load per
//                               (16-column tile, group);  Np = N rounded up to the 256-column tile, zero filled;
//   [off_b, + 4 Np Gp)          beta' = beta + 8 s as fp32 [Np][Gp], Gp = G rounded up to 32, zero filled: the A operand of the trailing K-extension.
//
// The kernel.  128 x 256 output tile per workgroup, 8 waves as 2 (M) x 4 (N), 64 x 64 outputs per wave = 4 x 4 tiles of 16 x 16; one workgroup
// per CU (144 KB of LDS).  One reduction step = one quantisation group = 128 bytes of either operand's row, so a step of the activation tile is
// 16 KB and of the weight tile 32 KB -- the geometry of gemm8's 64-wide bf16 step, and brought in the same way: LDS-DMA (buffer_load ... lds, 16
// bytes per lane, 8 rows per instruction, no registers), the LDS image lane-linear with the XOR swizzle applied to the SOURCE chunk (chunk p of row
// r holds global chunk p ^ ((r >> 1) & 7)), rows past M / N reading zeros through the buffer resource's range check.  THREE stages: the DMA of group
// g + 2 is issued behind the barrier of group g, into the stage group g - 1 was read from; one counted wait (the six pieces of the newest stage may
// still fly) and ONE raw s_barrier per group.
// Per group and 16 x 16 tile: one matrix instruction PER EXPONENT BAND of the activation codes, each into a zeroed accumulator, the four results added
// in fp32 on the VALU.  Measured on the MI355X: the instruction adds its products in blocks of 8 inside a window of about 14 bits below the largest
// product of the block -- a code of 288 beside codes of 2^-6 loses its 7 block neighbours whole, beside codes of 0.94 (weights 7) their last bit --
// so one instruction over a group with an outlier misses the bf16 GEMM's error band by up to 57 x where the output nearly cancels.  A band is the
// codes whose exponent field shares its two high bits (the other bytes zeroed, 5 bitwise operations per word and band): 3 bits of exponent span + 3 of
// the weights -8 .. 7 + 7 of a product's significand = 13 bits, inside the window, so every block sum is exact.  Four times the matrix work: it is what
// makes the kernel correct, and a large part of why it does not win.  Per instruction: the weight codes as its A operand (so a lane ends up with four
// CONSECUTIVE output columns of one activation row, the store-friendly transposed tile of gemm8), the activation codes as B, alpha[m,g] through the
// instruction's E8M0 block scale of B (the fp32 exponent field of alpha IS its E8M0 code; the A scale is 1.0) -- then four FMAs fold s[n..n+3, g]
// times that product into the running fp32 tile.  A lane's 32 code bytes of a row are two swizzled 16-byte chunks; both operands take the same
// chunks, so the instruction pairs every k with itself whatever order it walks them in.
// beta' . S is a rank-G update: behind the loop, as a K-EXTENSION on v_mfma_f32_16x16x32_bf16 -- beta' and S, both fp32, are each split EXACTLY into
// three bf16 pieces (8 + 8 + 8 significand bits by truncation: each remainder is exact in fp32) and the six piece products of combined order <= 2
// are formed (what is left out is below 2^-24 of the product): six instructions per 32 groups and tile, 18 for the 76 groups of w_down against
// 76 in the loop.
// Workgroups are dealt to the 8 XCDs in contiguous runs of tiles (launch order goes round-robin over the XCDs): one XCD's 32 CUs hold two weight
// panels x 16 row bands at 2,048 rows, 18 operand streams through its L2.
#pragma once
#include "common.h"
#include "kv8.h"
#include "qmv.h"

namespace tl {

struct GemmFp8Args {
    const uint8_t *codes;      // [M, K] E4M3 codes of the activations
    const float *scales;       // [M, K / 128] alpha
    const float *sums;         // [M, K / 128] S
    const uint8_t *wq;         // [N, K] E4M3 codes of q - 8
    const float *ws;           // [K / 128][Np] s
    const float *wb;           // [Np][Gp] beta' = beta + 8 s
    uint16_t *out;             // [M, N]  (EPI_SWIGLU: [M, N / 2], weight rows interleaved gate_i, up_i)
    const uint16_t *residual;  // EPI_RESIDUAL [M, N]
    int M, N, K;
};

constexpr int F8_BM = 128, F8_BN = 256, F8_BK = 128, F8_WAVES = 8, F8_STAGES = 3;
constexpr int F8_WM = 2, F8_WN = 4, F8_TM = 4, F8_TN = 4;
constexpr int F8_BANDS = 4;  // exponent bands of the activation codes, one matrix instruction each (header comment: the instruction's 8-product blocks)
constexpr int F8_STAGE_BYTES = (F8_BM + F8_BN) * F8_BK;
constexpr size_t F8_LDS_BYTES = (size_t)F8_STAGES * F8_STAGE_BYTES;
static_assert(F8_WM * F8_WN == F8_WAVES && 16 * F8_WM * F8_TM == F8_BM && 16 * F8_WN * F8_TN == F8_BN, "tile = waves x accumulator tiles");

// the layout of the weight copy
constexpr int gemm_fp8_np(int N) { return (N + F8_BN - 1) / F8_BN * F8_BN; }
constexpr int gemm_fp8_gp(int K) { return (K / 128 + 31) / 32 * 32; }
constexpr size_t gemm_fp8_off_s(int N, int K) { return ((size_t)N * K + 255) / 256 * 256; }
constexpr size_t gemm_fp8_off_b(int N, int K) { return gemm_fp8_off_s(N, K) + (size_t)(K / 128) * gemm_fp8_np(N) * 4; }
constexpr size_t gemm_fp8_weight_bytes(int N, int K) { return gemm_fp8_off_b(N, K) + (size_t)gemm_fp8_np(N) * gemm_fp8_gp(K) * 4; }

typedef int i32x8 __attribute__((ext_vector_type(8)));

template <int EPI>
__global__ __launch_bounds__(F8_WAVES * 64, 1) void gemm_fp8_kernel(const GemmFp8Args p) {
    constexpr int TM = F8_TM, TN = F8_TN;
    constexpr int QA = F8_BM / 64, QW = F8_BN / 64;  // LDS-DMA instructions (8 rows each) per wave and stage of either tile
    constexpr int NP = QA + QW;
    static_assert(NP == 6, "the counted wait below names the pieces of one stage");
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int wr = wave / F8_WN, wc = wave % F8_WN;
    const int r = lane & 15, c = lane >> 4;
    const int K = p.K, G = K >> 7;
    const int tiles_m = (p.M + F8_BM - 1) / F8_BM, tiles_n = (p.N + F8_BN - 1) / F8_BN;
    // workgroup -> tile: XCD x (= blockIdx % 8) takes the x-th run of `per` consecutive tiles, row bands fastest
    const int n_tiles = tiles_m * tiles_n, per = (n_tiles + 7) >> 3;
    const int t = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (t >= n_tiles) return;  // (uniform, before any barrier)
    const int bm0 = (t % tiles_m) * F8_BM, bn0 = (t / tiles_m) * F8_BN;
    const int Np = gemm_fp8_np(p.N), Gp = gemm_fp8_gp(K);

    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p.codes), 0, (int)((uint32_t)p.M * (uint32_t)K), 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p.wq), 0, (int)((uint32_t)p.N * (uint32_t)K), 0x00020000);
    // this lane's 16-byte pieces of either tile per group: instruction slot s covers rows 8 s .. 8 s + 7
    int voa[QA], vow[QW];
#pragma unroll
    for (int q = 0; q < QA; ++q) {
        const int row = (wave + 8 * q) * 8 + (lane >> 3);
        voa[q] = (bm0 + row) * K + (((lane & 7) ^ ((row >> 1) & 7)) << 4);
    }
#pragma unroll
    for (int q = 0; q < QW; ++q) {
        const int row = (wave + 8 * q) * 8 + (lane >> 3);
        vow[q] = (bn0 + row) * K + (((lane & 7) ^ ((row >> 1) & 7)) << 4);
    }
    auto issue = [&](int g, int st) __attribute__((always_inline)) {
        char *base = smem + st * F8_STAGE_BYTES + wave * 1024;
        const int soff = g * F8_BK;
#pragma unroll
        for (int q = 0; q < QA; ++q)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ars, (__attribute__((address_space(3))) void *)(base + q * 8192), 16, voa[q], soff, 0, 0);
#pragma unroll
        for (int q = 0; q < QW; ++q)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void *)(base + F8_BM * F8_BK + q * 8192), 16, vow[q], soff, 0, 0);
    };

    // per group: the four s of the lane's four columns of every column tile, and the E8M0 code of alpha of its row of every row tile (in all four
    // bytes of the scale operand: whichever the instruction selects)
    const float *ws_lane = p.ws + bn0 + wc * (16 * TN) + 4 * c;
    int arow[TM];
#pragma unroll
    for (int m = 0; m < TM; ++m) arow[m] = min(bm0 + wr * (16 * TM) + m * 16 + r, p.M - 1) * G;  // (a row past M: any row's scale, its products are never stored)
    auto load_scales = [&](int g, f32x4(&sv)[TN], float(&al)[TM]) __attribute__((always_inline)) {
#pragma unroll
        for (int n = 0; n < TN; ++n) sv[n] = *reinterpret_cast<const f32x4 *>(ws_lane + (size_t)g * Np + n * 16);
#pragma unroll
        for (int m = 0; m < TM; ++m) al[m] = p.scales[arow[m] + g];
    };
    auto e8m0 = [](float alpha) __attribute__((always_inline)) { return (int)(((__float_as_uint(alpha) >> 23) & 0xffu) * 0x01010101u); };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment addresses: lane (r, c) reads row (.. + r), logical chunks 2 c and 2 c + 1 (the 32 bytes of k-block c), each at chunk ^ ((r >> 1) & 7)
    const int a_row0 = (wr * (16 * TM) + r) * F8_BK, w_row0 = F8_BM * F8_BK + (wc * (16 * TN) + r) * F8_BK;
    const int sw = (r >> 1) & 7;
    const int ch0 = ((2 * c) ^ sw) << 4, ch1 = ((2 * c + 1) ^ sw) << 4;
    auto read_frag = [&](const char *row) __attribute__((always_inline)) {
        const u32x4 lo = *reinterpret_cast<const u32x4 *>(row + ch0), hi = *reinterpret_cast<const u32x4 *>(row + ch1);
        return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    };

    constexpr int SCALE_ONE = 0x7f7f7f7f;  // E8M0 127 = 2^0
    f32x4 sv[TN], sv_next[TN];
    float al_next[TM];  // (raw until the group's end: a use right behind the load would wait for the DMA pieces issued ahead of it)
    int ea[TM];
    // The loop has no branch: behind the last group the scales of group G - 1 are read again and its pieces requested again, into stages nobody reads
    // any more -- so every wait is the same count (a branch around the DMA makes the compiler wait for the scales with vmcnt(0), the fresh pieces included)
    load_scales(0, sv, al_next);
    issue(0, 0);
    issue(min(1, G - 1), 1);
#pragma unroll
    for (int m = 0; m < TM; ++m) ea[m] = e8m0(al_next[m]);
    int st = 0;  // the stage of the group at hand
    for (int g = 0; g < G; ++g) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // group g landed; the six pieces of group g + 1 may still fly
        __builtin_amdgcn_s_barrier();                      // ... everyone's pieces; and everyone has read group g - 1
        __builtin_amdgcn_sched_barrier(0);
        load_scales(min(g + 1, G - 1), sv_next, al_next);  // (ahead of the DMA: the counted wait of the next group covers them)
        __builtin_amdgcn_sched_barrier(0);
        issue(min(g + 2, G - 1), st == 0 ? 2 : st - 1);
        __builtin_amdgcn_sched_barrier(0);
        const char *stage = smem + st * F8_STAGE_BYTES;
        i32x8 bf[TN];
#pragma unroll
        for (int n = 0; n < TN; ++n) bf[n] = read_frag(stage + w_row0 + n * 2048);
#pragma unroll
        for (int m = 0; m < TM; ++m) {
            const i32x8 af = read_frag(stage + a_row0 + m * 2048);
            // the activation codes in F8_BANDS exponent bands (the two high bits of a code's exponent field), the other bytes zero
            i32x8 band[F8_BANDS];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t x = (uint32_t)af[i];
                const uint32_t b6 = (x >> 6) & 0x01010101u, b5 = (x >> 5) & 0x01010101u;
                const uint32_t m3 = (b6 & b5) * 0xffu, m2 = (b6 & ~b5) * 0xffu, m1 = (~b6 & b5 & 0x01010101u) * 0xffu;
                band[3][i] = (int)(x & m3), band[2][i] = (int)(x & m2), band[1][i] = (int)(x & m1), band[0][i] = (int)(x & ~(m3 | m2 | m1));
            }
#pragma unroll
            for (int n = 0; n < TN; ++n) {
                f32x4 d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[n], band[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, SCALE_ONE, 0, ea[m]);
#pragma unroll
                for (int j = 1; j < F8_BANDS; ++j) {  // (smallest band first; the bands meet in fp32 on the VALU, not in the instruction's own sum)
                    const f32x4 dj = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[n], band[j], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, SCALE_ONE, 0, ea[m]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[e] += dj[e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[m][n][e] = __builtin_fmaf(sv[n][e], d[e], acc[m][n][e]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // (the scales of the next group are waited for HERE, behind the products)
#pragma unroll
        for (int n = 0; n < TN; ++n) sv[n] = sv_next[n];
#pragma unroll
        for (int m = 0; m < TM; ++m) ea[m] = e8m0(al_next[m]);
        st = st == F8_STAGES - 1 ? 0 : st + 1;
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the re-requested pieces land before the LDS is given back)

    // K-extension: acc += beta'[n, :] . S[m, :] over the groups, 32 per step.  Either factor is split EXACTLY into three bf16 pieces by truncation
    // (x = x0 + x1 + x2, 8 significand bits each, every remainder exact in fp32); the six products of combined order <= 2 carry the sum to 2^-24
    auto split8 = [&](const float (&x)[8], u32x4(&piece)[3]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            uint32_t h[2][3];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const uint32_t b0 = __float_as_uint(x[j + u]) & 0xffff0000u;
                const float r1 = x[j + u] - __uint_as_float(b0);
                const uint32_t b1 = __float_as_uint(r1) & 0xffff0000u;
                const float r2 = r1 - __uint_as_float(b1);
                h[u][0] = b0, h[u][1] = b1, h[u][2] = __float_as_uint(r2) & 0xffff0000u;
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) piece[q][j >> 1] = (h[0][q] >> 16) | h[1][q];
        }
    };
    for (int ks = 0; ks < Gp / 32; ++ks) {
        const int g0 = ks * 32 + 8 * c;
        u32x4 bpiece[TN][3];
#pragma unroll
        for (int n = 0; n < TN; ++n) {
            const float *src = p.wb + (size_t)(bn0 + wc * (16 * TN) + n * 16 + r) * Gp + g0;
            const f32x4 lo = *reinterpret_cast<const f32x4 *>(src), hi = *reinterpret_cast<const f32x4 *>(src + 4);
            const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            split8(x, bpiece[n]);
        }
#pragma unroll
        for (int m = 0; m < TM; ++m) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = g0 + j < G ? p.sums[arow[m] + g0 + j] : 0.f;
            u32x4 spiece[3];
            split8(x, spiece);
#pragma unroll
            for (int qb = 0; qb < 3; ++qb)
#pragma unroll
                for (int qs = 0; qb + qs < 3; ++qs)
#pragma unroll
                    for (int n = 0; n < TN; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, bpiece[n][qb]), __builtin_bit_cast(bf16x8_t, spiece[qs]), acc[m][n], 0, 0, 0);
        }
    }

    // Epilogue, as gemm8's: acc[m][n] of lane (r, c), element j = activation row bm0 + 64 wr + 16 m + r, output column bn0 + 64 wc + 16 n + 4 c + j -- four
    // consecutive columns of one row per lane, 8 bytes per lane and instruction through range-checked buffer resources
    constexpr uint32_t DEAD = 0x7fffffffu;
    const int out_n = EPI == EPI_SWIGLU ? (p.N >> 1) : p.N;
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)((uint32_t)p.M * (uint32_t)out_n * 2u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint16_t *>(EPI == EPI_RESIDUAL ? p.residual : p.out), 0, EPI == EPI_RESIDUAL ? (int)((uint32_t)p.M * (uint32_t)p.N * 2u) : 0, 0x00020000);
    uint32_t col_off[TN];  // bytes of the lane's first column inside an output row, DEAD past the last column (N is a multiple of 4)
#pragma unroll
    for (int n = 0; n < TN; ++n) {
        const int col = bn0 + wc * (16 * TN) + n * 16 + 4 * c;
        col_off[n] = col < p.N ? (uint32_t)(EPI == EPI_SWIGLU ? col : 2 * col) : DEAD;  // SwiGLU: column / 2 of the half-wide output, 2 bytes each
    }
#pragma unroll
    for (int m = 0; m < TM; ++m) {
        const int row = bm0 + wr * (16 * TM) + m * 16 + r;
        const uint32_t row_off = row < p.M ? (uint32_t)row * (uint32_t)out_n * 2u : DEAD;
#pragma unroll
        for (int n = 0; n < TN; ++n) {
            const uint32_t off = (row_off | col_off[n]) >= DEAD ? DEAD : row_off + col_off[n];
            const f32x4 v = acc[m][n];
            if constexpr (EPI == EPI_SWIGLU) {
                // weight rows interleaved (even = gate_i, odd = up_i): the lane holds two pairs; silu by the hardware exponential and reciprocal
                const float g0 = bf16_round(v[0]), u0 = bf16_round(v[1]), g1 = bf16_round(v[2]), u1 = bf16_round(v[3]);
                const float s0 = __builtin_amdgcn_rcpf(1.0f + exp2_hw(-1.44269504f * g0)), s1 = __builtin_amdgcn_rcpf(1.0f + exp2_hw(-1.44269504f * g1));
                __builtin_amdgcn_raw_buffer_store_b32(BF16::pack2((g0 * s0) * u0, (g1 * s1) * u1), ors, off, 0, 0);
            } else if constexpr (EPI == EPI_RESIDUAL) {
                const u32x2 res = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rrs, off, 0, 0));
                u32x2 o;
                o[0] = BF16::pack2(__uint_as_float(res[0] << 16) + bf16_round(v[0]), __uint_as_float(res[0] & 0xffff0000u) + bf16_round(v[1]));
                o[1] = BF16::pack2(__uint_as_float(res[1] << 16) + bf16_round(v[2]), __uint_as_float(res[1] & 0xffff0000u) + bf16_round(v[3]));
                __builtin_amdgcn_raw_buffer_store_b64(o, ors, off, 0, 0);
            } else {
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{BF16::pack2(v[0], v[1]), BF16::pack2(v[2], v[3])}, ors, off, 0, 0);
            }
        }
    }
}

// gemm_fp8.hip
bool gemm_fp8_applicable(int M, int N, int K);
int launch_gemm_fp8(const GemmFp8Args &args, int epi, hipStream_t st);  // -1: not applicable, nothing launched
// bf16 rows [M, K] -> codes [M, K], scales and group sums [M, K / 128]: one launch, 16 lanes per group (kv8.h's row codec)
int quantize_rows_fp8(const uint16_t *a, uint8_t *codes, float *scales, float *sums, int M, int K, hipStream_t st);
// W4 (checkpoint layout) -> the weight copy described above, gemm_fp8_weight_bytes(rows, cols) bytes at `out`
int expand_w4_to_fp8(const uint32_t *weight, const uint16_t *scales, const uint16_t *biases, uint8_t *out, int rows, int cols, hipStream_t st);

}  // namespace tl
