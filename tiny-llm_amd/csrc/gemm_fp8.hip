// Launchers of the FP8-activation prefill GEMM (gemm_fp8.h): the activation quantiser, the one-time W4 -> E4M3 weight expansion, the GEMM.
#include "gemm_fp8.h"

#include <algorithm>

namespace tl {

// 16 lanes = one 128-column group of one row, 8 values per lane: kv8.h's row codec (codes and scale bit for bit oracle/kv_fp8.py quantize_rows),
// then S = the fp32 sum of the dequantised values (8 in the lane, then over the 16 lanes)
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(const uint16_t *__restrict__ a, uint8_t *__restrict__ codes, float *__restrict__ scales,
                                                                float *__restrict__ sums, size_t groups) {
    const size_t grp = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    const bool live = grp < groups;  // (a group of 16 lanes is live or dead as a whole; the dead ones walk the last group and store nothing)
    const size_t at = (live ? grp : groups - 1) * 128 + (size_t)l * 8;
    const u32x4 raw = *reinterpret_cast<const u32x4 *>(a + at);
    float x[8], deq[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[2 * i] = __uint_as_float(raw[i] << 16);
        x[2 * i + 1] = __uint_as_float(raw[i] & 0xffff0000u);
    }
    u32x2 c;
    float s;
    kv8_quantize_row16(x, c, s, deq);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) sum += deq[i];
    sum = group16_sum(sum);
    if (!live) return;
    *reinterpret_cast<u32x2 *>(codes + at) = c;
    if (l == 0) scales[grp] = s, sums[grp] = sum;
}

int quantize_rows_fp8(const uint16_t *a, uint8_t *codes, float *scales, float *sums, int M, int K, hipStream_t st) {
    if (!a || !codes || !scales || !sums || M <= 0 || K <= 0 || K % 128 != 0) return -1;
    const size_t groups = (size_t)M * (K / 128);
    hipLaunchKernelGGL(quantize_rows_fp8_kernel, dim3((unsigned)((groups + 15) / 16)), dim3(256), 0, st, a, codes, scales, sums, groups);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// one thread = one packed word = 8 consecutive weights of a row -> 8 E4M3 codes of q - 8 (the integers -8 .. 7 are exact: the hardware conversion rounds nothing)
__global__ __launch_bounds__(256) void expand_w4_fp8_codes_kernel(const uint32_t *__restrict__ weight, uint8_t *__restrict__ out, size_t words) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= words) return;
    const uint32_t w = weight[i];
    float q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = (float)((w >> (4 * e)) & 0xfu) - 8.f;
    *reinterpret_cast<u32x2 *>(out + i * 8) = kv8_pack8(q);
}
// s -> fp32 [G][Np], beta' = beta + 8 s -> fp32 [Np][Gp], the padding zero: one thread per element of [Np][Gp]
__global__ __launch_bounds__(256) void expand_w4_fp8_affine_kernel(const uint16_t *__restrict__ scales, const uint16_t *__restrict__ biases, float *__restrict__ ws,
                                                                   float *__restrict__ wb, int N, int G, int Np, int Gp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Np * Gp) return;
    const int n = (int)(i / Gp), g = (int)(i % Gp);
    const bool in = n < N && g < G;
    const float sc = in ? BF16::to_float(scales[(size_t)n * G + g]) : 0.f, be = in ? BF16::to_float(biases[(size_t)n * G + g]) : 0.f;
    wb[i] = __builtin_fmaf(8.f, sc, be);
    if (g < G) ws[(size_t)g * Np + n] = sc;
}

int expand_w4_to_fp8(const uint32_t *weight, const uint16_t *scales, const uint16_t *biases, uint8_t *out, int rows, int cols, hipStream_t st) {
    if (!weight || !scales || !biases || !out || rows <= 0 || cols <= 0 || cols % 128 != 0) return -1;
    const size_t words = (size_t)rows * (cols / 8);
    const int Np = gemm_fp8_np(rows), Gp = gemm_fp8_gp(cols);
    hipLaunchKernelGGL(expand_w4_fp8_codes_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, weight, out, words);
    hipLaunchKernelGGL(expand_w4_fp8_affine_kernel, dim3((unsigned)(((size_t)Np * Gp + 255) / 256)), dim3(256), 0, st, scales, biases,
                       reinterpret_cast<float *>(out + gemm_fp8_off_s(rows, cols)), reinterpret_cast<float *>(out + gemm_fp8_off_b(rows, cols)), rows, cols / 128, Np, Gp);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// whole quantisation groups; rows and columns are ragged-safe (buffer range checks, masked stores; a lane stores four consecutive columns); the byte
// offsets of a lane stay inside 31 bits
bool gemm_fp8_applicable(int M, int N, int K) {
    return M >= 1 && N >= 4 && N % 4 == 0 && K >= 128 && K % 128 == 0 && (size_t)(M + F8_BM) * K < (1ull << 31) && (size_t)(N + F8_BN) * K < (1ull << 31) &&
           (size_t)M * N * 2 < (1ull << 31);
}

template <int EPI>
static int launch_fp8(const GemmFp8Args &a, hipStream_t st) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_fp8_kernel<EPI>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)F8_LDS_BYTES);
    const int tiles = ((a.M + F8_BM - 1) / F8_BM) * ((a.N + F8_BN - 1) / F8_BN);
    hipLaunchKernelGGL(gemm_fp8_kernel<EPI>, dim3((tiles + 7) / 8 * 8), dim3(F8_WAVES * 64), F8_LDS_BYTES, st, a);  // eight runs of tiles, one per XCD
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_gemm_fp8(const GemmFp8Args &args, int epi, hipStream_t st) {
    if (!args.codes || !args.scales || !args.sums || !args.wq || !args.ws || !args.wb || !args.out) return -1;
    if (!gemm_fp8_applicable(args.M, args.N, args.K)) return -1;
    if (epi == EPI_RESIDUAL && !args.residual) return -1;
    if (epi == EPI_STORE) return launch_fp8<EPI_STORE>(args, st);
    if (epi == EPI_RESIDUAL) return launch_fp8<EPI_RESIDUAL>(args, st);
    if (epi == EPI_SWIGLU) return launch_fp8<EPI_SWIGLU>(args, st);
    return -1;
}

}  // namespace tl
