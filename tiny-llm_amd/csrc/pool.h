// Pooling of final-normalised hidden rows into text embeddings (include/tinyllm_engine.h "Embeddings", DESIGN.md section 4;
// tl_pool_rows, tl_engine_embed, tl_engine_embed_packed).  Host side of engine.hip only: no decode step launches these kernels.
//
// Input: bf16 rows [total, hidden], already final-normalised (the model's output rows); up to POOL_MAX_SEQS sequences per launch, each
// the rows [row0, row0 + len).  Semantics per sequence:
//   TL_POOL_LAST   v = the last row, widened to fp32 (exact)
//   TL_POOL_MEAN   the chunk's fp32 column sums join the sequence's running sum [hidden] (replace it when no row was accumulated
//                  before); on finish v = running sum / rows accumulated
//   finish         the first `dim` components of v; with normalize, divided by their Euclidean norm (sum of squares in fp32; a
//                  vector of norm 0 stays as it is, NaN propagates) -> fp32 [dim]
// The column sums: wave w of a workgroup adds rows w, w + 8, w + 16, ... of the SEQUENCE (not of the buffer) in ascending order, the
// eight partial sums are combined through LDS in wave order.  No atomics: the result depends on the sequence's rows and on how they were
// cut into chunks, never on row0 or on the other sequences of the launch.
#pragma once

#include "common.h"
#include "../../include/tinyllm_engine.h"

namespace tl {

constexpr int POOL_MAX_SEQS = 16;
constexpr int POOL_SUM_WAVES = 8;     // waves of a column-sum workgroup: one per row residue
constexpr int POOL_SUM_COLS = 128;    // columns of a column-sum workgroup: two per lane
constexpr int POOL_FINISH_THREADS = 256;

struct PoolArgs {
    const uint16_t *rows;  // [total, hidden] bf16
    float *sums;           // MEAN: running sums, sequence i at sums + sum_index[i] * hidden
    float *out;            // finishing sequence i at out + out_index[i] * dim
    int hidden, dim, mode, normalize;
    int row0[POOL_MAX_SEQS], len[POOL_MAX_SEQS], prior[POOL_MAX_SEQS], sum_index[POOL_MAX_SEQS], out_index[POOL_MAX_SEQS];
    int seq_of[POOL_MAX_SEQS];  // finish kernel: the sequence of workgroup b
};

// grid = (ceil(hidden / 128), n_seqs), block = 512.  hidden is even: a lane reads its two columns as one dword
static __global__ __launch_bounds__(POOL_SUM_WAVES * WAVE) void pool_sum_kernel(const PoolArgs a) {
    __shared__ f32x2 part[POOL_SUM_WAVES][WAVE];
    const int s = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = blockIdx.x * POOL_SUM_COLS + 2 * lane;
    const bool in = col < a.hidden;
    const int len = a.len[s];
    const uint16_t *base = a.rows + (size_t)a.row0[s] * a.hidden + col;
    f32x2 acc = {0.f, 0.f};
    if (in) {
#pragma unroll 4
        for (int r = w; r < len; r += POOL_SUM_WAVES) {
            const uint32_t two = *reinterpret_cast<const uint32_t *>(base + (size_t)r * a.hidden);
            acc[0] += __uint_as_float(two << 16);
            acc[1] += __uint_as_float(two & 0xffff0000u);
        }
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && in) {
        f32x2 t = part[0][lane];
#pragma unroll
        for (int k = 1; k < POOL_SUM_WAVES; ++k) {
            t[0] += part[k][lane][0];
            t[1] += part[k][lane][1];
        }
        float *dst = a.sums + (size_t)a.sum_index[s] * a.hidden + col;
        if (a.prior[s] > 0) {
            t[0] = dst[0] + t[0];
            t[1] = dst[1] + t[1];
        }
        dst[0] = t[0];
        dst[1] = t[1];
    }
}

// grid = finishing sequences, block = 256: thread t holds components t, t + 256, ... of its sequence's vector
static __global__ __launch_bounds__(POOL_FINISH_THREADS) void pool_finish_kernel(const PoolArgs a) {
    __shared__ float wave_ss[POOL_FINISH_THREADS / WAVE];
    const int s = a.seq_of[blockIdx.x], tid = threadIdx.x;
    const uint16_t *last = a.rows + (size_t)(a.row0[s] + a.len[s] - 1) * a.hidden;
    const bool mean = a.mode == TL_POOL_MEAN;
    const float *sum = mean ? a.sums + (size_t)a.sum_index[s] * a.hidden : nullptr;  // (LAST has no running sums)
    const float count = (float)(a.prior[s] + a.len[s]);
    float *out = a.out + (size_t)a.out_index[s] * a.dim;
    const auto value = [&](int c) { return mean ? sum[c] / count : BF16::to_float(last[c]); };
    if (!a.normalize) {
        for (int c = tid; c < a.dim; c += POOL_FINISH_THREADS) out[c] = value(c);
        return;
    }
    float ss = 0.f;
    for (int c = tid; c < a.dim; c += POOL_FINISH_THREADS) {
        const float v = value(c);
        ss += v * v;
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) wave_ss[tid >> 6] = ss;
    __syncthreads();
    const float total = (wave_ss[0] + wave_ss[1]) + (wave_ss[2] + wave_ss[3]);
    const float norm = sqrtf(total);
    for (int c = tid; c < a.dim; c += POOL_FINISH_THREADS) {
        const float v = value(c);
        out[c] = total == 0.f ? v : v / norm;
    }
}

// What tl_pool_rows and the engine share.  Stream ordered; sequence i accumulates into sums + sum_index[i] * hidden (MEAN) and, when
// finish[i], writes out + (its number among the finishing ones) * dim.  The caller vouches for the rows behind row0 / len.
static inline int pool_rows(const uint16_t *rows, int hidden, int n_seqs, const int *row0, const int *len, const int *finish, const int *prior,
                            const int *sum_index, int mode, float *sums, int normalize, int dim, float *out, hipStream_t stream) {
    TL_REQUIRE(rows && row0 && len && finish, "pool_rows: null argument");
    TL_REQUIRE(mode == TL_POOL_LAST || mode == TL_POOL_MEAN, "pool_rows: pooling is TL_POOL_LAST or TL_POOL_MEAN");
    TL_REQUIRE(n_seqs >= 1 && n_seqs <= POOL_MAX_SEQS, "pool_rows: between 1 and 16 sequences per call");
    TL_REQUIRE(hidden >= 2 && hidden % 2 == 0, "pool_rows: hidden must be even");
    TL_REQUIRE((uintptr_t)rows % 4 == 0, "pool_rows: the rows must be 4-byte aligned (a lane reads two columns as one dword)");
    TL_REQUIRE(dim >= 1 && dim <= hidden, "pool_rows: dim must be 1 .. hidden");
    TL_REQUIRE(mode == TL_POOL_LAST || (sums && prior), "pool_rows: mean pooling needs the running sums and their row counts");
    TL_REQUIRE(mode == TL_POOL_LAST || (uintptr_t)sums % 4 == 0, "pool_rows: the running sums must be 4-byte aligned");
    PoolArgs a{};
    a.rows = rows, a.sums = sums, a.out = out, a.hidden = hidden, a.dim = dim, a.mode = mode, a.normalize = normalize ? 1 : 0;
    int n_finish = 0;
    for (int i = 0; i < n_seqs; ++i) {
        TL_REQUIRE(row0[i] >= 0 && len[i] >= 1, "pool_rows: every sequence needs a nonnegative first row and at least one row");
        TL_REQUIRE((long)row0[i] + len[i] <= 0x7fffffffL, "pool_rows: row index out of range");
        a.row0[i] = row0[i], a.len[i] = len[i];
        a.prior[i] = mode == TL_POOL_MEAN ? prior[i] : 0;
        TL_REQUIRE(a.prior[i] >= 0 && (long)a.prior[i] + len[i] <= (1L << 24), "pool_rows: rows accumulated must be 0 .. 2^24 (exact in fp32)");
        a.sum_index[i] = sum_index ? sum_index[i] : i;
        TL_REQUIRE(a.sum_index[i] >= 0, "pool_rows: negative running-sum index");
        if (finish[i]) a.seq_of[n_finish] = i, a.out_index[i] = n_finish++;
    }
    TL_REQUIRE(n_finish == 0 || out, "pool_rows: a sequence finishes and there is no output");
    if (mode == TL_POOL_MEAN) {
        hipLaunchKernelGGL(pool_sum_kernel, dim3(ceil_div(hidden, POOL_SUM_COLS), n_seqs), dim3(POOL_SUM_WAVES * WAVE), 0, stream, a);
        TL_CHECK_LAUNCH("pool_rows column sums");
    }
    if (n_finish > 0) {
        hipLaunchKernelGGL(pool_finish_kernel, dim3(n_finish), dim3(POOL_FINISH_THREADS), 0, stream, a);
        TL_CHECK_LAUNCH("pool_rows finish");
    }
    return TL_OK;
}

}  // namespace tl
