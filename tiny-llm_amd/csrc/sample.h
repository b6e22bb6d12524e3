// Device-side sampling of one token from a bf16 logits row (include/tinyllm_engine.h "sampling").
//
// Semantics, per row, with the row's maximum m (NaN logits are never ranked, counted or drawn):
//   order   by logit, highest first; equal logits by the lower token id first (-0 and +0 are equal)
//   top-k   (top_k > 0) the first min(top_k, V) tokens of that order
//   top-p   (0 < top_p < 1) token i stays while the temperature-1 probability P = exp(l - m) / sum_V exp(l - m) of the kept tokens
//           ranked before it sums to less than top_p; the first token always stays
//   draw    w_i = exp((l_i - m) / T) over the kept set, W = sum w_i; u = Philox4x32-10(key = seed, counter = (position, 0, 'SAMP', 0))
//           word 0 >> 8 times 2^-24; the token is the first kept one in ascending id whose inclusive cumulative w exceeds u W (if
//           rounding leaves none: the last kept token)
//   T == 0  the greedy id (first maximum), exactly step_end_kernel's;  a row without a finite maximum (all NaN / -inf) gives token 0,
//           a row holding +inf its first +inf
//
// One workgroup of 1,024 threads per row.  Every pass reads the row (L2-resident after the first) in the order step_end_kernel reads
// it, token = 8,192 j + 8 thread + e, 16 bytes per thread and chunk j, several chunks' loads in flight.  (A register-resident row --
// 19 x 16 bytes per thread -- left too few of the 128 VGPRs a 1,024-thread workgroup allows: the compiler spilled.)
//   * the boundary of the kept set (exact, ties included) is found in windows of 256 consecutive 16-bit keys counted downwards from
//     the maximum's key (one LDS histogram of counts per window; a window's bin is ONE key, so its mass is count x P of that key and
//     the histogram holds integers only).  Empty stretches of keys are skipped; a row with a usual top-k / top-p needs one window;
//   * "first position in token order where a running sum exceeds a target" (the inverse CDF, the cut inside the boundary key, the
//     greedy id) is one routine: per-chunk totals, the chunk that crosses, then one workgroup scan over that chunk.
#pragma once
#include "common.h"

namespace tl {

constexpr int SMP_NV = 64;                     // most 8,192-token chunks of a row
constexpr int SMP_MAX_VOCAB = SMP_NV * 8192;   // 524,288 tokens (Qwen3: 151,936)
constexpr uint32_t SMP_PAD = 0x7fc0u;          // NaN bits: positions past the vocabulary are never ranked
constexpr uint32_t SMP_COUNTER_TAG = 0x53414d50u;  // "SAMP", the third counter word

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants).  In place: c = counter in, output out.
__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0, c[1] = lo1, c[2] = n2, c[3] = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// the uniform in [0, 1) of (seed, position): 24 bits, exact in fp32
__host__ __device__ inline float sample_uniform(uint64_t seed, uint32_t position) {
    uint32_t c[4] = {position, 0u, SMP_COUNTER_TAG, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (float)(c[0] >> 8) * 5.9604644775390625e-8f;
}

// order-preserving 16-bit key of a (non-NaN) bf16 value; -0 takes +0's key
__device__ __forceinline__ int smp_key(uint32_t b) {
    b = b == 0x8000u ? 0u : b;
    return (int)((b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u));
}
__device__ __forceinline__ float smp_key_value(int k) {
    const uint32_t b = (k & 0x8000) ? ((uint32_t)k & 0x7fffu) : (~(uint32_t)k & 0xffffu);
    return __uint_as_float(b << 16);
}
__device__ __forceinline__ bool smp_nan(uint32_t b) { return (b & 0x7fffu) > 0x7f80u; }
__device__ __forceinline__ uint32_t smp_bits(const u32x4 &r, int e) { return (r[e >> 1] >> ((e & 1) * 16)) & 0xffffu; }

// the row being sampled: chunk j of this thread = tokens 8,192 j + 8 threadIdx.x + [0, 8); past the vocabulary: NaN bits
struct SmpRow {
    const uint16_t *lg;
    int vocab, chunks;
    bool aligned;
    __device__ SmpRow(const uint16_t *row, int v) : lg(row), vocab(v), chunks((v + 8191) / 8192), aligned(((uintptr_t)row & 15) == 0) {}
    __device__ __forceinline__ u32x4 chunk(int j) const {
        const int c = j * 8192 + (int)threadIdx.x * 8;
        if (aligned && c + 8 <= vocab) return act_load(reinterpret_cast<const u32x4 *>(lg + c));
        u32x4 t;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t lo = c + 2 * q < vocab ? (uint32_t)act_load(lg + c + 2 * q) : SMP_PAD;
            const uint32_t hi = c + 2 * q + 1 < vocab ? (uint32_t)act_load(lg + c + 2 * q + 1) : SMP_PAD;
            t[q] = lo | (hi << 16);
        }
        return t;
    }
};
// f(j, e, bits) over every element of this thread, chunks in order, SMP_NB chunks' loads in flight
constexpr int SMP_NB = 4;
template <class F>
__device__ __forceinline__ void smp_for_each(const SmpRow &row, F f) {
    for (int j0 = 0; j0 < row.chunks; j0 += SMP_NB) {
        u32x4 r[SMP_NB];
#pragma unroll
        for (int q = 0; q < SMP_NB; ++q) r[q] = row.chunk(min(j0 + q, row.chunks - 1));
#pragma unroll
        for (int q = 0; q < SMP_NB; ++q) {
            if (j0 + q >= row.chunks) break;
#pragma unroll
            for (int e = 0; e < 8; ++e) f(j0 + q, e, smp_bits(r[q], e));
        }
    }
}

struct SampleSmem {
    float red[16][SMP_NV];  // per wave, per chunk
    float col[SMP_NV];
    uint32_t hist[256];
    float f[16];
    int i[16];
    int jstar, result, done, base, bkey, keep_r;
    float tprime;
};

// sum over the workgroup, in a fixed order (every thread gets it)
__device__ __forceinline__ float smp_block_sum(float v, SampleSmem &sm) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm.f[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += sm.f[w];
    __syncthreads();
    return t;
}
__device__ __forceinline__ float smp_block_max(float v, SampleSmem &sm) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sm.f[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = sm.f[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) t = fmaxf(t, sm.f[w]);
    __syncthreads();
    return t;
}

// First token id (in ascending order) at which the running sum of val(j, e) >= 0 exceeds  ufrac * total + abs_target.  When rounding
// leaves no such token inside the crossing chunk: the chunk's last token with a positive value; when no chunk crosses: -1.
template <class F>
__device__ __forceinline__ int smp_find(const SmpRow &row, F val, float ufrac, float abs_target, SampleSmem &sm) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    {
        float s = 0.f;
        int jc = 0;
        smp_for_each(row, [&](int j, int e, uint32_t b) {
            if (j != jc) {  // (uniform) chunk jc is complete
                s = wave_sum(s);
                if (lane == 0) sm.red[w][jc] = s;
                s = 0.f, jc = j;
            }
            s += val(j, e, b);
        });
        s = wave_sum(s);
        if (lane == 0) sm.red[w][jc] = s;
    }
    __syncthreads();
    if (tid < row.chunks) {
        float t = 0.f;
        for (int q = 0; q < 16; ++q) t += sm.red[q][tid];
        sm.col[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        float total = 0.f;
        for (int j = 0; j < row.chunks; ++j) total += sm.col[j];
        const float target = ufrac * total + abs_target;
        float cum = 0.f;
        int js = -1;
        float tp = 0.f;
        for (int j = 0; j < row.chunks; ++j) {
            if (js < 0 && cum + sm.col[j] > target) js = j, tp = target - cum;
            cum += sm.col[j];
        }
        sm.jstar = js;
        sm.tprime = tp;
    }
    __syncthreads();
    const int js = sm.jstar;
    const float tp = sm.tprime;
    if (js < 0) return -1;  // uniform
    const u32x4 rj = row.chunk(js);
    float v[8], c[8];
    float run = 0.f;
    int last_pos = -1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        v[e] = val(js, e, smp_bits(rj, e));
        run += v[e];
        c[e] = run;
        if (v[e] > 0.f) last_pos = js * 8192 + tid * 8 + e;
    }
    float incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.f;
    if (lane == 63) sm.f[w] = incl;
    const float lastf = wave_max((float)last_pos);  // the wave's last id with a positive value (ids are exact in fp32)
    if (lane == 0) sm.i[w] = (int)lastf;
    __syncthreads();
    float before = 0.f;
    int last_all = -1;
    for (int q = 0; q < 16; ++q) {
        if (q < w) before += sm.f[q];
        last_all = max(last_all, sm.i[q]);
    }
    const float e0 = before + excl;
    const bool cross = e0 + c[7] > tp;
    const unsigned long long bal = __ballot(cross);
    __syncthreads();  // sm.f / sm.i are reused below
    if (lane == 0) sm.i[w] = bal ? w * 64 + __ffsll((long long)bal) - 1 : 0x7fffffff;
    __syncthreads();
    int first = 0x7fffffff;
    for (int q = 0; q < 16; ++q) first = min(first, sm.i[q]);
    if (tid == first) {
        int e_hit = 7;
#pragma unroll
        for (int e = 7; e >= 0; --e)
            if (e0 + c[e] > tp) e_hit = e;
        sm.result = js * 8192 + tid * 8 + e_hit;
    }
    __syncthreads();
    const int res = first == 0x7fffffff ? last_all : sm.result;
    __syncthreads();
    return res;
}

// The boundary of the kept set, in windows of 256 keys counted down from kmax: sets bkey (the key of the last kept logit; -1: every
// ranked token is kept) and keep_r (how many tokens of that key are kept, the first ones in token order), keeping at most K tokens and,
// with use_p, stopping where the temperature-1 mass exp(l - m) * inv_z ranked before a token reaches top_p.  Expanded in place in
// smp_select and lp_row (logprob.h) over their locals row, sm, tid, lane, w, m, kmax, K, use_p, top_p, inv_z, bkey, keep_r: a function
// would be simplified on its own before it is inlined, and the sampler's machine code would change with it.
#define SMP_BOUNDARY_SEARCH() \
        /* wave 0's running totals over the windows already scanned */                                                          \
        float c_above = 0.f, m_above = 0.f;                                                                                     \
        int base = 0;                                                                                                           \
        for (;;) {                                                                                                              \
                    if (tid < 256) sm.hist[tid] = 0u;                                                                           \
            __syncthreads();                                                                                                    \
            int dnext = 0x7fffffff;                                                                                             \
            smp_for_each(row, [&](int, int, uint32_t b) {                                                                       \
                if (smp_nan(b)) return;                                                                                         \
                const int d = kmax - smp_key(b) - base;                                                                         \
                if ((unsigned)d < 256u) atomicAdd(&sm.hist[d], 1u);                                                             \
                else if (d >= 256) dnext = min(dnext, d + base);                                                                \
            });                                                                                                                 \
            {                                                                                                                   \
                const float dn = -wave_max(-(float)dnext);                                                                      \
                if (lane == 0) sm.f[w] = dn;                                                                                    \
            }                                                                                                                   \
            __syncthreads();                                                                                                    \
            if (w == 0) {                                                                                                       \
                float gmin = sm.f[0];                                                                                           \
                for (int q = 1; q < 16; ++q) gmin = fminf(gmin, sm.f[q]);                                                       \
                float cnt[4], pk[4];                                                                                            \
                float lc = 0.f, lm = 0.f;                                                                                       \
_Pragma("unroll")                                                                                                               \
                for (int q = 0; q < 4; ++q) {                                                                                   \
                    const int bin = lane * 4 + q;                                                                               \
                    cnt[q] = (float)sm.hist[bin];                                                                               \
                    const int key = kmax - base - bin;                                                                          \
                    pk[q] = (use_p && cnt[q] > 0.f) ? exp2_hw((smp_key_value(key) - m) * 1.44269504089f) * inv_z : 0.f;         \
                    lc += cnt[q];                                                                                               \
                    lm += cnt[q] * pk[q];                                                                                       \
                }                                                                                                               \
                float ic = lc, im = lm;  /* inclusive lane scans (counts are exact in fp32) */                                  \
_Pragma("unroll")                                                                                                               \
                for (int o = 1; o < 64; o <<= 1) {                                                                              \
                    const float yc = __shfl_up(ic, o, 64), ym = __shfl_up(im, o, 64);                                           \
                    if (lane >= o) ic += yc, im += ym;                                                                          \
                }                                                                                                               \
                float cb = c_above + (ic - lc), mb = m_above + __shfl_up(im, 1, 64);                                            \
                if (lane == 0) mb = m_above;                                                                                    \
                int hit_bin = -1, hit_r = 0;                                                                                    \
_Pragma("unroll")                                                                                                               \
                for (int q = 0; q < 4; ++q) {                                                                                   \
                    if (hit_bin < 0 && cnt[q] > 0.f) {                                                                          \
                        const float rk = (float)K - cb;                                                                         \
                        float rp = 3.0e38f;                                                                                     \
                        if (use_p && pk[q] > 0.f) rp = fminf(ceilf((top_p - mb) / pk[q]), 3.0e38f);                             \
                        if (cb == 0.f) rp = fmaxf(rp, 1.f);                                                                     \
                        const float r = fminf(cnt[q], fminf(rk, rp));                                                           \
                        const bool boundary = r < cnt[q] || cb + cnt[q] >= (float)K || (use_p && mb + cnt[q] * pk[q] >= top_p); \
                        if (boundary) hit_bin = lane * 4 + q, hit_r = (int)fmaxf(r, 1.f);                                       \
                    }                                                                                                           \
                    cb += cnt[q];                                                                                               \
                    mb += cnt[q] * pk[q];                                                                                       \
                }                                                                                                               \
                const unsigned long long bal = __ballot(hit_bin >= 0);                                                          \
                const float tot_c = __shfl(ic, 63, 64), tot_m = __shfl(im, 63, 64);                                             \
                if (bal) {                                                                                                      \
                    if (lane == __ffsll((long long)bal) - 1) {                                                                  \
                        sm.bkey = kmax - base - hit_bin;                                                                        \
                        sm.keep_r = hit_r;                                                                                      \
                        sm.done = 1;                                                                                            \
                    }                                                                                                           \
                } else {                                                                                                        \
                    c_above += tot_c;                                                                                           \
                    m_above += tot_m;                                                                                           \
                    if (lane == 0) {                                                                                            \
                        sm.done = gmin > 1.0e9f ? 2 : 0;  /* 2: no key below the window, every token is kept */                 \
                        sm.base = gmin > 1.0e9f ? base : (int)gmin;                                                             \
                    }                                                                                                           \
                }                                                                                                               \
            }                                                                                                                   \
            __syncthreads();                                                                                                    \
            const int done = sm.done;                                                                                           \
            base = sm.base;                                                                                                     \
            if (done == 1) {                                                                                                    \
                bkey = sm.bkey;                                                                                                 \
                keep_r = sm.keep_r;                                                                                             \
            }                                                                                                                   \
            __syncthreads();                                                                                                    \
            if (done) break;                                                                                                    \
        }

// The token of one row (the same value in every thread).  m_given: the row's maximum when the caller has it (the lm_head GEMV's tile
// maxima), NaN to reduce it here.
__device__ __forceinline__ int smp_select(const SmpRow &row, float m_given, float temperature, int top_k, float top_p,
                                 uint64_t seed, uint32_t position, SampleSmem &sm) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float m = m_given;
    if (m != m) {
        float t = -INFINITY;
        smp_for_each(row, [&](int, int, uint32_t b) { t = fmaxf(t, __uint_as_float(b << 16)); });  // fmaxf drops NaN
        m = smp_block_max(t, sm);
    }
    if (!(m > -INFINITY)) return 0;  // all NaN / -inf (uniform)
    if (temperature == 0.f || m == INFINITY) {  // greedy: the first maximum
        const int g = smp_find(row, [&](int, int, uint32_t b) { return __uint_as_float(b << 16) == m ? 1.f : 0.f; }, 0.f, 0.f, sm);
        return g < 0 ? 0 : g;
    }
    const int kmax = smp_key(__float_as_uint(m) >> 16);
    const bool use_k = top_k > 0 && top_k < row.vocab;
    const bool use_p = top_p > 0.f && top_p < 1.f;
    const int K = use_k ? top_k : 0x7fffffff;
    int bkey = -1, keep_r = 0x7fffffff;  // boundary key (-1: every ranked token is kept) and how many of its tokens are kept
    if (use_k || use_p) {
        float inv_z = 0.f;
        if (use_p) {
                    float z = 0.f;
            smp_for_each(row, [&](int, int, uint32_t b) {
                if (!smp_nan(b)) z += exp2_hw((__uint_as_float(b << 16) - m) * 1.44269504089f);
            });
            inv_z = 1.f / smp_block_sum(z, sm);
        }
        SMP_BOUNDARY_SEARCH();
    }
    // the cut inside the boundary key: the keep_r-th token of that key in token order is the last one kept
    int cutoff = 0x7fffffff;
    if (bkey >= 0) {
        const int bk = bkey;
        cutoff = smp_find(row, [&](int, int, uint32_t b) { return !smp_nan(b) && smp_key(b) == bk ? 1.f : 0.f; }, 0.f, (float)(keep_r - 1), sm);
        if (cutoff < 0) cutoff = 0x7fffffff;
    }
    const float s = 1.44269504089f / temperature, ms = m * s;
    const float u = sample_uniform(seed, position);
    const int bk = bkey, cut = cutoff;
    auto weight = [&](int j, int e, uint32_t b) {
        if (smp_nan(b)) return 0.f;
        if (bk >= 0) {
            const int k = smp_key(b);
            if (k < bk || (k == bk && j * 8192 + (int)threadIdx.x * 8 + e > cut)) return 0.f;
        }
        return exp2_hw(fmaf(__uint_as_float(b << 16), s, -ms));
    };
    const int tok = smp_find(row, weight, u, 0.f, sm);
    if (tok >= 0) return tok;
    // no chunk crossed (u W rounded to W): the last kept token
    float last = -1.f;
    smp_for_each(row, [&](int j, int e, uint32_t b) {
        if (weight(j, e, b) > 0.f) last = (float)(j * 8192 + tid * 8 + e);
    });
    const float lm = smp_block_max(last, sm);
    return lm < 0.f ? 0 : (int)lm;
}

}  // namespace tl
