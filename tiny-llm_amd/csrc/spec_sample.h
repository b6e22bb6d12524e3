// Speculative sampling: verification of draft proposals for sampling slots (include/tinyllm_engine.h "speculative sampling",
// DESIGN.md section 4; Leviathan et al. 2023, Chen et al. 2023).
//
// Per row: a target logits row and the draft logits row the proposal x was drawn from, each with its own sampler parameters.  With the
// sampler's kept set and weights of sample.h applied to each row (wp, Wp = sum wp for the target; wq, Wq for the draft):
//   one-hot  a row with temperature 0, or whose result the sampler's edge rules fix (no finite maximum, +inf), has w = 1 at the id
//            smp_select returns and 0 elsewhere, W = 1
//   draws    Philox4x32-10 with key = seed and counter (position, 0, tag, 0) as sample_uniform: u_acc with tag 'SPAC', u_res with 'SPRS'
//   x < 0    a bonus row: accept = 0, alt = smp_select on the target row with the ordinary 'SAMP' draw (bit for bit tl_sample_logits)
//   x >= V   rejected without a read at x
//   accept   iff u_acc wq_x Wp < wp_x Wq (fp32 products, no division): wp_x == 0 always rejects, wq_x == 0 < wp_x accepts; alt = -1
//   reject   r_j = max(wp_j Wq - wq_j Wp, 0), R = sum r; alt = the first id in ascending order whose inclusive cumulative r exceeds
//            u_res R (rounding leaving none: the last id with r > 0; R == 0: the plain inverse-CDF draw from wp with u_res)
// A one-hot target row makes this "accept iff x is that id, alt = that id": greedy verification.
//
// One workgroup of 1,024 threads per row, rows read as the sampler reads them (16 bytes per thread and chunk).  The passes over two rows
// keep two chunks of each in flight where the sampler keeps four of one.  sample.h is used as it stands; what needs both rows' bits
// (the totals, the residual search) is written here.
#pragma once
#include "sample.h"

namespace tl {

constexpr uint32_t SSP_ACCEPT_TAG = 0x53504143u;    // "SPAC"
constexpr uint32_t SSP_RESIDUAL_TAG = 0x53505253u;  // "SPRS"

struct SpecSampleArgs {
    const uint16_t *target;   // [rows, vocab]
    const uint16_t *draft;    // [rows, vocab]; the row of a bonus proposal is never read
    int vocab;
    const int32_t *proposal;  // [rows]
    const float *t_temperature;
    const int32_t *t_top_k;
    const float *t_top_p;
    const float *d_temperature;
    const int32_t *d_top_k;
    const float *d_top_p;
    const uint64_t *seed;
    const int32_t *position;
    int32_t *accept, *alt;    // [rows]
};

__host__ __device__ inline float ssp_uniform(uint64_t seed, uint32_t position, uint32_t tag) {
    uint32_t c[4] = {position, 0u, tag, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (float)(c[0] >> 8) * 5.9604644775390625e-8f;
}

// the kept set of one row as the sampler defines it, and the scale of its weights; onehot >= 0: the row is one-hot there
struct SspKept {
    float s, ms;
    int bkey, cutoff, onehot;
};
// w of token t (its bits b) under k
__device__ __forceinline__ float ssp_weight(const SspKept &k, int t, uint32_t b) {
    if (k.onehot >= 0) return t == k.onehot ? 1.f : 0.f;
    if (smp_nan(b)) return 0.f;
    if (k.bkey >= 0) {
        const int key = smp_key(b);
        if (key < k.bkey || (key == k.bkey && t > k.cutoff)) return 0.f;
    }
    return exp2_hw(fmaf(__uint_as_float(b << 16), k.s, -k.ms));
}
// the products are rounded one by one: a fused multiply-add would keep a rounding error where p and q agree exactly
__device__ __forceinline__ float ssp_residual(float wp, float wq, float Wp, float Wq) {
#pragma clang fp contract(off)
    const float a = wp * Wq, b = wq * Wp;
    return fmaxf(a - b, 0.f);
}
__device__ __forceinline__ bool ssp_accepts(float u, float wp, float wq, float Wp, float Wq) {
#pragma clang fp contract(off)
    const float a = u * wq, l = a * Wp, r = wp * Wq;
    return l < r;
}

// smp_select's steps up to the weights, for one row (the same value in every thread)
__device__ __forceinline__ SspKept ssp_kept(const SmpRow &row, float temperature, int top_k, float top_p, SampleSmem &sm) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    SspKept kd{0.f, 0.f, -1, 0x7fffffff, -1};
    float m;
    {
        float t = -INFINITY;
        smp_for_each(row, [&](int, int, uint32_t b) { t = fmaxf(t, __uint_as_float(b << 16)); });  // fmaxf drops NaN
        m = smp_block_max(t, sm);
    }
    if (!(m > -INFINITY)) {  // all NaN / -inf (uniform)
        kd.onehot = 0;
        return kd;
    }
    if (temperature == 0.f || m == INFINITY) {  // greedy: the first maximum
        const int g = smp_find(row, [&](int, int, uint32_t b) { return __uint_as_float(b << 16) == m ? 1.f : 0.f; }, 0.f, 0.f, sm);
        kd.onehot = g < 0 ? 0 : g;
        return kd;
    }
    const int kmax = smp_key(__float_as_uint(m) >> 16);
    const bool use_k = top_k > 0 && top_k < row.vocab;
    const bool use_p = top_p > 0.f && top_p < 1.f;
    const int K = use_k ? top_k : 0x7fffffff;
    int bkey = -1, keep_r = 0x7fffffff;
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
    if (bkey >= 0) {
        const int bk = bkey;
        const int cut = smp_find(row, [&](int, int, uint32_t b) { return !smp_nan(b) && smp_key(b) == bk ? 1.f : 0.f; }, 0.f, (float)(keep_r - 1), sm);
        kd.cutoff = cut < 0 ? 0x7fffffff : cut;
    }
    kd.bkey = bkey;
    kd.s = 1.44269504089f / temperature;
    kd.ms = m * kd.s;
    return kd;
}

// f(token, target bits, draft bits) over every element of this thread, chunks in order, SSP_NB chunks of each row in flight
constexpr int SSP_NB = 2;
template <class F>
__device__ __forceinline__ void ssp_for_each2(const SmpRow &p, const SmpRow &q, F f) {
    for (int j0 = 0; j0 < p.chunks; j0 += SSP_NB) {
        u32x4 a[SSP_NB], b[SSP_NB];
#pragma unroll
        for (int i = 0; i < SSP_NB; ++i) {
            a[i] = p.chunk(min(j0 + i, p.chunks - 1));
            b[i] = q.chunk(min(j0 + i, p.chunks - 1));
        }
#pragma unroll
        for (int i = 0; i < SSP_NB; ++i) {
            if (j0 + i >= p.chunks) break;
#pragma unroll
            for (int e = 0; e < 8; ++e) f((j0 + i) * 8192 + (int)threadIdx.x * 8 + e, smp_bits(a[i], e), smp_bits(b[i], e));
        }
    }
}

struct SpecSmem {
    SampleSmem s;
    float total;
};

// smp_find with a value formed from two rows' bits, val(token, target bits, draft bits) >= 0: the first token id at which the running
// sum exceeds ufrac * total; when rounding leaves none inside the crossing chunk, that chunk's last token with a positive value; when
// no chunk crosses, -1.  ss.total holds the total afterwards.
template <class F>
__device__ __forceinline__ int ssp_find2(const SmpRow &p, const SmpRow &q, F val, float ufrac, SpecSmem &ss) {
    SampleSmem &sm = ss.s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    {
        float s = 0.f;
        int jc = 0;
        ssp_for_each2(p, q, [&](int t, uint32_t bp, uint32_t bq) {
            const int j = t >> 13;
            if (j != jc) {  // (uniform) chunk jc is complete
                s = wave_sum(s);
                if (lane == 0) sm.red[w][jc] = s;
                s = 0.f, jc = j;
            }
            s += val(t, bp, bq);
        });
        s = wave_sum(s);
        if (lane == 0) sm.red[w][jc] = s;
    }
    __syncthreads();
    if (tid < p.chunks) {
        float t = 0.f;
        for (int i = 0; i < 16; ++i) t += sm.red[i][tid];
        sm.col[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        float total = 0.f;
        for (int j = 0; j < p.chunks; ++j) total += sm.col[j];
        const float target = ufrac * total;
        float cum = 0.f;
        int js = -1;
        float tp = 0.f;
        for (int j = 0; j < p.chunks; ++j) {
            if (js < 0 && cum + sm.col[j] > target) js = j, tp = target - cum;
            cum += sm.col[j];
        }
        sm.jstar = js;
        sm.tprime = tp;
        ss.total = total;
    }
    __syncthreads();
    const int js = sm.jstar;
    const float tp = sm.tprime;
    if (js < 0) return -1;  // uniform
    const u32x4 pj = p.chunk(js), qj = q.chunk(js);
    float c[8];
    float run = 0.f;
    int last_pos = -1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int t = js * 8192 + tid * 8 + e;
        const float v = val(t, smp_bits(pj, e), smp_bits(qj, e));
        run += v;
        c[e] = run;
        if (v > 0.f) last_pos = t;
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
    for (int i = 0; i < 16; ++i) {
        if (i < w) before += sm.f[i];
        last_all = max(last_all, sm.i[i]);
    }
    const float e0 = before + excl;
    const bool cross = e0 + c[7] > tp;
    const unsigned long long bal = __ballot(cross);
    __syncthreads();  // sm.f / sm.i are reused below
    if (lane == 0) sm.i[w] = bal ? w * 64 + __ffsll((long long)bal) - 1 : 0x7fffffff;
    __syncthreads();
    int first = 0x7fffffff;
    for (int i = 0; i < 16; ++i) first = min(first, sm.i[i]);
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

// One row: accept (0 / 1) and alt (-1 when accepted), the same values in every thread.
__device__ __forceinline__ void ssp_row(const SmpRow &p, const SmpRow &q, int x, float t_temp, int t_top_k, float t_top_p, float d_temp,
                                        int d_top_k, float d_top_p, uint64_t seed, uint32_t position, SpecSmem &ss, int *accept, int *alt) {
    SampleSmem &sm = ss.s;
    *accept = 0;
    if (x < 0) {  // a bonus row: the sampler's own draw
        *alt = smp_select(p, __builtin_nanf(""), t_temp, t_top_k, t_top_p, seed, position, sm);
        return;
    }
    const SspKept kp = ssp_kept(p, t_temp, t_top_k, t_top_p, sm);
    if (kp.onehot >= 0) {  // greedy verification (what the rules below give for a one-hot target, whatever the draft row holds)
        *accept = x == kp.onehot;
        *alt = *accept ? -1 : kp.onehot;
        return;
    }
    const SspKept kq = ssp_kept(q, d_temp, d_top_k, d_top_p, sm);
    float sp = 0.f, sq = 0.f;
    ssp_for_each2(p, q, [&](int t, uint32_t bp, uint32_t bq) {
        sp += ssp_weight(kp, t, bp);
        sq += ssp_weight(kq, t, bq);
    });
    const float Wp = smp_block_sum(sp, sm), Wq = smp_block_sum(sq, sm);
    if (x < p.vocab) {
        const float wpx = ssp_weight(kp, x, act_load(p.lg + x)), wqx = ssp_weight(kq, x, act_load(q.lg + x));
        if (ssp_accepts(ssp_uniform(seed, position, SSP_ACCEPT_TAG), wpx, wqx, Wp, Wq)) {
            *accept = 1;
            *alt = -1;
            return;
        }
    }
    const float u = ssp_uniform(seed, position, SSP_RESIDUAL_TAG);
    auto residual = [&](int t, uint32_t bp, uint32_t bq) { return ssp_residual(ssp_weight(kp, t, bp), ssp_weight(kq, t, bq), Wp, Wq); };
    int tok = ssp_find2(p, q, residual, u, ss);
    if (tok < 0) {
        const bool none = !(ss.total > 0.f);  // (read before the next search writes it)
        __syncthreads();
        if (none) {  // R == 0: the plain draw from wp
            auto weight = [&](int j, int e, uint32_t b) { return ssp_weight(kp, j * 8192 + (int)threadIdx.x * 8 + e, b); };
            tok = smp_find(p, weight, u, 0.f, sm);
            if (tok < 0) {
                float last = -1.f;
                smp_for_each(p, [&](int j, int e, uint32_t b) {
                    if (weight(j, e, b) > 0.f) last = (float)(j * 8192 + (int)threadIdx.x * 8 + e);
                });
                tok = (int)fmaxf(smp_block_max(last, sm), 0.f);
            }
        } else {  // u R rounded to R: the last id with a positive residual
            float last = -1.f;
            ssp_for_each2(p, q, [&](int t, uint32_t bp, uint32_t bq) {
                if (residual(t, bp, bq) > 0.f) last = (float)t;
            });
            tok = (int)fmaxf(smp_block_max(last, sm), 0.f);
        }
    }
    *alt = tok;
}

// grid = rows, block = 1024
static __global__ __launch_bounds__(1024) void spec_sample_rows_kernel(const SpecSampleArgs a) {
    __shared__ SpecSmem ss;
    const int i = blockIdx.x;
    const SmpRow p(a.target + (long)i * a.vocab, a.vocab), q(a.draft + (long)i * a.vocab, a.vocab);
    int accept, alt;
    ssp_row(p, q, a.proposal[i], a.t_temperature[i], a.t_top_k[i], a.t_top_p[i], a.d_temperature[i], a.d_top_k[i], a.d_top_p[i], a.seed[i],
            (uint32_t)a.position[i], ss, &accept, &alt);
    if (threadIdx.x == 0) {
        a.accept[i] = accept;
        a.alt[i] = alt;
    }
}
}  // namespace tl
