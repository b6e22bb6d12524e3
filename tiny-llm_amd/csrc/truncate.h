// Truncation of a bf16 logits row ahead of the token choice (include/tinyllm_engine.h "truncation"): min-p, locally
// typical sampling and Mirostat v2 turn the row the choice is made from into a FILTERED bf16 row -- kept tokens keep their bits, every
// other token becomes -inf -- and the greedy rule / the sampler then run on the filtered row unchanged.
//
// Per row, with temperature T > 0, the row's maximum m over non-NaN logits, t_i = (x_i - m) / T and w_i = exp(t_i) (fp32):
//   min-p     (0 < min_p <= 1)     i stays iff t_i >= ln(min_p)
//   typical-p (0 < typical_p < 1)  over the survivors: tbar = sum w t / sum w (so that |(-ln p_i) - H| = |t_i - tbar| = d_i); delta* = the
//             smallest d for which the mass of {d_i <= delta*} reaches typical_p; i stays iff d_i <= delta* (ties with the boundary stay)
//   Mirostat  (mu not NaN; no other truncation)  i stays iff -log2 p_i <= mu over the whole row; the first maximum always stays; the row
//             also leaves L = ln sum_kept exp(x_i / T), from which the update launch forms the surprise of the drawn token
// A row with T == 0, with every parameter off, or whose maximum is not finite (all NaN / -inf, a +inf) is copied bit for bit: the choice
// of such a row does not depend on a filter.  In every other row NaN logits become -inf like the dropped tokens.
//
// One workgroup of 1,024 threads per row, reading it through SmpRow / smp_for_each like the sampler (sample.h): maximum; sums (min-p
// already applied); the typical boundary; the write.  t, w and d are functions of the 16-bit key of a logit alone (smp_key), so the
// typical boundary is found exactly from INTEGER per-key counts: two LDS windows of TRN_W consecutive keys walk outwards from the
// entropy point (the first key with t >= tbar), one up, one down; each side is ordered by d already, so a bin's mass-before is its own
// side's prefix plus a binary search in the other side's.  A round decides every d up to the smaller of the two windows' ends; the rest
// waits for the next round (empty stretches of keys are skipped).  No float atomics: every sum runs in a fixed order.
#pragma once
#include "common.h"
#include "sample.h"

namespace tl {

constexpr int TRN_W = 2048;           // keys per window and side (16 binades of bf16)
constexpr int TRN_MAX_ROUNDS = 80;    // 2 x 65,536 / TRN_W + slack: the walk ends by itself; this bounds it whatever the input
constexpr int TRN_KEY_LO = 0x007f;    // smp_key(-inf)
constexpr int TRN_KEY_HI = 0xff80;    // smp_key(+inf)
constexpr float TRN_LOG2E = 1.44269504089f;

// (one struct by value, like every kernel of a decode step: csrc/aql.cpp copies a captured node's argument block as it is)
struct TruncateArgs {
    const uint16_t *logits;    // [rows, vocab] the rows the choice would be made from; row i belongs to slot slot0 + i
    uint16_t *out;             // [rows, vocab] filtered
    int vocab, slot0;
    const float *temperature;  // [slots]
    const float *min_p;        // [slots] 0: off
    const float *typical_p;    // [slots] outside (0, 1): off
    const float *mu;           // [slots] NaN: no Mirostat
    float *kept_logsum;        // [rows] L of a Mirostat row (NaN for every other row); nullptr: not wanted
    prof_t *prof;
};

struct TruncateSmem {
    SampleSmem s;
    uint32_t up[TRN_W], dn[TRN_W];  // per-key counts of a round, then (in place, as float bits) inclusive prefix masses
};

// t and d of a key: THE definitions (every pass uses these, so that a token and its histogram bin agree bit for bit)
__device__ __forceinline__ float trn_t(float x, float m, float T) { return (x - m) / T; }
__device__ __forceinline__ float trn_key_t(int key, float m, float T) { return trn_t(smp_key_value(key), m, T); }
__device__ __forceinline__ float trn_key_dev(int key, float m, float T, float tbar) {
    if (key <= TRN_KEY_LO || key >= TRN_KEY_HI) return INFINITY;  // no finite logit has this key
    return fabsf(trn_key_t(key, m, T) - tbar);
}

// exclusive prefix of v over the workgroup in thread order (fixed order); *total: the workgroup's sum
__device__ __forceinline__ float trn_block_scan(float v, SampleSmem &sm, float *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) sm.f[w] = incl;
    __syncthreads();
    float before = 0.f, tot = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (q < w) before += sm.f[q];
        tot += sm.f[q];
    }
    __syncthreads();
    *total = tot;
    return before + (incl - v);
}

// how many bins b of [0, TRN_W) on one side (key = base + dir * b) have d <= limit (d does not decrease with b)
__device__ __forceinline__ int trn_bins_within(int base, int dir, float limit, float m, float T, float tbar) {
    int lo = 0, hi = TRN_W;  // the answer is in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (trn_key_dev(base + dir * mid, m, T, tbar) <= limit) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the typical boundary delta* of a row (the same value in every thread).  keep1(bits): the token survived min-p.
template <class K>
__device__ __forceinline__ float trn_typical_boundary(const SmpRow &row, K keep1, float m, float T, float tbar, float inv_z, float typical_p,
                                                      TruncateSmem &ts) {
    SampleSmem &sm = ts.s;
    const int tid = threadIdx.x;
    // the entropy point: the first key with t >= tbar (t(key of m) = 0 >= tbar)
    int ubase;
    {
        int lo = TRN_KEY_LO + 1, hi = TRN_KEY_HI - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (trn_key_t(mid, m, T) >= tbar) hi = mid;
            else lo = mid + 1;
        }
        ubase = lo;
    }
    int dbase = ubase - 1;  // the down side's first key; bin b = key dbase - b
    float before = 0.f;
    for (int round = 0; round < TRN_MAX_ROUNDS; ++round) {
        for (int b = tid; b < TRN_W; b += 1024) ts.up[b] = 0u, ts.dn[b] = 0u;
        __syncthreads();
        // counts of the two windows, and the nearest key beyond each (ids and keys are exact in fp32)
        float umore = 1.0e9f, dmore = -1.f;
        smp_for_each(row, [&](int, int, uint32_t b) {
            if (smp_nan(b) || !keep1(b)) return;
            const int k = smp_key(b);
            if (k <= TRN_KEY_LO) return;  // -inf: weight 0, never inside a boundary
            const int du = k - ubase, dd = dbase - k;
            if ((unsigned)du < (unsigned)TRN_W) atomicAdd(&ts.up[du], 1u);
            else if (du >= TRN_W) umore = fminf(umore, (float)k);
            if ((unsigned)dd < (unsigned)TRN_W) atomicAdd(&ts.dn[dd], 1u);
            else if (dd >= TRN_W) dmore = fmaxf(dmore, (float)k);
        });
        umore = -smp_block_max(-umore, sm);
        dmore = smp_block_max(dmore, sm);
        const bool up_more = umore < 1.0e8f, dn_more = dmore >= 0.f;
        // masses (count x p of the key) and their inclusive prefixes, each side in bin order: thread i holds bins 2 i and 2 i + 1
        float mu2[2], md2[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int b = tid * 2 + q;
            const float cu = (float)ts.up[b], cd = (float)ts.dn[b];
            mu2[q] = cu > 0.f ? cu * (exp2_hw(trn_key_t(ubase + b, m, T) * TRN_LOG2E) * inv_z) : 0.f;
            md2[q] = cd > 0.f ? cd * (exp2_hw(trn_key_t(dbase - b, m, T) * TRN_LOG2E) * inv_z) : 0.f;
        }
        float tot_u, tot_d;
        const float eu = trn_block_scan(mu2[0] + mu2[1], sm, &tot_u);
        const float ed = trn_block_scan(md2[0] + md2[1], sm, &tot_d);
        ts.up[tid * 2] = __float_as_uint(eu + mu2[0]), ts.up[tid * 2 + 1] = __float_as_uint(eu + mu2[0] + mu2[1]);
        ts.dn[tid * 2] = __float_as_uint(ed + md2[0]), ts.dn[tid * 2 + 1] = __float_as_uint(ed + md2[0] + md2[1]);
        __syncthreads();
        // what this round can decide: a side with keys beyond its window only vouches for d up to its window's end
        const float lim_u = up_more ? trn_key_dev(ubase + TRN_W - 1, m, T, tbar) : INFINITY;
        const float lim_d = dn_more ? trn_key_dev(dbase - (TRN_W - 1), m, T, tbar) : INFINITY;
        const float dlim = fminf(lim_u, lim_d);
        float cand = INFINITY;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int b = tid * 2 + q;
            {  // the up bin: its own prefix + the down bins at least as close
                const float d = trn_key_dev(ubase + b, m, T, tbar);
                if (d <= dlim) {
                    const int j = trn_bins_within(dbase, -1, d, m, T, tbar);
                    const float cum = before + __uint_as_float(ts.up[b]) + (j > 0 ? __uint_as_float(ts.dn[j - 1]) : 0.f);
                    if (cum >= typical_p) cand = fminf(cand, d);
                }
            }
            {
                const float d = trn_key_dev(dbase - b, m, T, tbar);
                if (d <= dlim) {
                    const int j = trn_bins_within(ubase, 1, d, m, T, tbar);
                    const float cum = before + __uint_as_float(ts.dn[b]) + (j > 0 ? __uint_as_float(ts.up[j - 1]) : 0.f);
                    if (cum >= typical_p) cand = fminf(cand, d);
                }
            }
        }
        cand = -smp_block_max(-cand, sm);
        if (cand < INFINITY) return cand;                // uniform
        if (!(dlim < INFINITY)) return INFINITY;         // both sides exhausted (rounding left the mass short): every survivor stays
        // everything up to dlim joins `before`; each side goes on behind what it consumed (a whole window: at its next key, if any)
        const int cu = trn_bins_within(ubase, 1, dlim, m, T, tbar), cd = trn_bins_within(dbase, -1, dlim, m, T, tbar);
        if (cu > 0) before += __uint_as_float(ts.up[cu - 1]);
        if (cd > 0) before += __uint_as_float(ts.dn[cd - 1]);
        __syncthreads();  // the windows are cleared next
        ubase = cu < TRN_W ? ubase + cu : (up_more ? (int)umore : 0x20000);   // 0x20000: no key is inside or beyond this window
        dbase = cd < TRN_W ? dbase - cd : (dn_more ? (int)dmore : -0x20000);
    }
    return INFINITY;
}

static __global__ __launch_bounds__(1024) void truncate_rows_kernel(const TruncateArgs a) {
    __shared__ TruncateSmem ts;
    SampleSmem &sm = ts.s;
    const prof_t prof_t0 = prof_begin(a.prof);
    const int i = blockIdx.x, slot = a.slot0 + i, tid = threadIdx.x;
    const SmpRow row(a.logits + (long)i * a.vocab, a.vocab);
    uint16_t *out = a.out + (long)i * a.vocab;
    const bool out_aligned = ((uintptr_t)out & 15) == 0;
    const float T = a.temperature[slot], min_p = a.min_p[slot], typical_p = a.typical_p[slot], mu = a.mu[slot];
    const bool mir = mu == mu;
    const bool use_minp = !mir && min_p > 0.f, use_typ = !mir && typical_p > 0.f && typical_p < 1.f;
    // keep(bits) over every element: kept tokens keep their bits, the others become -inf; returns through `wsum` the kept weight
    auto write = [&](auto keep) {
        for (int j = 0; j < row.chunks; ++j) {
            const u32x4 r = row.chunk(j);
            uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t b = smp_bits(r, e);
                o[e >> 1] |= (keep(j, e, b) ? b : 0xff80u) << ((e & 1) * 16);
            }
            const int c = j * 8192 + tid * 8;
            if (out_aligned && c + 8 <= a.vocab) {
                act_store16(out + c, u32x4{o[0], o[1], o[2], o[3]});
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (c + e < a.vocab) act_store(out + c + e, (uint16_t)((o[e >> 1] >> ((e & 1) * 16)) & 0xffffu));
            }
        }
    };
    float logsum = __builtin_nanf("");
    bool copy = !(T > 0.f) || !(mir || use_minp || use_typ);  // uniform
    float m = -INFINITY;
    if (!copy) {
        float t = -INFINITY;
        smp_for_each(row, [&](int, int, uint32_t b) { t = fmaxf(t, __uint_as_float(b << 16)); });  // fmaxf drops NaN
        m = smp_block_max(t, sm);
        copy = !(m > -INFINITY) || m == INFINITY;
    }
    if (copy) {
        write([](int, int, uint32_t) { return true; });
    } else if (mir) {
        float z = 0.f;
        smp_for_each(row, [&](int, int, uint32_t b) {
            if (!smp_nan(b)) z += exp2_hw(trn_t(__uint_as_float(b << 16), m, T) * TRN_LOG2E);
        });
        z = smp_block_sum(z, sm);
        const float thr = (__log2f(z) - mu) / TRN_LOG2E;  // i stays iff t_i >= thr (natural units, like min-p)
        float kept = 0.f;
        if (thr > 0.f || !(thr == thr)) {  // nothing would stay: the first maximum does
            float first = -1.0e9f;
            smp_for_each(row, [&](int j, int e, uint32_t b) {
                if (__uint_as_float(b << 16) == m) first = fmaxf(first, -(float)(j * 8192 + tid * 8 + e));
            });
            const int g = (int)-smp_block_max(first, sm);
            write([&](int j, int e, uint32_t) { return j * 8192 + tid * 8 + e == g; });
            kept = 1.f;
        } else {
            float ws = 0.f;
            write([&](int, int, uint32_t b) {
                if (smp_nan(b)) return false;
                const float t = trn_t(__uint_as_float(b << 16), m, T);
                if (!(t >= thr)) return false;
                ws += exp2_hw(t * TRN_LOG2E);
                return true;
            });
            kept = smp_block_sum(ws, sm);
        }
        logsum = m / T + __logf(kept);
    } else {
        const float lnmp = use_minp ? logf(min_p) : -INFINITY;
        auto keep1 = [&](uint32_t b) { return trn_t(__uint_as_float(b << 16), m, T) >= lnmp; };
        float dstar = INFINITY, tbar = 0.f;
        if (use_typ) {
            float z = 0.f, zt = 0.f;
            smp_for_each(row, [&](int, int, uint32_t b) {
                if (smp_nan(b)) return;
                const float t = trn_t(__uint_as_float(b << 16), m, T);
                if (!(t >= lnmp) || !(t > -INFINITY)) return;
                const float w = exp2_hw(t * TRN_LOG2E);
                z += w;
                zt += w * t;
            });
            z = smp_block_sum(z, sm);
            zt = smp_block_sum(zt, sm);
            tbar = zt / z;
            dstar = trn_typical_boundary(row, keep1, m, T, tbar, 1.f / z, typical_p, ts);
        }
        write([&](int, int, uint32_t b) {
            if (smp_nan(b) || !keep1(b)) return false;
            return !use_typ || fabsf(trn_t(__uint_as_float(b << 16), m, T) - tbar) <= dstar;
        });
    }
    if (a.kept_logsum && tid == 0) act_store(a.kept_logsum + i, logsum);
    prof_end(a.prof, prof_t0);
}

// The Mirostat update, behind the choice: for the row's token t, s = -log2(p_t / sum_kept p) = (L - x_t / T) log2 e and
// mu <- mu - eta (s - tau), in fp32.  One wave per row; a row without Mirostat (tau == 0), a greedy row, a row whose slot does not run and
// a surprise that is not finite leave mu as it is.
struct MirostatUpdateArgs {
    const uint16_t *filtered;   // [rows, vocab]
    int vocab, slot0;
    const int32_t *tokens;      // [slots] the token just produced
    const float *temperature;   // [slots]
    const float *kept_logsum;   // [rows]
    const float *tau, *eta;     // [slots]
    float *mu;                  // [slots]
    const int32_t *live;        // [slots] or nullptr: every row runs
    prof_t *prof;
};

static __global__ __launch_bounds__(64) void mirostat_update_kernel(const MirostatUpdateArgs a) {
    const prof_t prof_t0 = prof_begin(a.prof);
    const int i = blockIdx.x, slot = a.slot0 + i;
    if (threadIdx.x == 0) {
        const float tau = a.tau[slot], T = a.temperature[slot];
        if (tau > 0.f && T > 0.f && (!a.live || a.live[slot])) {
            const int t = a.tokens[slot];
            if (t >= 0 && t < a.vocab) {
                const float x = BF16::to_float(act_load(a.filtered + (long)i * a.vocab + t));
                const float s = (act_load(a.kept_logsum + i) - x / T) * TRN_LOG2E;
                const float mu = a.mu[slot];
                if (fabsf(s) < INFINITY && mu == mu) a.mu[slot] = mu - a.eta[slot] * (s - tau);
            }
        }
    }
    prof_end(a.prof, prof_t0);
}

}  // namespace tl
