// Log-probabilities of a bf16 logits row (include/tinyllm_engine.h "log-probabilities"), on the device sampler's
// pieces (sample.h): the row maximum, the order-preserving keys, the exact top-k boundary in LDS windows and fixed-order block sums.
//
// Semantics, per row of V logits l with m their maximum over non-NaN entries:
//   lse      m + log(sum_j exp(l_j - m)) in fp32 over non-NaN entries; logprob(t) = l_t - lse (the model's temperature-1 distribution)
//   top-N    the first N tokens of the sampler's order (logit descending, equal logits by the lower id, NaN never ranked): the kept
//            set of top_k = N, listed in that order; entries past N or past the rankable tokens are id -1, logprob -inf
//   edges    a NaN logit has logprob NaN; a row without a finite maximum (all NaN / -inf, or holding +inf) has NaN everywhere
// One workgroup of 1,024 threads per row.  Passes over the row: the sum (top-N 0), or the boundary window, the cut inside the boundary
// key and the sum with the candidates' compaction (top-N > 0); the candidates (at most N) are ranked in LDS.  The result depends on
// the row alone: every sum runs in a fixed order whatever the batch, the launch or the route.
#pragma once
#include "sample.h"

namespace tl {

constexpr int LP_MAX_TOP = 20;                       // TL_MAX_TOP_LOGPROBS
constexpr int LP_RECORD_WORDS = 1 + 2 * LP_MAX_TOP;  // tl_token_logprob: logprob, top_ids[20], top_logprobs[20] (164 bytes)

struct LogprobSmem {
    int n;  // candidates of the top-N set found so far
    int key[LP_MAX_TOP], id[LP_MAX_TOP];
    uint32_t rec[LP_RECORD_WORDS];  // the row's record; rec[0] is left to the caller
    int greedy;
};

// The log-normaliser of one row (NaN without a finite maximum; the same value in every thread), the greedy id in ls.greedy (the first
// maximum, exactly step_end_kernel's: 0 for a row of NaN / -inf), and ls.rec[1, 41) = the top-N entries.  m_given: the row maximum
// when the caller has it (the lm_head GEMV's tile maxima), NaN to reduce it here.
__device__ __forceinline__ float lp_row(const SmpRow &row, float m_given, int top_n, SampleSmem &sm, LogprobSmem &ls) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float m = m_given;
    if (m != m) {
        float t = -INFINITY;
        smp_for_each(row, [&](int, int, uint32_t b) { t = fmaxf(t, __uint_as_float(b << 16)); });  // fmaxf drops NaN
        m = smp_block_max(t, sm);
    }
    const bool finite = m > -INFINITY && m < INFINITY;
    int bkey = -1, keep_r = 0x7fffffff, cut = 0x7fffffff;
    if (top_n > 0) {  // the kept set of top_k = top_n (sample.h), then the cut inside its boundary key
        const int kmax = smp_key(__float_as_uint(m) >> 16), K = top_n;
        const bool use_p = false;
        const float top_p = 0.f, inv_z = 0.f;
        SMP_BOUNDARY_SEARCH();
        if (bkey >= 0) {
            const int bk = bkey;
            cut = smp_find(row, [&](int, int, uint32_t b) { return !smp_nan(b) && smp_key(b) == bk ? 1.f : 0.f; }, 0.f, (float)(keep_r - 1), sm);
            if (cut < 0) cut = 0x7fffffff;
        }
    }
    if (tid == 0) ls.n = 0;
    __syncthreads();
    float z = 0.f, first = 3.0e38f;
    smp_for_each(row, [&](int j, int e, uint32_t b) {
        if (smp_nan(b)) return;
        const float v = __uint_as_float(b << 16);
        const int id = j * 8192 + tid * 8 + e;
        z += exp2_hw((v - m) * 1.44269504089f);
        if (v == m) first = fminf(first, (float)id);  // ids are exact in fp32
        if (top_n > 0) {
            const int k = smp_key(b);
            if (bkey < 0 || k > bkey || (k == bkey && id <= cut)) {
                const int s = atomicAdd(&ls.n, 1);
                if (s < LP_MAX_TOP) ls.key[s] = k, ls.id[s] = id;
            }
        }
    });
    const float zt = smp_block_sum(z, sm);  // (its barriers also publish ls.n / key / id)
    const float g = -smp_block_max(-first, sm);
    const float lse = finite ? m + logf(zt) : __builtin_nanf("");
    if (tid < LP_MAX_TOP) {
        const int n = min(ls.n, LP_MAX_TOP);
        if (tid < n) {  // rank among the candidates: logit descending, the lower id first
            const int k = ls.key[tid], id = ls.id[tid];
            int r = 0;
            for (int q = 0; q < n; ++q) r += (ls.key[q] > k || (ls.key[q] == k && ls.id[q] < id)) ? 1 : 0;
            ls.rec[1 + r] = (uint32_t)id;
            ls.rec[1 + LP_MAX_TOP + r] = __float_as_uint(smp_key_value(k) - lse);
        } else {
            ls.rec[1 + tid] = 0xffffffffu;  // id -1
            ls.rec[1 + LP_MAX_TOP + tid] = __float_as_uint(-INFINITY);
        }
    }
    if (tid == 0) ls.greedy = m > -INFINITY && g < 1.0e30f ? (int)g : 0;
    __syncthreads();
    return lse;
}

}  // namespace tl
