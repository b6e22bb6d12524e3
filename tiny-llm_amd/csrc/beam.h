// Beam-search candidate selection over bf16 logits rows (include/tinyllm_engine.h "beam search"), on the device
// sampler's pieces (sample.h) the way logprob.h is: the row maximum, the order-preserving keys, the exact top-k boundary in LDS windows
// and fixed-order block sums.
//
// Semantics, over `rows` logits rows l_p of V entries with one cumulative score s_p (fp32) per row:
//   per row    m the maximum over non-NaN entries; lse = m + log(sum_j exp(l_j - m)) in fp32 over non-NaN entries, logprob.h's
//              log-normaliser bit for bit; logprob(t) = l_t - lse.  NaN logits are never ranked.  A row without a finite maximum (all
//              NaN / -inf, or holding +inf) contributes no candidate, and neither does a row whose score is not finite (-inf: a dead beam)
//   candidate  (parent p, token t) with score s_p + logprob_p(t), one fp32 addition
//   order      score descending; equal scores by the lower parent, then by the row's own order, which is the sampler's (logit
//              descending, equal logits by the lower token id).  The score never decreases with the logit, so the order is total and
//              its first n lie among the rows' own first n
//   output     the first n_cand candidates of that order over all rows x V pairs, as tl_beam_candidate records; entries past the
//              rankable pairs are {-1, -1, -inf, -inf}
// Two launches.  beam_rows_kernel: one workgroup of 1,024 threads per row finds the row's first n_cand tokens -- lp_row's boundary
// window, cut inside the boundary key and sum with the candidates' compaction, with 32-entry arrays -- and writes them, ranked, to the
// row's 32 survivor records.  beam_merge_kernel: one workgroup ranks the at most 8 x 32 survivors in LDS by counting.  A survivor's
// place (32 parent + rank in its row) is the tie-break, so nothing depends on the order the compaction met the tokens in: every sum runs
// in a fixed order and the result is bit-identical from call to call.  No global atomics, no flags between workgroups: the launch
// boundary hands the survivors over.
#pragma once
#include "../../include/tinyllm_engine.h"
#include "sample.h"

namespace tl {

constexpr int BM_MAX_BEAMS = TL_MAX_BEAMS;                // rows of one call
constexpr int BM_MAX_CAND = TL_MAX_BEAM_CANDIDATES;       // candidates of one call, and survivor records per row
constexpr int BM_SURVIVORS = BM_MAX_BEAMS * BM_MAX_CAND;  // 256: one per thread of the merge

struct BeamSmem {
    int n;  // candidates of the row's first n_cand found so far
    int key[BM_MAX_CAND], id[BM_MAX_CAND];
};

struct BeamRowsArgs {
    const uint16_t *logits;  // [rows, vocab]
    const float *scores;     // [rows]
    int vocab, n_cand;
    tl_beam_candidate *survivors;  // [rows, BM_MAX_CAND]: the row's first n_cand in its own order, then empty records
};

__device__ __forceinline__ tl_beam_candidate beam_empty() { return tl_beam_candidate{-1, -1, -INFINITY, -INFINITY}; }

// grid = rows, block = 1024
static __global__ __launch_bounds__(1024) void beam_rows_kernel(const BeamRowsArgs a) {
    __shared__ SampleSmem sm;
    __shared__ BeamSmem bs;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    tl_beam_candidate *out = a.survivors + p * BM_MAX_CAND;
    const float s = a.scores[p];
    const SmpRow row(a.logits + (long)p * a.vocab, a.vocab);
    float m = -INFINITY;
    const bool alive = s > -INFINITY && s < INFINITY;  // (uniform)
    if (alive) {
        float t = -INFINITY;
        smp_for_each(row, [&](int, int, uint32_t b) { t = fmaxf(t, __uint_as_float(b << 16)); });  // fmaxf drops NaN
        m = smp_block_max(t, sm);
    }
    if (!(m > -INFINITY && m < INFINITY)) {  // a dead beam, or a row without a finite maximum (uniform)
        if (tid < BM_MAX_CAND) out[tid] = beam_empty();
        return;
    }
    // the kept set of top_k = n_cand (sample.h), then the cut inside its boundary key
    int bkey = -1, keep_r = 0x7fffffff, cut = 0x7fffffff;
    {
        const int kmax = smp_key(__float_as_uint(m) >> 16), K = a.n_cand;
        const bool use_p = false;
        const float top_p = 0.f, inv_z = 0.f;
        SMP_BOUNDARY_SEARCH();
        if (bkey >= 0) {
            const int bk = bkey;
            cut = smp_find(row, [&](int, int, uint32_t b) { return !smp_nan(b) && smp_key(b) == bk ? 1.f : 0.f; }, 0.f, (float)(keep_r - 1), sm);
            if (cut < 0) cut = 0x7fffffff;
        }
    }
    if (tid == 0) bs.n = 0;
    __syncthreads();
    float z = 0.f;
    smp_for_each(row, [&](int j, int e, uint32_t b) {
        if (smp_nan(b)) return;
        const float v = __uint_as_float(b << 16);
        const int id = j * 8192 + tid * 8 + e;
        z += exp2_hw((v - m) * 1.44269504089f);
        const int k = smp_key(b);
        if (bkey < 0 || k > bkey || (k == bkey && id <= cut)) {
            const int at = atomicAdd(&bs.n, 1);
            if (at < BM_MAX_CAND) bs.key[at] = k, bs.id[at] = id;
        }
    });
    const float zt = smp_block_sum(z, sm);  // (its barriers also publish bs.n / key / id)
    const float lse = m + logf(zt);
    if (tid < BM_MAX_CAND) {
        const int n = min(min(bs.n, BM_MAX_CAND), a.n_cand);
        tl_beam_candidate c = beam_empty();
        int r = tid;
        if (tid < min(bs.n, BM_MAX_CAND)) {  // rank among the candidates: logit descending, the lower id first
            const int k = bs.key[tid], id = bs.id[tid];
            r = 0;
            for (int q = 0; q < min(bs.n, BM_MAX_CAND); ++q) r += (bs.key[q] > k || (bs.key[q] == k && bs.id[q] < id)) ? 1 : 0;
            const float lp = smp_key_value(k) - lse;
            if (r < n) c = tl_beam_candidate{p, id, s + lp, lp};
        }
        // (ranks are a permutation of [0, found); the threads past them fill the rest of the 32 records)
        out[r] = c;
    }
}

// grid = 1, block = BM_SURVIVORS.  Thread i holds survivor i = 32 parent + rank; its place in the output is the number of survivors
// ahead of it: a higher score, or the same score and a lower i
static __global__ __launch_bounds__(BM_SURVIVORS) void beam_merge_kernel(const tl_beam_candidate *survivors, int rows, int n_cand,
                                                                         tl_beam_candidate *out) {
    __shared__ float score[BM_SURVIVORS];
    const int tid = threadIdx.x, n = rows * BM_MAX_CAND;
    tl_beam_candidate c = beam_empty();
    if (tid < n) c = survivors[tid];
    const bool ranked = c.parent >= 0;
    score[tid] = ranked ? c.score : __builtin_nanf("");  // (a survivor's score is never NaN: NaN marks the empty records)
    __syncthreads();
    int ahead = 0, total = 0;
    for (int j = 0; j < n; ++j) {
        const float sj = score[j];
        total += sj == sj ? 1 : 0;
        ahead += (sj > c.score || (sj == c.score && j < tid)) ? 1 : 0;
    }
    if (ranked && ahead < n_cand) out[ahead] = c;
    if (tid >= total && tid < n_cand) out[tid] = beam_empty();
}

// the two launches, stream ordered.  survivors_dev: BM_SURVIVORS records of scratch; the caller has checked the arguments
static inline int beam_rows_launch(const void *logits_dev, int rows, int vocab, const float *scores_dev, int n_cand,
                                   tl_beam_candidate *survivors_dev, tl_beam_candidate *out_dev, hipStream_t stream) {
    const BeamRowsArgs a{(const uint16_t *)logits_dev, scores_dev, vocab, n_cand, survivors_dev};
    hipLaunchKernelGGL(beam_rows_kernel, dim3(rows), dim3(1024), 0, stream, a);
    TL_CHECK_LAUNCH("beam_rows");
    hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(BM_SURVIVORS), 0, stream, survivors_dev, rows, n_cand, out_dev);
    TL_CHECK_LAUNCH("beam_rows merge");
    return TL_OK;
}

}  // namespace tl
