// Batched speculative sampling (include/tinyllm_engine.h "tl_engine_verify_batch_sampled"): the acceptance stage of
// a batched verification pass for slots that sample.  Row r of the pass belongs to sequence i = the one whose rows [seq_row0[i],
// seq_row0[i] + seq_len[i]) hold it, j = r - seq_row0[i]:
//   proposal   x = tokens[r + 1] for j < seq_len[i] - 1, -1 (a bonus row) on the sequence's last row
//   position   seq_ctx[i] - seq_len[i] + j + 1: the context length before the call + j + 1, the sampler's own position rule
//   target     (temperature, top_k, top_p, seed)[seq_index[i]] (seq_index NULL: i), read here: no record is uploaded per call
// Kept set, weights, one-hot rows and uniforms are spec_sample.h's.  Two proposal kinds:
//   drafted    row r of `draft` is the row x was drawn from under the call's one (d_temperature, d_top_k, d_top_p): ssp_row as it stands
//   point      draft == NULL: the proposal is a deterministic function of the sequence (prompt lookup), its distribution one-hot at x.
//              accept iff u_acc Wp < wp_x (one fp32 product); rejected: r_j = wp_j for j != x, r_x = 0, alt = the first id whose
//              inclusive cumulative r exceeds u_res R, with ssp_row's fallbacks; x >= V is rejected without a read at x and the
//              residual is wp whole.  This is what ssp_row gives for a draft row whose first maximum is x under draft temperature 0
//              (wq = Wq = 1), bit for bit -- without a draft row: the target row alone is streamed, the way sample.h streams it.
// One workgroup of 1,024 threads per row; one thread per sequence composes the result.  Plain stores, no atomics outside sample.h's LDS
// histogram of integer counts: the same inputs give the same outputs on every run.
#pragma once
#include "spec_sample.h"
#include "verify_attn_host.h"

namespace tl {

// One row against a one-hot draft at x: accept (0 / 1) and alt (-1 when accepted), the same values in every thread.
__device__ __forceinline__ void vsp_point_row(const SmpRow &p, int x, float t_temp, int t_top_k, float t_top_p, uint64_t seed, uint32_t position,
                                              SampleSmem &sm, int *accept, int *alt) {
    *accept = 0;
    if (x < 0) {  // a bonus row: the sampler's own draw
        *alt = smp_select(p, __builtin_nanf(""), t_temp, t_top_k, t_top_p, seed, position, sm);
        return;
    }
    const SspKept kp = ssp_kept(p, t_temp, t_top_k, t_top_p, sm);
    if (kp.onehot >= 0) {  // greedy verification
        *accept = x == kp.onehot;
        *alt = *accept ? -1 : kp.onehot;
        return;
    }
    const int t0 = (int)threadIdx.x * 8;
    float sp = 0.f;
    smp_for_each(p, [&](int j, int e, uint32_t b) { sp += ssp_weight(kp, j * 8192 + t0 + e, b); });
    const float Wp = smp_block_sum(sp, sm);
    if (x < p.vocab) {
        const float wpx = ssp_weight(kp, x, act_load(p.lg + x));
        if (ssp_uniform(seed, position, SSP_ACCEPT_TAG) * Wp < wpx) {
            *accept = 1;
            *alt = -1;
            return;
        }
    }
    const float u = ssp_uniform(seed, position, SSP_RESIDUAL_TAG);
    auto residual = [&](int j, int e, uint32_t b) {
        const int t = j * 8192 + t0 + e;
        return t == x ? 0.f : ssp_weight(kp, t, b);
    };
    int tok = smp_find(p, residual, u, 0.f, sm);
    if (tok < 0) {  // no chunk crossed: sm.col still holds the chunks' totals
        float total = 0.f;
        for (int j = 0; j < p.chunks; ++j) total += sm.col[j];
        const bool none = !(total > 0.f);
        __syncthreads();  // (read before the next search writes them)
        float last = -1.f;
        if (none) {  // R == 0: the plain draw from wp
            auto weight = [&](int j, int e, uint32_t b) { return ssp_weight(kp, j * 8192 + t0 + e, b); };
            tok = smp_find(p, weight, u, 0.f, sm);
            if (tok < 0) {
                smp_for_each(p, [&](int j, int e, uint32_t b) {
                    if (weight(j, e, b) > 0.f) last = (float)(j * 8192 + t0 + e);
                });
                tok = (int)fmaxf(smp_block_max(last, sm), 0.f);
            }
        } else {  // u R rounded to R: the last id with a positive residual
            smp_for_each(p, [&](int j, int e, uint32_t b) {
                if (residual(j, e, b) > 0.f) last = (float)(j * 8192 + t0 + e);
            });
            tok = (int)fmaxf(smp_block_max(last, sm), 0.f);
        }
    }
    *alt = tok;
}

// where a launch finds its sequences: the descriptors of the engine's pass on the device ...
struct VerifySeqsDev {
    const int32_t *row0_, *len_, *ctx_, *index_;
    __device__ __forceinline__ int row0(int i) const { return row0_[i]; }
    __device__ __forceinline__ int len(int i) const { return min(max(len_[i], 1), VA_MAX_LEN); }
    __device__ __forceinline__ int ctx(int i) const { return ctx_[i]; }
    __device__ __forceinline__ int index(int i) const { return index_ ? index_[i] : i; }
};
// ... or, for the routine over caller rows, the kernel arguments themselves (VerifySeqsInline, verify_attn_host.h): no upload, no allocation
struct VerifySeqsArg {
    const VerifySeqsInline &d;
    __device__ __forceinline__ int row0(int i) const { return d.row0[i]; }
    __device__ __forceinline__ int len(int i) const { return min(max((int)d.len[i], 1), VA_MAX_LEN); }
    __device__ __forceinline__ int ctx(int i) const { return d.ctx[i]; }
    __device__ __forceinline__ int index(int i) const { return i; }
};

// One row of the pass.  A row no sequence owns is written as "not accepted, no alt" and reads nothing else.
template <class Seqs>
__device__ __forceinline__ void verify_sample_row(const VerifySampleArgs &a, const Seqs &q, SpecSmem &ss) {
    const int r = blockIdx.x;
    int seq = -1, j = 0, len = 0;
    for (int i = 0; i < a.n_seqs; ++i) {
        const int r0 = q.row0(i), n = q.len(i);
        if (seq < 0 && r >= r0 && r < r0 + n) seq = i, j = r - r0, len = n;
    }
    int accept = 0, alt = -1;
    if (seq >= 0) {  // (uniform)
        const int x = j < len - 1 ? a.tokens[r + 1] : -1;
        const uint32_t position = (uint32_t)(q.ctx(seq) - len + j + 1);
        const int s = q.index(seq);
        const float t_temp = a.temperature[s], t_top_p = a.top_p[s];
        const int t_top_k = a.top_k[s];
        const uint64_t seed = a.seed[s];
        const SmpRow p(a.target + (long)r * a.vocab, a.vocab);
        if (a.draft) {
            const SmpRow d(a.draft + (long)r * a.vocab, a.vocab);
            ssp_row(p, d, x, t_temp, t_top_k, t_top_p, a.d_temperature, a.d_top_k, a.d_top_p, seed, position, ss, &accept, &alt);
        } else {
            vsp_point_row(p, x, t_temp, t_top_k, t_top_p, seed, position, ss.s, &accept, &alt);
        }
    }
    if (threadIdx.x == 0) {
        a.accept[r] = accept;
        a.alt[r] = alt;
    }
}

// grid = rows, block = 1024
static __global__ __launch_bounds__(1024) void verify_sample_kernel(const VerifySampleArgs a) {
    __shared__ SpecSmem ss;
    verify_sample_row(a, VerifySeqsDev{a.seq_row0, a.seq_len, a.seq_ctx, a.seq_index}, ss);
}
static __global__ __launch_bounds__(1024) void verify_sample_rows_kernel(const VerifySampleArgs a, const VerifySeqsInline d) {
    __shared__ SpecSmem ss;
    verify_sample_row(a, VerifySeqsArg{d}, ss);
}

// One thread per sequence: a = the first row j < len - 1 that rejects its proposal (len - 1 when none does); count = a + 1, ids[0 .. a)
// the accepted proposals tokens[row0 + 1 .. row0 + a], ids[a] row a's alt (the residual draw, or the bonus row's ordinary draw), the
// rest -1.  Rows behind the first rejection are never looked at.
//   grid = ceil(n_seqs / 64), block = 64
__device__ __forceinline__ void verify_sample_scan(const int32_t *__restrict__ accept, const int32_t *__restrict__ alt,
                                                   const int32_t *__restrict__ tokens, int b, int row0, int len, tl_verify_result *__restrict__ out) {
    int a = len - 1;
    for (int j = len - 2; j >= 0; --j)
        if (!accept[row0 + j]) a = j;
    tl_verify_result r;
    r.count = a + 1;
#pragma unroll
    for (int j = 0; j < VA_MAX_LEN; ++j) {
        int id = -1;
        if (j < a) id = tokens[row0 + j + 1];
        else if (j == a) id = alt[row0 + a];
        r.ids[j] = id;
    }
    out[b] = r;
}
static __global__ __launch_bounds__(64) void verify_sample_scan_kernel(const int32_t *__restrict__ accept, const int32_t *__restrict__ alt,
                                                                       const int32_t *__restrict__ tokens, const int32_t *__restrict__ seq_row0,
                                                                       const int32_t *__restrict__ seq_len, int n_seqs,
                                                                       tl_verify_result *__restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < n_seqs) verify_sample_scan(accept, alt, tokens, b, seq_row0[b], min(max(seq_len[b], 1), VA_MAX_LEN), out);
}
static __global__ __launch_bounds__(64) void verify_sample_rows_scan_kernel(const int32_t *__restrict__ accept, const int32_t *__restrict__ alt,
                                                                            const int32_t *__restrict__ tokens, const VerifySeqsInline d, int n_seqs,
                                                                            tl_verify_result *__restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < n_seqs) verify_sample_scan(accept, alt, tokens, b, d.row0[b], min(max((int)d.len[b], 1), VA_MAX_LEN), out);
}

}  // namespace tl
