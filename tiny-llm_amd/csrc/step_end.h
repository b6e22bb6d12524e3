// The end of a decode step (and of a prefill's last row): choose the token of every logits row, record it, advance the slot, and leave
// the next step's input -- the RoPE factors of the next position, the token's dequantised embedding row and its sum of squares.
// Three kernels differ in how the token is chosen and share what stands behind the choice (the logprob twin spells its commit out: it
// also needs `produced`, see step_commit):
//   step_end_kernel           greedy (first maximum wins)
//   sample_step_end_kernel    per-slot sampling (sample.h); a slot with temperature 0 takes the greedy id
//   logprob_step_end_kernel   the sampling twin's choice, then the log-probability record of the produced token (logprob.h)
// grid = rows; block = 1024.  Block i reads logits row i and serves slot slot0 + i.  Each takes one struct by value, like every kernel
// of a decode step: csrc/aql.cpp copies a captured node's argument block as it is.
//   reference: mx.argmax(logits[:, -1]) (benches/bench.py:234-243) + QuantizedEmbedding (embedding.py:38-54).
#pragma once
#include "sample.h"
#include "logprob.h"

namespace tl {

struct StepEndArgs {
    const uint16_t *logits;  // [rows, vocab]
    int vocab;
    int slot0;
    int32_t *tokens;        // [max_batch] pending input token per slot
    int32_t *context_lens;  // [max_batch]
    const int32_t *live;    // [max_batch] 1 = slot holds a sequence
    int32_t *produced;      // [max_batch] number of ids recorded so far
    int32_t *ring;          // [max_batch, ring_cap]
    int ring_cap;
    int advance;  // 1: context_lens[slot] += 1 (decode); 0: prefill sets it on the host side
    // next-step embedding
    const uint32_t *emb_w;
    const uint16_t *emb_s, *emb_b;
    uint16_t *x;  // [max_batch, hidden], row = slot
    int hidden;
    // RoPE factors of the slot's next position (read by the next step's attention kernels)
    const float2 *rope_table;
    float2 *rope_cur;
    int rope_positions, rope_half;
    // optional: [max_batch][8] partial sums of squares of the embedded row (entry 0; the rest zero) for the fused RMSNorm of
    // the next step's skinny QKV matmul (qmm3.h)
    float *ss_out;
    prof_t *prof;
    // optional: per 16-logit tile (largest bf16 logit, lowest index holding it), left by the lm_head GEMV's epilogue (qmv3.h tile_max):
    // [rows][tiles] pairs; the greedy id is then picked from `tiles` pairs and the logits row is not read again
    const f32x2 *tile_max;
    int tiles;
};

// ---- what the three kernels share ----------------------------------------------------------------------------------------------------
// The helpers take StepEndArgs BY VALUE: a reference to the kernel's argument block escapes into the call until it is inlined, and what
// the optimiser makes of the block afterwards differs enough to tip the logprob twin -- which holds all 56 argument dwords in SGPRs at
// 104 of 104 -- from nine SGPR spills into VGPR lanes to a 32-byte spill slot in scratch.  (Check -Rpass-analysis=kernel-resource-usage
// after any change here: tests/test_kernel_resources_cpu.py refuses scratch.)
//
// Thread 0's commit of the chosen token: the pending token, the ring entry, `produced` and the context advance of a live slot.  It hands
// back the slot's context after the step.  Called by the greedy kernel and the sampling twin; the logprob twin repeats these lines.
static __device__ __forceinline__ int step_commit(const StepEndArgs p, int slot, int live, int token) {
    int ctx_now = p.context_lens[slot];
    if (live) {
        p.tokens[slot] = token;
        const int n = p.produced[slot];
        p.ring[(long)slot * p.ring_cap + (n % p.ring_cap)] = token;
        p.produced[slot] = n + 1;
        if (p.advance) p.context_lens[slot] = ++ctx_now;
    }
    return ctx_now;
}

// The next step's input, by the whole block behind the barrier that publishes thread 0's commit: the RoPE factors of the slot's NEXT
// position (`ctx`), the embedding row of `token` dequantised into x[slot], and its sum of squares into ss_out.  s_val: 16 floats of
// shared memory that nobody reads any more.
static __device__ __forceinline__ void step_next_input(const StepEndArgs p, int slot, int token, int ctx, float *s_val) {
    if ((int)threadIdx.x < p.rope_half) {
        const int pos = min(ctx, p.rope_positions - 1);
        p.rope_cur[(long)slot * p.rope_half + threadIdx.x] = p.rope_table[(long)pos * p.rope_half + threadIdx.x];
    }
    const int words = p.hidden / 8;
    const int groups = p.hidden / 128;
    float sumsq = 0.f;
    for (int w = threadIdx.x; w < words; w += 1024) {
        const uint32_t packed = p.emb_w[(long)token * words + w];
        const float scale = BF16::to_float(p.emb_s[(long)token * groups + w / 16]);
        const float bias = BF16::to_float(p.emb_b[(long)token * groups + w / 16]);
        uint16_t o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            o[e] = BF16::from_float((float)((packed >> (4 * e)) & 0xfu) * scale + bias);
            const float v = BF16::to_float(o[e]);
            sumsq += v * v;
        }
        *reinterpret_cast<uint4 *>(p.x + (long)slot * p.hidden + w * 8) = *reinterpret_cast<const uint4 *>(o);
    }
    if (p.ss_out) {  // uniform
        const float ws = wave_sum(sumsq);
        if ((threadIdx.x & 63) == 0) s_val[threadIdx.x >> 6] = ws;
        __syncthreads();
        if (threadIdx.x == 0) {
            float tot = 0.f;
            for (int w = 0; w < 16; ++w) tot += s_val[w];
            p.ss_out[(long)slot * 8] = tot;
            for (int i = 1; i < 8; ++i) p.ss_out[(long)slot * 8 + i] = 0.f;
        }
    }
}

// The maximum of row i from the lm_head GEMV's per-tile pairs (uniform), for the two twins' selection; NaN where the step has none
static __device__ __forceinline__ float step_tile_row_max(const StepEndArgs p, int i, SampleSmem &sm) {
    if (!p.tile_max) return __builtin_nanf("");
    const f32x2 *tm = p.tile_max + (long)i * p.tiles;
    float t = -INFINITY;
    for (int k = threadIdx.x; k < p.tiles; k += 1024) t = fmaxf(t, act_load(tm + k)[0]);
    return smp_block_max(t, sm);
}

// ---- greedy: argmax over bf16 logits (first maximum wins, like argmax) ------------------------------------------------------------------
static __global__ __launch_bounds__(1024) void step_end_kernel(const StepEndArgs p) {
    __shared__ float s_val[16];
    __shared__ int s_idx[16];
    __shared__ int s_token, s_ctx;
    const prof_t prof_t0 = prof_begin(p.prof);
    const int i = blockIdx.x;
    const int slot = p.slot0 + i;
    const uint16_t *lg = p.logits + (long)i * p.vocab;
    float best = -INFINITY;
    int best_i = 0x7fffffff;
    int vec_end = ((uintptr_t)lg % 16 == 0) ? (p.vocab & ~7) : 0;
    int scalar_from = vec_end;
    if (p.tile_max) {  // uniform: 9,496 pairs instead of 151,936 logits; same rule (strictly greater wins, the lower index on a tie)
        const f32x2 *tm = p.tile_max + (long)i * p.tiles;
        constexpr int TM_NB = 10;
        for (int t0 = threadIdx.x; t0 < p.tiles; t0 += 1024 * TM_NB) {
            f32x2 pr[TM_NB];
#pragma unroll
            for (int j = 0; j < TM_NB; ++j) pr[j] = act_load(tm + min(t0 + j * 1024, p.tiles - 1));  // (the lm_head launch of this step wrote them)
#pragma unroll
            for (int j = 0; j < TM_NB; ++j) {
                if (t0 + j * 1024 >= p.tiles) continue;
                const float v = pr[j][0];
                const int idx = pr[j][1] < 1.0e30f ? (int)pr[j][1] : 0x7fffffff;
                if (v > best || (v == best && idx < best_i)) {
                    best = v;
                    best_i = idx;
                }
            }
        }
        vec_end = 0;
        scalar_from = p.vocab;  // nothing of the row itself is read
    }
    // ONE workgroup reads the whole row (304 KB at Qwen3's vocabulary): a plain loop is a chain of 19 dependent L2 round trips
    // (12 us in the step profile).  The loads go out ten 16-byte chunks at a time, from clamped addresses, and are looked at after:
    // two round trips.
    constexpr int SE_NB = 10;
    for (int c0 = threadIdx.x * 8; c0 < vec_end; c0 += 1024 * 8 * SE_NB) {
        u32x4 rawv[SE_NB];
#pragma unroll
        for (int j = 0; j < SE_NB; ++j) rawv[j] = act_load(reinterpret_cast<const u32x4 *>(lg + min(c0 + j * 8192, vec_end - 8)));
#pragma unroll
        for (int j = 0; j < SE_NB; ++j) {
            const int c = c0 + j * 8192;
            if (c >= vec_end) continue;
            uint16_t raw[8];
            *reinterpret_cast<u32x4 *>(raw) = rawv[j];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = BF16::to_float(raw[e]);
                if (v > best) {  // strictly greater: the earliest index of a tie stays
                    best = v;
                    best_i = c + e;
                }
            }
        }
    }
    for (int c = scalar_from + threadIdx.x; c < p.vocab; c += 1024) {
        const float v = BF16::to_float(act_load(lg + c));
        if (v > best || (v == best && c < best_i)) {
            best = v;
            best_i = c;
        }
    }
    {   // wave-wide (maximum, lowest index that holds it) by DPP rotations instead of twelve ds_bpermute round trips: indices are
        // below 2^24, exact as floats, so the lowest index is -max(-index) over the lanes that hold the maximum
        const float m = wave_max(best);
        const float cand = (best == m && best_i != 0x7fffffff) ? (float)best_i : 3.0e38f;
        const float lowest = -wave_max(-cand);
        best = m;
        best_i = lowest < 1.0e30f ? (int)lowest : 0x7fffffff;
    }
    if ((threadIdx.x & 63) == 0) {
        s_val[threadIdx.x >> 6] = best;
        s_idx[threadIdx.x >> 6] = best_i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float bv = s_val[0];
        int bi = s_idx[0];
        for (int w = 1; w < 16; ++w) {
            if (s_val[w] > bv || (s_val[w] == bv && s_idx[w] < bi)) {
                bv = s_val[w];
                bi = s_idx[w];
            }
        }
        if (bi < 0 || bi >= p.vocab) bi = 0;  // all-NaN / -inf row
        s_token = bi;
        s_ctx = step_commit(p, slot, p.live[slot], bi);
    }
    __syncthreads();
    step_next_input(p, slot, s_token, s_ctx, s_val);  // (s_val is free again: its last readers ran before the barrier above)
    prof_end(p.prof, prof_t0);
}

// ---- the sampling twin -------------------------------------------------------------------------------------------------------------------
// The token of every row is chosen by smp_select under its slot's parameters; it writes what step_end_kernel writes, nothing else.
struct SampleStepEndArgs {
    StepEndArgs s;
    const float *temperature;  // [max_batch]
    const int32_t *top_k;
    const float *top_p;
    const uint64_t *seed;
};

static __global__ __launch_bounds__(1024) void sample_step_end_kernel(const SampleStepEndArgs q) {
    const StepEndArgs &p = q.s;
    __shared__ SampleSmem sm;
    __shared__ float s_val[16];
    __shared__ int s_token, s_ctx;
    const prof_t prof_t0 = prof_begin(p.prof);
    const int i = blockIdx.x;
    const int slot = p.slot0 + i;
    const SmpRow row(p.logits + (long)i * p.vocab, p.vocab);
    const float temperature = q.temperature[slot], top_p = q.top_p[slot];
    const int top_k = q.top_k[slot];
    const uint64_t seed = q.seed[slot];
    const int live = p.live[slot];
    // the sampled token's position: tokens before it (decode: the context after this step's advance; prefill: the prompt length)
    const uint32_t position = (uint32_t)(p.context_lens[slot] + (p.advance && live ? 1 : 0));
    const float m_given = step_tile_row_max(p, i, sm);
    const int bi = smp_select(row, m_given, temperature, top_k, top_p, seed, position, sm);
    __syncthreads();  // every thread has read context_lens[slot] above
    if (threadIdx.x == 0) {
        s_token = bi;
        s_ctx = step_commit(p, slot, live, bi);
    }
    __syncthreads();
    step_next_input(p, slot, s_token, s_ctx, s_val);
    prof_end(p.prof, prof_t0);
}

// ---- the logprob twin (logprob.h, tl_engine_set_logprobs) ------------------------------------------------------------------------------------
// It chooses the token as the sampling twin does, and then writes the record of the produced token -- in the same launch, because the
// token a later launch of the step would read is a plain store of this one (no cache maintenance between the launches of a step on the
// AQL route).
struct LogprobStepEndArgs {
    SampleStepEndArgs q;
    const int32_t *top_n;  // [max_batch] -1: the slot records nothing
    uint32_t *ring;        // [max_batch, ring_cap] records of LP_RECORD_WORDS words
    uint32_t *pending;     // [max_batch] the record of each slot's pending token
    const uint16_t *choice;  // [rows, vocab] the processed rows the token is chosen from (logit_process.h); nullptr: q.s.logits themselves
};

static __global__ __launch_bounds__(1024) void logprob_step_end_kernel(const LogprobStepEndArgs lq) {
    const SampleStepEndArgs &q = lq.q;
    const StepEndArgs &p = q.s;
    __shared__ SampleSmem sm;
    __shared__ LogprobSmem ls;
    __shared__ float s_val[16];
    __shared__ int s_token, s_ctx, s_n;
    const prof_t prof_t0 = prof_begin(p.prof);
    const int i = blockIdx.x;
    const int slot = p.slot0 + i;
    const SmpRow row(p.logits + (long)i * p.vocab, p.vocab);
    // the record describes the raw row; with processed rows (uniform) the token is chosen from those
    const bool split = lq.choice != nullptr;
    const SmpRow crow(split ? lq.choice + (long)i * p.vocab : row.lg, p.vocab);
    const float temperature = q.temperature[slot], top_p = q.top_p[slot];
    const int top_k = q.top_k[slot];
    const uint64_t seed = q.seed[slot];
    const int live = p.live[slot];
    // the sampled token's position: tokens before it (decode: the context after this step's advance; prefill: the prompt length)
    const uint32_t position = (uint32_t)(p.context_lens[slot] + (p.advance && live ? 1 : 0));
    float m_given = step_tile_row_max(p, i, sm);
    const int top_n = lq.top_n[slot];
    const bool record = live && top_n >= 0;  // uniform
    if (m_given != m_given && (record || !split)) {  // the raw row's maximum, once for both routines
        float t = -INFINITY;
        smp_for_each(row, [&](int, int, uint32_t b) { t = fmaxf(t, __uint_as_float(b << 16)); });  // fmaxf drops NaN
        m_given = smp_block_max(t, sm);
    }
    // a greedy slot that records takes the routine's own first maximum (smp_select's greedy id): one pass instead of two -- unless the
    // choice is made on another row than the record's
    const bool lp_first = record && temperature == 0.f && !split;
    float lse = 0.f;
    if (lp_first) lse = lp_row(row, m_given, top_n, sm, ls);
    const int bi = lp_first ? ls.greedy : smp_select(crow, split ? __builtin_nanf("") : m_given, temperature, top_k, top_p, seed, position, sm);
    __syncthreads();  // every thread has read context_lens[slot] above
    if (threadIdx.x == 0) {
        s_token = bi;
        // step_commit, spelled out: this kernel also wants `n`, and every form of the helper that hands it back (a struct, a reference,
        // scalar parameters) left the kernel with 36 bytes of scratch (see above)
        int ctx_now = p.context_lens[slot];
        if (live) {
            p.tokens[slot] = bi;
            const int n = p.produced[slot];
            p.ring[(long)slot * p.ring_cap + (n % p.ring_cap)] = bi;
            p.produced[slot] = n + 1;
            if (p.advance) p.context_lens[slot] = ++ctx_now;
            s_n = n;
        }
        s_ctx = ctx_now;
    }
    __syncthreads();
    const int token = s_token;
    step_next_input(p, slot, token, s_ctx, s_val);
    if (record) {
        if (!lp_first) lse = lp_row(row, m_given, top_n, sm, ls);
        if (threadIdx.x == 0) ls.rec[0] = __float_as_uint(BF16::to_float(act_load(row.lg + token)) - lse);
        __syncthreads();
        if ((int)threadIdx.x < LP_RECORD_WORDS) {
            const uint32_t v = ls.rec[threadIdx.x];
            lq.ring[((long)slot * p.ring_cap + (s_n % p.ring_cap)) * LP_RECORD_WORDS + threadIdx.x] = v;
            lq.pending[(long)slot * LP_RECORD_WORDS + threadIdx.x] = v;
        }
    }
    prof_end(p.prof, prof_t0);
}

}  // namespace tl
