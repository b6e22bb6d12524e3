// Order-aware repetition control on the device (include/tinyllm_engine.h "DRY and the n-gram ban"): DRY ("don't
// repeat yourself") and no_repeat_ngram_size look at the ORDER of a slot's tokens, so each armed slot keeps its ordered id sequence
// resident on the device, and two launches between the processing launch (logit_process.h) and the truncation launch / step end rewrite
// the processed row.
//
// The contract.  At the moment a token is chosen the slot's recorded ids are S[s0 .. e]: s0 = the context length the slot had when it
// was armed (ids before s0 are unknown and never matched), S[e] = last = the token the step has just fed (the prompt's last token for
// the first token after a prefill).  M = DRY_MAX_MATCH = 64.
//   candidate      every i in [s0, e) with S[i] == last; its continuation is t = S[i + 1]
//   raw(i)         the largest m in [1, min(M, i - s0 + 1)] with S[i - j] == S[e - j] for all 0 <= j < m
//   n-gram ban     n = 0 (off) or 2 .. 64: every continuation with raw(i) >= n - 1 is banned (breakers and the range do not apply)
//   DRY            (multiplier >= 0, base >= 1, allowed_length >= 1, range >= 0, up to DRY_MAX_BREAKERS breaker ids); multiplier 0 = off
//     lo           range > 0 ? max(s0, e + 1 - range) : s0
//     B            the number of consecutive j >= 0 with e - j >= lo and S[e - j] no breaker, capped at M (a last token that is a
//                  breaker: B = 0, no DRY penalty on this choice)
//     d(i)         min(raw(i), B, i - lo + 1), for a candidate with i >= lo whose continuation is no breaker
//     L[t]         the largest d(i) over the candidates with continuation t; it counts where L[t] >= allowed_length
//   penalty        p = multiplier, then L[t] - allowed_length times p = p * base: fp32 products rounded one by one (no powf)
//   application    on the processed row: a banned token becomes bf16 -inf; a token with a DRY entry becomes bf16_rne(float(v) - p), -inf
//                  where p is not finite, and a NaN keeps its bits; every other token keeps its bits
//
// dry_record_kernel   a chunk's uploaded ids -> the slot's sequence row (beside logit_mark_prompt_kernel)
// dry_match_kernel    one workgroup per row: stores the fed token at S[e] (the only store to the sequence inside a step), stages the last
//                     M ids and the breakers in LDS, computes B, and walks the candidates -- the threads stride over the positions, each
//                     candidate compares backwards up to M ids -- leaving max(ban ? DRY_BAN : d) per continuation in the slot's table
//                     (one 32-bit word per token) by vector atomicMax on global memory: the result does not depend on the order in
//                     which threads run, and nothing caps the candidates or the distinct continuations
// dry_apply_kernel    the grid of logit_process_kernel (vocabulary chunks x rows, 16-byte loads): rewrites the processed row where the
//                     table has an entry and stores zero back over every entry it consumed -- the table is all zeros between steps, is
//                     never copied and has no stamps to wrap
// Rows of slots that are not armed (multiplier 0 and n 0: also how a parked slot's words stand) or not live leave after uniform loads.
#pragma once
#include "common.h"

namespace tl {

constexpr int DRY_MAX_MATCH = 64;     // TL_DRY_MAX_MATCH
constexpr int DRY_MAX_BREAKERS = 64;  // TL_MAX_DRY_BREAKERS
constexpr uint32_t DRY_BAN = 0x100u;  // a table entry above every match length
constexpr int DRY_MATCH_THREADS = 1024;
constexpr int DRY_APPLY_THREADS = 256;
constexpr int DRY_APPLY_CHUNK = DRY_APPLY_THREADS * 8;  // tokens per workgroup (LPR_CHUNK)

// (one struct by value, like every kernel of a decode step)
struct DryArgs {
    int32_t *seq;             // [slots, cap] the recorded ids; row i of the launch belongs to slot slot0 + i
    uint32_t *table;          // [slots, vocab] all zeros between steps
    uint16_t *rows;           // [rows, vocab] processed rows, rewritten in place
    int cap, vocab, slot0;
    int pos_bias;             // e = pos[slot] + pos_bias
    const int32_t *pos;       // [slots] a decode step: the context lengths (bias 0); a prefill's row: the same, bias -1; caller rows: `end`
    const int32_t *tokens;    // [slots] the fed tokens, stored at S[e] (a decode step); nullptr: S[e] is there already
    const int32_t *live;      // [slots] nullptr: every row runs
    const float *multiplier;  // [slots]
    const float *base;
    const int32_t *allowed;
    const int32_t *range;
    const int32_t *ngram;
    const int32_t *start;       // [slots] s0
    const int32_t *n_breakers;  // [slots]
    const int32_t *breakers;    // [slots, DRY_MAX_BREAKERS]
    prof_t *prof;
};

// does the row take part?  (uniform; the same answer in both launches of a step)
__device__ __forceinline__ bool dry_row_on(const DryArgs &a, int slot) {
    return (a.multiplier[slot] > 0.f || a.ngram[slot] > 0) && (!a.live || a.live[slot] != 0);
}

static __global__ __launch_bounds__(DRY_MATCH_THREADS) void dry_match_kernel(const DryArgs a) {
    __shared__ int32_t s_tail[DRY_MAX_MATCH];  // s_tail[j] = S[e - j]
    __shared__ int32_t s_brk[DRY_MAX_BREAKERS];
    __shared__ int s_B;
    const prof_t prof_t0 = prof_begin(a.prof);
    const int slot = a.slot0 + (int)blockIdx.x, tid = threadIdx.x;
    const int e = a.pos[slot] + a.pos_bias, s0 = max(a.start[slot], 0);
    if (!dry_row_on(a, slot) || e < s0 || e >= a.cap) {  // uniform
        prof_end(a.prof, prof_t0);
        return;
    }
    int32_t *S = a.seq + (long)slot * a.cap;
    uint32_t *table = a.table + (long)slot * a.vocab;
    const float mult = a.multiplier[slot];
    const int n = a.ngram[slot], allowed = max(a.allowed[slot], 1), range = a.range[slot];
    const int nb = min(max(a.n_breakers[slot], 0), DRY_MAX_BREAKERS);
    const int lo = range > 0 ? max(s0, e + 1 - range) : s0;
    const int last = a.tokens ? a.tokens[slot] : S[e];
    if (tid == 0 && a.tokens) S[e] = last;
    if (tid < DRY_MAX_MATCH) s_tail[tid] = tid == 0 ? last : (e - tid >= s0 ? S[e - tid] : -1);
    if (tid < nb) s_brk[tid] = a.breakers[(long)slot * DRY_MAX_BREAKERS + tid];
    __syncthreads();
    if (tid == 0) {
        int B = 0;
        if (mult > 0.f) {
            for (; B < DRY_MAX_MATCH && e - B >= lo; ++B) {
                bool brk = false;
                for (int k = 0; k < nb; ++k) brk |= s_brk[k] == s_tail[B];
                if (brk) break;
            }
        }
        s_B = B;
    }
    __syncthreads();
    const int B = s_B;
    for (int i = s0 + tid; i < e; i += DRY_MATCH_THREADS) {
        if (S[i] != last) continue;
        const int t = i + 1 == e ? last : S[i + 1];
        if ((unsigned)t >= (unsigned)a.vocab) continue;
        const int lim = min(DRY_MAX_MATCH, i - s0 + 1);
        int raw = 1;
        while (raw < lim && S[i - raw] == s_tail[raw]) ++raw;
        uint32_t entry = 0u;
        if (n > 0 && raw >= n - 1) {
            entry = DRY_BAN;
        } else if (B > 0 && i >= lo) {
            bool brk = false;
            for (int k = 0; k < nb; ++k) brk |= s_brk[k] == t;
            const int d = min(min(raw, B), i - lo + 1);
            if (!brk && d >= allowed) entry = (uint32_t)d;
        }
        if (entry != 0u) atomicMax(table + t, entry);
    }
    prof_end(a.prof, prof_t0);
}

// the entry's element: ban -> -inf; else p = multiplier * base^(L - allowed), one rounded product at a time (contraction off, like
// lpr_element), and v - p
__device__ __forceinline__ uint32_t dry_element(uint32_t l, uint32_t entry, float mult, float base, int allowed) {
#pragma clang fp contract(off)
    if (entry >= DRY_BAN) return 0xff80u;
    if ((l & 0x7f80u) == 0x7f80u && (l & 0x7fu) != 0u) return l;  // a NaN
    float p = mult;
    for (int k = (int)entry - allowed; k > 0; --k) p = p * base;
    if ((__float_as_uint(p) & 0x7f800000u) == 0x7f800000u) return 0xff80u;  // p is not finite
    return (uint32_t)BF16::from_float(__uint_as_float(l << 16) - p);
}

static __global__ __launch_bounds__(DRY_APPLY_THREADS) void dry_apply_kernel(const DryArgs a) {
    const prof_t prof_t0 = prof_begin(a.prof);
    const int row = blockIdx.y, slot = a.slot0 + row;
    const int e = a.pos[slot] + a.pos_bias;
    if (!dry_row_on(a, slot) || e < max(a.start[slot], 0) || e >= a.cap) {  // uniform: what dry_match_kernel decided
        prof_end(a.prof, prof_t0);
        return;
    }
    const int c = blockIdx.x * DRY_APPLY_CHUNK + (int)threadIdx.x * 8;
    uint16_t *out = a.rows + (long)row * a.vocab;
    uint32_t *table = a.table + (long)slot * a.vocab;
    const float mult = a.multiplier[slot], base = a.base[slot];
    const int allowed = max(a.allowed[slot], 1);
    const bool vec = (((uintptr_t)out | (uintptr_t)table) & 15) == 0 && c + 8 <= a.vocab;
    if (vec) {
        const u32x4 t0 = *reinterpret_cast<const u32x4 *>(table + c), t1 = *reinterpret_cast<const u32x4 *>(table + c + 4);
        if ((t0[0] | t0[1] | t0[2] | t0[3] | t1[0] | t1[1] | t1[2] | t1[3]) != 0u) {
            const u32x4 lv = act_load(reinterpret_cast<const u32x4 *>(out + c));
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t entry = k < 4 ? t0[k] : t1[k - 4];
                uint32_t l = (lv[k >> 1] >> ((k & 1) * 16)) & 0xffffu;
                if (entry != 0u) l = dry_element(l, entry, mult, base, allowed);
                o[k >> 1] = (k & 1) ? (o[k >> 1] | l << 16) : l;
            }
            act_store16(out + c, u32x4{o[0], o[1], o[2], o[3]});
            if ((t0[0] | t0[1] | t0[2] | t0[3]) != 0u) *reinterpret_cast<u32x4 *>(table + c) = u32x4{0u, 0u, 0u, 0u};
            if ((t1[0] | t1[1] | t1[2] | t1[3]) != 0u) *reinterpret_cast<u32x4 *>(table + c + 4) = u32x4{0u, 0u, 0u, 0u};
        }
    } else {
        for (int k = 0; k < 8; ++k) {
            if (c + k >= a.vocab) break;
            const uint32_t entry = table[c + k];
            if (entry == 0u) continue;
            act_store(out + c + k, (uint16_t)dry_element((uint32_t)act_load(out + c + k), entry, mult, base, allowed));
            table[c + k] = 0u;
        }
    }
    prof_end(a.prof, prof_t0);
}

// A chunk's ids into a slot's sequence row: S[start + i] = tokens[i], i < n (behind the token upload of a prefill / score chunk or a
// prefix attach).  grid = ceil(n / 256).
struct DryRecordArgs {
    const int32_t *tokens;  // [n]
    int32_t *row;           // the slot's sequence row
    int n, start, cap;
};
static __global__ __launch_bounds__(256) void dry_record_kernel(const DryRecordArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.n && a.start + i >= 0 && a.start + i < a.cap) a.row[a.start + i] = a.tokens[i];
}

}  // namespace tl
