// Logit processing ahead of the token choice (include/tinyllm_engine.h "penalties and logit bias"): repetition,
// presence and frequency penalties and a per-slot logit bias turn a raw bf16 logits row into a processed bf16 row; the greedy rule and
// the sampler then run on the processed row unchanged.
//
// Per element, in fp32, one IEEE-754 operation per line (no fused multiply-add; the division is the correctly rounded one):
//   v = float(l[j])
//   if prompt[j] or count[j] > 0:  v = v > 0 ? v / r : v * r
//   v = v - (f * float(count[j]))
//   if count[j] > 0:               v = v - p
//   v = v + bias[j]                (0 where the slot has no entry)
//   if not allowed[j]:  v = -inf   (a slot with a grammar only: grammar.h, grammar_stack.h; the grammar modes below)
//   out[j] = bf16(v), round to nearest even
// History: one uint16 per (slot, token): bit 15 = the token was in the prompt, bits 0-14 = how often the slot produced and fed it back,
// saturating at 32,767.  A row whose slot does not process (r = 1, p = f = 0, no bias entry) is copied bit for bit.
//
// One launch over (chunks of LPR_CHUNK tokens) x rows: a pass of ONE workgroup over a 304 KB row costs ~12 us, and this
// pass reads two rows and writes one.  8 logits per lane by 16-byte loads and stores where the rows are 16-byte aligned.  The workgroup
// whose chunk holds the slot's pending token counts it (the only store to the history inside a step); the slot's bias entries that fall
// into the chunk are scattered into LDS and added from there.
//
// The launch body is written once (lpr_process) and compiled in three grammar modes, one __global__ entry point each, one plan-key bit
// each: none (logit_process_kernel<false>), regex (logit_process_kernel<true>), and regex and stack (logit_process_stack_kernel).  A mode
// adds the LDS of its tables, the row's `allowed` byte and the advance of the slot's record (lpr_allowed8); everything else -- the copy
// path, the loads, the bias scatter, the history count, the element rule, the stores -- is the same text in all three.
#pragma once
#include <type_traits>

#include "common.h"
#include "grammar_stack.h"  // and with it grammar.h

namespace tl {

constexpr int LPR_THREADS = 256;
constexpr int LPR_CHUNK = LPR_THREADS * 8;  // tokens per workgroup
constexpr int LPR_MAX_BIAS = 1024;          // TL_MAX_LOGIT_BIAS
constexpr uint32_t LPR_PROMPT = 0x8000u, LPR_COUNT = 0x7fffu;

// (one struct by value, like every kernel of a decode step: csrc/aql.cpp copies a captured node's argument block as it is)
struct LogitProcessArgs {
    const uint16_t *logits;   // [rows, vocab] raw; row i belongs to slot slot0 + i
    uint16_t *out;            // [rows, vocab] processed
    int vocab, slot0;
    uint16_t *history;        // [slots, vocab]
    const float *repetition;  // [slots]
    const float *presence;
    const float *frequency;
    const int32_t *bias_n;       // [slots] entries in the slot's list
    const int32_t *bias_ids;     // [slots, LPR_MAX_BIAS]
    const float *bias_values;    // [slots, LPR_MAX_BIAS]
    const int32_t *tokens;       // [slots] pending token ids: a decode step counts them; nullptr: nothing is counted (prefill, caller rows)
    prof_t *prof;
    // the grammar modes only (grammar.h); poked between steps like the parameters above
    const GrammarDev *const *grammar;  // [slots] the slot's automaton; nullptr: none
    GrammarRecord *grammar_state;      // [slots]
    const int32_t *context_lens;       // [slots] the tag of a record is compared with
    // [slots] the slots' live words; nullptr: not looked at.  A slot whose word is 0 counts nothing and advances no grammar record: a slot
    // frozen by a stop (stop.h) keeps its pending token uncounted until it is resumed.  Every slot that processes otherwise is live.
    const int32_t *live;
};

__device__ __forceinline__ uint32_t lpr_count_up(uint32_t h) { return (h & LPR_COUNT) < LPR_COUNT ? h + 1u : h; }

// the six lines of the definition, each one instruction: contraction is off inside this function only (HIP's default would fuse the
// frequency product into the subtraction)
__device__ __forceinline__ uint32_t lpr_element(uint32_t l, uint32_t h, float r, float p, float f, float b) {
#pragma clang fp contract(off)
    float v = __uint_as_float(l << 16);
    const uint32_t count = h & LPR_COUNT;
    if (h != 0u) v = v > 0.f ? v / r : v * r;
    const float fc = f * (float)count;
    v = v - fc;
    if (count != 0u) v = v - p;
    v = v + b;
    return (uint32_t)BF16::from_float(v);
}

// The grammar mode of the launch.  none: the program of a step without a live grammar slot.  regex and stack (each its own plan-key bit):
// one more line at the end of the element -- a token that is not allowed in the slot's automaton state becomes -inf -- and the state's
// advance: every workgroup of a row derives the state that includes the pending token from the slot's record ({tag, state}: a record
// whose tag equals the slot's context length already includes it, any other record is advanced here), and the row's first workgroup
// stores it.  stack: the rows may also belong to slots with a STACK grammar (GrammarDev::kind), whose record is a GrammarStackRecord; a
// row with a regex grammar runs the regex mode's code there.
enum class LprGrammar { none, regex, stack };

// What a grammar mode adds for a row whose slot has the automaton `gp` (uniform): bit e = token c + e is allowed, the slot's record
// advanced on the way.  The LDS declared here is the mode's: the regex rows' uint16 table (GR_LDS_STATES rows) or, in the stack mode,
// the fused table (GRS_LDS_STATES rows), which holds either -- 32 KB both ways -- and the pop table.  Contains barriers.
template <LprGrammar G>
__device__ __forceinline__ uint32_t lpr_allowed8(const LogitProcessArgs a, GrammarStackRecord *stack_state, const GrammarDev *gp,
                                                 const int32_t *tokens, int slot, int c) {
    constexpr bool STACK = G == LprGrammar::stack;
    __shared__ __attribute__((aligned(16))) std::conditional_t<STACK, uint32_t, uint16_t> s_table[(STACK ? GRS_LDS_STATES : GR_LDS_STATES) * 256];
    __shared__ int s_state;
    static_assert(GRS_LDS_STATES * 256 * 4 >= GR_LDS_STATES * 256 * 2, "the stack mode's s_table holds either table");
    GrRef g = *GR_GLOBAL(GrammarDev, gp);
    if constexpr (STACK) {
        __shared__ __attribute__((aligned(16))) uint16_t s_pop[GRS_LDS_POPS * 8];
        __shared__ uint32_t s_cfg[4];
        if (g.kind != 0) {
            const GrsConfig cfg = grs_row_config(g, stack_state, tokens, a.context_lens, slot, a.vocab, blockIdx.x == 0, s_cfg);
            bool whole, pop_lds;
            grs_stage_tables(g, cfg.state, s_table, s_pop, LPR_THREADS, &whole, &pop_lds);
            return grs_allowed8(g, cfg, c, a.vocab, s_table, s_pop, whole, pop_lds);
        }
    }
    uint16_t *s_table16 = reinterpret_cast<uint16_t *>(s_table);
    const int state = gr_row_state(g, a.grammar_state, tokens, a.context_lens, slot, a.vocab, blockIdx.x == 0, &s_state);
    const bool whole = gr_stage_table(g, state, s_table16, LPR_THREADS);
    return gr_allowed8(g, state, c, a.vocab, s_table16, whole);
}

// The launch body, in grammar mode G.  (The argument struct by value, as the kernels take it: passed by reference, the step end's
// argument struct cost its logprob twin 36 bytes of scratch.)
template <LprGrammar G>
__device__ __forceinline__ void lpr_process(const LogitProcessArgs a, GrammarStackRecord *stack_state) {
    constexpr bool GRAMMAR = G != LprGrammar::none;
    __shared__ float s_bias[LPR_CHUNK];
    const prof_t prof_t0 = prof_begin(a.prof);
    const int row = blockIdx.y, slot = a.slot0 + row;
    const int c0 = blockIdx.x * LPR_CHUNK, c = c0 + (int)threadIdx.x * 8;
    const uint16_t *lg = a.logits + (long)row * a.vocab;
    uint16_t *out = a.out + (long)row * a.vocab;
    uint16_t *hist = a.history + (long)slot * a.vocab;
    const float r = a.repetition[slot], p = a.presence[slot], f = a.frequency[slot];
    const int nb = min(a.bias_n[slot], LPR_MAX_BIAS);
    const GrammarDev *gp = nullptr;
    if constexpr (GRAMMAR) gp = a.grammar[slot];
    const bool on = r != 1.f || p != 0.f || f != 0.f || nb > 0 || gp != nullptr;  // uniform
    const int32_t *tokens = (a.live && a.live[slot] == 0) ? nullptr : a.tokens;      // uniform
    const bool vec = (((uintptr_t)lg | (uintptr_t)out | (uintptr_t)hist) & 15) == 0 && c + 8 <= a.vocab;
    if (!on) {  // the row of a slot that does not process: copied, so that the step end reads one buffer
        if (vec) {
            act_store16(out + c, act_load(reinterpret_cast<const u32x4 *>(lg + c)));
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c + e < a.vocab) act_store(out + c + e, act_load(lg + c + e));
        }
        prof_end(a.prof, prof_t0);
        return;
    }
    // loads first: logits and history are in flight while the bias entries are scattered
    u32x4 lv = {0u, 0u, 0u, 0u}, hv = {0u, 0u, 0u, 0u};
    if (vec) {
        lv = act_load(reinterpret_cast<const u32x4 *>(lg + c));
        hv = *reinterpret_cast<const u32x4 *>(hist + c);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (c + e >= a.vocab) continue;
            lv[e >> 1] |= (uint32_t)act_load(lg + c + e) << ((e & 1) * 16);
            hv[e >> 1] |= (uint32_t)hist[c + e] << ((e & 1) * 16);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s_bias[threadIdx.x * 8 + e] = 0.f;
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += LPR_THREADS) {  // ids are distinct: no two lanes write one entry
        const int d = a.bias_ids[(long)slot * LPR_MAX_BIAS + k] - c0;
        if ((unsigned)d < (unsigned)LPR_CHUNK) s_bias[d] = a.bias_values[(long)slot * LPR_MAX_BIAS + k];
    }
    __syncthreads();
    uint32_t allowed = 0xffu;
    if constexpr (GRAMMAR) {
        if (gp) allowed = lpr_allowed8<G>(a, stack_state, gp, tokens, slot, c);  // uniform
    }
    // the pending token (what the previous step produced and this step consumed) is counted before the row is processed
    const int pending = tokens ? tokens[slot] : -1;
    uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        uint32_t h = (hv[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
        if (c + e == pending && c + e < a.vocab) {
            h = lpr_count_up(h);
            act_store(hist + c + e, (uint16_t)h);
        }
        const uint32_t l = (lv[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
        uint32_t v = lpr_element(l, h, r, p, f, s_bias[threadIdx.x * 8 + e]);
        if constexpr (GRAMMAR) v = (allowed >> e & 1u) ? v : 0xff80u;  // -inf
        o[e >> 1] |= v << ((e & 1) * 16);
    }
    if (vec) {
        act_store16(out + c, u32x4{o[0], o[1], o[2], o[3]});
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (c + e < a.vocab) act_store(out + c + e, (uint16_t)((o[e >> 1] >> ((e & 1) * 16)) & 0xffffu));
    }
    prof_end(a.prof, prof_t0);
}

// The three entry points: each its own kernel name, argument struct (by value: csrc/aql.cpp copies a captured node's block as it is) and
// plan-key bit.
template <bool GRAMMAR>
static __global__ __launch_bounds__(LPR_THREADS) void logit_process_kernel(const LogitProcessArgs a) {
    lpr_process<GRAMMAR ? LprGrammar::regex : LprGrammar::none>(a, nullptr);
}
struct LogitProcessStackArgs {
    LogitProcessArgs base;
    GrammarStackRecord *stack_state;  // [slots]
};
static __global__ __launch_bounds__(LPR_THREADS) void logit_process_stack_kernel(const LogitProcessStackArgs sa) {
    lpr_process<LprGrammar::stack>(sa.base, sa.stack_state);
}

// Prompt marking: bit 15 of history[token] for n consumed tokens of one slot (behind the token upload of a prefill / score chunk).
// A vector atomic OR on the containing 32-bit word: neighbours of one word may be marked by different lanes.  grid = ceil(n / 256).
struct LogitMarkArgs {
    const int32_t *tokens;  // [n]
    int n, vocab;
    uint32_t *table;        // the history table as 32-bit words (two tokens each)
    long row;               // the slot's first element in the table: slot * vocab (odd where the vocabulary is)
};
static __global__ __launch_bounds__(256) void logit_mark_prompt_kernel(const LogitMarkArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int t = a.tokens[i];
    if (t < 0 || t >= a.vocab) return;
    const long el = a.row + t;
    atomicOr(a.table + (el >> 1), (el & 1) ? (LPR_PROMPT << 16) : LPR_PROMPT);
}

}  // namespace tl
