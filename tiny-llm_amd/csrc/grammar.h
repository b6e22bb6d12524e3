// Regex-constrained decoding (include/tinyllm_engine.h "grammars"): the allowed set of a slot follows a byte-level
// DFA over the bytes of the tokens it produces.  The vocabulary (offsets + bytes) and the automaton (table [n_states][256] uint16,
// accepting, EOS ids) are uploaded once; the processing launch (logit_process.h) decides per token whether its bytes can be walked from the
// slot's state, and advances the state with the pending token.  Nothing is uploaded per step and no states x vocab table exists.
//
// The walk: a lane owns 8 consecutive tokens and walks them in lock-step as 8 chains, one table lookup per byte and chain; a round's 8
// lookups and 8 next-byte fetches are issued without a branch (a dead chain reads entry 0), so they are in flight together.  The table is
// read from LDS where the whole of it fits GR_LDS_STATES rows; a larger automaton keeps the ROW OF THE CURRENT STATE in LDS (every
// first-byte lookup of the launch, where most tokens die) and reads the rest through L2.
// Long tokens (more than GR_LONG bytes) are not walked there at all: tl_grammar_create walks each of them from every state once and
// leaves one bit per (state, long token), so a round-by-round walk never runs longer than GR_LONG rounds.
//
// What exists once, for this automaton and the stack automaton of grammar_stack.h alike: the transition rule of a byte (gr_step here,
// grs_step there: __host__ __device__, so the host's advance of a pending token is the device's rule), the opening of the walk
// (grammar_walk_open.inc), the EOS rule (gr_eos_rule) and the frame of the mask-rows kernels (gr_mask_rows).
#pragma once
#include "common.h"

namespace tl {

constexpr int GR_END = -1;                  // TL_GRAMMAR_END
constexpr uint32_t GR_DEAD = 0xffffu;       // no transition
constexpr int GR_MAX_STATES = 32768, GR_MAX_EOS = 8;
constexpr int GR_LDS_STATES = 64;           // automata up to this many states live in LDS whole (32 KB beside the bias chunk)
constexpr int GR_LONG = 16;                 // a token of more bytes than this is LONG: never walked by the processing launch (long_bits)

// what a slot's pointer leads to: device-resident, inside the grammar's own allocation (tl_grammar_create)
struct GrammarDev {
    const uint16_t *table;     // [n_states][256]
    const uint8_t *accepting;  // [n_states]
    const int32_t *offsets;    // [vocab + 1]  the vocabulary's
    const uint8_t *bytes;
    int n_states, n_eos;
    int32_t eos[GR_MAX_EOS];
    // long tokens (more than GR_LONG bytes; a few hundred of a BPE vocabulary, up to 200 bytes each): whether one can be walked from a
    // state is precomputed at tl_grammar_create -- bit (li & 31) of long_bits[state * long_words + li / 32], li = long_index[token]
    const int32_t *long_index;  // [vocab] the vocabulary's: the token's number among the long tokens (undefined for a short one)
    const uint32_t *long_bits;  // [n_states][long_words]
    int long_words;
    // a stack grammar only (grammar_stack.h; kind != 0): table, long_bits and long_words above are unused
    int kind, n_pop, n_long;
    const uint32_t *fused;   // [n_states][256] entry | op << 16
    const uint16_t *pop;     // [max(n_pop, 1)][8] the state after a pop by the new top (0 .. 3, 4 = empty stack); 5 .. 7 padding
    const uint8_t *long_m;   // [n_states][n_long]
};

// the slot's state record: `state` includes the pending token of the step in which the slot's context length was `tag`
struct GrammarRecord {
    int32_t tag, state;
};

// the tables are reached through GrammarDev's pointers, which the compiler cannot see are global memory: spelled out, so that the loads
// are global_load / ds_read and not FLAT loads (which wait on both counters and would serialise the chains below)
#define GR_GLOBAL(T, p) ((const T __attribute__((address_space(1))) *)(p))
// ... and GrammarDev itself through a global-address-space reference
using GrRef = const GrammarDev __attribute__((address_space(1))) &;

__device__ __forceinline__ bool gr_is_eos(GrRef g, int token) {
    bool is = false;
    for (int k = 0; k < g.n_eos; ++k) is |= g.eos[k] == token;
    return is;
}

// One byte of the automaton, the transition rule of the definition: the state after byte b from state s, GR_DEAD where there is none.
// The one copy of the rule, on the device (gr_advance, grammar_long_bits_kernel) and on the host (tl_grammar::advance); TABLE is the
// table's pointer type, so that a device caller keeps its address space (GR_GLOBAL above) and the host passes a plain pointer.
template <class TABLE>
__host__ __device__ __forceinline__ uint32_t gr_step(TABLE table, uint32_t s, uint32_t b) {
    return table[s * 256u + b];
}

// state' of the definition: END after an EOS id or from END, else the walk with DEAD -> END.  Called by ONE WAVE (all 64 lanes, uniform
// arguments): the lanes fetch 64 of the token's bytes with one load, then the serial chain is one table lookup per byte.
__device__ __forceinline__ int gr_advance(GrRef g, int state, int token, int vocab) {
    if (state < 0 || (unsigned)token >= (unsigned)vocab || gr_is_eos(g, token)) return GR_END;
    const auto offsets = GR_GLOBAL(int32_t, g.offsets);
    const auto bytes = GR_GLOBAL(uint8_t, g.bytes);
    const auto table = GR_GLOBAL(uint16_t, g.table);
    const int b0 = offsets[token], b1 = offsets[token + 1];
    if (b1 <= b0) return GR_END;
    const int lane = threadIdx.x & 63;
    uint32_t s = (uint32_t)state;
    for (int base = b0; base < b1; base += 64) {
        const uint32_t mine = base + lane < b1 ? bytes[base + lane] : 0u;
        const int n = min(64, b1 - base);
        for (int k = 0; k < n; ++k) {
            s = gr_step(table, s, (uint32_t)__shfl((int)mine, k));
            if (s == GR_DEAD) return GR_END;
        }
    }
    return (int)s;
}

// The walk of a lane's 8 tokens, c .. c + 7, from `state` (>= 0, uniform over the workgroup): bit e of the result = token c + e can be
// walked.  Every round issues its 8 table lookups and its 8 byte fetches WITHOUT a branch -- a chain that is dead reads entry 0 and its
// result is dropped by a select -- so that the 16 loads of a round are in flight together and a round costs one latency, not sixteen.
// LDS: `table` is the LDS copy (the whole table, row_base = state * 256, or the current row alone, row_base = 0, for the first byte).
template <bool WHOLE>
__device__ __forceinline__ uint32_t gr_walk8(GrRef g, int state, int c, int vocab, const uint16_t *s_table) {
    const auto offsets = GR_GLOBAL(int32_t, g.offsets);
    const auto bytes = GR_GLOBAL(uint8_t, g.bytes);
    const auto table = GR_GLOBAL(uint16_t, g.table);
    // a long token: the precomputed bit of (state, token)
    const auto long_ok = [&](int li) { return GR_GLOBAL(uint32_t, g.long_bits)[(size_t)state * g.long_words + (li >> 5)] >> (li & 31) & 1u; };
#include "grammar_walk_open.inc"
    uint32_t s[8], nxt[8], t[8];
    // byte 1 of every token
#pragma unroll
    for (int e = 0; e < 8; ++e) nxt[e] = bytes[len[e] > 1 ? off[e] + 1 : 0];
    // first byte: the current state's row, in LDS on both paths
    const uint32_t row0 = WHOLE ? (uint32_t)state * 256u : 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = s_table[row0 + cur[e]];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const bool on = alive >> e & 1u, dead = t[e] == GR_DEAD;
        s[e] = on && !dead ? t[e] : 0u;
        ok |= on && !dead && len[e] == 1 ? 1u << e : 0u;
        alive &= on && !dead && len[e] > 1 ? ~0u : ~(1u << e);
        cur[e] = nxt[e];
    }
    // the survivors: byte k of every live chain per round, byte k + 1 fetched in the same round
    for (int k = 1; alive != 0u; ++k) {
#pragma unroll
        for (int e = 0; e < 8; ++e) nxt[e] = bytes[(alive >> e & 1u) && len[e] > k + 1 ? off[e] + k + 1 : 0];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t at = (alive >> e & 1u) ? s[e] * 256u + cur[e] : 0u;
            if constexpr (WHOLE) t[e] = s_table[at];
            else t[e] = table[at];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool on = alive >> e & 1u, dead = t[e] == GR_DEAD;
            s[e] = on && !dead ? t[e] : 0u;
            ok |= on && !dead && len[e] == k + 1 ? 1u << e : 0u;
            alive &= on && !dead && len[e] > k + 1 ? ~0u : ~(1u << e);
            cur[e] = nxt[e];
        }
    }
    return ok;
}

// The EOS ids of a lane's 8 tokens are decided by the state alone, whatever their bytes (acceptance by final state): allowed in END and in
// an accepting state, never otherwise.  `ok`: what the walk found; returns it with the EOS bits set or cleared.
__device__ __forceinline__ uint32_t gr_eos_rule(GrRef g, int state, int c, int vocab, uint32_t ok) {
    const bool eos_ok = state < 0 || GR_GLOBAL(uint8_t, g.accepting)[state] != 0;
    for (int k = 0; k < g.n_eos; ++k) {
        const int d = g.eos[k] - c;
        if ((unsigned)d < 8u && g.eos[k] < vocab) ok = eos_ok ? (ok | 1u << d) : (ok & ~(1u << d));
    }
    return ok;
}

// bit e of the result: token c + e is allowed in `state` (uniform over the workgroup).  whole: s_table holds the table as it is;
// otherwise the row of `state` alone (256 entries).
__device__ __forceinline__ uint32_t gr_allowed8(GrRef g, int state, int c, int vocab, const uint16_t *s_table, bool whole) {
    uint32_t ok = 0u;
    if (state >= 0) ok = whole ? gr_walk8<true>(g, state, c, vocab, s_table) : gr_walk8<false>(g, state, c, vocab, s_table);  // uniform
    return gr_eos_rule(g, state, c, vocab, ok);
}

// the table (or the current state's row) into LDS; s_table holds GR_LDS_STATES * 256 entries.  Returns whether the whole table is there.
// Ends with a barrier.  `state` uniform.
__device__ __forceinline__ bool gr_stage_table(GrRef g, int state, uint16_t *s_table, int threads) {
    const bool whole = g.n_states <= GR_LDS_STATES;
    if (state >= 0) {
        // 16-byte pieces: a row is 512 bytes, the table is 16-byte aligned (tl_grammar_create)
        const auto src = reinterpret_cast<const u32x4 __attribute__((address_space(1))) *>(GR_GLOBAL(uint16_t, g.table) + (whole ? (size_t)0 : (size_t)state * 256));
        const int pieces = (whole ? g.n_states : 1) * 32;
        for (int k = threadIdx.x; k < pieces; k += threads) reinterpret_cast<u32x4 *>(s_table)[k] = src[k];
    }
    __syncthreads();
    return whole;
}

// the state of a row of the processing launch: the slot's record, advanced with the pending token unless the record says it is in
// already (tag == the slot's context length); wave 0 does the walk, the row's first workgroup stores the new record, everybody gets
// the result through LDS.  tokens == nullptr (a prefill's last row): the record as it stands.  Ends with a barrier.
__device__ __forceinline__ int gr_row_state(GrRef g, GrammarRecord *rec, const int32_t *tokens, const int32_t *context_lens,
                                            int slot, int vocab, bool store, int *s_state) {
    if (threadIdx.x < 64) {
        const uint64_t rec64 = act_load(reinterpret_cast<const uint64_t *>(rec + slot));
        int state = (int)(uint32_t)(rec64 >> 32);
        const int tag = (int)(uint32_t)rec64;
        if (tokens) {
            const int ctx = context_lens[slot];
            if (tag != ctx) {
                state = gr_advance(g, state, tokens[slot], vocab);
                if (store && threadIdx.x == 0)
                    act_store(reinterpret_cast<uint64_t *>(rec + slot), (uint64_t)(uint32_t)ctx | (uint64_t)(uint32_t)state << 32);
            }
        }
        if (threadIdx.x == 0) *s_state = state;
    }
    __syncthreads();
    return *s_state;
}

// tl_grammar_create: long_bits.  grid = (long_words / 2, n_states), block = 64: lane l of block (x, s) walks long token 64 x + l from state
// s (a serial walk, once per grammar), the wave's ballot is the 64 bits of two words
struct GrammarLongArgs {
    const uint16_t *table;
    const int32_t *offsets;
    const uint8_t *bytes;
    const int32_t *long_ids;  // [n_long] token ids, ascending
    int n_long, long_words;
    uint32_t *out;
};
static __global__ __launch_bounds__(64) void grammar_long_bits_kernel(const GrammarLongArgs a) {
    const int li = blockIdx.x * 64 + (int)threadIdx.x, state = blockIdx.y;
    bool ok = false;
    if (li < a.n_long) {
        const int j = a.long_ids[li];
        uint32_t s = (uint32_t)state;
        for (int k = a.offsets[j]; k < a.offsets[j + 1] && s != GR_DEAD; ++k) s = gr_step(a.table, s, a.bytes[k]);
        ok = s != GR_DEAD;
    }
    const unsigned long long m = __ballot(ok);
    if (threadIdx.x == 0) {
        uint32_t *row = a.out + (size_t)state * a.long_words + blockIdx.x * 2;
        row[0] = (uint32_t)m, row[1] = (uint32_t)(m >> 32);
    }
}

// The frame of the mask-rows kernels (tl_grammar_mask_rows, tl_grammar_mask_rows_stack): out[i][j] = logits[i][j] where j is allowed in
// row i's state, else -inf (bf16 0xff80).  grid = (chunks of 2048, rows); allowed(row, c): bit e = token c + e is allowed.
template <class ALLOWED>
__device__ __forceinline__ void gr_mask_rows(const uint16_t *logits, uint16_t *out, int vocab, ALLOWED allowed) {
    const int row = blockIdx.y, c = blockIdx.x * 2048 + (int)threadIdx.x * 8;
    const uint32_t ok = allowed(row, c);
    const uint16_t *lg = logits + (long)row * vocab;
    out += (long)row * vocab;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (c + e < vocab) out[c + e] = (ok >> e & 1u) ? lg[c + e] : (uint16_t)0xff80u;
}

struct GrammarMaskArgs {
    const GrammarDev *g;
    const uint16_t *logits;
    uint16_t *out;
    const int32_t *states;
    int vocab;
};
static __global__ __launch_bounds__(256) void grammar_mask_rows_kernel(const GrammarMaskArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t s_table[GR_LDS_STATES * 256];
    gr_mask_rows(a.logits, a.out, a.vocab, [&](int row, int c) {
        GrRef g = *GR_GLOBAL(GrammarDev, a.g);
        int state = a.states[row];
        if (state >= g.n_states) state = GR_END;  // (validated by the caller where it can be; never an index past the table)
        const bool whole = gr_stage_table(g, state, s_table, 256);
        return gr_allowed8(g, state, c, a.vocab, s_table, whole);
    });
}

}  // namespace tl
