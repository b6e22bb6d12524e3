// Stack grammars (include/tinyllm_engine.h "stack grammars"): the byte-level DFA of grammar.h with a bounded stack
// beside the state -- 32 levels of 2-bit symbols in one uint64 -- which is what nested JSON needs.  A slot's configuration is
// (state, depth, stack).  The processing launch (logit_process.h) serves such a slot in its stack mode -- logit_process_stack_kernel, its
// own plan-key bit -- which runs when some live slot of the step holds a stack grammar; this file holds what that mode calls: the
// transition rule, the walk, the staging of the tables, and the record.
//
// Device tables: the ABI's table [n_states][256] uint16 and ops [n_states][256] uint8 are FUSED into one uint32 per (state, byte) --
// bits 0-15 the entry (0xFFFF = no transition), bits 16-18 the op -- so a round of the walk is one lookup per chain, as in grammar.h; the
// pop table is padded to 8 uint16 per entry.  The host keeps the same two tables (tl_grammar), and one rule, grs_step, walks both.
// The walk keeps the shape of gr_walk8 and opens with the same text (grammar_walk_open.inc): a lane walks 8 tokens in lock-step, a
// round's lookups are issued without a branch.  A chain does not carry the 64-bit stack: a token of at most GR_LONG bytes pushes at most 16 symbols and
// consumes at most 16 levels of the slot's stack, so a chain carries what it pushed itself (32 bits), how many symbols of that are live,
// and how many levels of the slot's stack (uniform over the workgroup) it has popped.  The pop lookup depends on the table lookup: it is
// issued for all 8 chains of a round together (a chain that does not pop reads entry 0 and drops it), one more latency per round that
// pops, not eight.
// Long tokens: one byte per (state, long token), the largest depth the token's walk from (state, empty stack) reaches, 0xFF where that
// walk dies (it then pops below its starting level, or has no transition): allowed iff depth + m <= 32.
#pragma once
#include "grammar.h"

namespace tl {

constexpr int GRS_DEPTH = 32;               // levels of the stack
constexpr uint32_t GRS_POP = 5;             // op: pop; 1 .. 4 push symbol op - 1; 0 nothing
constexpr int GRS_LDS_STATES = 32;          // automata up to this many states live in LDS whole (32 KB of fused entries: the regex mode's LDS)
constexpr int GRS_LDS_POPS = 64;            // pop tables up to this many entries are read from LDS (1 KB)
constexpr int GRS_MAX_POPS = 65535;
constexpr uint32_t GRS_NO_DEPTH = 0xffu;    // long_m: the long token cannot be walked from the state

// a slot's configuration
struct GrsConfig {
    int state, depth;
    uint64_t stack;  // symbol of level i (0 = bottom) in bits 2i, 2i + 1; zero above 2 * depth
};

// The slot's record.  rec = {tag (low word), packed (high word)}: packed = 0xFFFFFFFF in END, else state | depth << 16 | which << 24;
// the stack of the record is stack[which].  An advance writes stack[!which] FIRST and then rec (one 64-bit store), so whoever reads rec
// and then stack[which of that rec] sees the old configuration whole or the new one whole: the launch that advances never writes the
// word the old record points at.  The three words share one 32-byte piece of a cache line on purpose: a cache that holds a copy of the
// line holds a state of memory in which rec and the word it points at agree, and copies fetched later are never older.
struct __attribute__((aligned(32))) GrammarStackRecord {
    uint64_t rec;
    uint64_t stack[2];
    uint64_t unused;
};

__device__ __host__ __forceinline__ uint64_t grs_mask(int depth) { return depth >= GRS_DEPTH ? ~0ull : (1ull << (2 * depth)) - 1ull; }
__device__ __host__ __forceinline__ uint32_t grs_pack(const GrsConfig &c, int which) {
    return c.state < 0 ? 0xffffffffu : (uint32_t)c.state | (uint32_t)c.depth << 16 | (uint32_t)which << 24;
}

// One byte of the automaton over the real stack, the transition rule of the definition: push op - 1, pop and look the state up by the new
// top; false where the configuration dies -- no transition, a push at depth 32, a pop at depth 0 -- and `c` is then not to be used.
// The one copy of the rule, on the device (grs_advance, grammar_long_depth_kernel) and on the host (tl_grammar::advance); FUSED
// and POP are the tables' pointer types, so that a device caller keeps its address space (grammar.h, GR_GLOBAL).
template <class FUSED, class POP>
__host__ __device__ __forceinline__ bool grs_step(FUSED fused, POP pop, GrsConfig &c, uint32_t b) {
    const uint32_t f = fused[(uint32_t)c.state * 256u + b], t = f & 0xffffu, op = f >> 16;
    if (t == GR_DEAD) return false;
    if (op == 0u) {
        c.state = (int)t;
    } else if (op < GRS_POP) {
        if (c.depth == GRS_DEPTH) return false;
        c.stack |= (uint64_t)(op - 1u) << (2 * c.depth);
        c.depth += 1;
        c.state = (int)t;
    } else {
        if (c.depth == 0) return false;
        c.depth -= 1;
        c.stack &= grs_mask(c.depth);
        const uint32_t top = c.depth ? (uint32_t)(c.stack >> (2 * (c.depth - 1))) & 3u : 4u;
        const uint32_t to = pop[t * 8u + top];
        if (to == GR_DEAD) return false;
        c.state = (int)to;
    }
    return true;
}

// advance of the definition on a configuration, END = (-1, 0, 0).  Called by ONE WAVE with uniform arguments, like gr_advance: walks the
// real stack, at any token length.
__device__ __forceinline__ GrsConfig grs_advance(GrRef g, GrsConfig c, int token, int vocab) {
    const GrsConfig end{GR_END, 0, 0ull};
    if (c.state < 0 || (unsigned)token >= (unsigned)vocab || gr_is_eos(g, token)) return end;
    const auto offsets = GR_GLOBAL(int32_t, g.offsets);
    const auto bytes = GR_GLOBAL(uint8_t, g.bytes);
    const auto fused = GR_GLOBAL(uint32_t, g.fused);
    const auto pop = GR_GLOBAL(uint16_t, g.pop);
    const int b0 = offsets[token], b1 = offsets[token + 1];
    if (b1 <= b0) return end;
    const int lane = threadIdx.x & 63;
    for (int base = b0; base < b1; base += 64) {
        const uint32_t mine = base + lane < b1 ? bytes[base + lane] : 0u;
        const int n = min(64, b1 - base);
        for (int k = 0; k < n; ++k)
            if (!grs_step(fused, pop, c, (uint32_t)__shfl((int)mine, k))) return end;
    }
    return c;
}

// The walk of a lane's 8 tokens, c .. c + 7, from `cfg` (state >= 0, uniform over the workgroup): bit e of the result = token c + e can
// be walked.  s_table: the fused table in LDS (whole, or the row of cfg.state alone); s_pop: the pop table in LDS where pop_lds.
template <bool WHOLE>
__device__ __forceinline__ uint32_t grs_walk8(GrRef g, const GrsConfig cfg, int c, int vocab, const uint32_t *s_table, const uint16_t *s_pop,
                                              bool pop_lds) {
    const auto offsets = GR_GLOBAL(int32_t, g.offsets);
    const auto bytes = GR_GLOBAL(uint8_t, g.bytes);
    const auto fused = GR_GLOBAL(uint32_t, g.fused);
    const auto pop = GR_GLOBAL(uint16_t, g.pop);
    // a long token: the precomputed depth of (state, token)
    const auto long_ok = [&](int li) {
        const uint32_t m = GR_GLOBAL(uint8_t, g.long_m)[(size_t)cfg.state * g.n_long + li];
        return m != GRS_NO_DEPTH && cfg.depth + (int)m <= GRS_DEPTH ? 1u : 0u;
    };
#include "grammar_walk_open.inc"
    // per chain: the state, what the chain pushed itself (`up` live symbols in `loc`) and how many levels of cfg.stack it has popped
    uint32_t s[8], nxt[8], f[8], loc[8], pidx[8], p[8];
    int up[8], below[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0u, loc[e] = 0u, up[e] = 0, below[e] = 0;
    for (int k = 0; alive != 0u; ++k) {
        // byte k + 1 of every live chain, fetched in the same round as the lookups of byte k
#pragma unroll
        for (int e = 0; e < 8; ++e) nxt[e] = bytes[(alive >> e & 1u) && len[e] > k + 1 ? off[e] + k + 1 : 0];
        if (k == 0) {  // first byte: the current state's row, in LDS on both paths
            const uint32_t row0 = WHOLE ? (uint32_t)cfg.state * 256u : 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = s_table[row0 + cur[e]];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t at = (alive >> e & 1u) ? s[e] * 256u + cur[e] : 0u;
                if constexpr (WHOLE) f[e] = s_table[at];
                else f[e] = fused[at];
            }
        }
        // the stack operation of every chain; a pop leaves the index of its dependent lookup (0 for a chain that does not pop)
        uint32_t pops = 0u;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool on = alive >> e & 1u;
            const uint32_t t = f[e] & 0xffffu, op = f[e] >> 16;
            bool dead = !on || t == GR_DEAD;
            const bool push = op != 0u && op < GRS_POP, is_pop = op == GRS_POP;
            const int left = cfg.depth - below[e];  // levels of the slot's stack the chain has not popped
            if (push) {
                dead |= left + up[e] == GRS_DEPTH;
                loc[e] = (loc[e] & ~(3u << (2 * (up[e] & 15)))) | (op - 1u) << (2 * (up[e] & 15));
                up[e] += 1;
            }
            uint32_t top = 4u;
            if (is_pop) {
                if (up[e] > 0) up[e] -= 1;
                else dead |= left == 0, below[e] += 1;
                const int under = cfg.depth - below[e];
                if (up[e] > 0) top = loc[e] >> (2 * ((up[e] - 1) & 15)) & 3u;
                else if (under > 0) top = (uint32_t)(cfg.stack >> (2 * ((under - 1) & 31))) & 3u;
            }
            const bool popping = is_pop && !dead;
            pops |= popping ? 1u << e : 0u;
            pidx[e] = popping ? t * 8u + top : 0u;
            s[e] = dead ? 0u : t;
            alive &= dead ? ~(1u << e) : ~0u;
        }
        if (__builtin_amdgcn_ballot_w64(pops != 0u)) {  // (wave-uniform: most rounds of most waves pop nothing)
#pragma unroll
            for (int e = 0; e < 8; ++e) p[e] = pop_lds ? (uint32_t)s_pop[pidx[e]] : (uint32_t)pop[pidx[e]];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (!(pops >> e & 1u)) continue;
                s[e] = p[e] == GR_DEAD ? 0u : p[e];
                alive &= p[e] == GR_DEAD ? ~(1u << e) : ~0u;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool on = alive >> e & 1u;
            ok |= on && len[e] == k + 1 ? 1u << e : 0u;
            alive &= on && len[e] > k + 1 ? ~0u : ~(1u << e);
            cur[e] = nxt[e];
        }
    }
    return ok;
}

// bit e of the result: token c + e is allowed in `cfg` (uniform over the workgroup)
__device__ __forceinline__ uint32_t grs_allowed8(GrRef g, const GrsConfig cfg, int c, int vocab, const uint32_t *s_table, const uint16_t *s_pop,
                                                 bool whole, bool pop_lds) {
    uint32_t ok = 0u;
    if (cfg.state >= 0) ok = whole ? grs_walk8<true>(g, cfg, c, vocab, s_table, s_pop, pop_lds) : grs_walk8<false>(g, cfg, c, vocab, s_table, s_pop, pop_lds);
    return gr_eos_rule(g, cfg.state, c, vocab, ok);
}

// the fused table (or the current state's row) and a small pop table into LDS; s_table holds GRS_LDS_STATES * 256 entries, s_pop
// GRS_LDS_POPS * 8.  Ends with a barrier.  `state` uniform.
__device__ __forceinline__ void grs_stage_tables(GrRef g, int state, uint32_t *s_table, uint16_t *s_pop, int threads, bool *whole, bool *pop_lds) {
    *whole = g.n_states <= GRS_LDS_STATES;
    *pop_lds = g.n_pop <= GRS_LDS_POPS;
    if (state >= 0) {
        // 16-byte pieces: a row is 1 KB, a pop entry 16 bytes; both tables are 16-byte aligned (tl_grammar_create_stack)
        const auto src = reinterpret_cast<const u32x4 __attribute__((address_space(1))) *>(GR_GLOBAL(uint32_t, g.fused) + (*whole ? (size_t)0 : (size_t)state * 256));
        const int pieces = (*whole ? g.n_states : 1) * 64;
        for (int k = threadIdx.x; k < pieces; k += threads) reinterpret_cast<u32x4 *>(s_table)[k] = src[k];
        if (*pop_lds) {
            const auto psrc = reinterpret_cast<const u32x4 __attribute__((address_space(1))) *>(GR_GLOBAL(uint16_t, g.pop));
            for (int k = threadIdx.x; k < g.n_pop; k += threads) reinterpret_cast<u32x4 *>(s_pop)[k] = psrc[k];
        }
    }
    __syncthreads();
}

// the configuration a record's words hold: END, or (state, depth, stack[which]) -- `which` names the stack word to read, and the word
// is masked by the depth (grs_mask) by whoever reads it
__device__ __host__ __forceinline__ GrsConfig grs_unpack(uint32_t packed, int *which) {
    *which = 0;
    if (packed == 0xffffffffu) return GrsConfig{GR_END, 0, 0ull};
    *which = (int)(packed >> 24 & 1u);
    const int depth = (int)(packed >> 16 & 0xffu);
    return GrsConfig{(int)(packed & 0xffffu), depth < GRS_DEPTH ? depth : GRS_DEPTH, 0ull};
}

// the configuration of a row of the processing launch: the slot's record, advanced with the pending token unless the record says it is in
// already; wave 0 does the walk, the row's first workgroup stores the new record (stack word first), everybody gets the result through
// LDS (s_cfg: 4 words).  tokens == nullptr (a prefill's last row): the record as it stands.  Ends with a barrier.
__device__ __forceinline__ GrsConfig grs_row_config(GrRef g, GrammarStackRecord *recs, const int32_t *tokens, const int32_t *context_lens,
                                                    int slot, int vocab, bool store, uint32_t *s_cfg) {
    if (threadIdx.x < 64) {
        GrammarStackRecord *r = recs + slot;
        const uint64_t rec64 = act_load(&r->rec);
        const int tag = (int)(uint32_t)rec64;
        int which;
        GrsConfig c = grs_unpack((uint32_t)(rec64 >> 32), &which);
        if (c.state >= 0) c.stack = act_load(&r->stack[which]) & grs_mask(c.depth);
        if (tokens) {
            const int ctx = context_lens[slot];
            if (tag != ctx) {
                c = grs_advance(g, c, tokens[slot], vocab);
                if (store && threadIdx.x == 0) {
                    act_store(&r->stack[which ^ 1], c.stack);
                    // the stack word leaves this lane before the record does (both go to one 32-byte piece of one line)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_s_waitcnt(0);
                    act_store(&r->rec, (uint64_t)(uint32_t)ctx | (uint64_t)grs_pack(c, which ^ 1) << 32);
                }
            }
        }
        if (threadIdx.x == 0) s_cfg[0] = (uint32_t)c.state, s_cfg[1] = (uint32_t)c.depth, s_cfg[2] = (uint32_t)c.stack, s_cfg[3] = (uint32_t)(c.stack >> 32);
    }
    __syncthreads();
    return GrsConfig{(int)s_cfg[0], (int)s_cfg[1], (uint64_t)s_cfg[2] | (uint64_t)s_cfg[3] << 32};
}

// tl_grammar_create_stack: long_m.  grid = (ceil(n_long / 64), n_states), block = 64: lane l of block (x, s) walks long token 64 x + l from
// (s, empty stack), serially, once per grammar, and stores the largest depth reached, or GRS_NO_DEPTH where the walk dies
struct GrammarLongDepthArgs {
    const uint32_t *fused;
    const uint16_t *pop;
    const int32_t *offsets;
    const uint8_t *bytes;
    const int32_t *long_ids;  // [n_long] token ids, ascending
    int n_long;
    uint8_t *out;             // [n_states][n_long]
};
static __global__ __launch_bounds__(64) void grammar_long_depth_kernel(const GrammarLongDepthArgs a) {
    const int li = blockIdx.x * 64 + (int)threadIdx.x, state = blockIdx.y;
    if (li >= a.n_long) return;
    const int j = a.long_ids[li];
    GrsConfig c{state, 0, 0ull};
    int m = 0;
    bool walked = true;
    for (int k = a.offsets[j]; k < a.offsets[j + 1] && walked; ++k) {
        walked = grs_step(a.fused, a.pop, c, a.bytes[k]);
        m = max(m, c.depth);
    }
    a.out[(size_t)state * a.n_long + li] = (uint8_t)(walked ? (uint32_t)m : GRS_NO_DEPTH);
}

// tl_grammar_mask_rows_stack: out[i][j] = logits[i][j] where j is allowed in (states[i], depths[i], stacks[i]), else -inf
struct GrammarStackMaskArgs {
    const GrammarDev *g;
    const uint16_t *logits;
    uint16_t *out;
    const int32_t *states, *depths;
    const uint64_t *stacks;
    int vocab;
};
static __global__ __launch_bounds__(256) void grammar_stack_mask_rows_kernel(const GrammarStackMaskArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_table[GRS_LDS_STATES * 256];
    __shared__ __attribute__((aligned(16))) uint16_t s_pop[GRS_LDS_POPS * 8];
    gr_mask_rows(a.logits, a.out, a.vocab, [&](int row, int c) {
        GrRef g = *GR_GLOBAL(GrammarDev, a.g);
        GrsConfig cfg{a.states[row], 0, 0ull};
        if (cfg.state >= g.n_states || cfg.state < 0) cfg.state = GR_END;  // (never an index past the table)
        if (cfg.state >= 0) cfg.depth = min(max(a.depths[row], 0), GRS_DEPTH), cfg.stack = a.stacks[row] & grs_mask(cfg.depth);
        bool whole, pop_lds;
        grs_stage_tables(g, cfg.state, s_table, s_pop, 256, &whole, &pop_lds);
        return grs_allowed8(g, cfg, c, a.vocab, s_table, s_pop, whole, pop_lds);
    });
}

}  // namespace tl
