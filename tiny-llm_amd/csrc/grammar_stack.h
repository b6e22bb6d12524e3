// Stack grammars (include/tinyllm_engine.h "stack grammars"): the byte-level DFA of grammar.h with a bounded stack
// beside the state -- 32 levels of 2-bit symbols in one uint64 -- which is what nested JSON needs.  A slot's configuration is
// (state, depth, stack).  The third twin of the processing launch (logit_process_stack_kernel, its own plan-key bit) runs when some live
// slot of the step holds a stack grammar; it serves the regex-grammar and grammar-less rows of that step through the very functions of
// the other twins, so those rows come out as they always did.
//
// Device tables: the ABI's table [n_states][256] uint16 and ops [n_states][256] uint8 are FUSED into one uint32 per (state, byte) --
// bits 0-15 the entry (0xFFFF = no transition), bits 16-18 the op -- so a round of the walk is one lookup per chain, as in grammar.h; the
// pop table is padded to 8 uint16 per entry.
// The walk keeps the shape of gr_walk8: a lane walks 8 tokens in lock-step, a round's lookups are issued without a branch.  A chain does
// not carry the 64-bit stack: a token of at most GR_LONG bytes pushes at most 16 symbols and consumes at most 16 levels of the slot's
// stack, so a chain carries what it pushed itself (32 bits), how many symbols of that are live, and how many levels of the slot's stack
// (uniform over the workgroup) it has popped.  The pop lookup depends on the table lookup: it is issued for all 8 chains of a round
// together (a chain that does not pop reads entry 0 and drops it), one more latency per round that pops, not eight.
// Long tokens: one byte per (state, long token), the largest depth the token's walk from (state, empty stack) reaches, 0xFF where that
// walk dies (it then pops below its starting level, or has no transition): allowed iff depth + m <= 32.
#pragma once
#include "logit_process.h"

namespace tl {

constexpr int GRS_DEPTH = 32;               // levels of the stack
constexpr uint32_t GRS_POP = 5;             // op: pop; 1 .. 4 push symbol op - 1; 0 nothing
constexpr int GRS_LDS_STATES = 32;          // automata up to this many states live in LDS whole (32 KB of fused entries: the regex twin's LDS)
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
    uint32_t s = (uint32_t)c.state;
    int d = c.depth;
    uint64_t st = c.stack;
    for (int base = b0; base < b1; base += 64) {
        const uint32_t mine = base + lane < b1 ? bytes[base + lane] : 0u;
        const int n = min(64, b1 - base);
        for (int k = 0; k < n; ++k) {
            const uint32_t b = (uint32_t)__shfl((int)mine, k);
            const uint32_t f = fused[s * 256u + b], t = f & 0xffffu, op = f >> 16;
            if (t == GR_DEAD) return end;
            if (op == 0u) {
                s = t;
            } else if (op < GRS_POP) {
                if (d == GRS_DEPTH) return end;
                st |= (uint64_t)(op - 1u) << (2 * d);
                d += 1;
                s = t;
            } else {
                if (d == 0) return end;
                d -= 1;
                st &= grs_mask(d);
                const uint32_t top = d ? (uint32_t)(st >> (2 * (d - 1))) & 3u : 4u;
                s = pop[t * 8u + top];
                if (s == GR_DEAD) return end;
            }
        }
    }
    return GrsConfig{(int)s, d, st};
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
    int off[9];
    if (c + 8 <= vocab) {
        const auto o4 = reinterpret_cast<const u32x4 __attribute__((address_space(1))) *>(offsets + c);
        const u32x4 a = o4[0], b = o4[1];
        off[0] = a[0], off[1] = a[1], off[2] = a[2], off[3] = a[3], off[4] = b[0], off[5] = b[1], off[6] = b[2], off[7] = b[3];
        off[8] = offsets[c + 8];
    } else {
#pragma unroll
        for (int e = 0; e < 9; ++e) off[e] = offsets[min(c + e, vocab)];
    }
    int len[8];
    uint32_t alive = 0u, ok = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) len[e] = c + e < vocab ? off[e + 1] - off[e] : 0;
    uint32_t is_long = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) is_long |= len[e] > GR_LONG ? 1u << e : 0u;
    if (is_long) {  // rare: the precomputed depth of (state, token); not a chain below
        const auto long_index = GR_GLOBAL(int32_t, g.long_index);
        const auto long_m = GR_GLOBAL(uint8_t, g.long_m) + (size_t)cfg.state * g.n_long;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (!(is_long >> e & 1u)) continue;
            const uint32_t m = long_m[long_index[c + e]];
            ok |= (m != GRS_NO_DEPTH && cfg.depth + (int)m <= GRS_DEPTH ? 1u : 0u) << e;
            len[e] = 0;
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) alive |= len[e] > 0 ? 1u << e : 0u;
    // per chain: the state, what the chain pushed itself (`up` live symbols in `loc`) and how many levels of cfg.stack it has popped
    uint32_t s[8], cur[8], nxt[8], f[8], loc[8], pidx[8], p[8];
    int up[8], below[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0u, loc[e] = 0u, up[e] = 0, below[e] = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) cur[e] = bytes[len[e] > 0 ? off[e] : 0];
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
    // the EOS ids are decided by the state alone (acceptance by final state), as in gr_allowed8
    const bool eos_ok = cfg.state < 0 || GR_GLOBAL(uint8_t, g.accepting)[cfg.state] != 0;
    for (int k = 0; k < g.n_eos; ++k) {
        const int d = g.eos[k] - c;
        if ((unsigned)d < 8u && g.eos[k] < vocab) ok = eos_ok ? (ok | 1u << d) : (ok & ~(1u << d));
    }
    return ok;
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

// the configuration of a row of the processing launch: the slot's record, advanced with the pending token unless the record says it is in
// already; wave 0 does the walk, the row's first workgroup stores the new record (stack word first), everybody gets the result through
// LDS (s_cfg: 4 words).  tokens == nullptr (a prefill's last row): the record as it stands.  Ends with a barrier.
__device__ __forceinline__ GrsConfig grs_row_config(GrRef g, GrammarStackRecord *recs, const int32_t *tokens, const int32_t *context_lens,
                                                    int slot, int vocab, bool store, uint32_t *s_cfg) {
    if (threadIdx.x < 64) {
        GrammarStackRecord *r = recs + slot;
        const uint64_t rec64 = act_load(&r->rec);
        const uint32_t packed = (uint32_t)(rec64 >> 32);
        const int tag = (int)(uint32_t)rec64;
        GrsConfig c{GR_END, 0, 0ull};
        int which = 0;
        if (packed != 0xffffffffu) {
            c.state = (int)(packed & 0xffffu), c.depth = min((int)(packed >> 16 & 0xffu), GRS_DEPTH), which = (int)(packed >> 24 & 1u);
            c.stack = act_load(&r->stack[which]) & grs_mask(c.depth);
        }
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

// The third twin of the processing launch: logit_process_kernel<true> whose rows may also belong to slots with a STACK grammar
// (GrammarDev::kind).  A row without a grammar, or with a regex grammar, runs the code of the other twins.
struct LogitProcessStackArgs {
    LogitProcessArgs base;
    GrammarStackRecord *stack_state;  // [slots]
};
static __global__ __launch_bounds__(LPR_THREADS) void logit_process_stack_kernel(const LogitProcessStackArgs sa) {
    const LogitProcessArgs &a = sa.base;
    __shared__ float s_bias[LPR_CHUNK];
    // the regex rows' uint16 table (GR_LDS_STATES rows) or the stack rows' fused table (GRS_LDS_STATES rows): 32 KB either way
    __shared__ __attribute__((aligned(16))) uint32_t s_table[GRS_LDS_STATES * 256];
    __shared__ __attribute__((aligned(16))) uint16_t s_pop[GRS_LDS_POPS * 8];
    __shared__ int s_state;
    __shared__ uint32_t s_cfg[4];
    static_assert(GRS_LDS_STATES * 256 * 4 >= GR_LDS_STATES * 256 * 2, "s_table holds either table");
    const prof_t prof_t0 = prof_begin(a.prof);
    const int row = blockIdx.y, slot = a.slot0 + row;
    const int c0 = blockIdx.x * LPR_CHUNK, c = c0 + (int)threadIdx.x * 8;
    const uint16_t *lg = a.logits + (long)row * a.vocab;
    uint16_t *out = a.out + (long)row * a.vocab;
    uint16_t *hist = a.history + (long)slot * a.vocab;
    const float r = a.repetition[slot], p = a.presence[slot], f = a.frequency[slot];
    const int nb = min(a.bias_n[slot], LPR_MAX_BIAS);
    const GrammarDev *gp = a.grammar[slot];
    const bool on = r != 1.f || p != 0.f || f != 0.f || nb > 0 || gp != nullptr;  // uniform
    const int32_t *tokens = (a.live && a.live[slot] == 0) ? nullptr : a.tokens;      // uniform (logit_process.h: a frozen slot)
    const bool vec = (((uintptr_t)lg | (uintptr_t)out | (uintptr_t)hist) & 15) == 0 && c + 8 <= a.vocab;
    if (!on) {
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
    for (int k = threadIdx.x; k < nb; k += LPR_THREADS) {
        const int d = a.bias_ids[(long)slot * LPR_MAX_BIAS + k] - c0;
        if ((unsigned)d < (unsigned)LPR_CHUNK) s_bias[d] = a.bias_values[(long)slot * LPR_MAX_BIAS + k];
    }
    __syncthreads();
    uint32_t allowed = 0xffu;
    if (gp) {  // uniform
        GrRef g = *GR_GLOBAL(GrammarDev, gp);
        if (g.kind != 0) {
            const GrsConfig cfg = grs_row_config(g, sa.stack_state, tokens, a.context_lens, slot, a.vocab, blockIdx.x == 0, s_cfg);
            bool whole, pop_lds;
            grs_stage_tables(g, cfg.state, s_table, s_pop, LPR_THREADS, &whole, &pop_lds);
            allowed = grs_allowed8(g, cfg, c, a.vocab, s_table, s_pop, whole, pop_lds);
        } else {
            uint16_t *s_table16 = reinterpret_cast<uint16_t *>(s_table);
            const int state = gr_row_state(g, a.grammar_state, tokens, a.context_lens, slot, a.vocab, blockIdx.x == 0, &s_state);
            const bool whole = gr_stage_table(g, state, s_table16, LPR_THREADS);
            allowed = gr_allowed8(g, state, c, a.vocab, s_table16, whole);
        }
    }
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
        v = (allowed >> e & 1u) ? v : 0xff80u;  // -inf
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
    uint32_t s = (uint32_t)state;
    int d = 0, m = 0;
    uint64_t st = 0ull;
    for (int k = a.offsets[j]; k < a.offsets[j + 1] && s != GR_DEAD; ++k) {
        const uint32_t f = a.fused[s * 256u + a.bytes[k]], t = f & 0xffffu, op = f >> 16;
        if (t == GR_DEAD || op == 0u) {
            s = t;
        } else if (op < GRS_POP) {
            s = d == GRS_DEPTH ? GR_DEAD : t;
            if (s != GR_DEAD) st |= (uint64_t)(op - 1u) << (2 * d), d += 1, m = max(m, d);
        } else if (d == 0) {
            s = GR_DEAD;
        } else {
            d -= 1;
            st &= grs_mask(d);
            s = a.pop[t * 8u + (d ? (uint32_t)(st >> (2 * (d - 1))) & 3u : 4u)];
        }
    }
    a.out[(size_t)state * a.n_long + li] = (uint8_t)(s == GR_DEAD ? GRS_NO_DEPTH : (uint32_t)m);
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
    GrRef g = *GR_GLOBAL(GrammarDev, a.g);
    const int row = blockIdx.y, c = blockIdx.x * 2048 + (int)threadIdx.x * 8;
    GrsConfig cfg{a.states[row], 0, 0ull};
    if (cfg.state >= g.n_states || cfg.state < 0) cfg.state = GR_END;  // (never an index past the table)
    if (cfg.state >= 0) cfg.depth = min(max(a.depths[row], 0), GRS_DEPTH), cfg.stack = a.stacks[row] & grs_mask(cfg.depth);
    bool whole, pop_lds;
    grs_stage_tables(g, cfg.state, s_table, s_pop, 256, &whole, &pop_lds);
    const uint32_t ok = grs_allowed8(g, cfg, c, a.vocab, s_table, s_pop, whole, pop_lds);
    const uint16_t *lg = a.logits + (long)row * a.vocab;
    uint16_t *out = a.out + (long)row * a.vocab;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (c + e < a.vocab) out[c + e] = (ok >> e & 1u) ? lg[c + e] : (uint16_t)0xff80u;
}

}  // namespace tl
