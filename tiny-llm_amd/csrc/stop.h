// Stop conditions on the device (include/tinyllm_engine.h "Stop conditions"): one launch behind the step end --
// behind the Mirostat update where a step has one -- that looks at the token the step end has just committed for every armed slot:
//   1. generated += 1
//   2. the token is one of the set's ids            -> TL_STOP_ID, index = its place in the list; its bytes are no text
//   3. its bytes join the slot's text (where the set has a vocabulary) and, walked through the set's automaton (stop_set.h), end a stop string at byte j (the first such byte)
//                                                   -> TL_STOP_STRING, index = the longest string ending at j, cut = the text before it
//   4. generated == max_new_tokens > 0              -> TL_STOP_LENGTH
// A slot that stops has its `live` word cleared: from the next launch on the step end commits nothing for it, the log-probability record
// and the Mirostat update skip it, and the processing launch counts and advances nothing (logit_process.h tests the word).
//
// grid = rows, block = one wave; row i serves slot slot0 + i.  One struct by value, like every kernel of a decode step.  A slot that is
// unarmed, not live or already stopped leaves after uniform loads.
//
// Long tokens.  Every byte is one dependent load of the table (at most 1,025 x 256 x 2 bytes: it stays in L2).  A token of up to
// STOP_SERIAL bytes is walked by lane 0 alone.  A longer one is cut into 64 segments, one per lane: the automaton's state is the longest
// suffix of the text that starts a stop string, never deeper than the longest string, so a lane that starts at the ROOT max_len - 1
// bytes ahead of its segment -- or at the token's first byte from the slot's own state, where the token begins later than that -- holds
// the true state from its segment's first byte on.  Each lane reports the first match inside its own segment, the wave takes the
// earliest, and the lane that owns the last byte hands the state on.  The dependent chain of an n-byte token is max_len - 1 +
// ceil(n / 64) loads instead of n; where that is no shorter (stop strings as long as the token) lane 0 walks alone.
#pragma once
#include "common.h"

namespace tl {

constexpr int STOP_NONE = 0, STOP_ID = 1, STOP_STRING = 2, STOP_LENGTH = 3;  // TL_STOP_*
constexpr int STOP_SERIAL = 16;

// tl_stop_state: the record of a slot / a row
struct StopRecord {
    int32_t reason, index, generated, context;
    uint32_t text_bytes, cut_bytes;
};

// a stop set on the device (tl_stop; immutable, shared between slots)
struct StopDev {
    const uint16_t *table;      // [n_states][256]; nullptr: no strings
    const int16_t *match;       // [n_states] the longest string ending in the state, -1: none
    const uint16_t *match_len;  // [n_states]
    const int32_t *ids;         // [n_ids]
    const int32_t *offsets;     // the vocabulary's [V + 1] (tl_vocab); nullptr: a set of ids made without one -- its text stays empty
    const uint8_t *bytes;
    int n_ids, max_len, vocab, n_states;
};

struct StopArgs {
    const int32_t *tokens;         // [slots] the token the step end just stored
    int slot0;
    const StopDev *const *sets;    // [slots] the slot's set (nullptr entry: a budget alone); nullptr: `one` serves every row
    const StopDev *one;
    const int32_t *armed;          // [slots] 1 = the slot is armed; nullptr: every row is
    const int32_t *max_new;        // [slots] the budget, 0 = none
    int32_t *automaton;            // [slots] the automaton's state
    StopRecord *rec;               // [slots]
    int32_t *live;                 // [slots] cleared on a stop; nullptr (caller rows): nothing to clear, every row runs
    const int32_t *context_lens;   // [slots] -> the record's context; nullptr: the field is left alone
    prof_t *prof;
};

static __global__ __launch_bounds__(64) void stop_check_kernel(const StopArgs a) {
    const prof_t prof_t0 = prof_begin(a.prof);
    const int slot = a.slot0 + (int)blockIdx.x, lane = threadIdx.x;
    const bool runs = (!a.armed || a.armed[slot] != 0) && (!a.live || a.live[slot] != 0) && a.rec[slot].reason == STOP_NONE;  // uniform
    if (runs) {
        const int token = a.tokens[slot];
        const StopDev *set = a.sets ? a.sets[slot] : a.one;
        StopRecord r = a.rec[slot];
        r.generated += 1;
        if (a.context_lens) r.context = a.context_lens[slot];
        int n_ids = 0, n_bytes = 0, b0 = 0, max_len = 0;
        if (set) {  // uniform
            n_ids = set->n_ids;
            if (set->offsets && token >= 0 && token < set->vocab) {  // (a set made without a vocabulary knows no token's bytes)
                b0 = set->offsets[token];
                n_bytes = set->offsets[token + 1] - b0;
                max_len = set->max_len;
            }
        }
        const unsigned long long hit = __ballot(lane < n_ids && set->ids[lane] == token);
        if (hit) {  // uniform: the ids are distinct, one lane at most
            r.reason = STOP_ID;
            r.index = __ffsll(hit) - 1;
            r.cut_bytes = r.text_bytes;
        } else {
            if (n_bytes > 0 && set->table) {  // uniform
                const uint16_t *table = set->table;
                const int16_t *match = set->match;
                const uint8_t *bytes = set->bytes + b0;
                // segments of `seg` bytes, lane l owns [l seg, (l + 1) seg): the whole token for lane 0 where cutting shortens nothing
                const int cut = (n_bytes + 63) / 64;
                const int seg = (n_bytes > STOP_SERIAL && max_len - 1 + cut < n_bytes) ? cut : n_bytes;
                const int own0 = min(lane * seg, n_bytes), own1 = min(own0 + seg, n_bytes);
                const int from = own0 < own1 ? max(own0 - (max_len - 1), 0) : own1;  // (a lane without a segment walks nothing)
                int state = 0;
                if (from == 0) {  // the slot's own state (a caller row's is the caller's to keep inside the table)
                    state = a.automaton[slot];
                    state = (unsigned)state < (unsigned)set->n_states ? state : 0;
                }
                int first = 0x7fffffff, which = -1;
                for (int k = from; k < own1; ++k) {
                    state = table[(long)state * 256 + bytes[k]];
                    if (k >= own0 && match[state] >= 0) {
                        first = k, which = state;
                        break;
                    }
                }
                // the earliest byte at which a string ends, over the lanes (positions are below 2^24: exact as floats)
                const int earliest = (int)-wave_max(first == 0x7fffffff ? -3.0e7f : -(float)first);
                if (earliest < n_bytes) {
                    const unsigned long long owner = __ballot(first == earliest);
                    const int st = __builtin_amdgcn_readlane(which, __ffsll(owner) - 1);
                    r.reason = STOP_STRING;
                    r.index = match[st];
                    r.cut_bytes = r.text_bytes + (uint32_t)(earliest + 1) - (uint32_t)set->match_len[st];
                } else {
                    const int last = (n_bytes - 1) / seg;  // the lane that owns the last byte
                    const int st = __builtin_amdgcn_readlane(state, last);
                    if (lane == 0) a.automaton[slot] = st;
                }
            }
            r.text_bytes += (uint32_t)n_bytes;
            if (r.reason == STOP_NONE) {
                r.cut_bytes = r.text_bytes;
                const int budget = a.max_new[slot];
                if (budget > 0 && r.generated == budget) r.reason = STOP_LENGTH, r.index = 0;
            }
        }
        if (lane == 0) {
            a.rec[slot] = r;
            if (r.reason != STOP_NONE && a.live) a.live[slot] = 0;
        }
    }
    prof_end(a.prof, prof_t0);
}

}  // namespace tl
