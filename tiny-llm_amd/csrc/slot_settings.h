// The engine's per-slot settings (include/tinyllm_engine.h; DESIGN.md "The slot settings"): the second half of the slot protocol, beside
// slot_table.h.  Host only, no HIP include and no device pointer dereferenced: engine.hip calls it and applies the edits it reports to
// the device, and tests/slot_settings_model_check.cpp drives the same code alone against byte arrays that stand for the device.
//
//   state     one State per batch slot: the host mirrors of sampling, log-probability records, penalties / bias / grammar / DRY, truncation
//             and Mirostat, the LoRA adapter id and the stop conditions, and three host-only flags (the pending token, the rows of a
//             running mean, parked).  The device copy of a live unparked slot follows its mirror; a parked slot's processing
//             parameters are neutral on the device, because the processing launch reads them whatever the `live` word says.
//   blocks    every feature's device arrays live in one lazily allocated block (the sampling block is made with the engine, the
//             adapter ids lie inside the LoRA block).  layout(b) is the block's size and how a fresh one is filled, `at` the offset of
//             every array.  A call that needs a block says so in SettingsEdits::needs; the caller allocates it and calls created(b).
//   calls     every operation is all-or-nothing.  It returns nullptr, or the refusal's message with nothing changed.
//   edits     a served call APPENDS what the device must learn, in the order the engine stream must see it: words (the caller pokes
//             consecutive ones together), copies inside a block, fills and uploads from the mirror.  Within one call no word is
//             written twice, so the words between two other edits may share a launch.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace tl {

enum SettingsBlock { SB_SAMPLE, SB_LOGPROB, SB_PROCESS, SB_GRAMMAR, SB_STACK, SB_TRUNC, SB_STOP, SB_LORA, SB_DRY, SB_LOOKUP, SB_COUNT };

// temperature 0 = greedy (the default, and what begin / release restore)
struct SampleParams {
    float temperature = 0.f;
    int top_k = 0;
    float top_p = 0.f;
    uint64_t seed = 0;
    bool samples() const { return temperature > 0.f; }
    bool is_default() const { return temperature == 0.f && top_k == 0 && top_p == 0.f && seed == 0; }
};
// a grammar / a stop set as the record needs it: the device address a slot's pointer is written to and the caller's identity of it
struct GrammarRef {
    uint64_t dev = 0;
    bool stack = false;
    int start = 0;
    const void *id = nullptr;  // null: no grammar
    explicit operator bool() const { return id != nullptr; }
};
struct StopRef {
    uint64_t dev = 0;
    const void *id = nullptr;  // null: no set (a budget alone)
};
struct PenaltyParams {
    float repetition = 1.f, presence = 0.f, frequency = 0.f;
    std::vector<int32_t> bias_ids;
    std::vector<float> bias_values;
    GrammarRef grammar;
    // DRY and the n-gram ban (dry.h): multiplier 0 = DRY off, ngram 0 = no ban; s0: the context length the slot had when it was armed
    float dry_multiplier = 0.f, dry_base = 1.75f;
    int dry_allowed = 2, dry_range = 0, ngram = 0, dry_s0 = 0;
    std::vector<int32_t> dry_breakers;
    bool dry_on() const { return dry_multiplier > 0.f || ngram > 0; }
    bool dry_same(const PenaltyParams &o) const {
        return dry_multiplier == o.dry_multiplier && dry_base == o.dry_base && dry_allowed == o.dry_allowed && dry_range == o.dry_range &&
               ngram == o.ngram && dry_s0 == o.dry_s0 && dry_breakers == o.dry_breakers;
    }
    bool processes() const { return repetition != 1.f || presence != 0.f || frequency != 0.f || !bias_ids.empty() || grammar || dry_on(); }
};
struct TruncParams {
    float min_p = 0.f, typical_p = 1.f, tau = 0.f, eta = 0.f;
    bool stateless() const { return min_p > 0.f || (typical_p > 0.f && typical_p < 1.f); }
    bool mirostat() const { return tau > 0.f; }
    bool truncates() const { return stateless() || mirostat(); }
};
struct StopSlot {
    StopRef set;
    int max_new = 0;
    bool armed = false;
};
// the device's stop record (stop.h StopRecord, tl_stop_state) as the host reads it
struct StopMirror {
    int32_t reason = 0, index = 0, generated = 0, context = 0;
    uint32_t text_bytes = 0, cut_bytes = 0;
};

// which launches a step over some slots needs: the per-slot predicates ORed (SlotSettings::features; the engine keys its plans by them)
struct StepFeatures {
    bool samples = false, logprobs = false, processes = false, grammar = false, stack_grammar = false, truncates = false, mirostat = false,
         lora = false, stop = false, dry = false;
};

struct SettingsEdit {
    enum Kind { WORD, COPY, FILL, UPLOAD } kind;
    int block;
    size_t off;        // where, inside the block
    int32_t word;      // WORD: the value
    size_t from;       // COPY: the source, inside the same block
    size_t bytes;      // COPY, FILL (zeros), UPLOAD
    const void *host;  // UPLOAD: an array of the mirror (it outlives the copy)
};
struct SettingsEdits {
    std::vector<SettingsEdit> list;
    unsigned needs = 0;  // bit b: block b must exist before the list is applied
    void clear() {
        list.clear();
        needs = 0;
    }
};

// every 32-bit word of [off, off + bytes) of a fresh block starts as `word`; bytes no rule covers start undefined (rows and rings that
// are written before they are read)
struct BlockFill {
    size_t off, bytes;
    uint32_t word;
};
struct BlockLayout {
    size_t bytes = 0;
    std::vector<BlockFill> fill;  // in order: a later rule overwrites an earlier one
};

class SlotSettings {
  public:
    // sizes that come from the device headers (engine.hip ties them to the structs the kernels use)
    struct Sizes {
        int slots, vocab, ring_cap;
        int lp_record_words, lp_max_top;               // logprob.h
        int max_bias;                                  // logit_process.h
        int grammar_record_bytes, stack_record_bytes;  // grammar.h, grammar_stack.h: {tag, state, ...} / {rec (tag in the low word), ...}
        int stop_record_bytes;                         // stop.h
        int sampler_max_vocab;                         // sample.h
        int lora_none;                                 // lora_tiles.h
        // (appended; zero: the feature is absent)
        int dry_seq_cap = 0;       // ids a slot's sequence row holds (max_pages_per_seq * page_size); 0: no DRY / n-gram ban on this engine
        int dry_max_breakers = 0;  // dry.h
        int dry_max_match = 0;
        int lookup_seq_cap = 0;   // ids a slot's lookup history row holds (max_pages_per_seq * page_size); 0: no prompt lookup on this engine
        int lookup_out_words = 0;  // lookup.h: the words one propose launch leaves for the host
    };
    struct State {
        SampleParams smp;
        int lp_n = -1, lp_from = 0;  // top-N (-1: off); the slot's `produced` when its records began
        PenaltyParams pen;
        TruncParams trn;
        int lora = -1;
        StopSlot stop;
        StopMirror stop_host;    // the record as the last reconciliation read it
        bool gr_pending = false;  // the slot holds a pending token no step has consumed yet
        bool parked = false;
        int emb_rows = -1;  // rows the slot's running mean holds (pool.h), -1: none
        // prompt lookup (lookup.h): the slot keeps its ordered ids H on the device.  H[j] is known for lk_s0 <= j < lk_rec; the ids of the
        // decode steps since (positions lk_rec .. ctx - 1) still lie in the token ring and are fetched by a catch-up
        bool lookup = false;
        int lk_s0 = 0, lk_rec = 0;
    };
    // byte offsets of every array inside its block, [slots] entries each unless said otherwise
    struct Offsets {
        size_t smp_seed, smp_temp, smp_topk, smp_topp;
        size_t lp_topn, lp_pending, lp_ring;  // records: [slots] pending, [slots, ring_cap] ring
        size_t pen_history, pen_rows, pen_rep, pen_pres, pen_freq, pen_bias_n, pen_bias_ids, pen_bias_values;  // [slots, vocab]; [max(slots, 8), vocab]
        size_t gr_ptr, gr_state;
        size_t trn_rows, trn_minp, trn_tau, trn_eta, trn_logsum, trn_typ, trn_mu;  // [max(slots, 8), vocab]; logsum [max(slots, 8)]
        size_t stop_sets, stop_armed, stop_max_new, stop_automaton, stop_rec;
        size_t dry_seq, dry_table, dry_mult, dry_base, dry_allowed, dry_range, dry_ngram, dry_s0, dry_nbreak, dry_breakers;  // [slots, dry_seq_cap]; [slots, vocab]; ...; [slots, dry_max_breakers]
        size_t lk_seq, lk_out;  // [slots, lookup_seq_cap]; [lookup_out_words]
    };
    std::vector<State> slots;
    Offsets at{};
    Sizes sz{};

    void init(const Sizes &sizes) {
        sz = sizes;
        slots.assign(sz.slots, State{});
        for (State &s : slots) s.lora = sz.lora_none;
        exists_ = 0;
        const size_t B = (size_t)sz.slots, R = std::max<size_t>(B, 8), V = (size_t)sz.vocab, rec = (size_t)sz.lp_record_words * 4;
        const uint32_t ones = 0xffffffffu, one_f = bits(1.0f);
        // sampling: all zero (greedy); seeds first for their 8-byte alignment
        at.smp_seed = 0, at.smp_temp = B * 8, at.smp_topk = B * 12, at.smp_topp = B * 16;
        layouts_[SB_SAMPLE] = {B * 20, {{0, B * 20, 0}}};
        // log-probabilities: all ones -- top-N -1 (off), and a pending record nobody wrote reads as logprob NaN with ids -1
        at.lp_topn = 0, at.lp_pending = B * 4, at.lp_ring = B * 4 + B * rec;
        layouts_[SB_LOGPROB] = {B * 4 + (B * (size_t)sz.ring_cap + B) * rec, {{0, B * 4 + B * rec, ones}}};
        // processing: everything zero (empty histories, presence / frequency 0, empty lists) but the repetition penalties: 1
        size_t off = 0;
        at.pen_history = carve(off, B * V * 2), at.pen_rows = carve(off, R * V * 2), at.pen_rep = carve(off, B * 4), at.pen_pres = carve(off, B * 4);
        at.pen_freq = carve(off, B * 4), at.pen_bias_n = carve(off, B * 4), at.pen_bias_ids = carve(off, B * sz.max_bias * 4);
        at.pen_bias_values = carve(off, B * sz.max_bias * 4);
        layouts_[SB_PROCESS] = {off, {{0, off, 0}, {at.pen_rep, B * 4, one_f}}};
        // grammars: the automaton pointers and the state records, zero; a stack grammar's records in a block of their own
        at.gr_ptr = 0, at.gr_state = B * 8;
        layouts_[SB_GRAMMAR] = {B * (8 + (size_t)sz.grammar_record_bytes), {{0, B * (8 + (size_t)sz.grammar_record_bytes), 0}}};
        layouts_[SB_STACK] = {B * (size_t)sz.stack_record_bytes, {{0, B * (size_t)sz.stack_record_bytes, 0}}};
        // truncation: zero (min-p, tau, eta off) up to the typical-p array; typical-p and mu all ones, a NaN (typical-p off, no Mirostat)
        off = 0;
        at.trn_rows = carve(off, R * V * 2), at.trn_minp = carve(off, B * 4), at.trn_tau = carve(off, B * 4), at.trn_eta = carve(off, B * 4);
        at.trn_logsum = carve(off, R * 4), at.trn_typ = carve(off, B * 4), at.trn_mu = carve(off, B * 4);
        layouts_[SB_TRUNC] = {off, {{0, at.trn_typ, 0}, {at.trn_typ, off - at.trn_typ, ones}}};
        // stop conditions: all zero (unarmed, no budget, automaton at the root, empty records)
        off = 0;
        at.stop_sets = carve(off, B * 8), at.stop_armed = carve(off, B * 4), at.stop_max_new = carve(off, B * 4);
        at.stop_automaton = carve(off, B * 4), at.stop_rec = carve(off, B * (size_t)sz.stop_record_bytes);
        layouts_[SB_STOP] = {off, {{0, off, 0}}};
        // the adapter ids inside the LoRA block: all none
        layouts_[SB_LORA] = {B * 4, {{0, B * 4, ones}}};
        // DRY and the n-gram ban: the table and every parameter zero (off); the sequence rows are written before they are read
        off = 0;
        at.dry_seq = carve(off, B * (size_t)sz.dry_seq_cap * 4), at.dry_table = carve(off, sz.dry_seq_cap ? B * V * 4 : 0);
        at.dry_mult = carve(off, B * 4), at.dry_base = carve(off, B * 4), at.dry_allowed = carve(off, B * 4), at.dry_range = carve(off, B * 4);
        at.dry_ngram = carve(off, B * 4), at.dry_s0 = carve(off, B * 4), at.dry_nbreak = carve(off, B * 4);
        at.dry_breakers = carve(off, B * (size_t)sz.dry_max_breakers * 4);
        layouts_[SB_DRY] = {sz.dry_seq_cap ? off : 0, {{at.dry_table, off - at.dry_table, 0}}};
        // prompt lookup: the history rows and the results of one propose launch, all written before they are read
        off = 0;
        at.lk_seq = carve(off, B * (size_t)sz.lookup_seq_cap * 4), at.lk_out = carve(off, (size_t)sz.lookup_out_words * 4);
        layouts_[SB_LOOKUP] = {sz.lookup_seq_cap ? off : 0, {}};
    }
    const BlockLayout &layout(int b) const { return layouts_[b]; }
    bool exists(int b) const { return exists_ >> b & 1u; }
    void created(int b) { exists_ |= 1u << b; }

    // ---- the setters ------------------------------------------------------------------------------------------------------------
    const char *set_sampling(int slot, float temperature, int top_k, float top_p, uint64_t seed, SettingsEdits &ed) {
        if (!(std::isfinite(temperature) && temperature >= 0.f)) return "engine_set_sampling: temperature must be finite and >= 0";
        if (top_k < 0) return "engine_set_sampling: top_k must be >= 0 (0 = no top-k)";
        if (std::isnan(top_p)) return "engine_set_sampling: top_p is NaN";
        if (temperature != 0.f && sz.vocab > sz.sampler_max_vocab) return "engine_set_sampling: vocabulary larger than the sampler's 524,288 tokens";
        SampleParams v;
        v.temperature = temperature;
        v.top_k = top_k >= sz.vocab ? 0 : top_k;             // beyond the vocabulary: no top-k
        v.top_p = top_p > 0.f && top_p < 1.f ? top_p : 0.f;  // outside (0, 1): no top-p
        v.seed = seed;
        if (slots[slot].trn.mirostat() && (v.top_k != 0 || v.top_p != 0.f)) return "engine_set_sampling: the slot has Mirostat on, which excludes top-k and top-p";
        smp_write(slot, v, ed);
        return nullptr;
    }
    const char *set_truncation(int slot, float min_p, float typical_p, SettingsEdits &ed) {
        if (!(min_p >= 0.f && min_p <= 1.f)) return "engine_set_truncation: min_p must be in [0, 1] (0 = off)";
        if (std::isnan(typical_p)) return "engine_set_truncation: typical_p is NaN";
        if (sz.vocab > sz.sampler_max_vocab) return "engine_set_truncation: vocabulary larger than the sampler's 524,288 tokens";
        TruncParams v = slots[slot].trn;
        v.min_p = min_p;
        v.typical_p = typical_p > 0.f && typical_p < 1.f ? typical_p : 1.f;  // outside (0, 1): off
        if (v.mirostat() && v.stateless()) return "engine_set_truncation: the slot has Mirostat on, which excludes min-p and typical-p";
        trn_write(slot, v, false, ed);
        return nullptr;
    }
    const char *set_mirostat(int slot, float tau, float eta, SettingsEdits &ed) {
        if (!(std::isfinite(tau) && tau >= 0.f)) return "engine_set_mirostat: tau must be finite and >= 0 (0 = off)";
        if (tau != 0.f && !(eta > 0.f && eta <= 1.f)) return "engine_set_mirostat: eta must be in (0, 1]";
        if (sz.vocab > sz.sampler_max_vocab) return "engine_set_mirostat: vocabulary larger than the sampler's 524,288 tokens";
        TruncParams v = slots[slot].trn;
        if (tau > 0.f && (v.stateless() || slots[slot].smp.top_k != 0 || slots[slot].smp.top_p != 0.f))
            return "engine_set_mirostat: Mirostat excludes every other truncation of the slot (top-k, top-p, min-p, typical-p)";
        v.tau = tau, v.eta = tau > 0.f ? eta : 0.f;
        trn_write(slot, v, true, ed);  // mu restarts at 2 tau
        return nullptr;
    }
    const char *set_penalties(int slot, float repetition, float presence, float frequency, SettingsEdits &ed) {
        if (!(std::isfinite(repetition) && repetition > 0.f)) return "engine_set_penalties: repetition_penalty must be finite and > 0 (1 = off)";
        if (!(std::isfinite(presence) && std::isfinite(frequency))) return "engine_set_penalties: presence_penalty and frequency_penalty must be finite (0 = off)";
        if (sz.vocab > sz.sampler_max_vocab) return "engine_set_penalties: vocabulary larger than 524,288 tokens";
        PenaltyParams v = slots[slot].pen;
        v.repetition = repetition, v.presence = presence, v.frequency = frequency;
        pen_write(slot, v, ed);
        return nullptr;
    }
    const char *set_logit_bias(int slot, const int32_t *ids, const float *values, int n, SettingsEdits &ed) {
        if (n < 0 || n > sz.max_bias) return "engine_set_logit_bias: between 0 and TL_MAX_LOGIT_BIAS (1,024) entries";
        if (n != 0 && !(ids && values)) return "engine_set_logit_bias: null argument";
        if (sz.vocab > sz.sampler_max_vocab) return "engine_set_logit_bias: vocabulary larger than 524,288 tokens";
        PenaltyParams v = slots[slot].pen;
        v.bias_ids.assign(ids, ids + n);
        v.bias_values.assign(values, values + n);
        std::vector<int32_t> sorted(v.bias_ids);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 0; i < n; ++i) {
            if (sorted[i] < 0 || sorted[i] >= sz.vocab) return "engine_set_logit_bias: token id out of range";
            if (i != 0 && sorted[i] == sorted[i - 1]) return "engine_set_logit_bias: a token id appears twice";
            if (!(std::isfinite(values[i]) || values[i] == -INFINITY)) return "engine_set_logit_bias: values must be finite or -inf";
        }
        pen_write(slot, v, ed);
        return nullptr;
    }
    // ctx: the slot's context length (slot_table.h).  Changing parameters of an armed slot keeps s0 and the sequence; switching
    // everything off and on again makes s0 the current context length
    const char *set_dry(int slot, float multiplier, float base, int allowed_length, int range, int no_repeat_ngram, const int32_t *breakers, int n_breakers,
                        int ctx, SettingsEdits &ed) {
        if (!(std::isfinite(multiplier) && multiplier >= 0.f)) return "engine_set_dry: multiplier must be finite and >= 0 (0 = off)";
        if (!(std::isfinite(base) && base >= 1.f)) return "engine_set_dry: base must be finite and >= 1";
        if (allowed_length < 1) return "engine_set_dry: allowed_length must be >= 1";
        if (range < 0) return "engine_set_dry: range must be >= 0 (0 = the whole recorded sequence)";
        if (no_repeat_ngram != 0 && (no_repeat_ngram < 2 || no_repeat_ngram > sz.dry_max_match)) return "engine_set_dry: no_repeat_ngram must be 0 (off) or 2 .. 64";
        if (n_breakers < 0 || n_breakers > sz.dry_max_breakers) return "engine_set_dry: between 0 and TL_MAX_DRY_BREAKERS (64) breakers";
        if (n_breakers != 0 && !breakers) return "engine_set_dry: null argument";
        if (sz.vocab > sz.sampler_max_vocab) return "engine_set_dry: vocabulary larger than 524,288 tokens";
        if (sz.dry_seq_cap <= 0) return "engine_set_dry: this engine holds no sequence rows";
        PenaltyParams v = slots[slot].pen;
        v.dry_breakers.assign(breakers, breakers + n_breakers);
        std::vector<int32_t> sorted(v.dry_breakers);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 0; i < n_breakers; ++i) {
            if (sorted[i] < 0 || sorted[i] >= sz.vocab) return "engine_set_dry: breaker id out of range";
            if (i != 0 && sorted[i] == sorted[i - 1]) return "engine_set_dry: a breaker id appears twice";
        }
        const bool was = v.dry_on();
        v.dry_multiplier = multiplier, v.dry_base = base, v.dry_allowed = allowed_length, v.dry_range = range, v.ngram = no_repeat_ngram;
        if (!v.dry_on()) {  // off: the defaults, so that two switched-off slots compare equal
            const PenaltyParams d{};
            v.dry_base = d.dry_base, v.dry_allowed = d.dry_allowed, v.dry_range = d.dry_range, v.dry_s0 = 0, v.dry_breakers.clear();
        } else if (!was) {
            v.dry_s0 = ctx;
        }
        pen_write(slot, v, ed);
        return nullptr;
    }
    // ---- prompt lookup (lookup.h): the host half of the history's accounting ---------------------------------------------------------
    // ctx: the slot's context length.  Arming an armed slot changes nothing; arming makes s0 = ctx and the caller records the pending
    // token at H[ctx] (lookup_pending).  Switching off forgets the history
    const char *set_lookup(int slot, bool on, int ctx, SettingsEdits &ed) {
        State &s = slots[slot];
        if (!on) {
            s.lookup = false, s.lk_s0 = s.lk_rec = 0;
            return nullptr;
        }
        if (sz.lookup_seq_cap <= 0) return "engine_set_lookup: this engine holds no history rows";
        if (sz.lookup_seq_cap > (1 << 24)) return "engine_set_lookup: sequences longer than 16,777,216 tokens (the match key holds 24 bits of position)";
        ed.needs |= 1u << SB_LOOKUP;
        if (!s.lookup) s.lookup = true, s.lk_s0 = s.lk_rec = ctx;
        return nullptr;
    }
    bool lookup_on(int slot) const { return slots[slot].lookup; }
    // is H short of the context?  (then the ids of positions lk_rec .. ctx - 1 are the ring's: the caller launches the catch-up)
    bool lookup_behind(int slot, int ctx) const { return slots[slot].lookup && slots[slot].lk_rec < ctx; }
    // the catch-up for context length ctx is on the stream
    void lookup_caught_up(int slot, int ctx) {
        if (slots[slot].lookup) slots[slot].lk_rec = std::max(slots[slot].lk_rec, ctx);
    }
    // ids for positions start .. start + n - 1 were recorded from an upload (the slot was caught up to `start` first)
    void lookup_recorded(int slot, int start, int n) {
        if (slots[slot].lookup) slots[slot].lk_rec = start + n;
    }
    // the pending token was stored at H[ctx] (arming, set_token, a fork's or move's destination): the ring does not hold it
    void lookup_pending(int slot, int ctx) {
        if (slots[slot].lookup) slots[slot].lk_rec = ctx + 1;
    }
    // the slot was rewound from context length `from` to ctx (behind a catch-up): what lay behind ctx is forgotten.  True: the pending
    // token had been stored at H[from] -- the ring may not hold it -- and the caller stores it again, at H[ctx]
    bool lookup_rewound(int slot, int from, int ctx) {
        State &s = slots[slot];
        if (!s.lookup) return false;
        const bool stored = s.lk_rec == from + 1;
        s.lk_s0 = std::min(s.lk_s0, ctx), s.lk_rec = std::min(s.lk_rec, ctx);
        return stored;
    }
    // does a step feed the slot a token the ring does not hold and H does not either?  (a prefill without a first token leaves whatever
    // tokens[slot] held: the caller stores it at H[ctx] ahead of the step, as tl_engine_set_token would have)
    bool lookup_pending_unknown(int slot, int ctx) const { return slots[slot].lookup && slots[slot].lk_rec <= ctx && !slots[slot].gr_pending; }
    // A decode call of `steps` steps is about to run on the slot at context length ctx.  The ring holds ring_cap ids, the last of them
    // the pending token: a catch-up reaches back ring_cap - 1 positions
    enum LookupDecode { LOOKUP_KEEP, LOOKUP_CATCH_UP, LOOKUP_RESTART };
    LookupDecode lookup_before_decode(int slot, int ctx, long steps) const {
        const State &s = slots[slot];
        if (!s.lookup) return LOOKUP_KEEP;
        if (steps > sz.ring_cap - 1) return LOOKUP_RESTART;  // the call alone outruns the ring: the history starts over behind it
        const int behind = std::max(ctx - s.lk_rec, 0);
        return behind + steps > sz.ring_cap - 1 ? LOOKUP_CATCH_UP : LOOKUP_KEEP;
    }
    // ... after such a call: the history is empty at the context length the call left
    void lookup_restart(int slot, int ctx) {
        if (slots[slot].lookup) slots[slot].lk_s0 = slots[slot].lk_rec = ctx;
    }

    // (the caller has checked the grammar's vocabulary)  The same automaton again: back to its start state
    const char *set_grammar(int slot, const GrammarRef &g, SettingsEdits &ed) {
        PenaltyParams v = slots[slot].pen;
        const bool same = g && v.grammar.id == g.id;
        v.grammar = g;
        pen_write(slot, v, ed);
        if (same) gr_state_words(slot, g, ed);
        return nullptr;
    }
    // `produced`: the ids the slot has produced (slot_table.h): records begin with the next one
    const char *set_logprobs(int slot, int top_n, int produced, SettingsEdits &ed) {
        if (top_n < -1 || top_n > sz.lp_max_top) return "engine_set_logprobs: top_n must be -1 (off) or 0 .. 20";
        if (top_n >= 0 && sz.vocab > sz.sampler_max_vocab) return "engine_set_logprobs: vocabulary larger than the routine's 524,288 tokens";
        lp_write(slot, top_n, produced, ed);
        return nullptr;
    }
    // (the caller has checked residency and that the slot holds no tokens)
    const char *set_lora(int slot, int adapter, SettingsEdits &ed) {
        lora_write(slot, adapter, ed);
        return nullptr;
    }
    // (the caller has checked the set's vocabulary and read what an earlier stop launch decided)  The call always restarts the record
    const char *set_stop(int slot, const StopRef &set, int max_new, SettingsEdits &ed) {
        if (max_new < 0) return "engine_set_stop: max_new_tokens must be nonnegative (0 = no budget)";
        const bool arm = set.id != nullptr || max_new > 0;
        if (!arm && !exists(SB_STOP)) return nullptr;  // disarming on an engine that never armed a slot: nothing to write
        ed.needs |= 1u << SB_STOP;
        slots[slot].stop = StopSlot{set, max_new, arm};
        slots[slot].stop_host = StopMirror{};
        stop_words(slot, ed);
        return nullptr;
    }

    // ---- the lifecycle ----------------------------------------------------------------------------------------------------------
    // begin / release: everything back to the defaults (each skipped while it is the default already)
    void reset(int slot, SettingsEdits &ed) {
        State &s = slots[slot];
        s.gr_pending = false, s.parked = false, s.emb_rows = -1;
        s.lookup = false, s.lk_s0 = s.lk_rec = 0;
        lp_write(slot, -1, 0, ed);
        if (s.pen.processes()) pen_write(slot, PenaltyParams{}, ed);
        trn_reset(slot, ed);
        lora_write(slot, sz.lora_none, ed);
        stop_reset(slot, ed);
        if (!s.smp.is_default()) smp_write(slot, SampleParams{}, ed);
    }
    // fork / move (move = true), after the table's: dst takes what src has -- parameters, and on the device the history row, the grammar
    // record, mu, the pending logprob record, the stop automaton and record -- and a move leaves src at the defaults.  A moved parked
    // sequence stays parked at dst.  The pending token travels, a running mean does not: the context of dst did not come from MEAN
    // chunks of its own.  (The seed travels too: give a fork's child its own, or both draw the same tokens.)
    void carry(int src, int dst, bool move, SettingsEdits &ed) {
        State &s = slots[src], &d = slots[dst];
        d.gr_pending = s.gr_pending, d.emb_rows = -1, d.parked = move && s.parked;
        if (move) s.gr_pending = false, s.emb_rows = -1, s.parked = false;
        if (!s.smp.is_default() || !d.smp.is_default()) {
            smp_write(dst, SampleParams(s.smp), ed);
            if (move) smp_write(src, SampleParams{}, ed);
        }
        if (exists(SB_LOGPROB)) {  // the setting with the pending token's record (the record ring restarts, like the token ring)
            lp_write(dst, s.lp_n, 0, ed);
            d.lp_from = 0;  // dst's `produced` restarts at 0 with the sequence
            const size_t rec = (size_t)sz.lp_record_words * 4;
            ed.list.push_back({SettingsEdit::COPY, SB_LOGPROB, at.lp_pending + dst * rec, 0, at.lp_pending + src * rec, rec, nullptr});
            if (move) lp_write(src, -1, 0, ed);
        }
        if (s.pen.processes() || d.pen.processes()) {
            const PenaltyParams v = s.pen;
            pen_write(dst, v, ed);  // (a dst that starts to process has its history row cleared ahead of the copy)
            const size_t V = (size_t)sz.vocab;
            if (v.processes()) ed.list.push_back({SettingsEdit::COPY, SB_PROCESS, at.pen_history + dst * V * 2, 0, at.pen_history + src * V * 2, V * 2, nullptr});
            if (v.dry_on()) {  // the sequence row travels too (the table is all zeros between steps)
                const size_t row = (size_t)sz.dry_seq_cap * 4;
                ed.list.push_back({SettingsEdit::COPY, SB_DRY, at.dry_seq + dst * row, 0, at.dry_seq + src * row, row, nullptr});
            }
            if (v.grammar) {  // the automaton state travels like the history
                const int b = v.grammar.stack ? SB_STACK : SB_GRAMMAR;
                const size_t r = (size_t)(v.grammar.stack ? sz.stack_record_bytes : sz.grammar_record_bytes), o = v.grammar.stack ? 0 : at.gr_state;
                ed.list.push_back({SettingsEdit::COPY, b, o + dst * r, 0, o + src * r, r, nullptr});
            }
            if (move && slots[src].pen.processes()) pen_write(src, PenaltyParams{}, ed);
        }
        if (s.trn.truncates() || d.trn.truncates()) {
            trn_write(dst, TruncParams(s.trn), false, ed);  // mu is the source's
            ed.list.push_back({SettingsEdit::COPY, SB_TRUNC, at.trn_mu + dst * 4, 0, at.trn_mu + src * 4, 4, nullptr});
            if (move) trn_reset(src, ed);
        }
        if (exists(SB_STOP) && (s.stop.armed || d.stop.armed)) {  // (the table carried `stopped`)
            d.stop = s.stop;
            d.stop_host = s.stop_host;
            word64(SB_STOP, at.stop_sets + dst * 8, d.stop.set.dev, ed);
            word(SB_STOP, at.stop_armed + dst * 4, d.stop.armed ? 1 : 0, ed);
            word(SB_STOP, at.stop_max_new + dst * 4, d.stop.max_new, ed);
            const size_t r = (size_t)sz.stop_record_bytes;
            ed.list.push_back({SettingsEdit::COPY, SB_STOP, at.stop_automaton + dst * 4, 0, at.stop_automaton + src * 4, 4, nullptr});
            ed.list.push_back({SettingsEdit::COPY, SB_STOP, at.stop_rec + dst * r, 0, at.stop_rec + src * r, r, nullptr});
            if (move) stop_reset(src, ed);
        }
        lora_write(dst, s.lora, ed);
        if (move) lora_write(src, sz.lora_none, ed);
        if (s.lookup) {  // the history row travels (the caller caught src up first and records dst's pending token behind this)
            const size_t row = (size_t)sz.lookup_seq_cap * 4;
            ed.list.push_back({SettingsEdit::COPY, SB_LOOKUP, at.lk_seq + dst * row, 0, at.lk_seq + src * row, row, nullptr});
        }
        d.lookup = s.lookup, d.lk_s0 = s.lk_s0, d.lk_rec = s.lk_rec;
        if (move) s.lookup = false, s.lk_s0 = s.lk_rec = 0;
    }
    // park / unpark, after the table's.  The processing launch of a step reads a row's parameters whatever the row's `live` word says,
    // and a row that processes counts its pending token and advances its grammar record: a parked slot keeps its pending token, so its
    // device parameters go neutral while it is parked and come back from the mirror with unpark.  The bias entries, the history row
    // and the grammar record are not touched either way.
    void park(int slot, SettingsEdits &ed) {
        slots[slot].parked = true, slots[slot].emb_rows = -1;
        if (slots[slot].pen.processes()) processing_words(slot, false, ed);
    }
    void unpark(int slot, SettingsEdits &ed) {
        slots[slot].parked = false, slots[slot].emb_rows = -1;
        if (slots[slot].pen.processes()) processing_words(slot, true, ed);
    }
    // a beam step (after the table's): slot slot0 + i takes the adapter and the pending flag of slot0 + parents[i], i < width; the slots
    // behind the new width are free
    void beam_reorder(int slot0, int n_src, int width, const int *parents, SettingsEdits &ed) {
        int lora[64];
        bool pending[64];
        for (int i = 0; i < n_src; ++i) lora[i] = slots[slot0 + i].lora, pending[i] = slots[slot0 + i].gr_pending;
        for (int i = 0; i < std::max(n_src, width); ++i) {
            slots[slot0 + i].gr_pending = i < width && pending[parents[i]];
            slots[slot0 + i].emb_rows = -1;
            lora_write(slot0 + i, i < width ? lora[parents[i]] : sz.lora_none, ed);
        }
    }

    // ---- the two flags ----------------------------------------------------------------------------------------------------------
    // tokens were appended behind the slot's context: a pending token that is prefilled past is never fed.  keeps_mean: the pass may
    // be an embedding's chunk, which continues the running mean itself (mean_rows)
    void appended(int slot, bool keeps_mean) {
        slots[slot].gr_pending = false;
        if (!keeps_mean) slots[slot].emb_rows = -1;
    }
    void rewound(int slot) { slots[slot].emb_rows = -1; }
    void pending_produced(int slot) { slots[slot].gr_pending = true; }

    // ---- what other calls ask -----------------------------------------------------------------------------------------------------
    const char *refuses_rewind(int slot) const {
        if (slots[slot].pen.processes()) return "engine_rewind: the slot processes its logits (its history would keep the dropped tokens; make it neutral first)";
        if (slots[slot].trn.mirostat()) return "engine_rewind: the slot has Mirostat on (mu would no longer belong to the tokens held; switch it off first)";
        return nullptr;
    }
    const char *refuses_set_token(int slot) const {
        if (slots[slot].pen.processes()) return "engine_set_token: the slot processes its logits (its history counts the tokens the engine produced; make it neutral first)";
        if (slots[slot].trn.mirostat()) return "engine_set_token: the slot has Mirostat on (mu would no longer belong to the tokens held; switch it off first)";
        return nullptr;
    }
    const char *refuses_verify(int slot) const {
        if (slots[slot].smp.samples()) return "engine_verify: the slot samples (verification is greedy; set temperature 0 first)";
        if (slots[slot].pen.processes()) return "engine_verify: the slot processes its logits (verification takes the raw rows; make it neutral first)";
        return nullptr;
    }
    const char *refuses_verify_sampled(int slot) const {
        if (slots[slot].pen.processes()) return "engine_verify_sampled: the slot processes its logits (verification takes the raw rows; make it neutral first)";
        if (slots[slot].trn.truncates()) return "engine_verify_sampled: the slot truncates (min-p / typical-p / Mirostat keep other sets than the verification's; switch them off first)";
        return nullptr;
    }
    const char *refuses_verify_batch(int slot) const {
        if (slots[slot].smp.samples()) return "engine_verify_batch: a slot samples (verification is greedy; set temperature 0 first)";
        if (slots[slot].pen.processes()) return "engine_verify_batch: a slot processes its logits (verification takes the raw rows; make it neutral first)";
        if (slots[slot].trn.mirostat()) return "engine_verify_batch: a slot has Mirostat on (switch it off first)";
        if (slots[slot].lora >= 0) return "engine_verify_batch: a slot carries a LoRA adapter (adapters are verified one slot at a time, tl_engine_verify)";
        return nullptr;
    }
    // what refuses_verify_batch refuses, except sampling; and truncation of any kind, as refuses_verify_sampled
    const char *refuses_verify_batch_sampled(int slot) const {
        if (slots[slot].pen.processes()) return "engine_verify_batch_sampled: a slot processes its logits (verification takes the raw rows; make it neutral first)";
        if (slots[slot].trn.truncates()) return "engine_verify_batch_sampled: a slot truncates (min-p / typical-p / Mirostat keep other sets than the verification's; switch them off first)";
        if (slots[slot].lora >= 0) return "engine_verify_batch_sampled: a slot carries a LoRA adapter (adapters are verified one slot at a time, tl_engine_verify_sampled)";
        return nullptr;
    }
    // a beam group decodes through the plain greedy program and selects from the raw rows
    const char *refuses_beam(int slot) const {
        if (slots[slot].smp.samples()) return "engine_beam: the slot samples (beam slots are greedy)";
        if (slots[slot].pen.processes()) return "engine_beam: the slot processes its logits (penalties, bias or a grammar)";
        if (slots[slot].trn.truncates()) return "engine_beam: the slot truncates";
        if (slots[slot].lp_n >= 0) return "engine_beam: the slot records log-probabilities";
        if (slots[slot].stop.armed) return "engine_beam: the slot is armed with a stop set";
        if (slots[slot].lookup) return "engine_beam: the slot is armed for prompt lookup (its history row does not follow a reorder)";
        return nullptr;
    }
    // Does the slot, taking part in a step, process its logits?  (runs: what the table says of the slot)
    bool processes(int slot, bool runs) const { return runs && slots[slot].pen.processes(); }
    // ... and does it record the ids it is fed (dry.h)?
    bool records(int slot, bool runs) const { return runs && slots[slot].pen.dry_on(); }
    // The step's plan over slots [slot0, slot0 + n): runs(slot) is the table's answer (live, neither parked nor stopped).  Truncation
    // applies to a slot that samples: a greedy slot is never filtered (every filter keeps the maximum), so its parameters do not change
    // the plan
    template <class Runs>
    StepFeatures features(int slot0, int n, Runs runs) const {
        StepFeatures f;
        for (int slot = slot0; slot < slot0 + n && slot < sz.slots; ++slot) {
            if (!runs(slot)) continue;
            const State &s = slots[slot];
            const bool processes = s.pen.processes(), truncates = s.trn.truncates() && s.smp.samples();
            f.samples |= s.smp.samples();
            f.logprobs |= s.lp_n >= 0;
            f.processes |= processes;
            f.grammar |= processes && s.pen.grammar;
            f.stack_grammar |= processes && s.pen.grammar && s.pen.grammar.stack;
            f.dry |= s.pen.dry_on();
            f.truncates |= truncates;
            f.mirostat |= truncates && s.trn.mirostat();
            f.lora |= exists(SB_LORA) && s.lora >= 0;
            f.stop |= s.stop.armed;
        }
        return f;
    }

    // ---- the host half of the stop reconciliation ---------------------------------------------------------------------------------
    // The mirrors advance per step for every running slot, so a slot that froze in mid-call leaves them ahead of the device.  `read`:
    // the records of every slot as just read back; view(slot): the table's {live, stopped, ctx, produced}.  out: the slots that newly
    // stopped, with the device's context length and the produced count that belongs to it (`produced` went up with the context, one
    // per step)
    struct StopEvent {
        int slot, context, produced;
    };
    template <class View>
    void stop_records_read(const StopMirror *read, View view, std::vector<StopEvent> &out) {
        for (int b = 0; b < sz.slots; ++b) {
            slots[b].stop_host = read[b];
            const auto &t = view(b);
            if (!t.live || t.stopped || !slots[b].stop.armed || read[b].reason == 0) continue;
            out.push_back({b, read[b].context, t.produced - (t.ctx - read[b].context)});
        }
    }

  private:
    static uint32_t bits(float v) {
        uint32_t w;
        memcpy(&w, &v, 4);
        return w;
    }
    static size_t carve(size_t &off, size_t bytes) {  // pieces start 256-byte aligned, front to back
        const size_t a = off;
        off = (off + bytes + 255) / 256 * 256;
        return a;
    }
    static void word(int block, size_t off, int32_t v, SettingsEdits &ed) { ed.list.push_back({SettingsEdit::WORD, block, off, v, 0, 0, nullptr}); }
    static void wordf(int block, size_t off, float v, SettingsEdits &ed) { word(block, off, (int32_t)bits(v), ed); }
    static void word64(int block, size_t off, uint64_t v, SettingsEdits &ed) {
        word(block, off, (int32_t)(uint32_t)v, ed);
        word(block, off + 4, (int32_t)(uint32_t)(v >> 32), ed);
    }
    bool has(int b, const SettingsEdits &ed) const { return exists(b) || (ed.needs >> b & 1u); }

    void smp_write(int slot, const SampleParams &v, SettingsEdits &ed) {
        wordf(SB_SAMPLE, at.smp_temp + slot * 4, v.temperature, ed);
        word(SB_SAMPLE, at.smp_topk + slot * 4, v.top_k, ed);
        wordf(SB_SAMPLE, at.smp_topp + slot * 4, v.top_p, ed);
        word64(SB_SAMPLE, at.smp_seed + slot * 8, v.seed, ed);
        slots[slot].smp = v;
    }
    // the first switch-on needs the records
    void lp_write(int slot, int top_n, int produced, SettingsEdits &ed) {
        State &s = slots[slot];
        if (!has(SB_LOGPROB, ed) ? top_n < 0 : s.lp_n == top_n) return;
        ed.needs |= 1u << SB_LOGPROB;
        word(SB_LOGPROB, at.lp_topn + slot * 4, top_n, ed);
        if (s.lp_n < 0) s.lp_from = produced;  // records begin with the next produced token
        s.lp_n = top_n;
    }
    // the slot's record becomes {no context length, state}; a stack grammar's: {no context length, (state, depth 0, word 0)} (the stack
    // words are masked by the depth when they are read)
    void gr_state_words(int slot, const GrammarRef &g, SettingsEdits &ed) {
        const int b = g.stack ? SB_STACK : SB_GRAMMAR;
        const size_t rec = g.stack ? (size_t)slot * sz.stack_record_bytes : at.gr_state + (size_t)slot * sz.grammar_record_bytes;
        word(b, rec, -1, ed);
        word(b, rec + 4, g.start, ed);
    }
    // the processing parameters the launch reads, from the mirror (on) or neutral: penalties 1 / 0 / 0, an empty bias list, no automaton
    // (the row is copied, nothing of the slot is written)
    void processing_words(int slot, bool on, SettingsEdits &ed) {
        const PenaltyParams neutral{};
        const PenaltyParams &v = on ? slots[slot].pen : neutral;
        wordf(SB_PROCESS, at.pen_rep + slot * 4, v.repetition, ed);
        wordf(SB_PROCESS, at.pen_pres + slot * 4, v.presence, ed);
        wordf(SB_PROCESS, at.pen_freq + slot * 4, v.frequency, ed);
        word(SB_PROCESS, at.pen_bias_n + slot * 4, (int32_t)v.bias_ids.size(), ed);
        if (has(SB_GRAMMAR, ed)) word64(SB_GRAMMAR, at.gr_ptr + slot * 8, v.grammar.dev, ed);
        if (has(SB_DRY, ed)) {  // the two words that arm a row (dry.h)
            wordf(SB_DRY, at.dry_mult + slot * 4, v.dry_multiplier, ed);
            word(SB_DRY, at.dry_ngram + slot * 4, v.ngram, ed);
        }
    }
    // the slot's parameters and bias list become `v` (validated).  History is tracked from the call that makes the slot process: that
    // call empties the slot's row of the table.  Only what differs from the mirror is written; a parked slot's words stay neutral
    void pen_write(int slot, const PenaltyParams &v, SettingsEdits &ed) {
        PenaltyParams &cur = slots[slot].pen;
        const bool was = cur.processes(), now = v.processes(), parked = slots[slot].parked;
        if (!has(SB_PROCESS, ed) && !now) return;  // neutral on an engine that never processed: nothing to write
        ed.needs |= 1u << SB_PROCESS;
        const size_t V = (size_t)sz.vocab;
        if (now && !was) ed.list.push_back({SettingsEdit::FILL, SB_PROCESS, at.pen_history + slot * V * 2, 0, 0, V * 2, nullptr});
        const bool rep = cur.repetition != v.repetition, pres = cur.presence != v.presence, freq = cur.frequency != v.frequency;
        const bool bias = cur.bias_ids != v.bias_ids || (!v.bias_values.empty() && memcmp(cur.bias_values.data(), v.bias_values.data(), v.bias_values.size() * 4) != 0);
        const bool grammar = cur.grammar.id != v.grammar.id;
        const bool dry = !cur.dry_same(v), dry_mult = cur.dry_multiplier != v.dry_multiplier, dry_ngram = cur.ngram != v.ngram;
        const bool dry_brk = cur.dry_breakers != v.dry_breakers;
        if (v.dry_on()) ed.needs |= 1u << SB_DRY;
        if (grammar) ed.needs |= 1u << SB_GRAMMAR | (v.grammar && v.grammar.stack ? 1u << SB_STACK : 0u);
        cur = v;
        if (bias && !cur.bias_ids.empty()) {  // (from the mirror: it outlives the copy)
            const size_t row = (size_t)slot * sz.max_bias * 4, n = cur.bias_ids.size() * 4;
            ed.list.push_back({SettingsEdit::UPLOAD, SB_PROCESS, at.pen_bias_ids + row, 0, 0, n, cur.bias_ids.data()});
            ed.list.push_back({SettingsEdit::UPLOAD, SB_PROCESS, at.pen_bias_values + row, 0, 0, n, cur.bias_values.data()});
        }
        if (dry && has(SB_DRY, ed)) {  // the words a row reads only once it is armed
            if (dry_brk && !cur.dry_breakers.empty())
                ed.list.push_back({SettingsEdit::UPLOAD, SB_DRY, at.dry_breakers + (size_t)slot * sz.dry_max_breakers * 4, 0, 0, cur.dry_breakers.size() * 4, cur.dry_breakers.data()});
            wordf(SB_DRY, at.dry_base + slot * 4, v.dry_base, ed);
            word(SB_DRY, at.dry_allowed + slot * 4, v.dry_allowed, ed);
            word(SB_DRY, at.dry_range + slot * 4, v.dry_range, ed);
            word(SB_DRY, at.dry_s0 + slot * 4, v.dry_s0, ed);
            word(SB_DRY, at.dry_nbreak + slot * 4, (int32_t)v.dry_breakers.size(), ed);
        }
        if (parked) {
            processing_words(slot, false, ed);
        } else {
            if (dry_mult && has(SB_DRY, ed)) wordf(SB_DRY, at.dry_mult + slot * 4, v.dry_multiplier, ed);
            if (dry_ngram && has(SB_DRY, ed)) word(SB_DRY, at.dry_ngram + slot * 4, v.ngram, ed);
            if (rep) wordf(SB_PROCESS, at.pen_rep + slot * 4, v.repetition, ed);
            if (pres) wordf(SB_PROCESS, at.pen_pres + slot * 4, v.presence, ed);
            if (freq) wordf(SB_PROCESS, at.pen_freq + slot * 4, v.frequency, ed);
            if (bias) word(SB_PROCESS, at.pen_bias_n + slot * 4, (int32_t)v.bias_ids.size(), ed);
            if (grammar) word64(SB_GRAMMAR, at.gr_ptr + slot * 8, v.grammar.dev, ed);
        }
        if (grammar && v.grammar) gr_state_words(slot, v.grammar, ed);  // a new automaton: the record at its start state
    }
    // restart_mu: mu becomes 2 tau (NaN without Mirostat); move / fork copy the source's mu behind this call instead
    void trn_write(int slot, const TruncParams &v, bool restart_mu, SettingsEdits &ed) {
        slots[slot].trn = v;
        if (!has(SB_TRUNC, ed) && !v.truncates()) return;  // an engine that never truncated: nothing to write
        ed.needs |= 1u << SB_TRUNC;
        wordf(SB_TRUNC, at.trn_minp + slot * 4, v.min_p, ed);
        wordf(SB_TRUNC, at.trn_typ + slot * 4, v.typical_p, ed);
        wordf(SB_TRUNC, at.trn_tau + slot * 4, v.tau, ed);
        wordf(SB_TRUNC, at.trn_eta + slot * 4, v.eta, ed);
        if (restart_mu) word(SB_TRUNC, at.trn_mu + slot * 4, v.mirostat() ? (int32_t)bits(2.f * v.tau) : (int32_t)0x7fc00000, ed);
    }
    void trn_reset(int slot, SettingsEdits &ed) {
        const TruncParams d{};
        const TruncParams &c = slots[slot].trn;
        if (c.min_p == d.min_p && c.typical_p == d.typical_p && c.tau == d.tau && c.eta == d.eta) return;
        trn_write(slot, d, true, ed);
    }
    // on the host and -- once an adapter has been loaded -- on the device (skipped while it is the value already)
    void lora_write(int slot, int adapter, SettingsEdits &ed) {
        if (slots[slot].lora == adapter) return;
        slots[slot].lora = adapter;
        if (exists(SB_LORA)) word(SB_LORA, (size_t)slot * 4, adapter, ed);
    }
    // the slot's device words: set pointer, armed, budget, automaton at the root, an empty record
    void stop_words(int slot, SettingsEdits &ed) {
        const StopSlot &v = slots[slot].stop;
        word64(SB_STOP, at.stop_sets + slot * 8, v.set.dev, ed);
        word(SB_STOP, at.stop_armed + slot * 4, v.armed ? 1 : 0, ed);
        word(SB_STOP, at.stop_max_new + slot * 4, v.max_new, ed);
        word(SB_STOP, at.stop_automaton + slot * 4, 0, ed);
        for (int w = 0; w < sz.stop_record_bytes / 4; ++w) word(SB_STOP, at.stop_rec + (size_t)slot * sz.stop_record_bytes + w * 4, 0, ed);
    }
    // the slot is unarmed and its record empty (the table's slot starts over: not stopped)
    void stop_reset(int slot, SettingsEdits &ed) {
        if (!exists(SB_STOP) || !slots[slot].stop.armed) return;
        slots[slot].stop = StopSlot{};
        slots[slot].stop_host = StopMirror{};
        stop_words(slot, ed);
    }

    BlockLayout layouts_[SB_COUNT];
    unsigned exists_ = 0;
};

}  // namespace tl
