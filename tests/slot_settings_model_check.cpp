// Model check of csrc/slot_settings.h alone (tests/test_slot_settings_cpu.py builds it with ASan + UBSan): a seeded random walk over a few
// slots and every operation of the record.  Host byte arrays stand for the device -- one per block, made from the layout's own fill
// rule when a call first needs it -- and change only by applying the edits a call reports.  Between operations the words a step would
// write (history rows, grammar records, mu, pending logprob records, stop automata and records) take fresh fingerprints for the slots
// that run.  After every operation the arrays are compared with what the mirrors say they must hold.
//   usage: slot_settings_model_check STEPS SEED      prints "ok steps=N <operation.feature>=<served calls> ... <refused.kind>=<calls>"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

#include "slot_settings.h"

using namespace tl;

#define REQUIRE(cond, ...)                                          \
    do {                                                            \
        if (!(cond)) {                                              \
            fprintf(stderr, "FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                           \
            fprintf(stderr, "\n  step %ld: %s\n", g_step, g_what.c_str()); \
            exit(1);                                                \
        }                                                           \
    } while (0)

static long g_step = 0;
static std::string g_what;

static const int B = 5, V = 96, RING = 4, LP_WORDS = 5, LP_TOP = 20, MAX_BIAS = 6, GR_REC = 8, STACK_REC = 24, STOP_REC = 24, MAX_VOCAB = 524288;
static const uint32_t NAN_BITS = 0x7fc00000u;

struct Rng {
    uint64_t s;
    uint32_t next() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return (uint32_t)(s >> 24);
    }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    bool chance(int percent) { return below(100) < percent; }
};

// one array of a block: [rows] rows of row_bytes each, row r belonging to slot r (per_slot) or to nobody (the rows of a launch)
struct Array {
    int block;
    size_t off, row_bytes;
    bool per_slot;
};

struct Model {
    SlotSettings st;
    std::vector<uint8_t> dev[SB_COUNT];
    bool made[SB_COUNT] = {};
    // the table's part: which slots hold a sequence, what they have produced
    bool live[B] = {}, stopped[B] = {};
    int produced[B] = {}, ctx[B] = {};
    std::vector<Array> arrays;
    std::map<std::string, long> counts;
    uint32_t stamp = 1;

    void init() {
        st.init({B, V, RING, LP_WORDS, LP_TOP, MAX_BIAS, GR_REC, STACK_REC, STOP_REC, MAX_VOCAB, -1});
        const SlotSettings::Offsets &a = st.at;
        arrays = {{SB_SAMPLE, a.smp_seed, 8, true}, {SB_SAMPLE, a.smp_temp, 4, true}, {SB_SAMPLE, a.smp_topk, 4, true}, {SB_SAMPLE, a.smp_topp, 4, true},
                  {SB_LOGPROB, a.lp_topn, 4, true}, {SB_LOGPROB, a.lp_pending, LP_WORDS * 4, true}, {SB_LOGPROB, a.lp_ring, (size_t)RING * LP_WORDS * 4, true},
                  {SB_PROCESS, a.pen_history, V * 2, true}, {SB_PROCESS, a.pen_rows, V * 2, false}, {SB_PROCESS, a.pen_rep, 4, true},
                  {SB_PROCESS, a.pen_pres, 4, true}, {SB_PROCESS, a.pen_freq, 4, true}, {SB_PROCESS, a.pen_bias_n, 4, true},
                  {SB_PROCESS, a.pen_bias_ids, MAX_BIAS * 4, true}, {SB_PROCESS, a.pen_bias_values, MAX_BIAS * 4, true},
                  {SB_GRAMMAR, a.gr_ptr, 8, true}, {SB_GRAMMAR, a.gr_state, GR_REC, true}, {SB_STACK, 0, STACK_REC, true},
                  {SB_TRUNC, a.trn_rows, V * 2, false}, {SB_TRUNC, a.trn_minp, 4, true}, {SB_TRUNC, a.trn_tau, 4, true}, {SB_TRUNC, a.trn_eta, 4, true},
                  {SB_TRUNC, a.trn_logsum, 4, false}, {SB_TRUNC, a.trn_typ, 4, true}, {SB_TRUNC, a.trn_mu, 4, true},
                  {SB_STOP, a.stop_sets, 8, true}, {SB_STOP, a.stop_armed, 4, true}, {SB_STOP, a.stop_max_new, 4, true}, {SB_STOP, a.stop_automaton, 4, true},
                  {SB_STOP, a.stop_rec, STOP_REC, true}, {SB_LORA, 0, 4, true}};
        make(SB_SAMPLE);  // (made with the engine)
    }
    // a fresh block from its layout: bytes no rule covers hold a pattern nobody may rely on
    void make(int b) {
        const BlockLayout &lay = st.layout(b);
        dev[b].assign(lay.bytes, 0xab);
        for (const BlockFill &f : lay.fill) {
            REQUIRE(f.off % 4 == 0 && f.bytes % 4 == 0 && f.off + f.bytes <= lay.bytes, "fill rule of block %d outside the block", b);
            for (size_t o = f.off; o < f.off + f.bytes; o += 4) memcpy(&dev[b][o], &f.word, 4);
        }
        made[b] = true;
        st.created(b);
    }
    uint32_t w(int b, size_t off) const {
        uint32_t v;
        memcpy(&v, &dev[b][off], 4);
        return v;
    }
    void put(int b, size_t off, uint32_t v) { memcpy(&dev[b][off], &v, 4); }
    // the slot a byte range belongs to, -1: nobody's (or it crosses a row)
    int slot_of(int b, size_t off, size_t bytes) const {
        for (const Array &a : arrays) {
            if (a.block != b || !a.per_slot || off < a.off || off >= a.off + B * a.row_bytes) continue;
            const size_t row = (off - a.off) / a.row_bytes;
            return off + bytes <= a.off + (row + 1) * a.row_bytes ? (int)row : -1;
        }
        return -1;
    }
    // everything of the slot in the blocks that exist
    std::vector<uint8_t> slot_bytes(const std::vector<uint8_t> *mem, int slot) const {
        std::vector<uint8_t> out;
        for (const Array &a : arrays)
            if (a.per_slot && !mem[a.block].empty()) out.insert(out.end(), mem[a.block].begin() + a.off + slot * a.row_bytes, mem[a.block].begin() + a.off + (slot + 1) * a.row_bytes);
        return out;
    }

    // ---- applying a served call's edits ------------------------------------------------------------------------------------------
    std::vector<uint8_t> before[SB_COUNT];  // the device as the call found it (a block the call made: fresh)
    std::vector<SlotSettings::State> mirrors_before;
    void snapshot() {
        for (int b = 0; b < SB_COUNT; ++b) before[b] = dev[b];
        mirrors_before = st.slots;
    }
    void apply(const SettingsEdits &ed, std::initializer_list<int> named) {
        for (int b = 0; b < SB_COUNT; ++b) {
            if (!(ed.needs >> b & 1u) || made[b]) continue;
            REQUIRE(b != SB_LORA && b != SB_SAMPLE, "a call asked for block %d, which is not its to ask for", b);
            make(b);
            before[b] = dev[b];
        }
        std::vector<std::pair<int, size_t>> words;
        for (const SettingsEdit &x : ed.list) {
            REQUIRE(x.block >= 0 && x.block < SB_COUNT && made[x.block], "an edit addresses block %d, which does not exist and was not asked for", x.block);
            const size_t n = x.kind == SettingsEdit::WORD ? 4 : x.bytes;
            const int slot = slot_of(x.block, x.off, n);
            REQUIRE(slot >= 0 && std::find(named.begin(), named.end(), slot) != named.end(), "an edit of block %d at %zu lands outside the rows of the call's slots", x.block, x.off);
            if (x.kind == SettingsEdit::WORD) {
                REQUIRE(x.off % 4 == 0, "misaligned word");
                for (const auto &p : words) REQUIRE(p != std::make_pair(x.block, x.off), "block %d word %zu is written twice by one call", x.block, x.off);
                words.emplace_back(x.block, x.off);
                put(x.block, x.off, (uint32_t)x.word);
            } else if (x.kind == SettingsEdit::COPY) {
                const int from = slot_of(x.block, x.from, n);
                REQUIRE(from >= 0 && std::find(named.begin(), named.end(), from) != named.end(), "a copy reads outside the rows of the call's slots");
                memmove(&dev[x.block][x.off], &dev[x.block][x.from], n);
            } else if (x.kind == SettingsEdit::FILL) {
                memset(&dev[x.block][x.off], 0, n);
            } else {
                REQUIRE(x.host != nullptr, "an upload without a source");
                memcpy(&dev[x.block][x.off], x.host, n);
            }
        }
        for (int s = 0; s < B; ++s)
            if (std::find(named.begin(), named.end(), s) == named.end()) {
                REQUIRE(slot_bytes(dev, s) == slot_bytes(before, s), "slot %d, which the call does not name, changed on the device", s);
                REQUIRE(same(st.slots[s], mirrors_before[s]), "the mirror of slot %d, which the call does not name, changed", s);
            }
    }
    static bool same(const SlotSettings::State &a, const SlotSettings::State &b) {
        return a.smp.temperature == b.smp.temperature && a.smp.top_k == b.smp.top_k && a.smp.top_p == b.smp.top_p && a.smp.seed == b.smp.seed && a.lp_n == b.lp_n && a.lp_from == b.lp_from && a.pen.repetition == b.pen.repetition &&
               a.pen.presence == b.pen.presence && a.pen.frequency == b.pen.frequency && a.pen.bias_ids == b.pen.bias_ids &&
               a.pen.bias_values == b.pen.bias_values && a.pen.grammar.id == b.pen.grammar.id && memcmp(&a.trn, &b.trn, sizeof(a.trn)) == 0 &&
               a.lora == b.lora && a.stop.set.id == b.stop.set.id && a.stop.max_new == b.stop.max_new && a.stop.armed == b.stop.armed &&
               memcmp(&a.stop_host, &b.stop_host, sizeof(a.stop_host)) == 0 && a.gr_pending == b.gr_pending && a.parked == b.parked && a.emb_rows == b.emb_rows;
    }
    // a refused call: no edit, no block, no mirror touched
    void refused(const char *got, const char *want, const SettingsEdits &ed, const std::string &kind) {
        REQUIRE(got && std::string(got) == want, "refusal '%s', expected '%s'", got ? got : "(served)", want);
        REQUIRE(ed.list.empty() && ed.needs == 0, "a refused call reported edits");
        for (int s = 0; s < B; ++s) REQUIRE(same(st.slots[s], mirrors_before[s]), "a refused call changed the mirror of slot %d", s);
        counts["refused." + kind]++;
    }

    // ---- what the device must hold, from the mirrors ---------------------------------------------------------------------------------
    static uint32_t fbits(float f) {
        uint32_t v;
        memcpy(&v, &f, 4);
        return v;
    }
    void check_all() {
        const SlotSettings::Offsets &a = st.at;
        for (int s = 0; s < B; ++s) {
            const SlotSettings::State &m = st.slots[s];
            REQUIRE(!(m.trn.mirostat() && (m.smp.top_k != 0 || m.smp.top_p != 0.f || m.trn.stateless())), "slot %d: Mirostat beside another truncation", s);
            REQUIRE(live[s] || (m.smp.is_default() && !m.pen.processes() && !m.trn.truncates() && m.lora == -1 && !m.stop.armed && !m.gr_pending && !m.parked && m.emb_rows == -1),
                    "free slot %d is not at the defaults", s);
            REQUIRE(w(SB_SAMPLE, a.smp_temp + s * 4) == fbits(m.smp.temperature) && w(SB_SAMPLE, a.smp_topk + s * 4) == (uint32_t)m.smp.top_k &&
                        w(SB_SAMPLE, a.smp_topp + s * 4) == fbits(m.smp.top_p) && w(SB_SAMPLE, a.smp_seed + s * 8) == (uint32_t)m.smp.seed &&
                        w(SB_SAMPLE, a.smp_seed + s * 8 + 4) == (uint32_t)(m.smp.seed >> 32),
                    "slot %d: sampling words differ from the mirror", s);
            if (made[SB_LOGPROB]) REQUIRE(w(SB_LOGPROB, a.lp_topn + s * 4) == (uint32_t)m.lp_n, "slot %d: top-N differs from the mirror", s);
            else REQUIRE(m.lp_n == -1, "slot %d records log-probabilities without a block", s);
            if (made[SB_PROCESS]) {
                const PenaltyParams neutral{};
                const PenaltyParams &p = m.parked ? neutral : m.pen;  // a parked slot's processing words are neutral
                REQUIRE(w(SB_PROCESS, a.pen_rep + s * 4) == fbits(p.repetition) && w(SB_PROCESS, a.pen_pres + s * 4) == fbits(p.presence) &&
                            w(SB_PROCESS, a.pen_freq + s * 4) == fbits(p.frequency) && w(SB_PROCESS, a.pen_bias_n + s * 4) == (uint32_t)p.bias_ids.size(),
                        "slot %d (parked %d): processing words differ from %s", s, (int)m.parked, m.parked ? "neutral" : "the mirror");
                for (size_t i = 0; i < m.pen.bias_ids.size(); ++i)
                    REQUIRE(w(SB_PROCESS, a.pen_bias_ids + (s * MAX_BIAS + i) * 4) == (uint32_t)m.pen.bias_ids[i] &&
                                w(SB_PROCESS, a.pen_bias_values + (s * MAX_BIAS + i) * 4) == fbits(m.pen.bias_values[i]),
                            "slot %d: bias entry %zu differs from the mirror", s, i);
            } else {
                REQUIRE(!m.pen.processes(), "slot %d processes without a block", s);
            }
            if (made[SB_GRAMMAR]) {
                const uint64_t want = m.parked ? 0 : m.pen.grammar.dev;
                REQUIRE(w(SB_GRAMMAR, a.gr_ptr + s * 8) == (uint32_t)want && w(SB_GRAMMAR, a.gr_ptr + s * 8 + 4) == (uint32_t)(want >> 32), "slot %d: automaton pointer", s);
            } else {
                REQUIRE(!m.pen.grammar, "slot %d has a grammar without a block", s);
            }
            REQUIRE(!(m.pen.grammar && m.pen.grammar.stack) || made[SB_STACK], "slot %d has a stack grammar without a block", s);
            if (made[SB_TRUNC]) {
                // (typical-p off is 1 once written and the fresh block's all-ones NaN before: the launch reads both as off)
                const uint32_t typ = w(SB_TRUNC, a.trn_typ + s * 4);
                REQUIRE(w(SB_TRUNC, a.trn_minp + s * 4) == fbits(m.trn.min_p) && (typ == fbits(m.trn.typical_p) || (m.trn.typical_p == 1.f && typ == 0xffffffffu)) &&
                            w(SB_TRUNC, a.trn_tau + s * 4) == fbits(m.trn.tau) && w(SB_TRUNC, a.trn_eta + s * 4) == fbits(m.trn.eta),
                        "slot %d: truncation words differ from the mirror", s);
                // (mu is a number exactly while Mirostat is on)
                const uint32_t mu = w(SB_TRUNC, a.trn_mu + s * 4);
                REQUIRE(m.trn.mirostat() ? (mu & 0x7f800000u) != 0x7f800000u : (mu & 0x7fffffffu) > 0x7f800000u, "slot %d: mu %08x with tau %g", s, mu, m.trn.tau);
            } else {
                REQUIRE(!m.trn.truncates(), "slot %d truncates without a block", s);
            }
            if (made[SB_STOP]) {
                REQUIRE(w(SB_STOP, a.stop_sets + s * 8) == (uint32_t)m.stop.set.dev && w(SB_STOP, a.stop_sets + s * 8 + 4) == (uint32_t)(m.stop.set.dev >> 32) &&
                            w(SB_STOP, a.stop_armed + s * 4) == (uint32_t)m.stop.armed && w(SB_STOP, a.stop_max_new + s * 4) == (uint32_t)m.stop.max_new,
                        "slot %d: stop words differ from the mirror", s);
                if (!m.stop.armed)
                    for (int k = 0; k < STOP_REC / 4 + 1; ++k)
                        REQUIRE(w(SB_STOP, k == 0 ? a.stop_automaton + s * 4 : a.stop_rec + s * STOP_REC + (k - 1) * 4) == 0, "unarmed slot %d: automaton or record not empty", s);
            } else {
                REQUIRE(!m.stop.armed, "slot %d is armed without a block", s);
            }
            if (made[SB_LORA]) REQUIRE(w(SB_LORA, s * 4) == (uint32_t)m.lora, "slot %d: adapter id differs from the mirror", s);
        }
    }

    // ---- a step's writes: fresh fingerprints in the words that evolve on the device, for the slots that run ------------------------------
    bool runs(int s) const { return live[s] && !st.slots[s].parked && !stopped[s]; }
    void step() {
        const SlotSettings::Offsets &a = st.at;
        for (int s = 0; s < B; ++s) {
            if (!runs(s)) continue;
            const SlotSettings::State &m = st.slots[s];
            if (m.pen.processes()) {
                put(SB_PROCESS, a.pen_history + (size_t)s * V * 2, stamp++);
                put(SB_PROCESS, a.pen_history + (size_t)(s + 1) * V * 2 - 4, stamp++);
                if (m.pen.grammar && m.pen.grammar.stack)
                    for (int k = 0; k < STACK_REC / 4; ++k) put(SB_STACK, s * STACK_REC + k * 4, stamp++);
                else if (m.pen.grammar)
                    put(SB_GRAMMAR, a.gr_state + s * GR_REC, stamp++), put(SB_GRAMMAR, a.gr_state + s * GR_REC + 4, stamp++);
            }
            if (m.trn.mirostat() && m.smp.samples()) put(SB_TRUNC, a.trn_mu + s * 4, fbits(1.f + (float)(stamp++ % 1000)));
            if (m.lp_n >= 0)
                for (int k = 0; k < LP_WORDS; ++k) put(SB_LOGPROB, a.lp_pending + (s * LP_WORDS + k) * 4, stamp++);
            if (m.stop.armed) {
                put(SB_STOP, a.stop_automaton + s * 4, stamp++);
                for (int k = 1; k < STOP_REC / 4; ++k) put(SB_STOP, a.stop_rec + s * STOP_REC + k * 4, stamp++);  // (the reason stays none: the slot runs)
            }
            produced[s]++, ctx[s]++;
            st.pending_produced(s);
        }
    }

    // the features of a slot, for the counts: a served lifecycle call is counted once per feature its slot has on
    void count(const std::string &op, const SlotSettings::State &m) {
        counts[op]++;
        if (!m.smp.is_default()) counts[op + ".sampling"]++;
        if (m.lp_n >= 0) counts[op + ".logprobs"]++;
        if (m.pen.processes()) counts[op + ".processing"]++;
        if (m.trn.truncates()) counts[op + ".truncation"]++;
        if (m.lora >= 0) counts[op + ".lora"]++;
        if (m.stop.armed) counts[op + ".stop"]++;
        if (m.gr_pending || m.emb_rows >= 0) counts[op + ".flags"]++;
    }
    // history is tracked from the call that makes the slot process: that call finds the row dirty and must leave it empty
    void check_history(int slot, const SlotSettings::State &was) {
        if (was.pen.processes() || !st.slots[slot].pen.processes()) return;
        for (size_t o = 0; o < (size_t)V * 2; o += 4) REQUIRE(w(SB_PROCESS, st.at.pen_history + (size_t)slot * V * 2 + o) == 0, "slot %d starts to process over a history row that is not empty", slot);
        counts["history_cleared"]++;
    }
    bool row_equal(int b, size_t off, int dst, int src, size_t row) const { return memcmp(&dev[b][off + dst * row], &before[b][off + src * row], row) == 0; }
};

static const GrammarRef GRAMMARS[3] = {{0x1111222233334444ull, false, 3, &GRAMMARS[0]}, {0x5555666677778888ull, false, 0, &GRAMMARS[1]},
                                       {0x9999aaaabbbbccccull, true, 7, &GRAMMARS[2]}};
static const StopRef STOPS[2] = {{0x0123456789abcdefull, &STOPS[0]}, {0xfedcba9876543210ull, &STOPS[1]}};

int main(int argc, char **argv) {
    const long steps = argc > 1 ? atol(argv[1]) : 20000;
    Rng rng{(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1) * 0x9e3779b97f4a7c15ull + 0x1234567ull};
    Model M;
    M.init();
    M.check_all();
    SlotSettings &st = M.st;
    const SlotSettings::Offsets &a = st.at;
    for (g_step = 0; g_step < steps; ++g_step) {
        if (rng.chance(40)) M.step();
        if (g_step == steps / 50) M.make(SB_LORA);  // the first adapter is loaded: the ids exist from here on
        M.snapshot();
        SettingsEdits ed;
        const int slot = rng.below(B), op = rng.below(100);
        const SlotSettings::State was = st.slots[slot];
        if (op < 8) {  // begin / release
            g_what = (M.live[slot] ? "release " : "begin ") + std::to_string(slot);
            M.count(M.live[slot] ? "reset" : "begin", was);
            st.reset(slot, ed);
            M.apply(ed, {slot});
            M.live[slot] = !M.live[slot], M.stopped[slot] = false, M.produced[slot] = M.ctx[slot] = 0;
            const SlotSettings::State &m = st.slots[slot];
            REQUIRE(m.smp.is_default() && m.lp_n == -1 && !m.pen.processes() && !m.trn.truncates() && m.trn.eta == 0.f && m.lora == -1 && !m.stop.armed &&
                        !m.gr_pending && !m.parked && m.emb_rows == -1,
                    "reset left a mirror off its default");  // (check_all ties every parameter word, mu and the stop record to these)
        } else if (op < 20) {  // set_sampling
            if (!M.live[slot]) continue;
            g_what = "set_sampling " + std::to_string(slot);
            const int bad = rng.chance(20) ? rng.below(3) : -1;
            const float t = bad == 0 ? (rng.chance(50) ? -1.f : INFINITY) : (rng.chance(30) ? 0.f : 0.5f + rng.below(4) * 0.25f);
            const int k = bad == 1 ? -1 - rng.below(3) : (rng.chance(50) ? 0 : rng.below(2 * V));
            const float p = bad == 2 ? NAN : (rng.chance(50) ? 0.f : rng.below(6) * 0.25f - 0.25f);
            const uint64_t seed = (uint64_t)rng.next() << 32 | rng.next();
            const char *why = st.set_sampling(slot, t, k, p, seed, ed);
            static const char *texts[3] = {"engine_set_sampling: temperature must be finite and >= 0", "engine_set_sampling: top_k must be >= 0 (0 = no top-k)",
                                           "engine_set_sampling: top_p is NaN"};
            const bool cut = (k > 0 && k < V) || (p > 0.f && p < 1.f);
            if (bad >= 0) M.refused(why, texts[bad], ed, std::string("sampling.") + (bad == 0 ? "temperature" : bad == 1 ? "top_k" : "top_p"));
            else if (was.trn.mirostat() && cut) M.refused(why, "engine_set_sampling: the slot has Mirostat on, which excludes top-k and top-p", ed, "sampling.mirostat");
            else {
                REQUIRE(!why, "refused: %s", why);
                M.apply(ed, {slot});
                const SampleParams &v = st.slots[slot].smp;
                REQUIRE(v.temperature == t && v.seed == seed && v.top_k == (k < V ? k : 0) && v.top_p == (p > 0.f && p < 1.f ? p : 0.f), "sampling mirror");
                M.counts["set_sampling"]++;
            }
        } else if (op < 27) {  // set_truncation
            if (!M.live[slot]) continue;
            g_what = "set_truncation " + std::to_string(slot);
            const int bad = rng.chance(15) ? rng.below(2) : -1;
            const float mp = bad == 0 ? (rng.chance(50) ? -0.5f : 1.5f) : (rng.chance(50) ? 0.f : 0.05f * (1 + rng.below(4)));
            const float ty = bad == 1 ? NAN : (rng.chance(50) ? 1.f : rng.below(5) * 0.3f);
            const char *why = st.set_truncation(slot, mp, ty, ed);
            if (bad == 0) M.refused(why, "engine_set_truncation: min_p must be in [0, 1] (0 = off)", ed, "truncation.min_p");
            else if (bad == 1) M.refused(why, "engine_set_truncation: typical_p is NaN", ed, "truncation.typical_p");
            else if (was.trn.mirostat() && (mp > 0.f || (ty > 0.f && ty < 1.f))) M.refused(why, "engine_set_truncation: the slot has Mirostat on, which excludes min-p and typical-p", ed, "truncation.mirostat");
            else {
                REQUIRE(!why, "refused: %s", why);
                M.apply(ed, {slot});
                if (M.made[SB_TRUNC]) REQUIRE(M.row_equal(SB_TRUNC, a.trn_mu, slot, slot, 4), "set_truncation restarted mu");
                M.counts["set_truncation"]++;
            }
        } else if (op < 36) {  // set_mirostat
            if (!M.live[slot]) continue;
            g_what = "set_mirostat " + std::to_string(slot);
            const int bad = rng.chance(15) ? rng.below(2) : -1;
            const float tau = bad == 0 ? (rng.chance(50) ? -1.f : NAN) : (rng.chance(35) ? 0.f : 1.f + rng.below(5));
            const float eta = bad == 1 ? (rng.chance(50) ? 0.f : 1.5f) : 0.1f * (1 + rng.below(10));
            const char *why = st.set_mirostat(slot, bad == 1 && tau == 0.f ? 3.f : tau, eta, ed);
            const float t = bad == 1 && tau == 0.f ? 3.f : tau;
            if (bad == 0) M.refused(why, "engine_set_mirostat: tau must be finite and >= 0 (0 = off)", ed, "mirostat.tau");
            else if (bad == 1) M.refused(why, "engine_set_mirostat: eta must be in (0, 1]", ed, "mirostat.eta");
            else if (t > 0.f && (was.trn.stateless() || was.smp.top_k != 0 || was.smp.top_p != 0.f))
                M.refused(why, "engine_set_mirostat: Mirostat excludes every other truncation of the slot (top-k, top-p, min-p, typical-p)", ed, "mirostat.excludes");
            else {
                REQUIRE(!why, "refused: %s", why);
                M.apply(ed, {slot});
                if (M.made[SB_TRUNC]) REQUIRE(M.w(SB_TRUNC, a.trn_mu + slot * 4) == (t > 0.f ? Model::fbits(2.f * t) : NAN_BITS), "mu does not restart at 2 tau");
                REQUIRE(st.slots[slot].trn.tau == t && st.slots[slot].trn.eta == (t > 0.f ? eta : 0.f), "mirostat mirror");
                M.counts["set_mirostat"]++;
            }
        } else if (op < 44) {  // set_penalties
            if (!M.live[slot]) continue;
            g_what = "set_penalties " + std::to_string(slot);
            const int bad = rng.chance(15) ? rng.below(2) : -1;
            const float rep = bad == 0 ? (rng.chance(50) ? 0.f : NAN) : (rng.chance(40) ? 1.f : 1.f + 0.1f * rng.below(5));
            const float pres = bad == 1 ? INFINITY : (rng.chance(50) ? 0.f : 0.25f * rng.below(4)), freq = rng.chance(60) ? 0.f : 0.125f * rng.below(4);
            const char *why = st.set_penalties(slot, rep, pres, freq, ed);
            if (bad == 0) M.refused(why, "engine_set_penalties: repetition_penalty must be finite and > 0 (1 = off)", ed, "penalties.repetition");
            else if (bad == 1) M.refused(why, "engine_set_penalties: presence_penalty and frequency_penalty must be finite (0 = off)", ed, "penalties.presence");
            else {
                REQUIRE(!why, "refused: %s", why);
                M.apply(ed, {slot});
                M.check_history(slot, was);
                M.counts["set_penalties"]++;
            }
        } else if (op < 52) {  // set_logit_bias
            if (!M.live[slot]) continue;
            g_what = "set_logit_bias " + std::to_string(slot);
            const int bad = rng.chance(40) ? rng.below(5) : -1;
            int n = rng.chance(40) ? 0 : 1 + rng.below(MAX_BIAS);
            if (bad >= 2 && n < 2) n = 2;
            int32_t ids[MAX_BIAS + 2];
            float values[MAX_BIAS + 2];
            for (int i = 0; i < n; ++i) ids[i] = (rng.below(V / MAX_BIAS)) * MAX_BIAS + i, values[i] = rng.chance(20) ? -INFINITY : (float)rng.below(9) - 4.f;  // (distinct)
            if (bad == 0) n = rng.chance(50) ? -1 : MAX_BIAS + 1;
            if (bad == 2) ids[rng.below(n)] = rng.chance(50) ? -1 : V;
            if (bad == 3) ids[1] = ids[0];
            if (bad == 4) values[rng.below(n)] = rng.chance(50) ? NAN : INFINITY;
            const char *why = st.set_logit_bias(slot, bad == 1 ? nullptr : ids, values, bad == 1 && n == 0 ? (n = 1) : n, ed);
            static const char *texts[5] = {"engine_set_logit_bias: between 0 and TL_MAX_LOGIT_BIAS (1,024) entries", "engine_set_logit_bias: null argument",
                                           "engine_set_logit_bias: token id out of range", "engine_set_logit_bias: a token id appears twice",
                                           "engine_set_logit_bias: values must be finite or -inf"};
            static const char *kinds[5] = {"count", "null", "id", "twice", "value"};
            if (bad >= 0) M.refused(why, texts[bad], ed, std::string("bias.") + kinds[bad]);
            else {
                REQUIRE(!why, "refused: %s", why);
                M.apply(ed, {slot});
                REQUIRE((int)st.slots[slot].pen.bias_ids.size() == n, "bias mirror");
                M.check_history(slot, was);
                M.counts["set_logit_bias"]++;
            }
        } else if (op < 60) {  // set_grammar
            if (!M.live[slot]) continue;
            g_what = "set_grammar " + std::to_string(slot);
            const GrammarRef g = rng.chance(30) ? GrammarRef{} : GRAMMARS[rng.below(3)];
            REQUIRE(!st.set_grammar(slot, g, ed), "set_grammar refused");
            M.apply(ed, {slot});
            if (g) {  // the record is at the automaton's start: {no context length, state}
                const int b = g.stack ? SB_STACK : SB_GRAMMAR;
                const size_t rec = g.stack ? (size_t)slot * STACK_REC : a.gr_state + slot * GR_REC;
                REQUIRE(M.w(b, rec) == 0xffffffffu && M.w(b, rec + 4) == (uint32_t)g.start, "the grammar record is not at the start state");
            }
            M.check_history(slot, was);
            M.counts["set_grammar"]++;
        } else if (op < 66) {  // set_logprobs (a free slot may be set too)
            g_what = "set_logprobs " + std::to_string(slot);
            const bool bad = rng.chance(15);
            const int n = bad ? (rng.chance(50) ? -2 : LP_TOP + 1) : (rng.chance(35) ? -1 : rng.below(LP_TOP + 1));
            if (!M.live[slot] && !bad && n >= 0) continue;  // (the walk keeps free slots at the defaults)
            const char *why = st.set_logprobs(slot, n, M.produced[slot], ed);
            if (bad) M.refused(why, "engine_set_logprobs: top_n must be -1 (off) or 0 .. 20", ed, "logprobs.top_n");
            else {
                REQUIRE(!why, "refused: %s", why);
                M.apply(ed, {slot});
                REQUIRE(st.slots[slot].lp_n == n && (was.lp_n >= 0 || n < 0 || st.slots[slot].lp_from == M.produced[slot]), "logprob mirror");
                M.counts["set_logprobs"]++;
            }
        } else if (op < 71) {  // set_lora
            if (!M.live[slot]) continue;
            g_what = "set_lora " + std::to_string(slot);
            const int ad = rng.chance(30) ? -1 : rng.below(4);
            if (!M.made[SB_LORA] && ad >= 0) continue;  // (no adapter is resident before the first load)
            REQUIRE(!st.set_lora(slot, ad, ed), "set_lora refused");
            REQUIRE(was.lora != ad || ed.list.empty(), "the adapter id was written although it is the value already");
            M.apply(ed, {slot});
            M.counts["set_lora"]++;
        } else if (op < 78) {  // set_stop
            if (!M.live[slot]) continue;
            g_what = "set_stop " + std::to_string(slot);
            const bool bad = rng.chance(15);
            const StopRef set = rng.chance(40) ? StopRef{} : STOPS[rng.below(2)];
            const int budget = bad ? -1 - rng.below(4) : (rng.chance(50) ? 0 : 1 + rng.below(64));
            const char *why = st.set_stop(slot, set, budget, ed);
            if (bad) M.refused(why, "engine_set_stop: max_new_tokens must be nonnegative (0 = no budget)", ed, "stop.budget");
            else {
                REQUIRE(!why, "refused: %s", why);
                REQUIRE(M.made[SB_STOP] || set.id || budget > 0 || (ed.list.empty() && ed.needs == 0), "disarming on a model that never armed wrote something");
                M.apply(ed, {slot});
                M.stopped[slot] = false;
                if (M.made[SB_STOP])
                    for (int k = 0; k < STOP_REC / 4 + 1; ++k)
                        REQUIRE(M.w(SB_STOP, k == 0 ? a.stop_automaton + slot * 4 : a.stop_rec + slot * STOP_REC + (k - 1) * 4) == 0, "set_stop did not restart the record");
                M.counts["set_stop"]++;
            }
        } else if (op < 88) {  // fork / move into a free slot
            int dst = -1;
            for (int k = 0, s0 = rng.below(B); k < B && dst < 0; ++k)
                if (!M.live[(s0 + k) % B]) dst = (s0 + k) % B;
            const bool move = rng.chance(50);
            if (!M.live[slot] || dst < 0 || (!move && st.slots[slot].parked)) continue;
            g_what = std::string(move ? "move " : "fork ") + std::to_string(slot) + " -> " + std::to_string(dst);
            M.count("carry", was);
            M.count(move ? "move" : "fork", was);
            st.carry(slot, dst, move, ed);
            M.apply(ed, {slot, dst});
            M.live[dst] = true, M.stopped[dst] = M.stopped[slot], M.produced[dst] = 0, M.ctx[dst] = M.ctx[slot];
            const SlotSettings::State &d = st.slots[dst], &s = st.slots[slot];
            SlotSettings::State want = was;
            want.lp_from = 0, want.emb_rows = -1, want.parked = move && was.parked;
            REQUIRE(Model::same(d, want), "dst's mirror is not src's (with lp_from 0, no running mean, the pending flag as it was)");
            // the words that evolve on the device travelled: dst's are src's as they were at the call
            if (was.pen.processes()) REQUIRE(M.row_equal(SB_PROCESS, a.pen_history, dst, slot, V * 2), "the history row did not travel");
            if (was.pen.grammar) REQUIRE(was.pen.grammar.stack ? M.row_equal(SB_STACK, 0, dst, slot, STACK_REC) : M.row_equal(SB_GRAMMAR, a.gr_state, dst, slot, GR_REC), "the grammar record did not travel");
            if (was.trn.truncates()) REQUIRE(M.row_equal(SB_TRUNC, a.trn_mu, dst, slot, 4), "mu did not travel");
            if (M.made[SB_LOGPROB]) REQUIRE(M.row_equal(SB_LOGPROB, a.lp_pending, dst, slot, LP_WORDS * 4), "the pending logprob record did not travel");
            if (was.stop.armed) REQUIRE(M.row_equal(SB_STOP, a.stop_automaton, dst, slot, 4) && M.row_equal(SB_STOP, a.stop_rec, dst, slot, STOP_REC), "the stop automaton and record did not travel");
            if (move) {
                M.live[slot] = M.stopped[slot] = false, M.produced[slot] = M.ctx[slot] = 0;
                SlotSettings::State fresh;
                fresh.lp_from = s.lp_from;  // (only read while top-N is on)
                fresh.stop_host = s.stop_host;
                REQUIRE(Model::same(s, fresh) && (!was.stop.armed || s.stop_host.context == 0), "a move left src off the defaults");
            } else {
                REQUIRE(Model::same(s, was) && M.slot_bytes(M.dev, slot) == M.slot_bytes(M.before, slot), "a fork touched src");
            }
        } else if (op < 94) {  // park / unpark
            if (!M.live[slot]) continue;
            const bool parked = st.slots[slot].parked;
            g_what = std::string(parked ? "unpark " : "park ") + std::to_string(slot);
            M.count(parked ? "unpark" : "park", was);
            if (parked) st.unpark(slot, ed);
            else st.park(slot, ed);
            M.apply(ed, {slot});
            SlotSettings::State want = was;
            want.parked = !parked, want.emb_rows = -1;
            REQUIRE(Model::same(st.slots[slot], want), "park / unpark changed more of the mirror than the parked flag and the running mean");
            // only the processing parameters change on the device
            for (const Array &x : M.arrays)
                if (x.per_slot && M.made[x.block] && !(x.block == SB_PROCESS && (x.off == a.pen_rep || x.off == a.pen_pres || x.off == a.pen_freq || x.off == a.pen_bias_n)) &&
                    !(x.block == SB_GRAMMAR && x.off == a.gr_ptr))
                    REQUIRE(memcmp(&M.dev[x.block][x.off + slot * x.row_bytes], &M.before[x.block][x.off + slot * x.row_bytes], x.row_bytes) == 0,
                            "park / unpark changed block %d at %zu", x.block, x.off);
        } else if (op < 97) {  // the flags, the predicates and the plan
            g_what = "flags " + std::to_string(slot);
            if (M.live[slot] && rng.chance(40)) {
                const bool keeps = rng.chance(50);
                st.appended(slot, keeps);
                REQUIRE(!st.slots[slot].gr_pending && (keeps ? st.slots[slot].emb_rows == was.emb_rows : st.slots[slot].emb_rows == -1), "appended");
            }
            if (M.live[slot] && rng.chance(30)) st.slots[slot].emb_rows = 1 + rng.below(9);  // (a MEAN chunk, engine-side)
            if (M.live[slot] && rng.chance(20)) {
                st.rewound(slot);
                REQUIRE(st.slots[slot].emb_rows == -1, "rewound");
            }
            const SlotSettings::State &m = st.slots[slot];
            REQUIRE((st.refuses_rewind(slot) != nullptr) == (m.pen.processes() || m.trn.mirostat()), "refuses_rewind");
            REQUIRE((st.refuses_set_token(slot) != nullptr) == (m.pen.processes() || m.trn.mirostat()), "refuses_set_token");
            REQUIRE((st.refuses_verify(slot) != nullptr) == (m.smp.samples() || m.pen.processes()), "refuses_verify");
            REQUIRE((st.refuses_verify_sampled(slot) != nullptr) == (m.pen.processes() || m.trn.truncates()), "refuses_verify_sampled");
            REQUIRE((st.refuses_verify_batch(slot) != nullptr) == (m.smp.samples() || m.pen.processes() || m.trn.mirostat() || m.lora >= 0), "refuses_verify_batch");
            REQUIRE((st.refuses_beam(slot) != nullptr) == (m.smp.samples() || m.pen.processes() || m.trn.truncates() || m.lp_n >= 0 || m.stop.armed), "refuses_beam");
            const int n = 1 + rng.below(B - slot);
            const StepFeatures f = st.features(slot, n, [&](int s) { return M.runs(s); });
            StepFeatures want;
            for (int s = slot; s < slot + n; ++s) {
                const SlotSettings::State &q = st.slots[s];
                if (!M.runs(s)) continue;
                want.samples |= q.smp.temperature > 0.f, want.logprobs |= q.lp_n >= 0, want.processes |= q.pen.processes();
                want.grammar |= (bool)q.pen.grammar, want.stack_grammar |= q.pen.grammar && q.pen.grammar.stack;
                want.truncates |= q.trn.truncates() && q.smp.temperature > 0.f, want.mirostat |= q.trn.tau > 0.f && q.smp.temperature > 0.f;
                want.lora |= q.lora >= 0, want.stop |= q.stop.armed;
            }
            REQUIRE(f.samples == want.samples && f.logprobs == want.logprobs && f.processes == want.processes && f.grammar == want.grammar &&
                        f.stack_grammar == want.stack_grammar && f.truncates == want.truncates && f.mirostat == want.mirostat && f.lora == want.lora && f.stop == want.stop,
                    "the plan of slots %d .. %d", slot, slot + n - 1);
            M.counts["asked"]++;
        } else {  // the stop reconciliation: some armed running slots have frozen on the device
            if (!M.made[SB_STOP]) continue;
            g_what = "stop reconciliation";
            std::vector<StopMirror> read(B);
            std::vector<int> froze;
            for (int s = 0; s < B; ++s) {
                memcpy(&read[s], &M.dev[SB_STOP][a.stop_rec + s * STOP_REC], STOP_REC);
                if (M.runs(s) && st.slots[s].stop.armed && M.ctx[s] > 2 && rng.chance(50)) {
                    read[s].reason = 1 + rng.below(3), read[s].context = M.ctx[s] - rng.below(3);
                    memcpy(&M.dev[SB_STOP][a.stop_rec + s * STOP_REC], &read[s], STOP_REC);  // (the stop launch wrote it)
                    froze.push_back(s);
                }
            }
            struct View {
                bool live, stopped;
                int ctx, produced;
            };
            std::vector<SlotSettings::StopEvent> out;
            st.stop_records_read(read.data(), [&](int s) { return View{M.live[s], M.stopped[s], M.ctx[s], M.produced[s]}; }, out);
            REQUIRE(out.size() == froze.size(), "%zu slots reported stopped, %zu froze", out.size(), froze.size());
            for (size_t i = 0; i < out.size(); ++i) {
                const int s = out[i].slot;
                REQUIRE(s == froze[i] && out[i].context == read[s].context && out[i].produced == M.produced[s] - (M.ctx[s] - read[s].context), "the event of slot %d", s);
                M.stopped[s] = true, M.ctx[s] = out[i].context, M.produced[s] = out[i].produced;
            }
            for (int s = 0; s < B; ++s) REQUIRE(memcmp(&st.slots[s].stop_host, &read[s], STOP_REC) == 0, "the mirror did not take the record read");
            M.counts["reconciled"] += (long)out.size();
        }
        M.check_all();
    }
    printf("ok steps=%ld", steps);
    for (const auto &kv : M.counts) printf(" %s=%ld", kv.first.c_str(), kv.second);
    printf("\n");
    return 0;
}
