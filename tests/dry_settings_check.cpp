// Stand-alone check of the DRY / n-gram part of csrc/slot_settings.h (tests/test_dry_cpu.py builds it with AddressSanitizer and UBSan and
// runs it as its own process): the setter's refusals, and what the device holds -- host byte arrays made from the layouts' fill rules,
// changed only by the edits a call reports -- after arming, re-arming, fork, move, park, unpark and reset.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "slot_settings.h"

using namespace tl;

static int g_checks = 0;
#define REQUIRE(c, ...)                                     \
    do {                                                    \
        ++g_checks;                                         \
        if (!(c)) {                                         \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                       \
            std::printf("\n");                              \
            std::exit(1);                                   \
        }                                                   \
    } while (0)

struct Model {
    SlotSettings st;
    std::vector<uint8_t> dev[SB_COUNT];
    bool made[SB_COUNT] = {};
    void make(int b) {
        const BlockLayout &lay = st.layout(b);
        dev[b].assign(lay.bytes, 0xAB);  // bytes no rule covers start undefined
        for (const BlockFill &f : lay.fill)
            for (size_t o = f.off; o + 4 <= f.off + f.bytes; o += 4) memcpy(&dev[b][o], &f.word, 4);
        made[b] = true;
        st.created(b);
    }
    void apply(const SettingsEdits &ed) {
        for (int b = 0; b < SB_COUNT; ++b)
            if ((ed.needs >> b & 1u) && !made[b]) make(b);
        for (const SettingsEdit &x : ed.list) {
            REQUIRE(x.block >= 0 && x.block < SB_COUNT && made[x.block], "an edit addresses block %d, which does not exist", x.block);
            std::vector<uint8_t> &m = dev[x.block];
            const size_t n = x.kind == SettingsEdit::WORD ? 4 : x.bytes;
            REQUIRE(x.off + n <= m.size(), "an edit of block %d ends at %zu of %zu bytes", x.block, x.off + n, m.size());
            if (x.kind == SettingsEdit::WORD) memcpy(&m[x.off], &x.word, 4);
            else if (x.kind == SettingsEdit::FILL) memset(&m[x.off], 0, n);
            else if (x.kind == SettingsEdit::UPLOAD) memcpy(&m[x.off], x.host, n);
            else {
                REQUIRE(x.from + n <= m.size(), "a copy of block %d reads past its end", x.block);
                memmove(&m[x.off], &m[x.from], n);
            }
        }
    }
    int32_t w(size_t off) const {
        int32_t v;
        memcpy(&v, &dev[SB_DRY][off], 4);
        return v;
    }
    float f(size_t off) const {
        float v;
        memcpy(&v, &dev[SB_DRY][off], 4);
        return v;
    }
};

static const char *set(Model &m, int slot, float mult, float base, int allowed, int range, int n, std::vector<int32_t> brk, int ctx) {
    SettingsEdits ed;
    const char *why = m.st.set_dry(slot, mult, base, allowed, range, n, brk.empty() ? nullptr : brk.data(), (int)brk.size(), ctx, ed);
    if (why) REQUIRE(ed.list.empty() && ed.needs == 0, "a refused call reported edits");
    else m.apply(ed);
    return why;
}
static void refused(Model &m, const char *want, float mult, float base, int allowed, int range, int n, std::vector<int32_t> brk) {
    const SlotSettings::State before = m.st.slots[0];
    const char *why = set(m, 0, mult, base, allowed, range, n, brk, 0);
    REQUIRE(why && std::string(why) == want, "expected \"%s\", got \"%s\"", want, why ? why : "(served)");
    REQUIRE(before.pen.dry_same(m.st.slots[0].pen), "a refused call changed the mirror");
    std::printf("refusal: %s\n", why);
}
// the device words of `slot` are the mirror's (neutral arming words where `neutral`)
static void follows(const Model &m, int slot, bool neutral) {
    const PenaltyParams &p = m.st.slots[slot].pen;
    const SlotSettings::Offsets &at = m.st.at;
    REQUIRE(m.f(at.dry_mult + slot * 4) == (neutral ? 0.f : p.dry_multiplier), "slot %d: multiplier", slot);
    REQUIRE(m.w(at.dry_ngram + slot * 4) == (neutral ? 0 : p.ngram), "slot %d: n-gram", slot);
    if (!p.dry_on()) return;
    REQUIRE(m.f(at.dry_base + slot * 4) == p.dry_base && m.w(at.dry_allowed + slot * 4) == p.dry_allowed && m.w(at.dry_range + slot * 4) == p.dry_range,
            "slot %d: base / allowed_length / range", slot);
    REQUIRE(m.w(at.dry_s0 + slot * 4) == p.dry_s0, "slot %d: s0", slot);
    REQUIRE(m.w(at.dry_nbreak + slot * 4) == (int)p.dry_breakers.size(), "slot %d: breaker count", slot);
    for (size_t k = 0; k < p.dry_breakers.size(); ++k)
        REQUIRE(m.w(at.dry_breakers + ((size_t)slot * m.st.sz.dry_max_breakers + k) * 4) == p.dry_breakers[k], "slot %d: breaker %zu", slot, k);
}

int main() {
    Model m;
    SlotSettings::Sizes sz{4, 1000, 8, 4, 20, 1024, 16, 32, 24, 524288, -1};
    sz.dry_seq_cap = 96, sz.dry_max_breakers = 64, sz.dry_max_match = 64;
    m.st.init(sz);
    m.make(SB_SAMPLE);

    // nothing is asked for before the first arming call; switching off an engine that never armed writes nothing
    REQUIRE(set(m, 0, 0.f, 1.75f, 2, 0, 0, {}, 0) == nullptr && !m.made[SB_DRY] && !m.made[SB_PROCESS], "an off call made a block");
    REQUIRE(!m.st.slots[0].pen.processes(), "an off slot processes");

    refused(m, "engine_set_dry: multiplier must be finite and >= 0 (0 = off)", -0.5f, 1.75f, 2, 0, 0, {});
    refused(m, "engine_set_dry: multiplier must be finite and >= 0 (0 = off)", INFINITY, 1.75f, 2, 0, 0, {});
    refused(m, "engine_set_dry: base must be finite and >= 1", 0.8f, 0.5f, 2, 0, 0, {});
    refused(m, "engine_set_dry: base must be finite and >= 1", 0.8f, NAN, 2, 0, 0, {});
    refused(m, "engine_set_dry: allowed_length must be >= 1", 0.8f, 1.75f, 0, 0, 0, {});
    refused(m, "engine_set_dry: range must be >= 0 (0 = the whole recorded sequence)", 0.8f, 1.75f, 2, -1, 0, {});
    refused(m, "engine_set_dry: no_repeat_ngram must be 0 (off) or 2 .. 64", 0.f, 1.75f, 2, 0, 1, {});
    refused(m, "engine_set_dry: no_repeat_ngram must be 0 (off) or 2 .. 64", 0.f, 1.75f, 2, 0, 65, {});
    refused(m, "engine_set_dry: between 0 and TL_MAX_DRY_BREAKERS (64) breakers", 0.8f, 1.75f, 2, 0, 0, std::vector<int32_t>(65, 1));
    refused(m, "engine_set_dry: breaker id out of range", 0.8f, 1.75f, 2, 0, 0, {3, 1000});
    refused(m, "engine_set_dry: breaker id out of range", 0.8f, 1.75f, 2, 0, 0, {-1});
    refused(m, "engine_set_dry: a breaker id appears twice", 0.8f, 1.75f, 2, 0, 0, {7, 3, 7});
    REQUIRE(!m.made[SB_DRY], "a refused call made the block");

    // arming: the block and the processed rows' block exist, the table is zero, s0 is the context length
    REQUIRE(set(m, 0, 0.8f, 1.75f, 2, 0, 3, {11, 5}, 20) == nullptr, "arming refused");
    REQUIRE(m.made[SB_DRY] && m.made[SB_PROCESS], "arming makes the sequence block and the processing block");
    REQUIRE(m.st.slots[0].pen.processes() && m.st.slots[0].pen.dry_s0 == 20, "an armed slot processes from its context length");
    for (size_t o = m.st.at.dry_table; o < m.st.at.dry_mult; ++o) REQUIRE(m.dev[SB_DRY][o] == 0, "a fresh table is all zeros");
    follows(m, 0, false);
    const StepFeatures f = m.st.features(0, 4, [](int) { return true; });
    REQUIRE(f.dry && f.processes && !f.grammar && !f.samples, "the plan of an armed slot");
    REQUIRE(!m.st.features(1, 3, [](int) { return true; }).dry, "the plan of the other slots");
    REQUIRE(m.st.refuses_rewind(0) && m.st.refuses_set_token(0) && m.st.refuses_verify(0) && m.st.refuses_verify_sampled(0) && m.st.refuses_verify_batch(0) &&
                m.st.refuses_beam(0), "an armed slot is refused like every processing slot");

    // changing parameters keeps s0; off and on again takes the new context length
    REQUIRE(set(m, 0, 0.5f, 2.f, 3, 40, 0, {9}, 33) == nullptr && m.st.slots[0].pen.dry_s0 == 20, "re-arming an armed slot keeps s0");
    follows(m, 0, false);
    REQUIRE(set(m, 0, 0.f, 1.75f, 2, 0, 0, {}, 35) == nullptr && !m.st.slots[0].pen.processes(), "switching off");
    follows(m, 0, false);
    REQUIRE(set(m, 0, 0.f, 1.75f, 2, 0, 4, {}, 35) == nullptr && m.st.slots[0].pen.dry_s0 == 35, "off and on again: s0 is the context length");
    follows(m, 0, false);

    // fork copies parameters, breakers, s0 and the sequence row; move carries them and leaves the source off
    REQUIRE(set(m, 0, 0.8f, 1.75f, 2, 0, 3, {11, 5}, 35) == nullptr, "re-arming refused");
    const size_t row = (size_t)sz.dry_seq_cap * 4;
    for (size_t o = 0; o < row; ++o) m.dev[SB_DRY][m.st.at.dry_seq + o] = (uint8_t)(o * 7 + 1);
    SettingsEdits ed;
    m.st.carry(0, 2, false, ed);
    m.apply(ed);
    follows(m, 0, false), follows(m, 2, false);
    REQUIRE(m.st.slots[2].pen.dry_same(m.st.slots[0].pen), "fork copies the mirror");
    REQUIRE(memcmp(&m.dev[SB_DRY][m.st.at.dry_seq + 2 * row], &m.dev[SB_DRY][m.st.at.dry_seq], row) == 0, "fork copies the sequence row");
    ed.clear();
    m.st.carry(2, 3, true, ed);
    m.apply(ed);
    follows(m, 3, false), follows(m, 2, false);
    REQUIRE(!m.st.slots[2].pen.processes() && m.st.slots[3].pen.dry_same(m.st.slots[0].pen), "move carries the mirror and leaves the source off");
    REQUIRE(memcmp(&m.dev[SB_DRY][m.st.at.dry_seq + 3 * row], &m.dev[SB_DRY][m.st.at.dry_seq], row) == 0, "move carries the sequence row");

    // park: the arming words go neutral, everything else stays; a setter on a parked slot keeps them neutral; unpark restores
    ed.clear();
    m.st.park(3, ed);
    m.apply(ed);
    follows(m, 3, true);
    REQUIRE(set(m, 3, 0.6f, 1.5f, 2, 0, 2, {4}, 50) == nullptr && m.st.slots[3].pen.dry_s0 == 35, "a parked slot takes parameters");
    follows(m, 3, true);
    ed.clear();
    m.st.unpark(3, ed);
    m.apply(ed);
    follows(m, 3, false);

    // reset: off
    ed.clear();
    m.st.reset(3, ed);
    m.apply(ed);
    REQUIRE(!m.st.slots[3].pen.processes(), "reset switches the slot off");
    follows(m, 3, false);
    follows(m, 0, false);

    std::printf("ok checks=%d\n", g_checks);
    return 0;
}
