// Stand-alone check of the prompt-lookup part of csrc/slot_settings.h (tests/test_lookup_cpu.py builds it with AddressSanitizer and UBSan
// and runs it as its own process): the host half of the history's accounting against a small model of the device.
//
// The model holds, per slot, what the engine's kernels see -- the token ring, `produced`, the context length, the pending token and the
// history row H inside the lookup block's bytes -- and beside them the TRUTH: the id that was really fed at every position.  Random
// calls (begin, arm, prefill chunks, multi-step decode calls, set_token, rewind, fork, move, release) go through the record exactly as
// engine.hip takes them; the catch-up is lookup.h's rule H[j] = ring[(produced - 1 - (ctx - j)) mod ring_cap].  After every call, for
// every armed slot, a propose launch's view is checked: caught up, H[j] equals the truth for s0 <= j < ctx, and no catch-up ever asked
// the ring for an id it no longer holds.  The ring is 8 ids, so calls that outrun it are common.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "slot_settings.h"

using namespace tl;

static long g_checks = 0;
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

constexpr int SLOTS = 4, RING = 8, CAP = 96, VOCAB = 5;

struct Dev {  // one slot of the device, and the truth beside it
    bool live = false;
    int ctx = 0, produced = 0;
    int32_t pending = 0;
    int32_t ring[RING] = {};
    std::vector<int32_t> truth;  // truth[j]: the id fed at position j
};

struct Model {
    SlotSettings st;
    std::vector<uint8_t> block;  // the lookup block
    bool made = false;
    Dev dev[SLOTS];
    std::mt19937 rng{12345};
    long catch_ups = 0, restarts = 0, fetched = 0, stale_pending = 0;

    int32_t *H(int slot) { return reinterpret_cast<int32_t *>(block.data() + st.at.lk_seq) + (size_t)slot * CAP; }
    int32_t fresh() { return (int32_t)(rng() % VOCAB); }

    void apply(const SettingsEdits &ed) {
        if ((ed.needs >> SB_LOOKUP & 1u) && !made) {
            block.assign(st.layout(SB_LOOKUP).bytes, 0xAB);  // (no fill rule: every byte starts undefined)
            REQUIRE(st.layout(SB_LOOKUP).fill.empty(), "the lookup block has no fill rules");
            made = true;
            st.created(SB_LOOKUP);
        }
        for (const SettingsEdit &x : ed.list) {
            if (x.block != SB_LOOKUP) continue;  // (sampling words and the like: not this program's)
            REQUIRE(made && x.kind == SettingsEdit::COPY, "the lookup block takes copies only");
            REQUIRE(x.off + x.bytes <= block.size() && x.from + x.bytes <= block.size(), "a copy leaves the lookup block");
            memmove(&block[x.off], &block[x.from], x.bytes);
        }
    }
    // ---- engine.hip's helpers ----
    void catch_up(int slot) {
        Dev &d = dev[slot];
        if (!st.lookup_behind(slot, d.ctx)) return;
        const int rec = st.slots[slot].lk_rec;
        REQUIRE(d.ctx - rec <= RING - 1, "slot %d: a catch-up of %d ids asks the ring of %d for ids it has lost", slot, d.ctx - rec, RING);
        for (int j = rec; j < d.ctx && j < CAP; ++j) {
            const int n = d.produced - 1 - (d.ctx - j);
            REQUIRE(n >= 0, "slot %d: the catch-up reaches behind the first produced id", slot);
            H(slot)[j] = d.ring[n % RING];
            ++fetched;
        }
        st.lookup_caught_up(slot, d.ctx);
        ++catch_ups;
    }
    void store_pending(int slot) {
        if (!st.lookup_on(slot)) return;
        catch_up(slot);
        if (dev[slot].ctx < CAP) H(slot)[dev[slot].ctx] = dev[slot].pending;
        st.lookup_pending(slot, dev[slot].ctx);
    }
    void produce(int slot) {  // a step end: the new id is the pending token and enters the ring
        Dev &d = dev[slot];
        d.pending = fresh();
        d.ring[d.produced % RING] = d.pending;
        d.produced++;
    }
    // ---- the calls ----
    void begin(int slot) {
        SettingsEdits ed;
        st.reset(slot, ed);
        apply(ed);
        dev[slot] = Dev{};
        dev[slot].live = true;
    }
    void release(int slot) {
        SettingsEdits ed;
        st.reset(slot, ed);
        apply(ed);
        dev[slot].live = false;
        REQUIRE(!st.lookup_on(slot), "release leaves slot %d armed", slot);
    }
    void arm(int slot, bool on) {
        SettingsEdits ed;
        const bool was = st.lookup_on(slot);
        REQUIRE(st.set_lookup(slot, on, dev[slot].ctx, ed) == nullptr, "set_lookup refused");
        apply(ed);
        if (on && !was) {
            REQUIRE(st.slots[slot].lk_s0 == dev[slot].ctx, "arming makes s0 the context length");
            store_pending(slot);
        }
    }
    void prefill(int slot, int n, bool want_logits) {
        Dev &d = dev[slot];
        if (d.ctx + n > CAP) return;
        std::vector<int32_t> chunk(n);
        for (int32_t &t : chunk) t = fresh();
        if (st.lookup_on(slot)) {  // lookup_record_chunk
            catch_up(slot);
            for (int i = 0; i < n; ++i) H(slot)[d.ctx + i] = chunk[i];
            st.lookup_recorded(slot, d.ctx, n);
        }
        d.truth.insert(d.truth.end(), chunk.begin(), chunk.end());
        d.ctx += n;
        st.appended(slot, true);
        if (want_logits) produce(slot), st.pending_produced(slot);
    }
    void decode(int steps) {  // over every live slot
        std::vector<int> restart;
        for (int b = 0; b < SLOTS; ++b)
            if (dev[b].live && dev[b].ctx + steps > CAP) return;  // (the engine refuses the call: no room)
        for (int b = 0; b < SLOTS; ++b) {
            if (!dev[b].live || !st.lookup_on(b)) continue;
            if (st.lookup_pending_unknown(b, dev[b].ctx)) store_pending(b), ++stale_pending;
            const SlotSettings::LookupDecode a = st.lookup_before_decode(b, dev[b].ctx, steps);
            if (a == SlotSettings::LOOKUP_CATCH_UP) catch_up(b);
            if (a == SlotSettings::LOOKUP_RESTART) restart.push_back(b);
        }
        for (int s = 0; s < steps; ++s)
            for (int b = 0; b < SLOTS; ++b) {
                if (!dev[b].live) continue;
                dev[b].truth.push_back(dev[b].pending);  // the step feeds the pending token at position ctx
                dev[b].ctx++;
                produce(b);
                st.pending_produced(b);
            }
        for (int b : restart) st.lookup_restart(b, dev[b].ctx), ++restarts;
    }
    void set_token(int slot) {
        dev[slot].pending = fresh();  // (not in the ring)
        store_pending(slot);
    }
    void rewind(int slot, int n) {
        Dev &d = dev[slot];
        if (n > d.ctx) return;
        catch_up(slot);
        d.ctx -= n;
        d.truth.resize(d.ctx);
        if (st.lookup_rewound(slot, d.ctx + n, d.ctx)) store_pending(slot);
    }
    void carry(int src, int dst, bool move) {
        catch_up(src);
        SettingsEdits ed;
        st.carry(src, dst, move, ed);
        apply(ed);
        dev[dst] = dev[src];
        dev[dst].produced = 0;  // the ring does not travel
        for (int32_t &r : dev[dst].ring) r = -7;
        if (move) dev[src] = Dev{};
        store_pending(dst);
        REQUIRE(!move || !st.lookup_on(src), "move leaves the source armed");
    }
    // what a propose launch would see
    void check(const char *after) {
        for (int b = 0; b < SLOTS; ++b) {
            if (!dev[b].live) {
                REQUIRE(!st.lookup_on(b), "after %s: free slot %d is armed", after, b);
                continue;
            }
            if (!st.lookup_on(b)) continue;
            const SlotSettings::State &s = st.slots[b];
            const Dev &d = dev[b];
            REQUIRE((int)d.truth.size() == d.ctx, "the model lost count");
            REQUIRE(s.lk_s0 >= 0 && s.lk_s0 <= d.ctx, "after %s: slot %d has s0 %d beyond its context %d", after, b, s.lk_s0, d.ctx);
            REQUIRE(s.lk_rec >= s.lk_s0 && s.lk_rec <= d.ctx + 1, "after %s: slot %d is recorded to %d at context %d", after, b, s.lk_rec, d.ctx);
            catch_up(b);  // (the launch's own fetch)
            for (int j = s.lk_s0; j < d.ctx; ++j)
                REQUIRE(H(b)[j] == d.truth[j], "after %s: slot %d holds %d at position %d, the id fed there was %d (s0 %d, context %d)", after, b, H(b)[j], j,
                        d.truth[j], s.lk_s0, d.ctx);
            if (s.lk_rec == d.ctx + 1 && d.ctx < CAP) REQUIRE(H(b)[d.ctx] == d.pending, "after %s: slot %d's stored pending token is stale", after, b);
        }
    }
};

int main() {
    Model m;
    SlotSettings::Sizes sz{SLOTS, 1000, RING, 4, 20, 1024, 16, 32, 24, 524288, -1};
    sz.lookup_seq_cap = CAP, sz.lookup_out_words = 576;
    m.st.init(sz);
    REQUIRE(m.st.layout(SB_LOOKUP).bytes >= (size_t)SLOTS * CAP * 4 + 576 * 4, "the block holds the rows and one launch's results");

    {  // the refusals and the plain cases
        SlotSettings none;
        SlotSettings::Sizes z = sz;
        z.lookup_seq_cap = 0;
        none.init(z);
        SettingsEdits ed;
        const char *why = none.set_lookup(0, true, 0, ed);
        REQUIRE(why && ed.needs == 0 && !none.lookup_on(0), "an engine without history rows arms nothing");
        std::printf("refusal: %s\n", why);
        REQUIRE(none.layout(SB_LOOKUP).bytes == 0, "... and its block is empty");
        REQUIRE(none.set_lookup(0, false, 0, ed) == nullptr && ed.needs == 0, "switching off asks for no block");
        z.lookup_seq_cap = (1 << 24) + 1;
        none.init(z);
        why = none.set_lookup(0, true, 0, ed);
        REQUIRE(why && ed.needs == 0, "positions beyond 24 bits are refused");
        std::printf("refusal: %s\n", why);
    }
    m.begin(0);
    m.prefill(0, 5, true);
    REQUIRE(!m.made, "nothing is made before the first arming");
    m.arm(0, true);
    REQUIRE(m.made && m.st.slots[0].lk_s0 == 5 && m.st.slots[0].lk_rec == 6, "armed at context 5 with the pending token stored");
    m.arm(0, true);
    REQUIRE(m.st.slots[0].lk_s0 == 5, "arming an armed slot changes nothing");
    m.decode(3);
    REQUIRE(m.st.slots[0].lk_rec == 6 && m.catch_ups == 0, "decode steps record nothing");
    m.check("three steps");
    REQUIRE(m.catch_ups == 1 && m.st.slots[0].lk_rec == 8, "the launch fetched positions 6 and 7");
    m.rewind(0, 5);
    REQUIRE(m.st.slots[0].lk_s0 == 3 && m.st.slots[0].lk_rec == 3, "a rewind below s0 lowers s0");
    REQUIRE(m.st.refuses_beam(0) != nullptr, "beam search refuses an armed slot");
    std::printf("refusal: %s\n", m.st.refuses_beam(0));
    m.decode(RING - 1);
    REQUIRE(m.restarts == 0, "a call of ring_cap - 1 steps keeps the history");
    m.check("ring_cap - 1 steps");
    m.decode(RING);
    REQUIRE(m.restarts == 1 && m.st.slots[0].lk_s0 == m.dev[0].ctx, "a call of ring_cap steps starts the history over behind it");
    m.check("ring_cap steps");
    m.arm(0, false);
    REQUIRE(!m.st.lookup_on(0), "switched off");
    m.release(0);

    // the random walk
    for (int b = 0; b < SLOTS; ++b) m.dev[b] = Dev{};
    const char *names[] = {"begin", "arm", "prefill", "decode", "set_token", "rewind", "fork", "move", "release", "disarm"};
    long served[10] = {};
    for (int it = 0; it < 60000; ++it) {
        const int op = (int)(m.rng() % 10), slot = (int)(m.rng() % SLOTS), other = (int)(m.rng() % SLOTS);
        Dev &d = m.dev[slot];
        bool ran = true;
        switch (op) {
        case 0: if (!d.live) m.begin(slot); else ran = false; break;
        case 1: if (d.live) m.arm(slot, true); else ran = false; break;
        case 2: if (d.live) m.prefill(slot, 1 + (int)(m.rng() % 6), m.rng() % 3 != 0); else ran = false; break;
        case 3: {
            static const int steps[] = {1, 1, 2, 3, 5, RING - 2, RING - 1, RING, RING + 3};
            m.decode(steps[m.rng() % 9]);  // (a slot fresh from begin, or prefilled without a first token, feeds whatever its pending word holds)
            break;
        }
        case 4: if (d.live) m.set_token(slot); else ran = false; break;
        case 5: if (d.live && d.ctx > 0) m.rewind(slot, 1 + (int)(m.rng() % std::min(d.ctx, 4))); else ran = false; break;
        case 6: case 7: if (d.live && !m.dev[other].live && slot != other) m.carry(slot, other, op == 7); else ran = false; break;
        case 8: if (d.live && (d.ctx > CAP - 12 || m.rng() % 4 == 0)) m.release(slot); else ran = false; break;
        case 9: if (d.live && m.rng() % 8 == 0) m.arm(slot, false); else ran = false; break;
        }
        if (!ran) continue;
        served[op]++;
        m.check(names[op]);
    }
    for (int op = 0; op < 10; ++op) {
        REQUIRE(served[op] > 100, "the walk hardly ever served %s", names[op]);
        std::printf("%s=%ld ", names[op], served[op]);
    }
    REQUIRE(m.catch_ups > 1000 && m.restarts > 100 && m.fetched > 1000 && m.stale_pending > 10, "the walk hardly ever caught up or started over");
    std::printf("\ncatch_ups=%ld restarts=%ld fetched=%ld stale_pending=%ld\nok checks=%ld\n", m.catch_ups, m.restarts, m.fetched, m.stale_pending, g_checks);
    return 0;
}
