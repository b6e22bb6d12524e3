// Stand-alone check of csrc/stop_set.h (the automaton every stop set is built with) and of the slot table's stopped state
// (csrc/slot_table.h), without a device.  Built with AddressSanitizer and UBSan by tests/test_stop_cpu.py.
//
//   stop_set_check <rounds> <seed>
//
// Random string sets over a three-letter alphabet, where overlaps are dense, plus the fixed sets that have bitten automata before: one
// string a suffix of another, "aab" against "aaab", 16 strings of exactly 1,024 bytes together, a 1-byte string.  For every prefix of
// random texts the automaton's answer -- does a string end here, and which is the longest -- is compared with a naive scan.  Then the
// invalid sets: each is refused and leaves the output untouched.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "slot_table.h"
#include "stop_set.h"

using namespace tl;

static long checked = 0, matches = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static const char *build(const std::vector<std::string> &strings, const std::vector<int32_t> &ids, int vocab, StopSet &out) {
    std::vector<uint8_t> bytes;
    std::vector<int32_t> offsets(1, 0);
    for (const std::string &s : strings) {
        bytes.insert(bytes.end(), s.begin(), s.end());
        offsets.push_back((int32_t)bytes.size());
    }
    return stop_set_build(vocab, ids.data(), (int)ids.size(), bytes.data(), offsets.data(), (int)strings.size(), out);
}

// the longest string that ends at text[0 .. end), or -1
static int naive(const std::vector<std::string> &strings, const std::string &text, size_t end) {
    int best = -1;
    for (size_t k = 0; k < strings.size(); ++k) {
        const std::string &s = strings[k];
        if (s.size() <= end && text.compare(end - s.size(), s.size(), s) == 0 && (best < 0 || s.size() > strings[best].size())) best = (int)k;
    }
    return best;
}

static void check_set(const std::vector<std::string> &strings, std::mt19937 &rng, int texts, int text_len, int letters) {
    StopSet set;
    CHECK(build(strings, {}, 0, set) == nullptr);
    size_t total = 0, longest = 0;
    for (const std::string &s : strings) total += s.size(), longest = std::max(longest, s.size());
    CHECK(set.n_states >= 2 && set.n_states <= (int)total + 1 && set.max_len == (int)longest);
    CHECK((int)set.table.size() == set.n_states * 256 && (int)set.match.size() == set.n_states);
    for (uint16_t t : set.table) CHECK(t < set.n_states);
    for (int t = 0; t < texts; ++t) {
        std::string text;
        for (int i = 0; i < text_len; ++i) text.push_back((char)('a' + rng() % letters));
        int state = 0;
        for (size_t i = 0; i < text.size(); ++i) {
            state = set.table[(size_t)state * 256 + (uint8_t)text[i]];
            const int want = naive(strings, text, i + 1);
            CHECK(set.match[state] == want);
            if (want >= 0) {
                CHECK(set.match_len[state] == strings[want].size());
                ++matches;
            }
            ++checked;
        }
        // the walk the rows use: from a state, over a piece of text, to the first byte at which a string ends
        const size_t cut = rng() % text.size();
        int st = 0, at = -1, index = -1, len = -1;
        (void)stop_set_walk(set, &st, (const uint8_t *)text.data(), (int)cut, &at, &index, &len);
        st = 0;
        for (size_t i = 0; i < cut; ++i) st = set.table[(size_t)st * 256 + (uint8_t)text[i]];
        const bool hit = stop_set_walk(set, &st, (const uint8_t *)text.data() + cut, (int)(text.size() - cut), &at, &index, &len);
        size_t first = cut;
        while (first < text.size() && naive(strings, text, first + 1) < 0) ++first;
        CHECK(hit == (first < text.size()));
        if (hit) CHECK(at == (int)(first - cut) && index == naive(strings, text, first + 1) && len == (int)strings[index].size());
    }
}

static void invalid_sets() {
    StopSet out;
    out.n_states = 77;  // a refusal leaves it alone
    auto refused = [&](const std::vector<std::string> &strings, const std::vector<int32_t> &ids, int vocab) {
        const char *why = build(strings, ids, vocab, out);
        CHECK(why != nullptr && out.n_states == 77 && out.table.empty() && out.ids.empty());
    };
    refused({"ab", ""}, {}, 0);                       // an empty string
    refused({"ab", "c", "ab"}, {}, 0);                // a duplicate
    refused(std::vector<std::string>(17, "x"), {}, 0);  // 17 strings (duplicates too; the count is checked first)
    {
        std::vector<std::string> many;
        for (int i = 0; i < 17; ++i) many.push_back(std::string(1, (char)('a' + i)));
        refused(many, {}, 0);
    }
    refused({std::string(1000, 'a'), std::string(25, 'b')}, {}, 0);  // 1,025 bytes
    refused({}, {5, 1024}, 1024);                     // an id out of range
    refused({}, {-1}, 0);
    refused({}, {3, 9, 3}, 1024);                     // a duplicate id
    refused({}, std::vector<int32_t>{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, 1024);
    refused({}, {}, 1024);                            // nothing at all
    CHECK(build({std::string(1000, 'a'), std::string(24, 'b')}, {1023}, 1024, out) == nullptr);  // exactly 1,024 bytes, the last id
    CHECK(out.n_states == 1025 && out.ids.size() == 1 && out.id_index(1023) == 0 && out.id_index(5) == -1);
}

// the slot table's stopped state: no decode step takes the slot, stop() takes the device's counters, the pages stay, fork copies and
// move carries the state, park / unpark keep it, begin and release clear it, and the page identity holds throughout
static void slot_table_stopped() {
    SlotTable t;
    t.init(4, 16, 4, 8);
    SlotEdits ed;
    auto identity = [&]() { CHECK(t.pages_in_use() + t.pages_free() + t.pool.retained == 16); };
    CHECK(t.begin(0) == nullptr && t.begin(1) == nullptr);
    const int32_t toks[5] = {1, 2, 3, 4, 5};
    CHECK(t.reserve(0, 5, ed) == nullptr && t.reserve(1, 5, ed) == nullptr);
    t.appended(0, toks, 5);
    t.appended(1, toks, 5);
    int max_ctx = 0;
    for (int s = 0; s < 6; ++s) {  // six steps for both; slot 0 froze after two of them
        CHECK(t.reserve_step(2, ed, &max_ctx) == nullptr);
        t.step_done(2);
    }
    CHECK(t.slots[0].ctx == 11 && t.slots[0].produced == 6 && t.slots[0].pages.size() == 3);
    t.stop(0, 7, 2);
    CHECK(!t.runs(0) && t.runs(1) && t.slots[0].stopped && t.slots[0].ctx == 7 && t.slots[0].produced == 2);
    CHECK(t.slots[0].pages.size() == 3);  // the pages of the steps it did not take stay
    identity();
    const int in_use = t.pages_in_use();
    CHECK(t.reserve_step(2, ed, &max_ctx) == nullptr);
    t.step_done(2);
    CHECK(t.slots[0].ctx == 7 && t.slots[0].produced == 2 && t.slots[1].ctx == 12 && t.pages_in_use() == in_use);
    // fork copies, move carries
    CHECK(t.fork(0, 2, ed) == nullptr && t.slots[2].stopped && t.slots[2].ctx == 7 && !t.runs(2));
    CHECK(t.move(2, 3, ed) == nullptr && t.slots[3].stopped && !t.slots[2].live && !t.slots[2].stopped);
    identity();
    // park / unpark keep it
    t.arena.init(8);
    CHECK(t.park_begin(3) == nullptr);
    t.park_commit(3, ed);
    CHECK(t.slots[3].parked && t.slots[3].stopped);
    std::vector<int> records;
    CHECK(t.unpark(3, ed, records) == nullptr && t.slots[3].stopped && !t.runs(3));
    identity();
    // a rewind works on a stopped slot and returns the pages beyond the context; resume: a step takes it again
    CHECK(t.rewind(0, 4, ed) == nullptr && t.slots[0].ctx == 3 && t.slots[0].pages.size() == 1 && t.slots[0].stopped);
    t.resume(0);
    CHECK(t.runs(0));
    t.stop(0, 3, 2);
    CHECK(t.release(0, ed) == nullptr && !t.slots[0].stopped && t.begin(0) == nullptr && t.runs(0) && !t.slots[0].stopped);
    CHECK(t.release(0, ed) == nullptr && t.release(1, ed) == nullptr && t.release(3, ed) == nullptr);
    identity();
    CHECK(t.pages_in_use() == 0);
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 200;
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    // the fixed sets
    check_set({"abc", "bc"}, rng, 50, 60, 3);                       // one string a suffix of another
    check_set({"aab", "aaab"}, rng, 50, 60, 2);
    check_set({"a"}, rng, 20, 30, 3);                               // a 1-byte string
    check_set({"b", "ab", "cab", "abcab"}, rng, 50, 60, 3);
    {   // 16 strings summing to exactly 1,024 bytes: distinct random strings of 64 bytes
        std::vector<std::string> big;
        while (big.size() < 16) {
            std::string s;
            for (int i = 0; i < 64; ++i) s.push_back((char)('a' + rng() % 3));
            if (std::find(big.begin(), big.end(), s) == big.end()) big.push_back(s);
        }
        StopSet set;
        CHECK(build(big, {}, 0, set) == nullptr && set.max_len == 64);
        check_set(big, rng, 4, 400, 3);
        // ... and texts that hold the strings themselves
        std::string text = "ccab";
        for (const std::string &s : big) text += s + "a";
        int state = 0;
        long hits = 0;
        for (size_t i = 0; i < text.size(); ++i) {
            state = set.table[(size_t)state * 256 + (uint8_t)text[i]];
            CHECK(set.match[state] == naive(big, text, i + 1));
            hits += set.match[state] >= 0;
        }
        CHECK(hits >= 16);
    }
    for (int r = 0; r < rounds; ++r) {
        const int n = 1 + (int)(rng() % 16);
        std::vector<std::string> strings;
        size_t total = 0;
        while ((int)strings.size() < n) {
            const size_t len = 1 + rng() % (rng() % 4 == 0 ? 40 : 6);
            std::string s;
            for (size_t i = 0; i < len; ++i) s.push_back((char)('a' + rng() % 3));
            if (total + len > 1024 || std::find(strings.begin(), strings.end(), s) != strings.end()) continue;
            strings.push_back(s), total += len;
        }
        check_set(strings, rng, 6, 120, 3);
    }
    invalid_sets();
    slot_table_stopped();
    std::printf("ok rounds=%d checked=%ld matches=%ld\n", rounds, checked, matches);
    return 0;
}
