// Stand-alone model check of csrc/kv_swap_model.h over csrc/prefix_cache.h (built and run by tests/test_kv_swap_cpu.py with
// -fsanitize=address,undefined): seeded random begin / append / fork / park / unpark / move / release / evict operations of the engine's
// slot protocol on a small pool -- pages of 4 tokens, a 3-token alphabet so that shared prefixes are the rule, 20 pages, an arena of 9
// records, the prefix cache on for one half of the run -- and after EVERY operation:
//   * pages_in_use + pages_free + pages_retained == num_pages, reference counts equal the number of holding slots, free-list hygiene;
//   * a page a slot references is never free (and never handed to anybody else: every row carries a fingerprint of the token prefix
//     that wrote it, and every unparked slot must read its own prefix back -- after an unpark from the records' copy);
//   * host records in use == sum over parked slots of ceil(context / page_size), no record held twice, a parked slot holds no page;
//   * a park or unpark that is refused changes nothing.
// Prints one line: the operation counts and a digest of every answer.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "kv_swap_model.h"

using namespace tl;

static constexpr int P = 4, PAGES = 20, SLOTS = 5, MAXP = 6, ALPHABET = 3, RECORDS = 9;

static long g_op = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED op %ld line %d: %s\n", g_op, __LINE__, #cond);  \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static uint64_t g_digest = 1469598103934665603ull;
static void note(uint64_t v) { g_digest = (g_digest ^ v) * 1099511628211ull; }

struct Slot {
    bool live = false, parked = false;
    std::vector<int> pages, records;
    std::vector<int32_t> actual;  // the tokens the slot holds: context = actual.size()
    SlotRecord rec;
};

static PagePool pool;
static SwapArena arena;
static Slot slots[SLOTS];
static uint64_t content[PAGES][P];    // fingerprint of the prefix that wrote each row of a page
static uint64_t stored[RECORDS][P];   // ... of a host record
static std::mt19937 rng;

static uint64_t fingerprint(const std::vector<int32_t> &t, size_t upto) {
    uint64_t h = 88172645463325252ull;
    for (size_t i = 0; i <= upto; ++i) h = (h ^ (uint64_t)(t[i] + 1)) * 6364136223846793005ull + 1442695040888963407ull;
    return h;
}
static int pick(int n) { return (int)(rng() % (uint32_t)n); }

static void check_invariants() {
    std::vector<int> holders(PAGES, 0), record_holders(RECORDS, 0);
    int parked_records = 0;
    for (const Slot &s : slots) {
        CHECK(s.live || (s.pages.empty() && s.actual.empty() && s.records.empty() && !s.parked));
        if (s.parked) {
            CHECK(s.pages.empty());
            CHECK((int)s.records.size() == swap_pages_of((int)s.actual.size(), P));
            parked_records += (int)s.records.size();
            for (int r : s.records) record_holders[r]++;
            for (size_t i = 0; i < s.actual.size(); ++i) CHECK(stored[s.records[i / P]][i % P] == fingerprint(s.actual, i));
        } else {
            CHECK(s.records.empty());
            CHECK((int)s.pages.size() == swap_pages_of((int)s.actual.size(), P));
            for (int p : s.pages) holders[p]++;
            for (size_t i = 0; i < s.actual.size(); ++i) CHECK(content[s.pages[i / P]][i % P] == fingerprint(s.actual, i));
        }
        CHECK(s.rec.known.size() <= s.actual.size());
        for (size_t i = 0; i < s.rec.known.size(); ++i) CHECK(s.rec.known[i] == s.actual[i]);
    }
    std::vector<char> is_free(PAGES, 0);
    for (int p : pool.free_pages) {
        CHECK(!is_free[p]);
        is_free[p] = 1;
        CHECK(holders[p] == 0);  // a page a slot references is never free
        CHECK(pool.refs[p] == 0 && !pool.is_indexed(p));
    }
    int in_use = 0, retained = 0;
    for (int p = 0; p < PAGES; ++p) {
        CHECK(pool.refs[p] == holders[p]);
        in_use += pool.refs[p] > 0;
        retained += pool.refs[p] == 0 && pool.is_indexed(p);
        CHECK(pool.refs[p] > 0 || pool.is_indexed(p) || is_free[p]);
    }
    CHECK(in_use == pool.in_use() && retained == pool.retained);
    CHECK(in_use + (int)pool.free_pages.size() + retained == PAGES);
    int used = 0;
    for (int r = 0; r < RECORDS; ++r) {
        CHECK(record_holders[r] == (arena.used[r] ? 1 : 0));
        used += arena.used[r];
    }
    CHECK(used == arena.in_use && used == parked_records);  // host records in use == sum over parked slots
}

// one more token for an unparked slot: a fresh page where the context ends on a boundary, copy-on-write of a shared / indexed tail
static bool append(Slot &s) {
    const size_t n = s.actual.size();
    if (n >= (size_t)MAXP * P) return false;
    if (n % P == 0) {
        if (!pool.can_take(1)) return false;
        s.pages.push_back(pool.take());
    } else if (pool.refs[s.pages.back()] > 1 || pool.is_indexed(s.pages.back())) {
        if (!pool.can_take(1)) return false;
        const int fresh = pool.take(), old = s.pages.back();
        for (int r = 0; r < P; ++r) content[fresh][r] = content[old][r];
        pool.drop(old);
        s.pages.back() = fresh;
    }
    s.actual.push_back(pick(ALPHABET));
    content[s.pages[n / P]][n % P] = fingerprint(s.actual, n);
    if (pool.enabled && pick(2)) {  // declared, like a prefill: full pages inside the known tokens are registered
        s.rec.known = s.actual;
        pool.register_slot(s.rec, s.pages);
    }
    return true;
}

int main(int argc, char **argv) {
    const long ops = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? (uint32_t)std::atol(argv[2]) : 12345u);
    pool.init(PAGES, P);
    arena.init(RECORDS);
    long begins = 0, appends = 0, forks = 0, parks = 0, park_refusals = 0, unparks = 0, unpark_refusals = 0, moves = 0, releases = 0, evicts = 0;
    for (g_op = 0; g_op < ops; ++g_op) {
        if (g_op == ops / 2) pool.enable(0);
        Slot &s = slots[pick(SLOTS)];
        const int op = pick(100);
        if (!s.live) {
            if (op < 60) {
                s.live = true;
                s.rec.clear();
                ++begins;
            }
        } else if (op < 40 && !s.parked) {
            for (int k = 1 + pick(6); k > 0 && append(s); --k) ++appends;
        } else if (op < 50 && !s.parked) {  // fork into a free slot: full pages shared, a partial tail copied
            Slot *d = nullptr;
            for (Slot &t : slots)
                if (!t.live) d = &t;
            const size_t n = s.actual.size();
            if (d && (n % P == 0 || pool.can_take(1))) {
                d->live = true;
                for (size_t j = 0; j < n / P; ++j) {
                    pool.share(s.pages[j]);
                    d->pages.push_back(s.pages[j]);
                }
                if (n % P) {
                    const int fresh = pool.take();
                    for (int r = 0; r < P; ++r) content[fresh][r] = content[s.pages.back()][r];
                    d->pages.push_back(fresh);
                }
                d->actual = s.actual;
                d->rec = s.rec;
                ++forks;
            }
        } else if (op < 65 && !s.parked) {
            const std::vector<int> pages_before = s.pages, free_before = pool.free_pages;
            std::vector<uint64_t> rows(s.actual.size());
            for (size_t i = 0; i < rows.size(); ++i) rows[i] = content[s.pages[i / P]][i % P];  // the gather, before the pages go
            const int free_records = arena.available();
            const bool ok = swap_park_host(pool, arena, pool.enabled ? &s.rec : nullptr, s.pages, (int)s.actual.size(), s.records);
            CHECK(ok == (!s.actual.empty() && swap_pages_of((int)s.actual.size(), P) <= free_records));
            if (ok) {
                for (size_t i = 0; i < rows.size(); ++i) stored[s.records[i / P]][i % P] = rows[i];
                s.parked = true;
                ++parks;
            } else {
                CHECK(s.pages == pages_before && pool.free_pages == free_before && s.records.empty());
                ++park_refusals;
            }
            note((uint64_t)ok);
        } else if (op < 85 && s.parked) {
            const std::vector<int> records = s.records, free_before = pool.free_pages;
            const size_t available = pool.available();
            const bool ok = swap_unpark_host(pool, arena, pool.enabled ? &s.rec : nullptr, s.pages, (int)s.actual.size(), s.records);
            CHECK(ok == ((size_t)records.size() <= available));
            if (ok) {
                for (size_t i = 0; i < s.actual.size(); ++i) content[s.pages[i / P]][i % P] = stored[records[i / P]][i % P];  // the scatter
                for (int p : s.pages) CHECK(pool.refs[p] == 1);  // fresh private pages
                s.parked = false;
                ++unparks;
            } else {
                CHECK(s.records == records && s.pages.empty() && pool.free_pages == free_before);
                ++unpark_refusals;
            }
            note((uint64_t)ok);
        } else if (op < 90) {  // move to a free slot: pages or records change hands
            Slot *d = nullptr;
            for (Slot &t : slots)
                if (!t.live) d = &t;
            if (d) {
                *d = std::move(s);
                s = Slot{};
                ++moves;
            }
        } else if (op < 97) {
            for (int p : s.pages) pool.drop(p);
            arena.give(s.records);
            s = Slot{};
            ++releases;
        } else if (pool.enabled) {  // eviction pressure: a cap that forces victims out, then no cap again
            const long before = pool.ctr.pages_evicted;
            pool.set_cap(1 + pick(3));
            pool.set_cap(0);
            evicts += pool.ctr.pages_evicted - before;
        }
        note((uint64_t)pool.free_pages.size() << 32 | (uint64_t)arena.in_use << 8 | (uint64_t)pool.retained);
        check_invariants();
    }
    std::printf("ok ops=%ld begins=%ld appends=%ld forks=%ld parks=%ld park_refusals=%ld unparks=%ld unpark_refusals=%ld moves=%ld releases=%ld "
                "evicted=%ld registered=%ld digest=%016llx\n",
                ops, begins, appends, forks, parks, park_refusals, unparks, unpark_refusals, moves, releases, pool.ctr.pages_evicted,
                pool.ctr.pages_registered, (unsigned long long)g_digest);
    (void)evicts;
    return 0;
}
