// Stand-alone model check of csrc/prefix_cache.h (built and run by tests/test_prefix_cache_index_cpu.py with
// -fsanitize=address,undefined): seeded random operations of the engine's slot protocol on a small pool -- pages of 4 tokens, a
// 3-token alphabet so that shared prefixes are the rule, 24 pages -- and after EVERY operation a comparison with brute force:
//   * attach: the number of shared pages, the tail's source page and rows, and whether a page could be had for it, recomputed by
//     scanning every indexed page's full token sequence (rebuilt by walking parents) -- never through the hash;
//   * page contents: every page row carries a fingerprint of the whole token prefix that "wrote" it; every live slot must read its
//     own prefix back, so a referenced page that was evicted, or an indexed page that was written again, shows at once;
//   * the page-count identity, reference counts, free-list hygiene, no entry under a missing parent, ancestors never older than
//     descendants, every eviction taking exactly the brute-force victim (least recent, childless, unreferenced, lower id), the cap.
// Prints one line: the operation counts and a digest of every answer.  A second build with the hash forced to a constant must print
// the same line.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "prefix_cache.h"

using namespace tl;

static constexpr int P = 4, PAGES = 24, SLOTS = 6, MAXP = 8, ALPHABET = 3;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::printf("FAILED op %ld line %d: %s\n", g_op, __LINE__, #cond);       \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static long g_op = 0;
static uint64_t g_digest = 1469598103934665603ull;
static void note(uint64_t v) { g_digest = (g_digest ^ v) * 1099511628211ull; }

struct Slot {
    bool live = false;
    std::vector<int> pages;
    std::vector<int32_t> actual;  // the tokens the slot really holds: context = actual.size()
    SlotRecord rec;
};

static PagePool pool;
static Slot slots[SLOTS];
static uint64_t content[PAGES][P];  // fingerprint of the prefix that wrote each row
static std::mt19937 rng;

static uint64_t fingerprint(const std::vector<int32_t> &t, size_t upto) {  // of t[0 .. upto]
    uint64_t h = 88172645463325252ull;
    for (size_t i = 0; i <= upto; ++i) h = (h ^ (uint64_t)(t[i] + 1)) * 6364136223846793005ull + 1442695040888963407ull;
    return h;
}

// ---- brute force over the pool's public state -----------------------------------------------------------------------------------
static bool bf_is_ancestor(int a, int q) {  // a is q or above it
    for (; q != PagePool::ROOT; q = pool.parent[q])
        if (q == a) return true;
    return false;
}
static bool bf_has_child(int p, const std::vector<char> &indexed) {
    for (int q = 0; q < PAGES; ++q)
        if (indexed[q] && q != p && pool.parent[q] == p) return true;
    return false;
}
static int bf_victim(const std::vector<char> &indexed, const std::vector<int> &refs) {
    int best = -1;
    for (int p = 0; p < PAGES; ++p) {
        if (!indexed[p] || refs[p] > 0 || bf_has_child(p, indexed)) continue;
        if (best < 0 || pool.tick[p] < pool.tick[best]) best = p;
    }
    return best;
}
static int bf_evictable() {
    if (!pool.enabled) return 0;
    int n = 0;
    for (int p = 0; p < PAGES; ++p) {
        if (!pool.indexed[p] || pool.refs[p] > 0) continue;
        bool blocked = false;
        for (int q = 0; q < PAGES; ++q) blocked |= pool.indexed[q] && pool.refs[q] > 0 && bf_is_ancestor(p, q);
        n += blocked ? 0 : 1;
    }
    return n;
}
static std::vector<int32_t> bf_sequence(int p) {  // the tokens from the root through entry p
    std::vector<int> chain;
    for (int q = p; q != PagePool::ROOT; q = pool.parent[q]) {
        CHECK(pool.indexed[q]);  // no entry under a missing parent
        chain.push_back(q);
        CHECK(chain.size() <= (size_t)PAGES);
    }
    std::vector<int32_t> seq;
    for (auto it = chain.rbegin(); it != chain.rend(); ++it) seq.insert(seq.end(), &pool.toks[(size_t)*it * P], &pool.toks[(size_t)*it * P] + P);
    return seq;
}

static void check_invariants() {
    std::vector<int> holders(PAGES, 0);
    for (const Slot &s : slots) {
        CHECK(s.live || (s.pages.empty() && s.actual.empty()));
        CHECK(s.pages.size() == (s.actual.size() + P - 1) / P || s.pages.size() == s.actual.size() / P + (s.actual.size() % P ? 1 : 0));
        for (int p : s.pages) holders[p]++;
        for (size_t i = 0; i < s.actual.size(); ++i) CHECK(content[s.pages[i / P]][i % P] == fingerprint(s.actual, i));  // nothing a slot holds was lost
        CHECK(s.rec.known.size() <= s.actual.size());
        for (size_t i = 0; i < s.rec.known.size(); ++i) CHECK(s.rec.known[i] == s.actual[i]);
    }
    std::vector<char> is_free(PAGES, 0);
    for (int p : pool.free_pages) {
        CHECK(!is_free[p]);
        is_free[p] = 1;
        CHECK(pool.refs[p] == 0 && !pool.is_indexed(p));
    }
    int in_use = 0, retained = 0, entries = 0;
    for (int p = 0; p < PAGES; ++p) {
        CHECK(pool.refs[p] == holders[p]);
        in_use += pool.refs[p] > 0;
        retained += pool.refs[p] == 0 && pool.is_indexed(p);
        CHECK(pool.refs[p] > 0 || pool.is_indexed(p) || is_free[p]);
        if (!pool.is_indexed(p)) continue;
        entries++;
        const std::vector<int32_t> seq = bf_sequence(p);
        if (pool.parent[p] != PagePool::ROOT) CHECK(pool.tick[pool.parent[p]] >= pool.tick[p]);  // ancestors are never older
        for (int q = 0; q < p; ++q)  // one entry per (parent, tokens)
            if (pool.is_indexed(q) && pool.parent[q] == pool.parent[p]) CHECK(std::memcmp(&pool.toks[(size_t)q * P], &pool.toks[(size_t)p * P], P * 4) != 0);
        // an indexed page holds what its key says: its rows were written by exactly that token prefix
        for (int r = 0; r < P; ++r) CHECK(content[p][r] == fingerprint(seq, seq.size() - P + r));
    }
    CHECK(in_use + (int)pool.free_pages.size() + retained == PAGES);  // the page-count identity
    CHECK(retained == pool.retained && in_use == pool.in_use() && entries == pool.n_entries);
    if (pool.enabled && pool.max_retained > 0 && retained > pool.max_retained) {
        std::vector<char> idx(pool.indexed.begin(), pool.indexed.end());
        CHECK(bf_victim(idx, pool.refs) < 0);  // over the cap only while nothing can be evicted
    }
    CHECK((int)pool.available() == (int)pool.free_pages.size() + bf_evictable());
}

// ---- the engine's operations, on the pool -----------------------------------------------------------------------------------------
static int take_checked() {  // the one allocation path, with the eviction order checked
    int expect = -1;
    if (pool.free_pages.empty()) {
        std::vector<char> idx(pool.indexed.begin(), pool.indexed.end());
        expect = bf_victim(idx, pool.refs);
        CHECK(expect >= 0);
    } else {
        expect = pool.free_pages.back();
    }
    const int id = pool.take();
    CHECK(id == expect);
    note((uint64_t)id);
    return id;
}
static void drop_checked(int id) {  // a drop, with the evictions the cap asks for checked against brute force
    std::vector<char> idx;
    std::vector<int> refs = pool.refs;
    if (pool.enabled) idx.assign(pool.indexed.begin(), pool.indexed.end());
    std::vector<int> expect_evicted;
    if (pool.enabled && --refs[id] == 0 && idx[id] && pool.max_retained > 0) {
        int retained = pool.retained + 1;
        while (retained > pool.max_retained) {
            const int v = bf_victim(idx, refs);
            if (v < 0) break;
            idx[v] = 0;
            expect_evicted.push_back(v);
            retained--;
        }
    }
    const long before = pool.ctr.pages_evicted;
    pool.drop(id);
    CHECK(pool.ctr.pages_evicted - before == (long)expect_evicted.size());
    for (int v : expect_evicted) {
        CHECK(!pool.indexed[v] && pool.refs[v] == 0);
        note((uint64_t)v + 1000);
    }
}
static void write_row(Slot &s, int32_t token) {  // append one token's K/V
    const size_t at = s.actual.size();
    const int page = s.pages[at / P];
    CHECK(pool.refs[page] == 1 && !pool.is_indexed(page));  // an indexed or shared page is never written again
    s.actual.push_back(token);
    content[page][at % P] = fingerprint(s.actual, at);
}
// prefill (known = true) or decode steps (known = false) of `toks`: all or nothing
static bool append(Slot &s, const std::vector<int32_t> &toks, bool known) {
    const size_t total = s.actual.size() + toks.size();
    const size_t need = (total + P - 1) / P;
    if (need > (size_t)MAXP) return false;
    const size_t extra = need > s.pages.size() ? need - s.pages.size() : 0;
    const bool can = extra <= pool.free_pages.size() + (size_t)bf_evictable();
    CHECK(pool.can_take(extra) == can);
    if (!can) return false;
    for (size_t j = 0; j < extra; ++j) s.pages.push_back(take_checked());
    const bool extends = known && pool.enabled && s.rec.known.size() == s.actual.size();
    for (int32_t t : toks) write_row(s, t);
    if (extends) {
        s.rec.known.insert(s.rec.known.end(), toks.begin(), toks.end());
        pool.register_slot(s.rec, s.pages);
    }
    return true;
}
static void release(Slot &s) {
    for (int p : s.pages) drop_checked(p);
    s = Slot{};
}
static void copy_page_rows(int from, int to, int rows) {
    for (int r = 0; r < rows; ++r) content[to][r] = content[from][r];
}
static bool rewind(Slot &s, int n) {
    const int ctx = (int)s.actual.size() - n, keep = (ctx + P - 1) / P;
    auto cow_needed = [&] { return keep > 0 && ctx % P != 0 && (pool.refs[s.pages[keep - 1]] > 1 || pool.is_indexed(s.pages[keep - 1])); };
    if (cow_needed()) {
        size_t will_free = 0;
        for (int j = keep; j < (int)s.pages.size(); ++j) will_free += --pool.refs[s.pages[j]] == 0 && !pool.is_indexed(s.pages[j]) ? 1 : 0;
        const bool ok = will_free >= 1 || pool.can_take(1);
        const bool expect = will_free >= 1 || pool.free_pages.size() + (size_t)bf_evictable() >= 1;
        for (int j = keep; j < (int)s.pages.size(); ++j) pool.refs[s.pages[j]]++;
        CHECK(ok == expect);
        if (!ok) return false;
    }
    while ((int)s.pages.size() > keep) {
        drop_checked(s.pages.back());
        s.pages.pop_back();
    }
    if (cow_needed()) {
        const int old_id = s.pages[keep - 1], fresh = take_checked();
        copy_page_rows(old_id, fresh, P);
        drop_checked(old_id);
        s.pages[keep - 1] = fresh;
    }
    s.actual.resize(ctx);
    if (pool.enabled) s.rec.rewind(ctx, P);
    return true;
}
static bool fork(Slot &src, Slot &dst) {
    const int ctx = (int)src.actual.size(), full = ctx / P;
    const bool partial = ctx % P != 0;
    if (partial && !pool.can_take(1)) return false;
    dst = Slot{};
    dst.live = true;
    for (int j = 0; j < full; ++j) {
        pool.share(src.pages[j]);
        dst.pages.push_back(src.pages[j]);
    }
    if (partial) {
        const int fresh = take_checked();
        copy_page_rows(src.pages[full], fresh, P);
        dst.pages.push_back(fresh);
    }
    dst.actual = src.actual;
    if (pool.enabled) dst.rec = src.rec;
    return true;
}

// the brute-force answer to an attach, from every indexed page's full sequence
struct Expect {
    int full = 0, tail_from = -1, tail_rows = 0;
};
static Expect bf_attach(const std::vector<int32_t> &t) {
    Expect x;
    const int limit = (int)t.size() - 1;
    std::vector<std::vector<int32_t>> seqs(PAGES);
    for (int p = 0; p < PAGES; ++p)
        if (pool.indexed[p]) seqs[p] = bf_sequence(p);
    auto common = [&](const std::vector<int32_t> &s) {
        size_t i = 0;
        while (i < s.size() && (int)i < limit && s[i] == t[i]) ++i;
        return (int)i;
    };
    for (int p = 0; p < PAGES; ++p)  // the longest fully matched sequence of whole pages
        if (pool.indexed[p] && (int)seqs[p].size() <= limit && common(seqs[p]) == (int)seqs[p].size() && (int)seqs[p].size() / P <= MAXP)
            x.full = std::max(x.full, (int)seqs[p].size() / P);
    if (x.full >= MAXP) return x;
    for (int p = 0; p < PAGES; ++p) {  // its children (sequences one page longer that agree on the matched part) by common prefix
        if (!pool.indexed[p] || (int)seqs[p].size() != (x.full + 1) * P) continue;
        const int c = common(seqs[p]);
        if (c < x.full * P) continue;
        const int rows = std::min(c, limit) - x.full * P;
        if (rows < 1) continue;
        if (rows > x.tail_rows || (rows == x.tail_rows && (pool.tick[p] > pool.tick[x.tail_from] || (pool.tick[p] == pool.tick[x.tail_from] && p < x.tail_from))))
            x.tail_from = p, x.tail_rows = rows;
    }
    return x;
}
static void attach(Slot &s, const std::vector<int32_t> &t) {
    const Expect x = bf_attach(t);
    // can a page be had for the tail, with the shared pages and the source held?
    bool tail_page = false;
    int expect_to = -1;
    if (x.tail_rows > 0) {
        std::vector<int> refs = pool.refs;
        int par = PagePool::ROOT;
        for (int j = 0; j < x.full; ++j) {
            par = pool.find_child(par, &t[(size_t)j * P]);
            CHECK(par >= 0);
            refs[par]++;
        }
        refs[x.tail_from]++;
        if (!pool.free_pages.empty()) {
            tail_page = true, expect_to = pool.free_pages.back();
        } else {
            std::vector<char> idx(pool.indexed.begin(), pool.indexed.end());
            expect_to = bf_victim(idx, refs);
            tail_page = expect_to >= 0;
        }
    }
    const long lookups = pool.ctr.lookups, matched_before = pool.ctr.tokens_matched;
    const AttachResult a = pool.attach(s.rec, s.pages, t.data(), (int)t.size(), MAXP);
    CHECK(a.full == x.full);
    CHECK(a.tail_rows == (tail_page ? x.tail_rows : 0));
    if (a.tail_rows > 0) {
        CHECK(a.tail_from == x.tail_from && a.tail_to == expect_to);
        copy_page_rows(a.tail_from, a.tail_to, a.tail_rows);
    }
    CHECK(a.matched == a.full * P + a.tail_rows && a.matched <= (int)t.size() - 1);
    CHECK(pool.ctr.lookups == lookups + 1 && pool.ctr.tokens_matched == matched_before + a.matched);
    s.actual.assign(t.begin(), t.begin() + a.matched);
    CHECK(s.rec.known == s.actual);
    note((uint64_t)a.matched * 131 + (uint64_t)(a.tail_from + 1) * 7 + (uint64_t)(a.tail_to + 1));
}

int main(int argc, char **argv) {
    const long ops = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? (unsigned)std::atol(argv[2]) : 12345u);
    pool.init(PAGES, P);
    pool.enable(0);
    std::vector<std::vector<int32_t>> history;  // what requests asked for: new ones extend old ones
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    auto random_tokens = [&](int n) {
        std::vector<int32_t> t(n);
        for (auto &v : t) v = pick(ALPHABET);
        return t;
    };
    long counts[10] = {0};
    check_invariants();
    for (g_op = 0; g_op < ops; ++g_op) {
        Slot &s = slots[pick(SLOTS)];
        const int kind = pick(100);
        if (!s.live) {
            if (kind < 12) {  // fork a live slot into this one
                Slot &src = slots[pick(SLOTS)];
                if (&src != &s && src.live) counts[6] += fork(src, s);
            } else {          // a new request: a prefix of an earlier one + fresh tokens; attach, then prefill the rest in chunks
                std::vector<int32_t> t;
                if (!history.empty() && pick(4) != 0) {
                    const auto &h = history[pick((int)history.size())];
                    t.assign(h.begin(), h.begin() + pick((int)h.size() + 1));
                }
                const std::vector<int32_t> more = random_tokens(1 + pick(10));
                t.insert(t.end(), more.begin(), more.end());
                if ((int)t.size() > MAXP * P) t.resize(MAXP * P);
                s.live = true;
                if (pool.enabled) attach(s, t);
                counts[0]++;
                bool ok = true;
                while (ok && s.actual.size() < t.size()) {  // publish the rest
                    const size_t n = std::min(t.size() - s.actual.size(), (size_t)(1 + pick(7)));
                    ok = append(s, std::vector<int32_t>(t.begin() + s.actual.size(), t.begin() + s.actual.size() + n), true);
                }
                counts[1] += ok;
                if (history.size() < 24) history.push_back(t);
                else history[pick(24)] = t;
            }
        } else if (kind < 25) {
            release(s);
            counts[2]++;
        } else if (kind < 45) {  // decode steps: tokens the engine does not know
            counts[3] += append(s, random_tokens(1 + pick(6)), false);
        } else if (kind < 60) {  // ... declared afterwards, in part or in whole
            const size_t unknown = s.actual.size() - s.rec.known.size();
            if (pool.enabled && unknown > 0) {
                const size_t n = 1 + pick((int)unknown);
                s.rec.known.insert(s.rec.known.end(), s.actual.begin() + s.rec.known.size(), s.actual.begin() + s.rec.known.size() + n);
                pool.register_slot(s.rec, s.pages);
                counts[4]++;
            }
        } else if (kind < 75) {  // allocate under pressure: a long prefill
            counts[1] += append(s, random_tokens(4 + pick(12)), true);
        } else if (kind < 90) {
            if (!s.actual.empty()) counts[5] += rewind(s, pick((int)s.actual.size() + 1));
        } else if (kind < 93) {
            pool.clear();
            counts[7]++;
        } else if (kind < 99) {
            pool.set_cap(pick(3) == 0 ? 0 : 1 + pick(10));
            counts[8]++;
        } else {  // off and on again: every entry goes, the records of live slots start over
            pool.disable();
            for (Slot &x : slots) x.rec.clear();
            check_invariants();
            pool.enable(pick(8));
            counts[9]++;
        }
        check_invariants();
        note((uint64_t)pool.retained * 31 + (uint64_t)pool.free_pages.size());
    }
    std::printf("ok ops=%ld requests=%ld appends=%ld releases=%ld decodes=%ld extends=%ld rewinds=%ld forks=%ld clears=%ld caps=%ld toggles=%ld "
                "hits=%ld matched=%ld tails=%ld registered=%ld evicted=%ld digest=%016llx\n",
                ops, counts[0], counts[1], counts[2], counts[3], counts[4], counts[5], counts[6], counts[7], counts[8], counts[9], pool.ctr.hits,
                pool.ctr.tokens_matched, pool.ctr.tail_rows_copied, pool.ctr.pages_registered, pool.ctr.pages_evicted, (unsigned long long)g_digest);
    return 0;
}
