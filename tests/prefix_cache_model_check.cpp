// Stand-alone model check of csrc/slot_table.h over csrc/prefix_cache.h (built and run by tests/test_prefix_cache_index_cpu.py with
// -fsanitize=address,undefined): seeded random operations of the engine's slot protocol -- SlotTable's own calls, the code the engine
// runs -- on a small pool: pages of 4 tokens, a 3-token alphabet so that shared prefixes are the rule, 24 pages.  After EVERY
// operation a comparison with brute force (slot_model_check.h holds what this check shares with kv_swap_model_check.cpp: the device
// model fed by the table's edits alone, the replay of every take and drop, "a refusal changes nothing", the page invariants):
//   * attach: the number of shared pages, the tail's source page and rows, and whether a page could be had for it, recomputed by
//     scanning every indexed page's full token sequence (rebuilt by walking parents) -- never through the hash;
//   * page contents: every page row carries a fingerprint of the whole token prefix that "wrote" it; every live slot must read its
//     own prefix back through the block table the edits built, so a referenced page that was evicted, an indexed page that was
//     written again or an edit that was not reported shows at once;
//   * the page-count identity, reference counts, free-list hygiene, no entry under a missing parent, ancestors never older than
//     descendants, every eviction taking exactly the brute-force victim (least recent, childless, unreferenced, lower id), the cap.
// Prints one line: the operation counts and a digest of every answer.  A second build with the hash forced to a constant must print
// the same line.
#include <string>

static constexpr int P = 4, PAGES = 24, SLOTS = 6, MAXP = 8, ALPHABET = 3, RECORDS = 0;
#include "slot_model_check.h"

static PagePool &pool = T.pool;

// the tokens from the root through entry p
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
    check_slots_pages_and_records();
    int entries = 0;
    for (int p = 0; p < PAGES; ++p) {
        if (!pool.is_indexed(p)) continue;
        entries++;
        const std::vector<int32_t> seq = bf_sequence(p);
        if (pool.parent[p] != PagePool::ROOT) CHECK(pool.tick[pool.parent[p]] >= pool.tick[p]);  // ancestors are never older
        for (int q = 0; q < p; ++q)  // one entry per (parent, tokens)
            if (pool.is_indexed(q) && pool.parent[q] == pool.parent[p]) CHECK(std::memcmp(&pool.toks[(size_t)q * P], &pool.toks[(size_t)p * P], P * 4) != 0);
        // an indexed page holds what its key says: its rows were written by exactly that token prefix
        for (int r = 0; r < P; ++r) CHECK(content[p][r] == fingerprint(seq, seq.size() - P + r));
    }
    CHECK(entries == pool.n_entries);
    if (pool.enabled && pool.max_retained > 0 && pool.retained > pool.max_retained) CHECK(bf_victim(pool) < 0);  // over the cap only while nothing can be evicted
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
static void op_attach(int slot, const std::vector<int32_t> &t) {
    const Snapshot was;
    const Expect x = bf_attach(t);
    // can a page be had for the tail, with the shared pages and the source held?
    PagePool m = was.pool;
    int expect_to = -1;
    if (x.tail_rows > 0) {
        int par = PagePool::ROOT;
        for (int j = 0; j < x.full; ++j) {
            par = pool.find_child(par, &t[(size_t)j * P]);
            CHECK(par >= 0);
            m.share(par);
        }
        m.share(x.tail_from);
        expect_to = m.free_pages.empty() ? bf_victim(m) : m.free_pages.back();
    }
    const long lookups = pool.ctr.lookups, matched_before = pool.ctr.tokens_matched;
    SlotEdits ed;
    int matched = -1;
    CHECK(T.attach(slot, t.data(), (int)t.size(), ed, &matched) == nullptr);
    apply(ed);
    const int tail_rows = ed.copies.empty() ? 0 : ed.copies[0].rows, full = (int)ed.rows.size() - (int)ed.copies.size();
    CHECK(full == x.full && ed.copies.size() <= 1);
    CHECK(tail_rows == (expect_to >= 0 ? x.tail_rows : 0));
    m = was.pool;  // the replay: the chain shared, the source held while the fresh page is taken
    for (int j = 0; j < full; ++j) m.share(ed.rows[j].page);
    if (tail_rows > 0) {
        CHECK(ed.copies[0].from == x.tail_from && ed.copies[0].to == expect_to && ed.rows.back().page == expect_to);
        m.share(x.tail_from);
        replay_take(m, ed.taken.at(0));
        if (--m.refs[x.tail_from] == 0) m.retained++;
    }
    replay_end(m, ed, tail_rows > 0 ? 1 : 0);
    CHECK(matched == full * P + tail_rows && matched <= (int)t.size() - 1);
    CHECK(pool.ctr.lookups == lookups + 1 && pool.ctr.tokens_matched == matched_before + matched);
    actual[slot].assign(t.begin(), t.begin() + matched);
    CHECK(T.slots[slot].rec.known == actual[slot]);
    note((uint64_t)matched * 131 + (uint64_t)(x.tail_from + 1) * 7 + (uint64_t)(expect_to + 1));
}

int main(int argc, char **argv) {
    const long ops = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? (unsigned)std::atol(argv[2]) : 12345u);
    model_init();
    T.prefix_enable(0);
    std::vector<std::vector<int32_t>> history;  // what requests asked for: new ones extend old ones
    auto random_tokens = [&](int n) {
        std::vector<int32_t> t(n);
        for (auto &v : t) v = pick(ALPHABET);
        return t;
    };
    long counts[10] = {0};
    check_invariants();
    for (g_op = 0; g_op < ops; ++g_op) {
        const int slot = pick(SLOTS);
        const Slot &s = T.slots[slot];
        const int kind = pick(100);
        if (!s.live) {
            if (kind < 12) {  // fork a slot (in whatever state) into this one
                counts[6] += op_fork(pick(SLOTS), slot);
            } else {          // a new request: a prefix of an earlier one + fresh tokens; attach, then prefill the rest in chunks
                std::vector<int32_t> t;
                if (!history.empty() && pick(4) != 0) {
                    const auto &h = history[pick((int)history.size())];
                    t.assign(h.begin(), h.begin() + pick((int)h.size() + 1));
                }
                const std::vector<int32_t> more = random_tokens(1 + pick(10));
                t.insert(t.end(), more.begin(), more.end());
                if ((int)t.size() > MAXP * P) t.resize(MAXP * P);
                CHECK(op_begin(slot));
                op_attach(slot, t);
                counts[0]++;
                bool ok = true;
                while (ok && actual[slot].size() < t.size()) {  // publish the rest
                    const size_t at = actual[slot].size(), n = std::min(t.size() - at, (size_t)(1 + pick(7)));
                    ok = op_prefill(slot, std::vector<int32_t>(t.begin() + at, t.begin() + at + n));
                }
                counts[1] += ok;
                if (history.size() < 24) history.push_back(t);
                else history[pick(24)] = t;
            }
        } else if (kind < 25) {
            counts[2] += op_release(slot);
        } else if (kind < 45) {  // decode steps over the first slots: tokens the engine does not know
            const int batch = 1 + pick(SLOTS);
            for (int k = 1 + pick(6); k > 0 && op_step(batch); --k) counts[3]++;
        } else if (kind < 60) {  // ... declared afterwards, in part or in whole; one token too many is refused
            const std::vector<int32_t> &have = actual[slot];
            const size_t known = s.rec.known.size(), unknown = have.size() - known;
            const Snapshot was;
            std::vector<int32_t> more(have.begin() + known, have.end());
            more.push_back(0);
            CHECK(T.extend(slot, more.data(), (int)more.size()) != nullptr);
            check_unchanged(was, SlotEdits{});
            if (pool.enabled && unknown > 0) {
                CHECK(T.extend(slot, more.data(), 1 + pick((int)unknown)) == nullptr);
                counts[4]++;
            }
        } else if (kind < 75) {  // allocate under pressure: a long prefill
            counts[1] += op_prefill(slot, random_tokens(4 + pick(12)));
        } else if (kind < 90) {
            if (s.ctx > 0) counts[5] += op_rewind(slot, pick(s.ctx + 1));
        } else if (kind < 93) {
            pool.clear();
            counts[7]++;
        } else if (kind < 99) {
            pool.set_cap(pick(3) == 0 ? 0 : 1 + pick(10));
            counts[8]++;
        } else {  // off and on again: every entry goes, the records of live slots start over
            T.prefix_disable();
            check_invariants();
            T.prefix_enable(pick(8));
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
