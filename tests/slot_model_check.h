// What the two stand-alone model checks share (prefix_cache_model_check.cpp, kv_swap_model_check.cpp): they drive csrc/slot_table.h --
// the code the engine runs -- and keep a model of the DEVICE beside it that learns of the table's decisions only through the edits a
// call reports:
//   * bt[][]       the block table: written from SlotEdits::rows alone.  Every slot reads its K/V through it, as the kernels do.
//   * content[][]  per page row a fingerprint of the token prefix that wrote it: written by an appended token's row, by
//                  SlotEdits::copies and by an unpark's scatter.  stored[][]: the same for the host records (a park's gather).
// So an edit the table forgets to report, a page handed out twice or a shared page written again shows as a slot that cannot read its
// own prefix back.  Beside that, after EVERY operation:
//   * the pool operations the call must have made (drops, shares, the reported `taken` ids in order) are replayed on a copy of the pool
//     taken before the call, every take against the brute-force victim and every drop against the brute-force evictions of the cap,
//     and the copy must end where the table's pool ended;
//   * a refused call reports no edit and changes nothing (a snapshot of every slot, the pool and the arena is compared);
//   * page identity, reference counts == holders, free-list hygiene, record accounting.
// The including file defines P, PAGES, SLOTS, MAXP, ALPHABET and RECORDS first.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "slot_table.h"

using namespace tl;

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

static SlotTable T;
static std::vector<int32_t> actual[SLOTS];  // the tokens each slot really holds: context = actual.size()
static int bt[SLOTS][MAXP];
static uint64_t content[PAGES][P];
static uint64_t stored[RECORDS + 1][P];
static long g_taken = 0;  // pages the edits reported as taken
static const char *g_why = nullptr;  // the last op_* call's refusal, as the table worded it (nullptr: it was served)
static bool refused_for(const char *what) { return g_why && std::strstr(g_why, what); }
static std::mt19937 rng;
static int pick(int n) { return (int)(rng() % (uint32_t)n); }

static uint64_t fingerprint(const std::vector<int32_t> &t, size_t upto) {  // of t[0 .. upto]
    uint64_t h = 88172645463325252ull;
    for (size_t i = 0; i <= upto; ++i) h = (h ^ (uint64_t)(t[i] + 1)) * 6364136223846793005ull + 1442695040888963407ull;
    return h;
}

static void model_init() {
    T.init(SLOTS, PAGES, P, MAXP);
    T.arena.init(RECORDS);
    for (auto &row : bt)
        for (int &id : row) id = -1;
}

// ---- brute force over a pool's public state -------------------------------------------------------------------------------------
static bool bf_is_ancestor(const PagePool &m, int a, int q) {  // a is q or above it
    for (; q != PagePool::ROOT; q = m.parent[q])
        if (q == a) return true;
    return false;
}
static int bf_victim(const PagePool &m) {  // least recent, childless, unreferenced, lower id
    int best = -1;
    if (!m.enabled) return best;
    for (int p = 0; p < PAGES; ++p) {
        if (!m.indexed[p] || m.refs[p] > 0) continue;
        bool child = false;
        for (int q = 0; q < PAGES; ++q) child |= m.indexed[q] && q != p && m.parent[q] == p;
        if (!child && (best < 0 || m.tick[p] < m.tick[best])) best = p;
    }
    return best;
}
static int bf_available(const PagePool &m) {  // free pages + retained pages whose subtree holds no referenced page
    int n = (int)m.free_pages.size();
    if (!m.enabled) return n;
    for (int p = 0; p < PAGES; ++p) {
        if (!m.indexed[p] || m.refs[p] > 0) continue;
        bool blocked = false;
        for (int q = 0; q < PAGES; ++q) blocked |= m.indexed[q] && m.refs[q] > 0 && bf_is_ancestor(m, p, q);
        n += blocked ? 0 : 1;
    }
    return n;
}

// ---- the replay of a call's pool operations on `m`, a copy of the pool from before the call --------------------------------------------
static void replay_take(PagePool &m, int reported) {
    const int expect = m.free_pages.empty() ? bf_victim(m) : m.free_pages.back();
    CHECK(expect >= 0 && reported == expect);
    CHECK(m.take() == expect);
    note((uint64_t)reported);
}
static void replay_drop(PagePool &m, int id) {
    PagePool q = m;  // the evictions the cap asks for, by brute force
    std::vector<int> expect_evicted;
    if (q.enabled && --q.refs[id] == 0 && q.indexed[id] && q.max_retained > 0) {
        for (int retained = q.retained + 1; retained > q.max_retained; --retained) {
            const int v = bf_victim(q);
            if (v < 0) break;
            q.indexed[v] = 0;
            expect_evicted.push_back(v);
        }
    }
    const long before = m.ctr.pages_evicted;
    m.drop(id);
    CHECK(m.ctr.pages_evicted - before == (long)expect_evicted.size());
    for (int v : expect_evicted) {
        CHECK(!m.indexed[v] && m.refs[v] == 0);
        note((uint64_t)v + 1000);
    }
}
static void replay_end(const PagePool &m, const SlotEdits &ed, size_t takes) {
    CHECK(ed.taken.size() == takes);
    g_taken += (long)takes;
    CHECK(m.refs == T.pool.refs && m.free_pages == T.pool.free_pages && m.retained == T.pool.retained);
    CHECK(m.ctr.pages_evicted == T.pool.ctr.pages_evicted);
    if (m.enabled)
        for (int p = 0; p < PAGES; ++p) CHECK(m.indexed[p] == T.pool.indexed[p] || (T.pool.indexed[p] && T.pool.refs[p] > 0));  // (a call may register pages in use)
}

// ---- "a refusal changes nothing" ----------------------------------------------------------------------------------------------------
struct Snapshot {
    std::vector<Slot> slots = T.slots;
    PagePool pool = T.pool;
    std::vector<char> used = T.arena.used;
    long allocations = T.page_allocations;
};
static void check_unchanged(const Snapshot &was, const SlotEdits &ed) {
    CHECK(ed.rows.empty() && ed.copies.empty() && ed.taken.empty());
    for (int i = 0; i < SLOTS; ++i) {
        const Slot &a = was.slots[i], &b = T.slots[i];
        CHECK(a.live == b.live && a.parked == b.parked && a.ctx == b.ctx && a.produced == b.produced && a.pages == b.pages && a.records == b.records);
        CHECK(a.rec.known == b.rec.known && a.rec.nodes == b.rec.nodes && a.rec.stuck == b.rec.stuck);
    }
    const PagePool &m = was.pool;
    CHECK(m.refs == T.pool.refs && m.free_pages == T.pool.free_pages && m.retained == T.pool.retained && m.n_entries == T.pool.n_entries);
    CHECK(m.indexed == T.pool.indexed && m.tick == T.pool.tick && m.ctr.pages_evicted == T.pool.ctr.pages_evicted);
    CHECK(was.used == T.arena.used && was.allocations == T.page_allocations);
}

// ---- the device model ---------------------------------------------------------------------------------------------------------------
static void apply(const SlotEdits &ed) {  // copies first, then the rows: the order the engine keeps
    for (const auto &c : ed.copies) {
        CHECK(c.rows >= 1 && c.rows <= P && c.from != c.to);
        for (int r = 0; r < c.rows; ++r) content[c.to][r] = content[c.from][r];
    }
    for (const auto &r : ed.rows) {
        CHECK(r.slot >= 0 && r.slot < SLOTS && r.index >= 0 && r.index < MAXP && r.page >= -1 && r.page < PAGES);
        bt[r.slot][r.index] = r.page;
    }
}
static void write_row(int slot, int32_t token) {  // one token's K/V lands where the block table says
    const size_t at = actual[slot].size();
    const int page = bt[slot][at / P];
    CHECK(page >= 0 && T.pool.refs[page] == 1 && !T.pool.is_indexed(page));  // an indexed or shared page is never written again
    actual[slot].push_back(token);
    content[page][at % P] = fingerprint(actual[slot], at);
}

// ---- the operations: the table's call, the expected answer, the edits applied, the replay ----------------------------------------------
// a prefill of `toks` (declared tokens: they extend the slot's known ones where those end)
static bool op_prefill(int slot, const std::vector<int32_t> &toks) {
    const Snapshot was;
    const Slot &s = T.slots[slot];
    const int need = swap_pages_of(s.ctx + (int)toks.size(), P), extra = std::max(0, need - (int)s.pages.size());
    const bool expect = need <= MAXP && extra <= bf_available(T.pool);
    SlotEdits ed;
    const bool ok = (g_why = T.reserve(slot, s.ctx + (int)toks.size(), ed)) == nullptr;
    CHECK(ok == expect);
    if (!ok) return check_unchanged(was, ed), false;
    apply(ed);
    PagePool m = was.pool;
    for (int id : ed.taken) replay_take(m, id);
    replay_end(m, ed, (size_t)extra);
    for (int32_t t : toks) write_row(slot, t);
    T.appended(slot, toks.data(), (int)toks.size());
    return true;
}
// one decode step over slots [0, batch): every running slot gets one token the engine does not know
static bool op_step(int batch) {
    const Snapshot was;
    bool expect = true;
    int extra = 0;
    for (int b = 0; b < batch; ++b) {
        if (!T.runs(b)) continue;
        const int need = swap_pages_of(T.slots[b].ctx + 1, P);
        expect &= need <= MAXP;
        extra += std::max(0, need - (int)T.slots[b].pages.size());
    }
    expect &= extra <= bf_available(T.pool);
    SlotEdits ed;
    int max_ctx = 1;
    const bool ok = (g_why = T.reserve_step(batch, ed, &max_ctx)) == nullptr;
    CHECK(ok == expect);
    if (!ok) return check_unchanged(was, ed), false;
    apply(ed);
    PagePool m = was.pool;
    for (int id : ed.taken) replay_take(m, id);
    replay_end(m, ed, (size_t)extra);
    for (int b = 0; b < batch; ++b) {
        if (!T.runs(b)) continue;
        CHECK(max_ctx >= T.slots[b].ctx + 1);
        write_row(b, pick(ALPHABET));
    }
    T.step_done(batch);
    return true;
}
static bool op_begin(int slot) {
    const Snapshot was;
    const bool ok = (g_why = T.begin(slot)) == nullptr;
    CHECK(ok == !was.slots[slot].live);
    if (!ok) check_unchanged(was, SlotEdits{});
    return ok;
}
static bool op_release(int slot) {
    const Snapshot was;
    SlotEdits ed;
    const bool ok = (g_why = T.release(slot, ed)) == nullptr;
    CHECK(ok == was.slots[slot].live);
    if (!ok) return check_unchanged(was, ed), false;
    apply(ed);
    PagePool m = was.pool;
    for (int p : was.slots[slot].pages) replay_drop(m, p);
    replay_end(m, ed, 0);
    actual[slot].clear();
    return true;
}
static bool op_rewind(int slot, int n) {
    const Snapshot was;
    const Slot &b = was.slots[slot];
    const int ctx = b.ctx - n, keep = swap_pages_of(ctx, P);
    bool expect = b.live && !b.parked && n >= 0 && n <= b.ctx, cow = false;
    if (expect) {
        cow = keep > 0 && ctx % P != 0 && (was.pool.refs[b.pages[keep - 1]] > 1 || was.pool.is_indexed(b.pages[keep - 1]));
        PagePool q = was.pool;  // the copy of the tail needs a page: one this rewind returns, or one that can be had once it has let go
        int will_free = 0;
        for (int j = keep; j < (int)b.pages.size(); ++j) will_free += --q.refs[b.pages[j]] == 0 && !q.is_indexed(b.pages[j]);
        expect = !cow || will_free >= 1 || bf_available(q) >= 1;
    }
    SlotEdits ed;
    const bool ok = (g_why = T.rewind(slot, n, ed)) == nullptr;
    CHECK(ok == expect);
    if (!ok) return check_unchanged(was, ed), false;
    apply(ed);
    PagePool m = was.pool;
    for (int j = (int)b.pages.size() - 1; j >= keep; --j) replay_drop(m, b.pages[j]);
    if (cow) {
        CHECK(ed.copies.size() == 1 && ed.copies[0].from == b.pages[keep - 1] && ed.copies[0].to == ed.taken.at(0) && ed.copies[0].rows == P);
        replay_take(m, ed.taken[0]);
        replay_drop(m, b.pages[keep - 1]);
    }
    replay_end(m, ed, cow ? 1 : 0);
    actual[slot].resize(ctx);
    return true;
}
static bool op_fork(int src, int dst) {
    const Snapshot was;
    const Slot &b = was.slots[src];
    const bool partial = b.ctx % P != 0;
    const bool expect = b.live && !b.parked && src != dst && !was.slots[dst].live && (!partial || bf_available(was.pool) >= 1);
    SlotEdits ed;
    const bool ok = (g_why = T.fork(src, dst, ed)) == nullptr;
    CHECK(ok == expect);
    if (!ok) return check_unchanged(was, ed), false;
    apply(ed);
    PagePool m = was.pool;
    for (int j = 0; j < b.ctx / P; ++j) m.share(b.pages[j]);
    if (partial) {
        CHECK(ed.copies.size() == 1 && ed.copies[0].from == b.pages[b.ctx / P] && ed.copies[0].to == ed.taken.at(0) && ed.copies[0].rows == P);
        replay_take(m, ed.taken[0]);
    }
    replay_end(m, ed, partial ? 1 : 0);
    actual[dst] = actual[src];
    return true;
}
static bool op_move(int src, int dst) {
    const Snapshot was;
    SlotEdits ed;
    const bool ok = (g_why = T.move(src, dst, ed)) == nullptr;
    CHECK(ok == (was.slots[src].live && src != dst && !was.slots[dst].live));
    if (!ok) return check_unchanged(was, ed), false;
    apply(ed);
    replay_end(was.pool, ed, 0);
    CHECK(T.slots[dst].parked == was.slots[src].parked && T.slots[dst].records == was.slots[src].records && !T.slots[src].live);
    actual[dst] = std::move(actual[src]);
    actual[src].clear();
    return true;
}
// park: the gather is "enqueued" between park_begin and park_commit; `enqueue_fails` plays a failed enqueue (park_abort)
static bool op_park(int slot, bool enqueue_fails) {
    const Snapshot was;
    const Slot &b = was.slots[slot];
    const int n = swap_pages_of(b.ctx, P);
    const bool expect = b.live && !b.parked && b.ctx >= 1 && n <= T.arena.available();
    SlotEdits ed;
    const bool ok = (g_why = T.park_begin(slot)) == nullptr;
    CHECK(ok == expect);
    if (!ok) return check_unchanged(was, ed), false;
    const std::vector<int> &records = T.slots[slot].records;
    CHECK((int)records.size() == n && T.slots[slot].pages == b.pages && !T.slots[slot].parked);
    if (enqueue_fails) {
        g_why = "(the copies could not be enqueued)";
        T.park_abort(slot);
        return check_unchanged(was, ed), false;
    }
    for (int i = 0; i < b.ctx; ++i) stored[records[i / P]][i % P] = content[bt[slot][i / P]][i % P];  // the gather reads the row on the device
    T.park_commit(slot, ed);
    apply(ed);
    PagePool m = was.pool;
    for (int p : b.pages) replay_drop(m, p);
    replay_end(m, ed, 0);
    return true;
}
static bool op_unpark(int slot) {
    const Snapshot was;
    const Slot &b = was.slots[slot];
    const bool expect = b.live && b.parked && (int)b.records.size() <= bf_available(was.pool);
    SlotEdits ed;
    std::vector<int> records;
    const bool ok = (g_why = T.unpark(slot, ed, records)) == nullptr;
    CHECK(ok == expect);
    if (!ok) return check_unchanged(was, ed), false;
    CHECK(records == b.records && T.slots[slot].records.empty());
    apply(ed);  // the row first: the scatter reads the page ids from it
    for (int i = 0; i < b.ctx; ++i) content[bt[slot][i / P]][i % P] = stored[records[i / P]][i % P];
    PagePool m = was.pool;
    for (int id : ed.taken) replay_take(m, id);
    replay_end(m, ed, records.size());
    for (int p : T.slots[slot].pages) CHECK(T.pool.refs[p] == 1);  // fresh private pages
    return true;
}

// ---- after every operation ----------------------------------------------------------------------------------------------------------
static void check_slots_pages_and_records() {
    std::vector<int> holders(PAGES, 0), record_holders(RECORDS + 1, 0);
    int parked_records = 0;
    for (int i = 0; i < SLOTS; ++i) {
        const Slot &s = T.slots[i];
        const std::vector<int32_t> &have = actual[i];
        CHECK(s.live || (s.pages.empty() && s.records.empty() && !s.parked && s.ctx == 0));
        CHECK(s.ctx == (int)have.size());
        if (s.parked) {
            CHECK(s.pages.empty() && (int)s.records.size() == swap_pages_of(s.ctx, P));
            parked_records += (int)s.records.size();
            for (int r : s.records) record_holders[r]++;
            for (size_t k = 0; k < have.size(); ++k) CHECK(stored[s.records[k / P]][k % P] == fingerprint(have, k));
        } else {
            CHECK(s.records.empty() && (int)s.pages.size() == swap_pages_of(s.ctx, P));
            for (int p : s.pages) holders[p]++;
        }
        for (int j = 0; j < MAXP; ++j) CHECK(bt[i][j] == (j < (int)s.pages.size() ? s.pages[j] : -1));  // the edits told the whole story
        if (!s.parked)
            for (size_t k = 0; k < have.size(); ++k) CHECK(content[bt[i][k / P]][k % P] == fingerprint(have, k));  // nothing a slot holds was lost
        CHECK(s.rec.known.size() <= have.size());
        for (size_t k = 0; k < s.rec.known.size(); ++k) CHECK(s.rec.known[k] == have[k]);
    }
    const PagePool &pool = T.pool;
    std::vector<char> is_free(PAGES, 0);
    for (int p : pool.free_pages) {
        CHECK(!is_free[p]);
        is_free[p] = 1;
        CHECK(holders[p] == 0 && pool.refs[p] == 0 && !pool.is_indexed(p));  // a page a slot references is never free
    }
    int in_use = 0, retained = 0;
    for (int p = 0; p < PAGES; ++p) {
        CHECK(pool.refs[p] == holders[p]);
        in_use += pool.refs[p] > 0;
        retained += pool.refs[p] == 0 && pool.is_indexed(p);
        CHECK(pool.refs[p] > 0 || pool.is_indexed(p) || is_free[p]);
    }
    CHECK(in_use + (int)pool.free_pages.size() + retained == PAGES);  // the page-count identity
    CHECK(retained == pool.retained && in_use == T.pages_in_use() && (int)pool.free_pages.size() == T.pages_free());
    CHECK(T.peak_pages_in_use >= in_use && T.page_allocations == g_taken && T.reused_page_allocations <= T.page_allocations);
    int used = 0;
    for (int r = 0; r < RECORDS; ++r) {
        CHECK(record_holders[r] == (T.arena.used[r] ? 1 : 0));
        used += T.arena.used[r];
    }
    CHECK(used == T.arena.in_use && used == parked_records);  // host records in use == sum over parked slots
    CHECK((int)pool.available() == bf_available(pool));
}
