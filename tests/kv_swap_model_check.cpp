// Stand-alone model check of csrc/slot_table.h with KV swap (built and run by tests/test_kv_swap_cpu.py with
// -fsanitize=address,undefined): seeded random begin / prefill / decode step / rewind / attach / fork / park / unpark / move / release /
// evict operations -- SlotTable's own calls, the code the engine runs, on slots in every state -- on a small pool: pages of 4 tokens, a
// 3-token alphabet so that shared prefixes are the rule, 12 pages (the six slots can ask for 36), an arena of 9 records, the prefix cache on for one half of the run.
// After EVERY operation (slot_model_check.h holds what this check shares with prefix_cache_model_check.cpp):
//   * pages_in_use + pages_free + pages_retained == num_pages, reference counts equal the number of holding slots, free-list hygiene;
//   * a page a slot references is never free (and never handed to anybody else: every row carries a fingerprint of the token prefix
//     that wrote it, and every unparked slot must read its own prefix back through the block table the edits built -- after an unpark
//     from the records' copy); a shared or indexed page is never written again;
//   * host records in use == sum over parked slots of ceil(context / page_size), no record held twice, a parked slot holds no page;
//   * every take and every cap-forced eviction is the brute-force victim;
//   * a call that is refused -- a park, an unpark, a fork, a rewind, a decode step over several slots that the pool cannot serve, a
//     park whose copies could not be enqueued -- changes nothing.
// Prints one line: the operation counts and a digest of every answer.  The *_refusals count calls refused for want of pages or records,
// by the table's own message, not calls on a slot in the wrong state (those are made and checked too).
static constexpr int P = 4, PAGES = 12, SLOTS = 6, MAXP = 6, ALPHABET = 3, RECORDS = 9;
#include "slot_model_check.h"

// attach without the brute-force answer (prefix_cache_model_check.cpp has it): what it shared and copied must read back as t's prefix
static int op_attach(int slot, const std::vector<int32_t> &t) {
    const Snapshot was;
    SlotEdits ed;
    int matched = -1;
    const Slot &b = was.slots[slot];
    const bool ok = T.attach(slot, t.data(), (int)t.size(), ed, &matched) == nullptr;
    CHECK(ok == (b.live && !b.parked && b.ctx == 0 && b.pages.empty()));
    if (!ok) return check_unchanged(was, ed), -1;
    apply(ed);
    PagePool m = was.pool;
    CHECK(ed.copies.size() <= 1 && ed.copies.size() <= ed.rows.size());
    const size_t full = ed.rows.size() - ed.copies.size();
    for (size_t j = 0; j < full; ++j) m.share(ed.rows[j].page);
    if (!ed.copies.empty()) {
        const int from = ed.copies[0].from;
        CHECK(ed.copies[0].to == ed.taken.at(0) && ed.rows.back().page == ed.taken[0]);
        m.share(from);  // held while the fresh page is taken
        replay_take(m, ed.taken[0]);
        if (--m.refs[from] == 0) m.retained++;
    }
    replay_end(m, ed, ed.copies.size());
    CHECK(matched == (int)full * P + (ed.copies.empty() ? 0 : ed.copies[0].rows) && matched < (int)t.size());
    actual[slot].assign(t.begin(), t.begin() + matched);
    return matched;
}

int main(int argc, char **argv) {
    const long ops = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? (uint32_t)std::atol(argv[2]) : 12345u);
    model_init();
    auto random_tokens = [&](int n) {
        std::vector<int32_t> t(n);
        for (auto &v : t) v = pick(ALPHABET);
        return t;
    };
    std::vector<int32_t> last;
    long begins = 0, appends = 0, forks = 0, fork_refusals = 0, parks = 0, park_refusals = 0, unparks = 0, unpark_refusals = 0, moves = 0, releases = 0,
         rewinds = 0, rewind_refusals = 0, attaches = 0, step_refusals = 0;
    for (g_op = 0; g_op < ops; ++g_op) {
        if (g_op == ops / 2) T.prefix_enable(0);
        int slot = pick(SLOTS);
        int other = pick(SLOTS);  // the second slot of a fork or move: mostly a free one, sometimes any
        for (int i = 0; i < SLOTS && pick(8); ++i)
            if (!T.slots[i].live) other = i;
        int op = pick(100);
        const bool exhausted = T.pool.available() == 0;
        if (exhausted && pick(2)) {  // an exhausted pool: forks and rewinds that need a page meet it often
            op = 42 + pick(18);
            for (int i = 0; i < SLOTS; ++i) {  // a source with a partial tail; a slot whose last page is full and shared or indexed
                const Slot &c = T.slots[i];
                if (op < 52 ? T.runs(i) && c.ctx % P != 0
                            : T.runs(i) && c.ctx > 0 && c.ctx % P == 0 && (T.pool.refs[c.pages.back()] > 1 || T.pool.is_indexed(c.pages.back())))
                    slot = i;
            }
        }
        const Slot &s = T.slots[slot];
        if (!s.live && op < 80) {  // a new sequence: with the cache on it looks its prompt up, then prefills the rest (or what fits)
            begins += op_begin(slot);
            std::vector<int32_t> t = random_tokens(1 + pick(MAXP * P));
            if (pick(2)) std::copy(last.begin(), last.begin() + std::min(last.size(), t.size()), t.begin());  // (often a prompt seen before)
            last = t;
            if (T.pool.enabled && op_attach(slot, t) > 0) ++attaches;
            const size_t at = actual[slot].size();
            if (pick(4) && op_prefill(slot, std::vector<int32_t>(t.begin() + at, t.end()))) appends += (long)(t.size() - at);
        } else if (op < 35) {  // decode steps over the first slots, parked and free ones among them: all of them or none
            const int batch = 1 + pick(SLOTS);
            for (int k = 1 + pick(4); k > 0; --k) {
                int running = 0;
                for (int b = 0; b < batch; ++b) running += T.runs(b);
                if (op_step(batch)) appends += running;
                else step_refusals += refused_for("KV page pool exhausted");
            }
        } else if (op < 42) {  // a prefill chunk (refused for a free or parked slot)
            const std::vector<int32_t> t = random_tokens(1 + pick(6));
            if (T.runs(slot)) {
                appends += op_prefill(slot, t) ? (long)t.size() : 0;
            } else {
                const Snapshot was;
                SlotEdits ed;
                CHECK(T.reserve(slot, s.ctx + (int)t.size(), ed) != nullptr);
                check_unchanged(was, ed);
            }
        } else if (op < 52) {  // fork, whatever state the two slots are in: full pages shared, a partial tail copied
            if (op_fork(slot, other)) ++forks;
            else fork_refusals += refused_for("KV page pool exhausted");
        } else if (op < 60) {
            if (op_rewind(slot, pick(2) && !exhausted ? pick(s.ctx + 2) : 1 + pick(P - 1))) ++rewinds;  // (one past the start, and a free or parked slot: refused)
            else rewind_refusals += refused_for("KV page pool exhausted");
        } else if (op < 72) {  // (one park in eight meets an enqueue that fails: the records go back)
            if (op_park(slot, pick(8) == 0)) ++parks;
            else park_refusals += refused_for("not enough free host records") || refused_for("enqueued");
            note((uint64_t)T.slots[slot].parked);
        } else if (op < 83) {
            if (op_unpark(slot)) ++unparks;
            else unpark_refusals += refused_for("KV page pool exhausted");
            note((uint64_t)T.slots[slot].parked);
        } else if (op < 90) {  // move, whatever state the two slots are in: pages or records change hands
            moves += op_move(slot, other);
        } else if (op < 97) {
            releases += op_release(slot);
        } else if (T.pool.enabled) {  // eviction pressure: a cap that forces victims out, then no cap again
            T.pool.set_cap(1 + pick(3));
            T.pool.set_cap(0);
        }
        note((uint64_t)T.pool.free_pages.size() << 32 | (uint64_t)T.arena.in_use << 8 | (uint64_t)T.pool.retained);
        check_slots_pages_and_records();
    }
    std::printf("ok ops=%ld begins=%ld appends=%ld forks=%ld fork_refusals=%ld parks=%ld park_refusals=%ld unparks=%ld unpark_refusals=%ld moves=%ld "
                "releases=%ld rewinds=%ld rewind_refusals=%ld attaches=%ld step_refusals=%ld evicted=%ld registered=%ld digest=%016llx\n",
                ops, begins, appends, forks, fork_refusals, parks, park_refusals, unparks, unpark_refusals, moves, releases, rewinds, rewind_refusals,
                attaches, step_refusals, T.pool.ctr.pages_evicted, T.pool.ctr.pages_registered, (unsigned long long)g_digest);
    return 0;
}
