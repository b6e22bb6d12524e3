// Stand-alone model check of SlotTable::beam_reorder (csrc/slot_table.h; built and run by tests/test_beam_cpu.py with
// -fsanitize=address,undefined, once per page size -DBEAM_P=1 .. 4): seeded random genealogies (slot0, n_src, width, parents) -- valid
// ones and ones on slots in the wrong state -- over a pool of 10 pages that ten slots share, so that pools too small for the tail
// copies are the rule, with contexts on and off a page boundary, interleaved with begin / prefill / decode step / fork / rewind / move /
// park / unpark / release of any slot and with the prefix cache on for the second half.  The model of the device (slot_model_check.h)
// learns of the table's decisions only through the edits.  After EVERY operation: reference counts equal the number of rows naming a
// page, every slot reads its own tokens' fingerprints back through the block table the edits built (so a child reads its parent's
// prefix, through shared pages and through the copied tail), pages_in_use + pages_free + pages_retained == num_pages.  After a reorder:
// the pool operations it must have made, replayed in order on a copy of the pool (shares and the reported takes of the further
// children, then the drops of the unchosen parents), end where the table's pool ended; the pages it took are exactly the further
// children of parents with a partial tail; no writable tail is shared; `produced` restarts.  A refused reorder -- for want of pages, by
// the table's own message, or on slots in the wrong state -- changed nothing.
// Prints one line: the operation counts and a digest of every answer.
#ifndef BEAM_P
#define BEAM_P 4
#endif
static constexpr int P = BEAM_P, PAGES = 10, SLOTS = 10, MAXP = 6, ALPHABET = 3, RECORDS = 4;
#include "slot_model_check.h"

static constexpr int BEAMS = 8;  // TL_MAX_BEAMS

static bool op_beam(int slot0, int n_src, int width, const int *parents) {
    const Snapshot was;
    const int span = std::max(n_src, width);
    bool expect = n_src >= 1 && n_src <= BEAMS && width >= 1 && width <= BEAMS && slot0 >= 0 && slot0 + span <= SLOTS;
    int children[BEAMS] = {}, heir[BEAMS], need = 0;
    if (expect) {
        for (int i = 0; i < n_src; ++i) expect &= was.slots[slot0 + i].live && !was.slots[slot0 + i].parked && !was.slots[slot0 + i].stopped;
        for (int i = n_src; i < width; ++i) expect &= !was.slots[slot0 + i].live;
        for (int i = 0; i < width; ++i) expect &= parents[i] >= 0 && parents[i] < n_src;
    }
    if (expect) {
        // the heir of a parent: the child in the parent's own slot, else its first child
        for (int i = width - 1; i >= 0; --i) heir[parents[i]] = i, children[parents[i]]++;
        for (int i = 0; i < width; ++i)
            if (parents[i] == i) heir[i] = i;
        for (int p = 0; p < n_src; ++p) need += children[p] > 1 && was.slots[slot0 + p].ctx % P != 0 ? children[p] - 1 : 0;
        expect = need <= bf_available(was.pool);  // (what the unchosen parents would give back is not counted)
    }
    SlotEdits ed;
    const bool ok = (g_why = T.beam_reorder(slot0, n_src, width, parents, ed)) == nullptr;
    CHECK(ok == expect);
    if (!ok) return check_unchanged(was, ed), false;
    apply(ed);
    PagePool m = was.pool;
    size_t takes = 0;
    for (int i = 0; i < width; ++i) {
        const Slot &b = was.slots[slot0 + parents[i]];
        if (heir[parents[i]] == i) {
            CHECK(T.slots[slot0 + i].pages == b.pages);  // as a move: the row changes hands, private tail included
            continue;
        }
        for (int j = 0; j < b.ctx / P; ++j) m.share(b.pages[j]);
        if (b.ctx % P != 0) {
            CHECK(takes < ed.copies.size() && ed.copies[takes].from == b.pages[b.ctx / P] && ed.copies[takes].to == ed.taken.at(takes) &&
                  ed.copies[takes].rows == b.ctx % P);
            replay_take(m, ed.taken[takes++]);
        }
    }
    for (int p = 0; p < n_src; ++p)
        if (children[p] == 0)
            for (int id : was.slots[slot0 + p].pages) replay_drop(m, id);
    CHECK((int)takes == need && ed.copies.size() == takes);
    replay_end(m, ed, takes);
    std::vector<int32_t> held[BEAMS];
    for (int i = 0; i < span; ++i) held[i] = actual[slot0 + i];
    for (int i = 0; i < span; ++i) {
        const Slot &s = T.slots[slot0 + i];
        if (i >= width) {
            CHECK(!s.live && s.pages.empty() && s.produced == was.slots[slot0 + i].produced);
            actual[slot0 + i].clear();
            continue;
        }
        const Slot &b = was.slots[slot0 + parents[i]];
        CHECK(s.live && !s.parked && !s.stopped && s.ctx == b.ctx && s.produced == 0 && s.rec.known == b.rec.known);
        if (s.ctx % P != 0) CHECK(T.pool.refs[s.pages[s.ctx / P]] == 1 && !T.pool.is_indexed(s.pages[s.ctx / P]));  // no writable tail is shared
        actual[slot0 + i] = held[parents[i]];
    }
    return true;
}

int main(int argc, char **argv) {
    const long ops = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? (uint32_t)std::atol(argv[2]) : 12345u);
    model_init();
    long begins = 0, appends = 0, forks = 0, moves = 0, releases = 0, rewinds = 0, parks = 0, unparks = 0, reorders = 0, reorder_refusals = 0,
         reorder_wrong_state = 0, fanouts = 0, copies = 0, shrinks = 0, permutations = 0, step_refusals = 0;
    for (g_op = 0; g_op < ops; ++g_op) {
        if (g_op == ops / 2) T.prefix_enable(0);
        const int slot = pick(SLOTS);
        int other = pick(SLOTS);
        for (int i = 0; i < SLOTS && pick(8); ++i)
            if (!T.slots[i].live) other = i;
        const int op = pick(100);
        const Slot &s = T.slots[slot];
        if (op < 40) {  // a reorder: mostly over a run of running slots with free slots behind it, sometimes over anything
            int slot0 = pick(SLOTS), run = 0, room = 0;
            for (int i = 0; i < SLOTS && pick(6); ++i)
                if (T.runs(i) && (i == 0 || !T.runs(i - 1))) slot0 = i;  // (the start of some run)
            while (slot0 + run < SLOTS && run < BEAMS && T.runs(slot0 + run)) ++run;
            int n_src = run > 0 ? 1 + pick(run) : 1 + pick(3);
            while (slot0 + n_src + room < SLOTS && n_src + room < BEAMS && !T.slots[slot0 + n_src + room].live) ++room;
            int width = pick(5) ? 1 + pick(n_src + room) : 1 + pick(BEAMS + 1);  // (now and then 9, or over live slots)
            if (pick(40) == 0) n_src = pick(2) ? 0 : BEAMS + 1;
            int parents[BEAMS + 1];
            const int kind = pick(4);  // any genealogy; a fan-out from few parents; a permutation; out of range now and then
            for (int i = 0; i <= BEAMS; ++i) parents[i] = kind == 1 ? pick(1 + pick(2)) % std::max(n_src, 1) : pick(std::max(n_src, 1));
            if (kind == 2 && width == n_src)
                for (int i = 0; i < n_src; ++i) parents[i] = (i + 1) % n_src;
            if (pick(50) == 0) parents[pick(std::max(std::min(width, BEAMS), 1))] = pick(2) ? -1 : n_src;
            const long copies_before = g_taken;
            if (op_beam(slot0, n_src, width, parents)) {
                ++reorders;
                copies += g_taken - copies_before;
                fanouts += width > n_src;
                shrinks += width < n_src;
                permutations += kind == 2 && width == n_src;
            } else if (refused_for("KV page pool exhausted")) {
                ++reorder_refusals;
            } else {
                ++reorder_wrong_state;
            }
            note((uint64_t)reorders << 20 | (uint64_t)reorder_refusals);
        } else if (!s.live && op < 75) {  // a new sequence with a prompt that ends on or off a page boundary
            begins += op_begin(slot);
            std::vector<int32_t> t(1 + pick(3 * P));
            for (auto &v : t) v = pick(ALPHABET);
            if (op_prefill(slot, t)) appends += (long)t.size();
        } else if (op < 55) {  // decode steps over the first slots: all of them or none
            const int batch = 1 + pick(SLOTS);
            int running = 0;
            for (int b = 0; b < batch; ++b) running += T.runs(b);
            if (op_step(batch)) appends += running;
            else step_refusals += refused_for("KV page pool exhausted");
        } else if (op < 62) {
            forks += op_fork(slot, other);
        } else if (op < 68) {
            rewinds += op_rewind(slot, 1 + pick(P + 1));
        } else if (op < 74) {
            moves += op_move(slot, other);
        } else if (op < 78) {
            parks += op_park(slot, false);
        } else if (op < 82) {
            unparks += op_unpark(slot);
        } else {
            releases += op_release(slot);
        }
        note((uint64_t)T.pool.free_pages.size() << 32 | (uint64_t)T.arena.in_use << 8 | (uint64_t)T.pool.retained);
        check_slots_pages_and_records();
    }
    std::printf("ok ops=%ld page_size=%d begins=%ld appends=%ld forks=%ld moves=%ld releases=%ld rewinds=%ld parks=%ld unparks=%ld reorders=%ld "
                "reorder_refusals=%ld reorder_wrong_state=%ld fanouts=%ld shrinks=%ld permutations=%ld copies=%ld step_refusals=%ld digest=%016llx\n",
                ops, P, begins, appends, forks, moves, releases, rewinds, parks, unparks, reorders, reorder_refusals, reorder_wrong_state, fanouts,
                shrinks, permutations, copies, step_refusals, (unsigned long long)g_digest);
    return 0;
}
