// The engine's slot protocol (include/tinyllm_engine.h): which sequence holds which KV pages and host records.
// Host only, no HIP include and no device pointer: engine.hip calls it and applies the edits it reports to the device, and
// tests/prefix_cache_model_check.cpp and tests/kv_swap_model_check.cpp drive the same code alone against brute-force models.
//
//   state     the page pool (prefix_cache.h: free list, reference counts, the prefix index), the host arena's records
//             (kv_swap_model.h) and one Slot per batch slot.  A slot is free | live | live and parked (its KV lies in host records,
//             it holds no page).  A live unparked slot holds at least ceil(ctx / page_size) pages.  A live slot may also be STOPPED
//             (parked or not): it keeps its pages or records and every call works on it, but no decode step takes it.
//   calls     every operation is all-or-nothing.  It returns nullptr, or the refusal's message with nothing changed.
//   edits     a call that succeeds APPENDS to the caller's SlotEdits what the device must learn: block-table writes, page copies and
//             the ids of the pages it took, each in the order it made them.  The caller applies the copies before the writes (a
//             fresh page is filled before the row entry that publishes it) and clears the list when it likes: a call that has
//             nothing to report allocates nothing.
//   shared    full pages are shared by reference count (fork, attach) and never written again; a partial tail page that is shared or
//   tails     indexed is copied eagerly by fork, rewind and attach, so an append always lands in a private, unindexed page.
#pragma once

#include "kv_swap_model.h"

namespace tl {

struct Slot {
    bool live = false, parked = false;
    bool stopped = false;             // a stop condition froze the sequence on the device (stop.h): no decode step takes it
    int ctx = 0, produced = 0;        // tokens whose K/V the slot holds; ids produced since begin / fork / move
    std::vector<int> pages, records;  // pages in block-table order; a parked slot's host records, one per page
    SlotRecord rec;                   // what the prefix index knows of the slot (empty while the cache is off)
};

struct SlotEdits {
    struct Row {
        int slot, index, page;  // block_table[slot][index] = page (-1: no page)
    };
    struct Copy {
        int from, to, rows;  // the first `rows` rows of page `from` into page `to`: page_size (a whole page) for a fork's or rewind's tail
    };
    std::vector<Row> rows;
    std::vector<Copy> copies;
    std::vector<int> taken;
    void clear() {
        rows.clear();
        copies.clear();
        taken.clear();
    }
};

#define TL_SLOT_TRY(expr)                          \
    do {                                           \
        if (const char *why__ = (expr)) return why__; \
    } while (0)

class SlotTable {
public:
    PagePool pool;
    SwapArena arena;
    std::vector<Slot> slots;
    // what the statistics report of the allocation path
    long page_allocations = 0, reused_page_allocations = 0;
    int peak_pages_in_use = 0;

    void init(int n_slots, int pages, int page_tokens, int pages_per_seq) {
        slots.assign(n_slots, Slot{});
        pool.init(pages, page_tokens);
        arena.init(0);
        was_used.assign(pages, 0);
        page_size = page_tokens, max_pages = pages_per_seq;
    }
    bool runs(int slot) const { return slots[slot].live && !slots[slot].parked && !slots[slot].stopped; }  // what a decode step asks

    // A stop condition froze the slot on the device after the steps up to context `ctx` and `produced` ids: the mirrors, which went on
    // with every step of the call, take the device's values.  The slot keeps every page it holds -- those reserved for the steps it
    // did not take too, as after reserve(); release() or a rewind() returns them.  resume(): a decode step takes the slot again.
    void stop(int slot, int ctx, int produced) {
        Slot &s = slots[slot];
        s.ctx = ctx, s.produced = produced, s.stopped = true;
    }
    void resume(int slot) { slots[slot].stopped = false; }
    int pages_in_use() const { return pool.in_use(); }
    int pages_free() const { return (int)pool.free_pages.size(); }

    const char *check(int slot, bool must_be_live) const {
        if (slot < 0 || slot >= (int)slots.size()) return "engine: slot out of range";
        if (must_be_live && !slots[slot].live) return "engine: slot holds no sequence";
        return nullptr;
    }
    // ... for the calls that read or write the slot's K/V: a parked slot has none on the device
    const char *check_unparked(int slot) const {
        TL_SLOT_TRY(check(slot, true));
        if (slots[slot].parked) return "engine: the slot is parked (its KV lies in host memory; tl_engine_unpark first)";
        return nullptr;
    }

    // ---- the prefix index's switches: the slots' records start over with it -------------------------------------------------
    void prefix_enable(int cap) {
        if (!pool.enabled) clear_records();
        pool.enable(cap);
    }
    void prefix_disable() {
        pool.disable();
        clear_records();
    }

    // ---- the protocol ----------------------------------------------------------------------------------------------------------
    const char *begin(int slot) {
        TL_SLOT_TRY(check(slot, false));
        Slot &s = slots[slot];
        if (s.live) return "engine_begin: slot already holds a sequence (release it first)";
        s.live = true;
        s.stopped = false;
        s.ctx = s.produced = 0;
        s.rec.clear();
        return nullptr;
    }

    // pages for `total_tokens` tokens in the slot
    const char *reserve(int slot, int total_tokens, SlotEdits &ed) {
        TL_SLOT_TRY(check_unparked(slot));
        Slot &s = slots[slot];
        const int need = swap_pages_of(total_tokens, page_size), have = (int)s.pages.size();
        if (need <= have) return nullptr;
        if (need > max_pages) return "engine: sequence exceeds max_pages_per_seq * page_size tokens";
        if (!pool.can_take((size_t)(need - have))) return "engine: KV page pool exhausted";
        for (int j = have; j < need; ++j) {
            s.pages.push_back(take(ed));
            ed.rows.push_back({slot, j, s.pages.back()});
        }
        return nullptr;
    }

    // Pages for ONE more token in every running slot of [0, batch).  The totals are checked before anything is mutated: a half-applied
    // reservation would leave a slot that owns a page on the host and -1 on the device (silently dropped K/V).  *max_ctx grows to the
    // longest context the step will see.
    const char *reserve_step(int batch, SlotEdits &ed, int *max_ctx) {
        size_t extra = 0;
        for (int b = 0; b < batch; ++b) {
            if (!runs(b)) continue;
            const int need = swap_pages_of(slots[b].ctx + 1, page_size);
            if (need > max_pages) return "engine: sequence exceeds max_pages_per_seq * page_size tokens";
            if (need > (int)slots[b].pages.size()) extra += (size_t)need - slots[b].pages.size();
        }
        if (!pool.can_take(extra)) return "engine: KV page pool exhausted";
        for (int b = 0; b < batch; ++b) {
            if (!runs(b)) continue;
            TL_SLOT_TRY(reserve(b, slots[b].ctx + 1, ed));  // cannot fail after the checks above
            *max_ctx = std::max(*max_ctx, slots[b].ctx + 1);
        }
        return nullptr;
    }
    // after the step: every running slot holds one more token and has produced one more id
    void step_done(int batch) {
        for (int b = 0; b < batch; ++b)
            if (runs(b)) slots[b].ctx++, slots[b].produced++;
    }
    // after a prefill of n tokens into pages reserved before: tokens appended where the slot's known tokens end extend them, and pages
    // that filled up enter the index
    // (record = false: the tokens stay unknown to the prefix cache -- a slot whose K/V the token ids alone do not determine)
    void appended(int slot, const int32_t *tokens, int n, bool record = true) {
        Slot &s = slots[slot];
        const bool extends = record && pool.enabled && (int)s.rec.known.size() == s.ctx;
        s.ctx += n;
        if (extends) {
            s.rec.known.insert(s.rec.known.end(), tokens, tokens + n);
            pool.register_slot(s.rec, s.pages);
        }
    }

    const char *release(int slot, SlotEdits &ed) {
        TL_SLOT_TRY(check(slot, true));
        Slot &s = slots[slot];
        for (size_t j = 0; j < s.pages.size(); ++j) {
            pool.drop(s.pages[j]);
            ed.rows.push_back({slot, (int)j, -1});
        }
        arena.give(s.records);  // a parked slot's (stream order protects their bytes)
        const int produced = s.produced;  // the ids it produced stay readable
        s = Slot{};
        s.produced = produced;
        return nullptr;
    }

    // drop the last n tokens.  The next append lands in the tail page: if somebody shares it or the index holds it, the slot gets
    // its own copy, which needs one page; pages this rewind itself returns count.
    const char *rewind(int slot, int n, SlotEdits &ed) {
        TL_SLOT_TRY(check_unparked(slot));
        Slot &s = slots[slot];
        if (n < 0 || n > s.ctx) return "engine_rewind: cannot rewind past the start of the sequence";
        const int ctx = s.ctx - n, keep = swap_pages_of(ctx, page_size);
        const bool cow = keep > 0 && ctx % page_size != 0 && keep <= (int)s.pages.size() &&
                         (pool.refs[s.pages[keep - 1]] > 1 || pool.is_indexed(s.pages[keep - 1]));
        if (cow) {  // (the pages it returns are counted as they will stand: their holds are taken off while the pool is asked)
            size_t will_free = 0;
            for (int j = keep; j < (int)s.pages.size(); ++j) will_free += --pool.refs[s.pages[j]] == 0 && !pool.is_indexed(s.pages[j]) ? 1 : 0;
            const bool ok = will_free >= 1 || pool.can_take(1);
            for (int j = keep; j < (int)s.pages.size(); ++j) pool.refs[s.pages[j]]++;
            if (!ok) return "engine_rewind: KV page pool exhausted (copy of a shared tail page)";
        }
        while ((int)s.pages.size() > keep) {
            pool.drop(s.pages.back());
            s.pages.pop_back();
            ed.rows.push_back({slot, (int)s.pages.size(), -1});
        }
        if (cow) {
            const int old_id = s.pages[keep - 1], fresh = take(ed);
            ed.copies.push_back({old_id, fresh, page_size});
            pool.drop(old_id);
            s.pages[keep - 1] = fresh;
            ed.rows.push_back({slot, keep - 1, fresh});
        }
        s.ctx = ctx;
        s.rec.rewind(ctx, page_size);
        return nullptr;
    }

    // dst becomes a second sequence with src's prefix: full pages shared, a partial tail page copied
    const char *fork(int src, int dst, SlotEdits &ed) {
        TL_SLOT_TRY(check_unparked(src));
        TL_SLOT_TRY(check(dst, false));
        if (src == dst) return "engine_fork: source and destination are the same slot";
        if (slots[dst].live) return "engine_fork: destination slot already holds a sequence";
        const Slot &s = slots[src];
        Slot &d = slots[dst];
        const int full = s.ctx / page_size;
        const bool partial = s.ctx % page_size != 0;
        if (partial && !pool.can_take(1)) return "engine_fork: KV page pool exhausted";
        d = Slot{};
        for (int j = 0; j < full; ++j) {
            pool.share(s.pages[j]);
            d.pages.push_back(s.pages[j]);
            ed.rows.push_back({dst, j, s.pages[j]});
        }
        if (partial) {
            d.pages.push_back(take(ed));
            ed.copies.push_back({s.pages[full], d.pages.back(), page_size});
            ed.rows.push_back({dst, full, d.pages.back()});
        }
        d.live = true;
        d.stopped = s.stopped;
        d.ctx = s.ctx;
        d.rec = s.rec;
        return nullptr;
    }

    // tl_engine_beam_reorder: a beam group changes generation in place.  Before, the sources [slot0, slot0 + n_src) run (live, not parked,
    // not stopped) and [slot0 + n_src, slot0 + width) are free; after, slot0 + i (i < width) holds the sequence slot0 + parents[i] held.
    // One child of every chosen parent -- the one in the parent's own slot where there is one, else its first -- inherits the parent's
    // pages as a move does, private tail and pages reserved ahead included; every further child is a fork: the full pages shared, a partial
    // tail copied (its ctx % page_size rows).  A parent nobody chose, and a source at index >= width, lets go as a release does.  The
    // pages the copies need are asked of the pool BEFORE anything changes, and the pages the unchosen parents give back are not counted
    // towards them: the copies are taken while every parent still holds its pages, so a group that fits only with those pages is refused.
    static constexpr int BEAM_MAX = 8;  // TL_MAX_BEAMS
    const char *beam_reorder(int slot0, int n_src, int width, const int *parents, SlotEdits &ed) {
        if (n_src < 1 || n_src > BEAM_MAX || width < 1 || width > BEAM_MAX) return "engine_beam_reorder: n_src and width are 1 .. 8";
        const int span = std::max(n_src, width);
        if (slot0 < 0 || slot0 > (int)slots.size() - span) return "engine_beam_reorder: slots out of range";
        if (!parents) return "engine_beam_reorder: null parents";
        for (int i = 0; i < n_src; ++i) {
            TL_SLOT_TRY(check_unparked(slot0 + i));
            if (slots[slot0 + i].stopped) return "engine_beam_reorder: a source slot has stopped";
        }
        for (int i = n_src; i < width; ++i)
            if (slots[slot0 + i].live) return "engine_beam_reorder: destination slot already holds a sequence";
        int children[BEAM_MAX] = {}, heir[BEAM_MAX];
        for (int i = 0; i < width; ++i) {
            if (parents[i] < 0 || parents[i] >= n_src) return "engine_beam_reorder: parent out of range";
            if (children[parents[i]]++ == 0 || parents[i] == i) heir[parents[i]] = i;
        }
        size_t need = 0;
        for (int p = 0; p < n_src; ++p)
            if (children[p] > 1 && slots[slot0 + p].ctx % page_size != 0) need += (size_t)children[p] - 1;
        if (!pool.can_take(need)) return "engine_beam_reorder: KV page pool exhausted";
        const std::vector<Slot> old(slots.begin() + slot0, slots.begin() + slot0 + span);
        std::vector<Slot> now(span);
        for (int i = 0; i < width; ++i) {
            const Slot &s = old[parents[i]];
            Slot &d = now[i];
            if (heir[parents[i]] == i) {
                d = s;
            } else {
                const int full = s.ctx / page_size;
                for (int j = 0; j < full; ++j) {
                    pool.share(s.pages[j]);
                    d.pages.push_back(s.pages[j]);
                }
                if (s.ctx % page_size != 0) {
                    d.pages.push_back(take(ed));
                    ed.copies.push_back({s.pages[full], d.pages.back(), s.ctx % page_size});
                }
                d.live = true;
                d.ctx = s.ctx;
                d.rec = s.rec;
            }
            d.produced = 0;
        }
        for (int p = 0; p < n_src; ++p)
            if (children[p] == 0)
                for (int id : old[p].pages) pool.drop(id);
        for (int i = width; i < span; ++i) now[i].produced = old[i].produced;  // (as after a release: the ids it produced stay readable)
        for (int i = 0; i < span; ++i) {
            const std::vector<int> &was = old[i].pages, &is = now[i].pages;
            for (size_t j = 0; j < std::max(was.size(), is.size()); ++j) {
                const int a = j < was.size() ? was[j] : -1, b = j < is.size() ? is[j] : -1;
                if (a != b) ed.rows.push_back({slot0 + i, (int)j, b});
            }
            slots[slot0 + i] = std::move(now[i]);
        }
        return nullptr;
    }

    // the sequence, parked or not, changes slots: pages or records change hands, no K/V byte moves
    const char *move(int src, int dst, SlotEdits &ed) {
        TL_SLOT_TRY(check(src, true));
        TL_SLOT_TRY(check(dst, false));
        if (src == dst) return "engine_move: source and destination are the same slot";
        if (slots[dst].live) return "engine_move: destination slot already holds a sequence";
        Slot &s = slots[src], &d = slots[dst];
        for (size_t j = 0; j < s.pages.size(); ++j) {
            ed.rows.push_back({dst, (int)j, s.pages[j]});
            ed.rows.push_back({src, (int)j, -1});
        }
        d = std::move(s);
        s = Slot{};
        d.produced = 0;
        return nullptr;
    }

    // tl_engine_prefix_attach: the empty slot shares the longest indexed chain of full pages below n - 1 tokens and copies the rows of
    // the best partial match into a fresh page (PagePool::attach).  *matched: the tokens now in the slot
    const char *attach(int slot, const int32_t *tokens, int n, SlotEdits &ed, int *matched) {
        TL_SLOT_TRY(check_unparked(slot));
        Slot &s = slots[slot];
        if (s.ctx != 0 || !s.pages.empty()) return "engine_prefix_attach: the slot already holds tokens or pages";
        *matched = 0;
        if (!pool.enabled) return nullptr;
        const AttachResult a = pool.attach(s.rec, s.pages, tokens, n, max_pages);
        if (a.tail_rows > 0) {
            count_page(a.tail_to, ed);
            ed.copies.push_back({a.tail_from, a.tail_to, a.tail_rows});
        }
        peak_pages_in_use = std::max(peak_pages_in_use, pool.in_use());
        for (size_t j = 0; j < s.pages.size(); ++j) ed.rows.push_back({slot, (int)j, s.pages[j]});
        s.ctx = *matched = a.matched;
        return nullptr;
    }

    // tl_engine_prefix_extend: n more of the slot's tokens become known
    const char *extend(int slot, const int32_t *tokens, int n) {
        TL_SLOT_TRY(check_unparked(slot));
        Slot &s = slots[slot];
        if (!pool.enabled) return nullptr;
        if ((long)s.rec.known.size() + n > s.ctx) return "engine_prefix_extend: more tokens than the slot holds beyond its known ones";
        s.rec.known.insert(s.rec.known.end(), tokens, tokens + n);
        pool.register_slot(s.rec, s.pages);
        return nullptr;
    }

    // Park in three steps, because the device copies out of the slot's pages are enqueued while it still holds them and may fail:
    // park_begin checks and takes the records (s.records), then park_commit lets the pages go exactly as a release does (the slot's
    // known tokens stay, the entries of its pages are forgotten: unpark registers again), or park_abort returns the records.
    const char *park_begin(int slot) {
        TL_SLOT_TRY(check_unparked(slot));
        Slot &s = slots[slot];
        const int n = swap_pages_of(s.ctx, page_size);
        if (s.ctx < 1) return "engine_park: the slot holds no tokens";
        if (arena.capacity() == 0) return "engine_park: no swap space (tl_engine_swap_space)";
        if (n > arena.available()) return "engine_park: not enough free host records";
        if (n > (int)s.pages.size()) return "engine_park: the slot holds fewer pages than its context needs";
        arena.take(n, s.records);
        return nullptr;
    }
    void park_commit(int slot, SlotEdits &ed) {
        Slot &s = slots[slot];
        for (size_t j = 0; j < s.pages.size(); ++j) {
            pool.drop(s.pages[j]);
            ed.rows.push_back({slot, (int)j, -1});
        }
        s.pages.clear();
        s.rec.nodes.clear();
        s.rec.stuck = false;
        s.parked = true;
    }
    void park_abort(int slot) { arena.give(slots[slot].records); }

    // fresh private pages from the one allocation path; the records (handed to the caller, who copies out of them in stream order)
    // return to the arena; the full pages inside the known tokens are registered like a prefill's
    const char *unpark(int slot, SlotEdits &ed, std::vector<int> &records) {
        TL_SLOT_TRY(check(slot, true));
        Slot &s = slots[slot];
        if (!s.parked) return "engine_unpark: the slot is not parked";
        const int n = swap_pages_of(s.ctx, page_size);
        if (!pool.can_take((size_t)n)) return "engine_unpark: KV page pool exhausted";
        if (n != (int)s.records.size() || !s.pages.empty()) return "engine_unpark: the slot's records do not cover its context";
        for (int j = 0; j < n; ++j) {
            s.pages.push_back(take(ed));
            ed.rows.push_back({slot, j, s.pages.back()});
        }
        records = s.records;
        arena.give(s.records);
        if (pool.enabled) pool.register_slot(s.rec, s.pages);
        s.parked = false;
        return nullptr;
    }

private:
    int page_size = 0, max_pages = 0;
    std::vector<char> was_used;

    void clear_records() {
        for (Slot &s : slots) s.rec.clear();
    }
    void count_page(int id, SlotEdits &ed) {
        page_allocations++;
        reused_page_allocations += was_used[id];
        was_used[id] = 1;
        ed.taken.push_back(id);
    }
    // the one allocation path (prefix_cache.h): the free list first, then the least recently used retained page.  The caller has
    // checked pool.can_take
    int take(SlotEdits &ed) {
        const int id = pool.take();
        count_page(id, ed);
        peak_pages_in_use = std::max(peak_pages_in_use, pool.in_use());
        return id;
    }
};

#undef TL_SLOT_TRY

}  // namespace tl
