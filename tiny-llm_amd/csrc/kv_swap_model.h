// KV swap, host side (include/tinyllm_engine.h "KV swap"): the allocator of the host arena's page records and the
// page accounting of tl_engine_park / tl_engine_unpark over PagePool (prefix_cache.h).  Host only, no HIP include: engine.hip calls
// it, and tests/kv_swap_model_check.cpp drives it alone.
//
//   record    room for one KV page of every pool in the pinned host arena; record r lies at r * record_bytes.  A parked slot holds
//             ceil(context / page_size) records, one per page, in page order.
//   park      the slot lets go of its pages exactly as a release does (reference counts drop, pages others share stay with them, indexed
//             pages become retained, the rest go to the free list) and keeps its records; its known tokens stay, the entries of its pages
//             are forgotten (unpark registers again).
//   unpark    fresh private pages from the one allocation path (free list first, then eviction), the records return to the arena, the
//             full pages inside the known tokens go through PagePool::register_slot like a prefill's.
// Both are all-or-nothing: a call that cannot be served changes nothing.
#pragma once

#include "prefix_cache.h"

namespace tl {

class SwapArena {
public:
    void init(int records) {
        used.assign(records, 0);
        in_use = 0;
    }
    int capacity() const { return (int)used.size(); }
    int available() const { return capacity() - in_use; }
    // n records, lowest ids first (an arena nobody fragmented hands out one contiguous run: one copy per group)
    bool take(int n, std::vector<int> &out) {
        if (n < 0 || n > available()) return false;
        for (int r = 0; r < capacity() && n > 0; ++r) {
            if (used[r]) continue;
            used[r] = 1;
            out.push_back(r);
            ++in_use;
            --n;
        }
        return true;
    }
    void give(std::vector<int> &records) {
        for (int r : records) {
            used[r] = 0;
            --in_use;
        }
        records.clear();
    }
    std::vector<char> used;
    int in_use = 0;
};

inline int swap_pages_of(int context, int page_size) { return (context + page_size - 1) / page_size; }

// records[j0, j1) as runs of consecutive record ids: (index of the run's first page, pages in the run)
inline std::vector<std::pair<int, int>> swap_runs(const std::vector<int> &records, int j0, int j1) {
    std::vector<std::pair<int, int>> runs;
    for (int j = j0; j < j1; ++j) {
        if (!runs.empty() && records[j] == records[j - 1] + 1) runs.back().second++;
        else runs.emplace_back(j, 1);
    }
    return runs;
}

// park on the host.  `rec`: the slot's prefix record, or nullptr while the cache is off.  false: not enough free records, nothing changed
inline bool swap_park_host(PagePool &pool, SwapArena &arena, SlotRecord *rec, std::vector<int> &pages, int context, std::vector<int> &records) {
    const int n = swap_pages_of(context, pool.page_size);
    if (context < 1 || n > (int)pages.size() || !records.empty() || !arena.take(n, records)) return false;
    for (int id : pages) pool.drop(id);
    pages.clear();
    if (rec) {
        rec->nodes.clear();
        rec->stuck = false;
    }
    return true;
}

// unpark on the host: `pages` becomes n fresh private pages.  false: fewer than n pages can be had, nothing changed
inline bool swap_unpark_host(PagePool &pool, SwapArena &arena, SlotRecord *rec, std::vector<int> &pages, int context, std::vector<int> &records) {
    const int n = swap_pages_of(context, pool.page_size);
    if (n != (int)records.size() || !pages.empty() || !pool.can_take((size_t)n)) return false;
    for (int j = 0; j < n; ++j) pages.push_back(pool.take());
    arena.give(records);
    if (rec) pool.register_slot(*rec, pages);
    return true;
}

}  // namespace tl
