// KV swap, host side (include/tinyllm_engine.h "KV swap"): the allocator of the host arena's page records.  The
// page and record accounting of tl_engine_park / tl_engine_unpark is SlotTable's (slot_table.h: park_begin / park_commit / park_abort,
// unpark), which owns the arena.  Host only, no HIP include.
//
//   record    room for one KV page of every pool in the pinned host arena; record r lies at r * record_bytes.  A parked slot holds
//             ceil(context / page_size) records, one per page, in page order.
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

}  // namespace tl
