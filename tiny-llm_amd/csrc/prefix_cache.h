// Cross-request prefix cache: the KV page pool's bookkeeping (free list, reference counts) and the index of full pages by the
// tokens they hold (include/tinyllm_engine.h, "Prefix cache").  Host only, no HIP include.  Which slot holds
// which page is SlotTable's business (slot_table.h), which owns the pool: engine.hip and tests/prefix_cache_model_check.cpp both reach
// it through the table, the latter against a brute-force model.
//
//   page states   free (on the free list) | in use (refs > 0) | retained (refs == 0 and indexed).  in_use + free + retained ==
//                 num_pages after every call.
//   entry         an indexed page: (parent entry or ROOT, its page_size tokens).  The entry's id IS the physical page id.  A hash of
//                 (parent, tokens) finds candidates; a match is decided by comparing parent and tokens, never by the hash alone
//                 (TL_PREFIX_HASH_HOOK lets a test force every hash to one value).
//   recency       every attach and every registration stamps the whole chain, leaf to root, with one new tick: an ancestor is
//                 never older than a descendant.
//   eviction      victims are entries with refs == 0 and no indexed child, least recent tick first, ties by the lower page id.  A
//                 retained page whose subtree holds a referenced page is not evictable until that page is let go.
//   cap           max_retained > 0: whenever a page becomes retained, victims are evicted to the free list until retained <=
//                 max_retained or no victim is left.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <utility>
#include <vector>

#ifndef TL_PREFIX_HASH_HOOK
#define TL_PREFIX_HASH_HOOK(h) (h)
#endif

namespace tl {

struct PrefixCounters {
    long lookups = 0, hits = 0, tokens_matched = 0, tail_rows_copied = 0, pages_registered = 0, pages_evicted = 0;
};

// What the engine knows of one slot's tokens: ids of positions [0, known.size()), and for each of the slot's leading full pages that
// has been looked up or registered the entry that stands for it (the slot's own page, or an equal entry that was there first).
struct SlotRecord {
    std::vector<int32_t> known;
    std::vector<std::pair<int, uint64_t>> nodes;  // (entry, its serial when the slot met it)
    bool stuck = false;                           // the chain was lost (its parent evicted or cleared, or declared tokens disagree): publishes nothing more
    void clear() {
        known.clear();
        nodes.clear();
        stuck = false;
    }
    // tl_engine_rewind to `context` tokens
    void rewind(int context, int page_size) {
        if ((int)known.size() > context) known.resize(context);
        const size_t full = (size_t)(known.size() / page_size);
        if (nodes.size() > full) nodes.resize(full);
    }
};

struct AttachResult {
    int matched = 0;    // tokens now in the slot
    int full = 0;       // shared pages
    int tail_rows = 0;  // rows to copy from page tail_from into the fresh page tail_to (0: no tail)
    int tail_from = -1, tail_to = -1;
};

class PagePool {
public:
    static constexpr int ROOT = -1;

    void init(int pages, int page_tokens) {
        num_pages = pages, page_size = page_tokens;
        free_pages.resize(pages);
        for (int i = 0; i < pages; ++i) free_pages[i] = pages - 1 - i;  // pop_back hands out 0, 1, 2, ...
        refs.assign(pages, 0);
    }

    // ---- the one allocation path ------------------------------------------------------------------------------------------
    int in_use() const { return num_pages - (int)free_pages.size() - retained; }
    // free + evictable pages; the index is walked only when the free list alone does not answer
    bool can_take(size_t n) const { return n <= free_pages.size() || n <= free_pages.size() + (size_t)evictable(); }
    size_t available() const { return free_pages.size() + (size_t)evictable(); }
    // a page with refs = 1: from the free list first, then the eviction victim.  Precondition: can_take(1)
    int take() {
        if (free_pages.empty()) {
            const int v = victim();
            unindex(v);  // retained -> free list
            ctr.pages_evicted++;
        }
        const int id = free_pages.back();
        free_pages.pop_back();
        refs[id] = 1;
        return id;
    }
    void share(int id) {
        if (refs[id]++ == 0) retained--;
    }
    // a holder lets go: the page stays in use, becomes retained (indexed) or returns to the free list
    void drop(int id) {
        if (--refs[id] > 0) return;
        if (enabled && indexed[id]) {
            retained++;
            enforce_cap();
        } else {
            free_pages.push_back(id);
        }
    }
    bool is_indexed(int id) const { return enabled && indexed[id]; }

    // ---- the index ------------------------------------------------------------------------------------------------------------
    void enable(int cap) {
        if (!enabled) {
            indexed.assign(num_pages, 0);
            parent.assign(num_pages, ROOT);
            tick.assign(num_pages, 0);
            serial.assign(num_pages, 0);
            kids.assign(num_pages, {});
            toks.assign((size_t)num_pages * page_size, 0);
            enabled = true;
        }
        max_retained = cap;
        enforce_cap();
    }
    // drop every entry: retained pages return to the free list (ascending ids: the next take hands out the highest), pages in use stay
    // with their holders, unindexed
    void clear() {
        if (!enabled) return;
        for (int p = 0; p < num_pages; ++p) {
            if (!indexed[p]) continue;
            indexed[p] = 0;
            kids[p].clear();
            if (refs[p] == 0) {
                retained--;
                free_pages.push_back(p);
            }
        }
        root_kids.clear();
        by_hash.clear();
        n_entries = 0;
    }
    void disable() {
        clear();
        enabled = false;
        max_retained = 0;
        indexed = {}, parent = {}, kids = {}, toks = {};
        tick = {}, serial = {};
    }

    // the child of `par` holding exactly these page_size tokens, or -1
    int find_child(int par, const int32_t *t) const {
        auto range = by_hash.equal_range(hash_of(par, t));
        for (auto it = range.first; it != range.second; ++it) {
            const int p = it->second;
            if (parent[p] == par && std::memcmp(&toks[(size_t)p * page_size], t, (size_t)page_size * 4) == 0) return p;
        }
        return -1;
    }

    // Register the slot's full pages that lie inside its known tokens and are not registered yet.  An equal entry under another
    // physical page stays: the slot's page remains private and its later pages become children of the existing entry.
    void register_slot(SlotRecord &r, const std::vector<int> &pages) {
        if (!enabled || r.stuck) return;
        bool grew = false;
        while ((r.nodes.size() + 1) * (size_t)page_size <= r.known.size() && r.nodes.size() < pages.size()) {
            const size_t j = r.nodes.size();
            int par = ROOT;
            if (j > 0) {
                par = r.nodes[j - 1].first;
                if (!indexed[par] || serial[par] != r.nodes[j - 1].second) {  // the entry the chain hung from is gone
                    r.stuck = true;
                    break;
                }
            }
            const int32_t *t = &r.known[j * page_size];
            const int own = pages[j];
            int at = find_child(par, t);
            if (at < 0) {
                if (indexed[own]) {  // the page already stands for other tokens (a fork declared something else): leave it
                    r.stuck = true;
                    break;
                }
                at = own;
                indexed[own] = 1;
                parent[own] = par;
                serial[own] = ++serials;
                std::memcpy(&toks[(size_t)own * page_size], t, (size_t)page_size * 4);
                (par == ROOT ? root_kids : kids[par]).push_back(own);
                by_hash.emplace(hash_of(par, t), own);
                n_entries++;
                ctr.pages_registered++;
            }
            r.nodes.emplace_back(at, serial[at]);
            grew = true;
        }
        if (grew) touch(r.nodes.back().first);
    }

    // tl_engine_prefix_attach on the host: share the longest chain of full pages below n - 1 tokens, then take a fresh page for the rows
    // of the best partial match (skipped when no page can be had).  `pages` / `r`: the empty slot.  max_pages: block-table width.
    AttachResult attach(SlotRecord &r, std::vector<int> &pages, const int32_t *tokens, int n, int max_pages) {
        AttachResult a;
        ctr.lookups++;
        const int limit = n - 1;  // the last token is prefilled: its row yields the logits
        int par = ROOT;
        while ((a.full + 1) * page_size <= limit && a.full < max_pages) {
            const int p = find_child(par, tokens + (size_t)a.full * page_size);
            if (p < 0) break;
            share(p);
            pages.push_back(p);
            r.nodes.emplace_back(p, serial[p]);
            par = p;
            a.full++;
        }
        a.matched = a.full * page_size;
        const int room = std::min(limit - a.matched, page_size);
        if (room > 0 && a.full < max_pages) {
            const int32_t *t = tokens + a.matched;
            int best = -1, best_rows = 0;
            for (int p : (par == ROOT ? root_kids : kids[par])) {
                const int32_t *have = &toks[(size_t)p * page_size];
                int rows = 0;
                while (rows < room && have[rows] == t[rows]) ++rows;
                if (rows > best_rows || (rows == best_rows && rows > 0 && (tick[p] > tick[best] || (tick[p] == tick[best] && p < best))))
                    best = p, best_rows = rows;
            }
            if (best >= 0) {
                share(best);  // held while the fresh page is taken: the source of the copy is never the victim
                if (can_take(1)) {
                    a.tail_to = take();
                    a.tail_from = best;
                    a.tail_rows = best_rows;
                    a.matched += best_rows;
                    pages.push_back(a.tail_to);
                    touch(best);
                }
                if (--refs[best] == 0) retained++;  // back as it was (no cap check: nothing became retained that was not before)
            }
        }
        if (a.tail_rows == 0 && a.full > 0) touch(par);
        r.known.assign(tokens, tokens + a.matched);
        if (a.matched > 0) ctr.hits++;
        ctr.tokens_matched += a.matched;
        ctr.tail_rows_copied += a.tail_rows;
        return a;
    }

    void set_cap(int cap) {
        max_retained = cap;
        enforce_cap();
    }

    // ---- state (read by the engine's statistics and by the model check) ----------------------------------------------------------
    int num_pages = 0, page_size = 0;
    std::vector<int> free_pages, refs;
    bool enabled = false;
    int max_retained = 0, retained = 0, n_entries = 0;
    PrefixCounters ctr;
    std::vector<char> indexed;
    std::vector<int> parent;
    std::vector<uint64_t> tick, serial;
    std::vector<std::vector<int>> kids;  // indexed children of each entry
    std::vector<int> root_kids;
    std::vector<int32_t> toks;           // [num_pages][page_size]

    // retained pages whose whole subtree is unreferenced: what leaf-first eviction can reach
    int evictable() const {
        if (!enabled) return 0;
        std::vector<char> blocked(num_pages, 0);
        for (int p = 0; p < num_pages; ++p)
            if (indexed[p] && refs[p] > 0)
                for (int q = p; q != ROOT && !blocked[q]; q = parent[q]) blocked[q] = 1;
        int n = 0;
        for (int p = 0; p < num_pages; ++p) n += indexed[p] && !blocked[p] ? 1 : 0;
        return n;
    }
    // the next page eviction takes, or -1
    int victim() const {
        int best = -1;
        if (!enabled) return best;
        for (int p = 0; p < num_pages; ++p)
            if (indexed[p] && refs[p] == 0 && kids[p].empty() && (best < 0 || tick[p] < tick[best])) best = p;
        return best;
    }

private:
    uint64_t clock = 0, serials = 0;
    std::unordered_multimap<uint64_t, int> by_hash;

    uint64_t hash_of(int par, const int32_t *t) const {
        uint64_t h = 1469598103934665603ull ^ (uint64_t)(uint32_t)par;
        for (int i = 0; i < page_size; ++i) h = (h ^ (uint32_t)t[i]) * 1099511628211ull;
        return TL_PREFIX_HASH_HOOK(h);
    }
    void touch(int entry) {
        const uint64_t now = ++clock;
        for (int q = entry; q != ROOT; q = parent[q]) tick[q] = now;
    }
    // take a childless entry out of the index; an unreferenced one returns to the free list
    void unindex(int p) {
        auto &sibs = parent[p] == ROOT ? root_kids : kids[parent[p]];
        sibs.erase(std::find(sibs.begin(), sibs.end(), p));
        auto range = by_hash.equal_range(hash_of(parent[p], &toks[(size_t)p * page_size]));
        for (auto it = range.first; it != range.second; ++it)
            if (it->second == p) {
                by_hash.erase(it);
                break;
            }
        indexed[p] = 0;
        n_entries--;
        if (refs[p] == 0) {
            retained--;
            free_pages.push_back(p);
        }
    }
    void enforce_cap() {
        while (max_retained > 0 && retained > max_retained) {
            const int v = victim();
            if (v < 0) break;
            unindex(v);
            ctr.pages_evicted++;
        }
    }
};

}  // namespace tl
