// Stop sets (include/tinyllm_engine.h "Stop conditions"): the ids and byte strings that end a sequence, and the byte
// automaton the device walks for the strings.  Host only, no HIP include and no device pointer: engine.hip uploads what this builds, and
// tests/stop_set_check.cpp drives the same code alone against a naive scan.
//
//   automaton  a dense Aho-Corasick DFA over the strings: table[n_states][256] uint16, state 0 the root, n_states <= 1 + the sum of the
//              string lengths (at most 1,025).  After any text the state is the longest suffix of the text that is a prefix of some string,
//              so a state's depth never exceeds the longest string: a walk that starts at the root max_len - 1 bytes early has reached the
//              true state (stop.h cuts long tokens into segments on that).
//   match      per state the LONGEST string that ends there (the state's own string where one ends exactly there -- nothing longer can,
//              the state is the whole match -- else what its failure state reports), -1 for none, and that string's length.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace tl {

constexpr int STOP_MAX_IDS = 16;       // TL_MAX_STOP_IDS
constexpr int STOP_MAX_STRINGS = 16;   // TL_MAX_STOP_STRINGS
constexpr int STOP_MAX_BYTES = 1024;   // TL_MAX_STOP_BYTES

struct StopSet {
    std::vector<int32_t> ids;
    std::vector<int32_t> offsets;  // [n_strings + 1]
    std::vector<uint8_t> bytes;
    int n_strings = 0, max_len = 0;
    int n_states = 0;              // 0: no strings
    std::vector<uint16_t> table;   // [n_states][256]
    std::vector<int16_t> match;    // [n_states] the longest string ending in the state, -1: none
    std::vector<uint16_t> match_len;

    int id_index(int32_t token) const {
        for (size_t i = 0; i < ids.size(); ++i)
            if (ids[i] == token) return (int)i;
        return -1;
    }
};

// Validates and builds.  nullptr, or the refusal's message with `out` untouched.  vocab > 0: ids must lie in [0, vocab); vocab <= 0 (a
// set made without a vocabulary): they must be nonnegative, and the call that arms a slot checks them against the engine's size.
inline const char *stop_set_build(int vocab, const int32_t *ids, int n_ids, const uint8_t *bytes, const int32_t *offsets, int n_strings, StopSet &out) {
    if (n_ids < 0 || n_ids > STOP_MAX_IDS) return "stop_create: at most 16 stop ids";
    if (n_strings < 0 || n_strings > STOP_MAX_STRINGS) return "stop_create: at most 16 stop strings";
    if (n_ids + n_strings == 0) return "stop_create: a stop set needs an id or a string (a budget alone needs no set)";
    if (n_ids > 0 && !ids) return "stop_create: null ids";
    if (n_strings > 0 && (!bytes || !offsets)) return "stop_create: null strings";
    for (int i = 0; i < n_ids; ++i) {
        if (ids[i] < 0 || (vocab > 0 && ids[i] >= vocab)) return "stop_create: stop id out of range";
        for (int j = 0; j < i; ++j)
            if (ids[j] == ids[i]) return "stop_create: duplicate stop id";
    }
    if (n_strings > 0 && offsets[0] != 0) return "stop_create: offsets[0] must be 0";
    for (int i = 0; i < n_strings; ++i) {
        if (offsets[i + 1] <= offsets[i]) return "stop_create: a stop string is empty (or the offsets decrease)";
        if (offsets[i + 1] > STOP_MAX_BYTES) return "stop_create: the stop strings hold more than 1,024 bytes";
        const int len = offsets[i + 1] - offsets[i];
        for (int j = 0; j < i; ++j)
            if (offsets[j + 1] - offsets[j] == len && memcmp(bytes + offsets[j], bytes + offsets[i], (size_t)len) == 0) return "stop_create: duplicate stop string";
    }

    StopSet s;
    s.ids.assign(ids, ids + n_ids);
    s.n_strings = n_strings;
    if (n_strings > 0) {
        s.offsets.assign(offsets, offsets + n_strings + 1);
        s.bytes.assign(bytes, bytes + offsets[n_strings]);
        // the trie: children 0 = none (the root is nobody's child)
        std::vector<uint16_t> &t = s.table;
        std::vector<int16_t> own(1, -1);
        std::vector<uint16_t> depth(1, 0);
        t.assign(256, 0);
        for (int i = 0; i < n_strings; ++i) {
            int st = 0;
            for (int k = offsets[i]; k < offsets[i + 1]; ++k) {
                uint16_t next = t[(size_t)st * 256 + bytes[k]];
                if (next == 0) {
                    next = (uint16_t)own.size();
                    t[(size_t)st * 256 + bytes[k]] = next;
                    t.resize(t.size() + 256, 0);
                    own.push_back(-1);
                    depth.push_back((uint16_t)(depth[st] + 1));
                }
                st = next;
            }
            own[st] = (int16_t)i;
            s.max_len = std::max(s.max_len, offsets[i + 1] - offsets[i]);
        }
        // breadth first: a state's failure state is shallower, so its row and its match are final when the state is reached
        const int n = (int)own.size();
        s.n_states = n;
        s.match.assign(n, -1);
        s.match_len.assign(n, 0);
        std::vector<uint16_t> fail(n, 0), order;
        order.reserve(n);
        for (int b = 0; b < 256; ++b)
            if (t[b]) order.push_back(t[b]);
        for (size_t at = 0; at < order.size(); ++at) {
            const int st = order[at], f = fail[st];
            if (own[st] >= 0) s.match[st] = own[st], s.match_len[st] = depth[st];
            else s.match[st] = s.match[f], s.match_len[st] = s.match_len[f];
            for (int b = 0; b < 256; ++b) {
                const uint16_t child = t[(size_t)st * 256 + b];
                if (child) {
                    fail[child] = t[(size_t)f * 256 + b];
                    order.push_back(child);
                } else {
                    t[(size_t)st * 256 + b] = t[(size_t)f * 256 + b];
                }
            }
        }
    }
    out = std::move(s);
    return nullptr;
}

// The definition's step 3 for one token's bytes on the host (tl_engine_stop_state never needs it; the check program and the rows it
// feeds do): walks `n` bytes from *state; true when a string ends inside, with *at = the first such byte's index, *index = the longest
// string ending there and *len its length.  *state is the state after the last byte walked.
inline bool stop_set_walk(const StopSet &s, int *state, const uint8_t *bytes, int n, int *at, int *index, int *len) {
    for (int k = 0; k < n; ++k) {
        *state = s.table[(size_t)*state * 256 + bytes[k]];
        if (s.match[*state] >= 0) {
            *at = k, *index = s.match[*state], *len = s.match_len[*state];
            return true;
        }
    }
    return false;
}

}  // namespace tl
