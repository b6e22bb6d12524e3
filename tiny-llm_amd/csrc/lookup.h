// Prompt-lookup proposals on the device (include/tinyllm_engine.h "Prompt lookup"): the draft-free proposer of
// speculative decoding ("ngram" speculation, prompt_lookup_num_tokens).  It finds the last few ids of a row earlier in the row and
// proposes what followed them; tl_engine_verify_batch then checks the proposals.
//
// The contract.  T[s0 .. e] are a row's ids and last = T[e].  N = max_ngram in 1 .. LOOKUP_MAX_NGRAM, min_ngram in 1 .. N, K proposals in
// 1 .. LOOKUP_MAX_PROPOSALS.
//   candidate   every i in [s0, e) with T[i] == last
//   raw(i)      the largest m <= min(N, i - s0 + 1) with T[i - j] == T[e - j] for all 0 <= j < m
//   eligible    raw(i) >= min_ngram
//   avail(i)    min(K, e - i)
//   choice      the eligible candidate with the largest (raw, avail, i), compared in that order: the longest match, then the most
//               continuation ids, then the most recent
//   proposals   T[i + 1 .. i + avail]; the count is avail, 0 where nothing is eligible
// Integer compares decide everything.  Each thread keeps the largest key raw << 27 | avail << 24 | i of the candidates it walks (one
// 32-bit word: positions below 2^24), the wave takes the maximum over its lanes, the waves meet in LDS: the result does not depend on the
// order in which threads run, and no atomic touches global memory.  Ids outside [s0, e] are never read as data.
//
// lookup_rows_kernel     one workgroup per caller row: T[e] is in the row
// lookup_engine_kernel   one workgroup per named slot of the engine.  The slot's history row H holds the ids of positions s0 .. rec - 1;
//                        the ids of the decode steps since -- positions rec .. ctx - 1 -- still lie in the slot's token ring, and the
//                        workgroup first fetches them, H[j] = ring[(produced - 1 - (ctx - j)) mod ring_cap], ahead of a barrier.  e = ctx,
//                        and last is the slot's pending token, read from tokens[slot]: H[e] is never read.  The result row is the pending
//                        token followed by the proposals, which is a chunk of tl_engine_verify_batch
// lookup_catch_up_kernel the same fetch as a launch of its own (rewind, fork, move, park, a chunk that is about to be recorded, a decode
//                        call that would outrun the ring)
// lookup_record_kernel   uploaded ids -> the history row (behind the token upload of a prefill / score / embed / verify chunk or a prefix
//                        attach; the pending token behind tl_engine_set_token)
#pragma once
#include "common.h"

namespace tl {

constexpr int LOOKUP_MAX_NGRAM = 16;     // TL_LOOKUP_MAX_NGRAM
constexpr int LOOKUP_MAX_PROPOSALS = 7;  // TL_LOOKUP_MAX_PROPOSALS
constexpr int LOOKUP_ROW = 8;            // words of a result row
constexpr int LOOKUP_MAX_SLOTS = 64;     // slots of one engine launch (the sequences of one tl_engine_verify_batch)
constexpr int LOOKUP_THREADS = 1024;
constexpr int LOOKUP_POS_BITS = 24;      // positions in a key
constexpr int LOOKUP_OUT_WORDS = LOOKUP_MAX_SLOTS * LOOKUP_ROW + LOOKUP_MAX_SLOTS;  // the result rows, then the counts

struct LookupArgs {
    int32_t *seq;          // [rows, cap] caller rows; the engine: [slots, cap] history rows
    int cap;
    const int32_t *start;  // [rows] s0 (caller rows)
    const int32_t *end;    // [rows] e (caller rows)
    int max_ngram, min_ngram, k;
    int32_t *proposals;    // [rows, LOOKUP_ROW]: the proposals, -1 behind them (the engine: the pending token first)
    int32_t *counts;       // [rows]
    int32_t *match;        // [rows, 2] (i, raw) of the choice, (-1, 0) without one; nullptr: not wanted
};
// a slot of an engine launch, as the host's accounting has it (slot_settings.h)
struct LookupSlot {
    int32_t slot, s0, rec, ctx, produced;
    int32_t k;  // proposals wanted: min(K, the caller's max_len - 1), may be 0
};
struct LookupSlots {
    LookupSlot s[LOOKUP_MAX_SLOTS];
};
struct LookupRing {
    const int32_t *ring;    // [slots, ring_cap]
    const int32_t *tokens;  // [slots] the pending tokens
    int ring_cap;
};

template <int N>
__device__ __forceinline__ uint32_t lookup_dpp_ror(uint32_t v) {  // (common.h dpp_row_ror_self on an unsigned word)
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x120 + N, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t lookup_wave_max(uint32_t v) {
    v = max(v, lookup_dpp_ror<8>(v));
    v = max(v, lookup_dpp_ror<4>(v));
    v = max(v, lookup_dpp_ror<2>(v));
    v = max(v, lookup_dpp_ror<1>(v));
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return max(max(r0, r1), max(r2, r3));
}

// H[j] = the id fed at position j, for rec <= j < ctx, from the ring (the last ring entry is the pending token, fed at ctx)
__device__ __forceinline__ void lookup_fetch(int32_t *H, const int32_t *ring, int ring_cap, int rec, int ctx, int produced, int cap, int first, int stride) {
    for (int j = max(rec, 0) + first; j < min(ctx, cap); j += stride) {
        const int n = produced - 1 - (ctx - j);
        H[j] = ring[((n % ring_cap) + ring_cap) % ring_cap];
    }
}

// The rule over T[s0 .. e] by the whole workgroup (every thread calls it; uniform arguments): T[e] is `last` and is not read.
// out[0 .. LOOKUP_ROW - shift) takes the proposals and -1 behind them.  0 <= s0, e < cap, K <= LOOKUP_ROW - shift
__device__ __forceinline__ void lookup_row(const int32_t *T, int s0, int e, int32_t last, int N, int min_ngram, int K, int32_t *out, int shift,
                                           int32_t *count, int32_t *match) {
    __shared__ int32_t s_tail[LOOKUP_MAX_NGRAM];  // s_tail[j] = T[e - j]
    __shared__ uint32_t s_key[LOOKUP_THREADS / WAVE];
    const int tid = threadIdx.x;
    if (tid < LOOKUP_MAX_NGRAM) s_tail[tid] = tid == 0 ? last : (e - tid >= s0 ? T[e - tid] : -1);
    __syncthreads();
    uint32_t best = 0u;
    if (K > 0) {
        for (int i = s0 + tid; i < e; i += LOOKUP_THREADS) {
            if (T[i] != last) continue;
            const int lim = min(N, i - s0 + 1);
            int raw = 1;
            while (raw < lim && T[i - raw] == s_tail[raw]) ++raw;
            if (raw < min_ngram) continue;
            best = max(best, (uint32_t)raw << (LOOKUP_POS_BITS + 3) | (uint32_t)min(K, e - i) << LOOKUP_POS_BITS | (uint32_t)i);
        }
    }
    best = lookup_wave_max(best);
    if ((tid & (WAVE - 1)) == 0) s_key[tid / WAVE] = best;
    __syncthreads();
    if (tid < LOOKUP_ROW) {
        uint32_t key = 0u;
#pragma unroll
        for (int w = 0; w < LOOKUP_THREADS / WAVE; ++w) key = max(key, s_key[w]);
        const int i = (int)(key & ((1u << LOOKUP_POS_BITS) - 1u)), avail = (int)(key >> LOOKUP_POS_BITS & 7u), raw = (int)(key >> (LOOKUP_POS_BITS + 3));
        if (tid < LOOKUP_ROW - shift) {
            int32_t v = -1;
            if (tid < avail) v = i + 1 + tid == e ? last : T[i + 1 + tid];
            out[shift + tid] = v;
        }
        if (tid == 0) {
            *count = avail;
            if (match) match[0] = key ? i : -1, match[1] = raw;
        }
    }
}

static __global__ __launch_bounds__(LOOKUP_THREADS) void lookup_rows_kernel(const LookupArgs a) {
    const int row = blockIdx.x;
    const int s0 = max(a.start[row], 0), e = a.end[row];
    int32_t *out = a.proposals + (long)row * LOOKUP_ROW;
    if (e < s0 || e >= a.cap) {  // uniform: no ids, no proposals
        if (threadIdx.x < LOOKUP_ROW) out[threadIdx.x] = -1;
        if (threadIdx.x == 0) {
            a.counts[row] = 0;
            if (a.match) a.match[2 * row] = -1, a.match[2 * row + 1] = 0;
        }
        return;
    }
    const int32_t *T = a.seq + (long)row * a.cap;
    lookup_row(T, s0, e, T[e], a.max_ngram, a.min_ngram, a.k, out, 0, a.counts + row, a.match ? a.match + 2 * row : nullptr);
}

static __global__ __launch_bounds__(LOOKUP_THREADS) void lookup_engine_kernel(const LookupArgs a, const LookupRing r, const LookupSlots slots) {
    const LookupSlot s = slots.s[blockIdx.x];
    int32_t *H = a.seq + (long)s.slot * a.cap;
    int32_t *out = a.proposals + (long)blockIdx.x * LOOKUP_ROW;
    const int32_t last = r.tokens[s.slot];
    lookup_fetch(H, r.ring + (long)s.slot * r.ring_cap, r.ring_cap, s.rec, s.ctx, s.produced, a.cap, threadIdx.x, LOOKUP_THREADS);
    __syncthreads();  // the fetched ids are read by other threads of this workgroup only
    if (threadIdx.x == 0) out[0] = last;
    const int s0 = max(s.s0, 0), e = min(s.ctx, a.cap);  // (e == cap: the row is full; H[e] is never read)
    lookup_row(H, s0, e, last, a.max_ngram, a.min_ngram, e >= s0 ? s.k : 0, out, 1, a.counts + blockIdx.x, nullptr);
}

struct LookupCatchUpArgs {
    int32_t *row;         // the slot's history row
    const int32_t *ring;  // the slot's ring
    int ring_cap, rec, ctx, produced, cap;
};
static __global__ __launch_bounds__(256) void lookup_catch_up_kernel(const LookupCatchUpArgs a) {
    lookup_fetch(a.row, a.ring, a.ring_cap, a.rec, a.ctx, a.produced, a.cap, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// H[start + i] = tokens[i], i < n.  grid = ceil(n / 256)
struct LookupRecordArgs {
    const int32_t *tokens;  // [n]
    int32_t *row;
    int n, start, cap;
};
static __global__ __launch_bounds__(256) void lookup_record_kernel(const LookupRecordArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.n && a.start + i >= 0 && a.start + i < a.cap) a.row[a.start + i] = a.tokens[i];
}

}  // namespace tl
