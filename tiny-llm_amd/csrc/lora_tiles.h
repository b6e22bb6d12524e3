// Host-only part of the LoRA kernels (lora.h): the tile list of a launch and the size of its workspace.  No HIP in here, so that
// tests/lora_tiles_check.cpp can build it alone under the address and undefined-behaviour sanitizers.
//
// A TILE is up to 16 consecutive activation rows that one workgroup serves with ONE pass over an adapter's matrices:
//   (row0, rows, adapter)   adapter >= 0: every row of the tile carries that adapter (a prefill chunk: the host knows the sequences);
//                           adapter == LORA_NONE: nothing to add -- the shrink workgroup exits at once;
//                           adapter == LORA_ROW_LOOKUP: each row looks its adapter up in a device array (a decode step: lora_of_slot).
// A prefill tile never straddles two sequences: a sequence of `len` rows becomes ceil(len / 16) tiles of its own.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace tl {

constexpr int LORA_TILE = 16;          // rows of a tile: the M of v_mfma_f32_16x16x32_bf16
constexpr int LORA_KS = 512;           // input columns of one shrink workgroup (a function of nothing: a row's sums never depend on the launch)
constexpr int LORA_MAX_SLICES = 64;    // in <= 32,768
constexpr int LORA_MAX_RANK = 64;      // TL_MAX_LORA_RANK
constexpr int LORA_MAX_RTOT = 3 * LORA_MAX_RANK;  // rows of a fused A: [A_q; A_k; A_v]
constexpr int LORA_NONE = -1;
constexpr int LORA_ROW_LOOKUP = -2;

struct LoraTile {
    int32_t row0, rows, adapter, pad;
};

static inline int lora_slices(int in) { return (in + LORA_KS - 1) / LORA_KS; }
// fp32 words of the shrink's partial results + the per-slice sums of squares, for n_tiles tiles of a projection with `in` columns
static inline size_t lora_partial_floats(int n_tiles, int in) { return (size_t)n_tiles * lora_slices(in) * LORA_MAX_RTOT * LORA_TILE; }
static inline size_t lora_ss_floats(int n_tiles, int in) { return (size_t)n_tiles * lora_slices(in) * LORA_TILE; }
// most tiles a pass of `rows` rows in `n_seqs` sequences can have (every sequence may end in a partial tile)
static inline int lora_max_tiles(int rows, int n_seqs) { return (rows + LORA_TILE - 1) / LORA_TILE + (n_seqs > 0 ? n_seqs - 1 : 0); }

// The tiles of a pass over sequences side by side: sequence i holds the rows [row0[i], row0[i] + len[i]) and carries adapter[i]
// (LORA_NONE or an id).  Tiles come out in the order of the call, ascending rows inside a sequence.  Returns false on bad input
// (a negative row, an empty sequence, an adapter below LORA_NONE) with `out` cleared.
static inline bool lora_build_tiles(int n_seqs, const int *row0, const int *len, const int *adapter, std::vector<LoraTile> &out) {
    out.clear();
    if (n_seqs < 0 || (n_seqs > 0 && (!row0 || !len || !adapter))) return false;
    for (int i = 0; i < n_seqs; ++i) {
        if (row0[i] < 0 || len[i] < 1 || adapter[i] < LORA_NONE || (long)row0[i] + len[i] > 0x7fffffffL) {
            out.clear();
            return false;
        }
        for (int r = 0; r < len[i]; r += LORA_TILE) {
            const int rows = len[i] - r < LORA_TILE ? len[i] - r : LORA_TILE;
            out.push_back(LoraTile{row0[i] + r, rows, adapter[i], 0});
        }
    }
    return true;
}
// The tiles of `rows` rows whose adapters a device array names per row (a decode step, tl_lora_rows without a tile list)
static inline void lora_lookup_tiles(int rows, std::vector<LoraTile> &out) {
    out.clear();
    for (int r = 0; r < rows; r += LORA_TILE) out.push_back(LoraTile{r, rows - r < LORA_TILE ? rows - r : LORA_TILE, LORA_ROW_LOOKUP, 0});
}

}  // namespace tl
