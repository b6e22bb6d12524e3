// Stand-alone check of csrc/lora_tiles.h, the host-only part of the LoRA kernels (built and run by tests/test_lora_cpu.py with
// -fsanitize=address,undefined): seeded random passes of 1 .. 16 sequences -- lengths 1 .. 300, adapters -1 .. 31 -- through
// lora_build_tiles.  After every pass:
//   * every row of every sequence lies in exactly one tile, no tile holds a row of no sequence;
//   * a tile has 1 .. 16 rows, all of ONE sequence, and carries that sequence's adapter; a sequence's tiles ascend and only its last
//     may be partial;
//   * the tile count is within lora_max_tiles, and the workspace sizes grow with it;
//   * bad input (an empty sequence, a negative row, an adapter below -1) is refused with the list cleared.
// Prints one line: the counts.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "lora_tiles.h"

using namespace tl;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);         \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main(int argc, char **argv) {
    const int passes = argc > 1 ? std::atoi(argv[1]) : 2000;
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    long tiles_seen = 0, partial = 0, adapted = 0, refused = 0;
    std::vector<LoraTile> tiles;
    for (int p = 0; p < passes; ++p) {
        const int n = 1 + (int)(rng() % 16);
        std::vector<int> row0(n), len(n), ad(n);
        int at = (int)(rng() % 3);  // (a pass need not start at row 0)
        for (int i = 0; i < n; ++i) {
            const unsigned pick = rng() % 8;
            len[i] = pick == 0 ? 1 : (pick == 1 ? 16 : (pick == 2 ? 17 : 1 + (int)(rng() % 300)));
            row0[i] = at;
            at += len[i];
            ad[i] = (int)(rng() % 33) - 1;
        }
        CHECK(lora_build_tiles(n, row0.data(), len.data(), ad.data(), tiles));
        CHECK((int)tiles.size() <= lora_max_tiles(at, n));
        std::vector<int> owner(at, -1);
        size_t t = 0;
        for (int i = 0; i < n; ++i) {
            int next = row0[i];
            while (next < row0[i] + len[i]) {
                CHECK(t < tiles.size());
                const LoraTile &tile = tiles[t++];
                CHECK(tile.row0 == next && tile.rows >= 1 && tile.rows <= LORA_TILE && tile.adapter == ad[i]);
                CHECK(tile.row0 + tile.rows <= row0[i] + len[i]);
                CHECK(tile.rows == LORA_TILE || tile.row0 + tile.rows == row0[i] + len[i]);
                for (int r = 0; r < tile.rows; ++r) {
                    CHECK(owner[tile.row0 + r] == -1);
                    owner[tile.row0 + r] = i;
                }
                next += tile.rows;
                partial += tile.rows < LORA_TILE;
                adapted += tile.adapter >= 0;
            }
        }
        CHECK(t == tiles.size());
        for (int i = 0; i < n; ++i)
            for (int r = row0[i]; r < row0[i] + len[i]; ++r) CHECK(owner[r] == i);
        tiles_seen += (long)tiles.size();
        CHECK(lora_partial_floats((int)tiles.size(), 2560) == tiles.size() * 5 * LORA_MAX_RTOT * LORA_TILE);
        CHECK(lora_ss_floats((int)tiles.size(), 9728) == tiles.size() * 19 * LORA_TILE);
        // one bad field refuses the whole pass
        const int victim = (int)(rng() % n), kind = (int)(rng() % 3);
        std::vector<int> r2 = row0, l2 = len, a2 = ad;
        if (kind == 0) l2[victim] = 0;
        if (kind == 1) r2[victim] = -1 - (int)(rng() % 5);
        if (kind == 2) a2[victim] = -2 - (int)(rng() % 5);
        CHECK(!lora_build_tiles(n, r2.data(), l2.data(), a2.data(), tiles) && tiles.empty());
        refused += 1;
    }
    lora_lookup_tiles(65, tiles);
    CHECK(tiles.size() == 5 && tiles[4].row0 == 64 && tiles[4].rows == 1 && tiles[0].adapter == LORA_ROW_LOOKUP);
    CHECK(lora_build_tiles(0, nullptr, nullptr, nullptr, tiles) && tiles.empty());
    std::printf("ok passes=%d tiles=%ld partial=%ld adapted=%ld refused=%ld\n", passes, tiles_seen, partial, adapted, refused);
    return 0;
}
