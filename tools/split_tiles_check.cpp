// split_tiles_check.cpp — a stand-alone host run of the tile walk of qdrant_amd/csrc/split_tiles.hpp: which tiles a launch of a prefilter scan
// visits (every tile | the strided S-th | the complement), how a grid's blocks share them, and the grid the launchers pick.  No GPU, no HIP runtime:
//   c++ -std=c++17 -O1 -Iqdrant_amd/csrc tools/split_tiles_check.cpp -o /tmp/split_tiles_check && /tmp/split_tiles_check
#include <stdint.h>
#include <stdio.h>

#include <set>
#include <vector>

#include "split_tiles.hpp"

using namespace qmx;

static int failures = 0;
#define CHECK(cond, ...)                           \
    do {                                           \
        if (!(cond)) {                             \
            if (failures++ < 20) {                 \
                printf("FAILED %s: ", #cond);      \
                printf(__VA_ARGS__);               \
                printf("\n");                      \
            }                                      \
        }                                          \
    } while (0)

// one (stride, all_tiles): phases 1 and 2 together visit 0 .. all_tiles - 1 once each, phase 0 is the identity, a grid's blocks take every tile of a launch
static void check(uint32_t stride, uint64_t all_tiles) {
    const uint32_t word = stride << 8;      // (the stride's default, 16, also as "no stride given")
    for (int with_word = 0; with_word < (stride == SP_PHASE_STRIDE ? 2 : 1); ++with_word) {
        const uint32_t hi = with_word ? 0u : word;
        CHECK(split_phase_stride(hi | 1u) == stride, "stride %u", stride);
        std::vector<uint8_t> seen(all_tiles, 0);
        uint64_t total = 0;
        for (uint32_t ph = 1; ph <= 2; ++ph) {
            const uint64_t n = split_phase_tiles(all_tiles, hi | ph);
            total += n;
            uint64_t prev = 0;
            for (uint64_t j = 0; j < n; ++j) {
                const uint64_t t = split_phase_tile(j, hi | ph);
                CHECK(t < all_tiles, "stride %u tiles %llu phase %u: tile %llu of %llu", stride, (unsigned long long)all_tiles, ph, (unsigned long long)t,
                      (unsigned long long)j);
                CHECK(j == 0 || t > prev, "stride %u tiles %llu phase %u: not ascending at %llu", stride, (unsigned long long)all_tiles, ph, (unsigned long long)j);
                CHECK((t % stride == 0) == (ph == 1), "stride %u phase %u: tile %llu on the wrong side", stride, ph, (unsigned long long)t);
                if (t < all_tiles) ++seen[t];
                prev = t;
            }
        }
        CHECK(total == all_tiles, "stride %u tiles %llu: the phases hold %llu", stride, (unsigned long long)all_tiles, (unsigned long long)total);
        for (uint64_t t = 0; t < all_tiles; ++t) CHECK(seen[t] == 1, "stride %u tiles %llu: tile %llu visited %u times", stride, (unsigned long long)all_tiles,
                                                       (unsigned long long)t, (unsigned)seen[t]);
        CHECK(split_phase_tiles(all_tiles, hi) == all_tiles, "phase 0 of %llu tiles", (unsigned long long)all_tiles);
        for (uint64_t j = 0; j < all_tiles; j += (all_tiles > 4096 ? 97 : 1)) CHECK(split_phase_tile(j, hi) == j, "phase 0 is the identity at %llu", (unsigned long long)j);
        for (uint32_t ph = 0; ph <= 2; ++ph) {
            const uint64_t n = split_phase_tiles(all_tiles, hi | ph);
            static std::set<uint64_t> shared_out;      // (the blocks' shares depend on the launch's tile count alone: each count once)
            const bool first_time = shared_out.insert(n).second;
            for (uint64_t g = 1; g <= 300 && first_time; ++g) {
                uint64_t sum = 0;
                for (uint64_t b = 0; b < g; ++b) sum += split_block_tiles(n, b, g);
                CHECK(sum == n, "stride %u tiles %llu phase %u grid %llu: the blocks take %llu of %llu", stride, (unsigned long long)all_tiles, ph,
                      (unsigned long long)g, (unsigned long long)sum, (unsigned long long)n);
            }
            // the launchers' grid, for tiles of 256 and of 128 rows, full and ragged last tiles
            static const int cus[] = {1, 2, 64, 256, 304};
            for (int c = 0; c < 5; ++c)
                for (uint32_t bm = 128; bm <= 256; bm *= 2)
                    for (int ragged = 0; ragged < 2; ++ragged) {
                        if (all_tiles == 0 && ragged) continue;
                        const uint64_t rows = all_tiles * bm - (ragged ? bm - 1 : 0);
                        const SplitGrid sg = split_scan_grid(rows, bm, hi | ph, cus[c]);
                        CHECK(sg.n_tiles == n, "grid helper: %llu rows in tiles of %u, phase %u: %llu tiles, not %llu", (unsigned long long)rows, bm, ph,
                              (unsigned long long)sg.n_tiles, (unsigned long long)n);
                        CHECK(sg.grid <= (uint32_t)cus[c] && sg.grid <= sg.n_tiles, "grid helper: grid %u for %llu tiles on %d CUs", sg.grid,
                              (unsigned long long)sg.n_tiles, cus[c]);
                        CHECK((sg.grid == 0) == (sg.n_tiles == 0), "grid helper: grid %u for %llu tiles", sg.grid, (unsigned long long)sg.n_tiles);
                    }
        }
    }
}

int main() {
    for (uint32_t stride = 2; stride <= 255; ++stride) {
        for (uint64_t all = 0; all <= 69; ++all) check(stride, all);
        const uint64_t more[] = {stride - 1ull, stride, stride + 1ull, 2ull * stride, 2ull * stride + 1, 1000, 39063};
        for (uint64_t all : more) check(stride, all);
    }
    for (uint32_t ph = 0; ph <= 2; ++ph) {
        const SplitGrid sg = split_scan_grid(0, 256, ph, 256);
        CHECK(sg.n_tiles == 0 && sg.grid == 0, "no rows: %llu tiles, grid %u", (unsigned long long)sg.n_tiles, sg.grid);
    }
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
