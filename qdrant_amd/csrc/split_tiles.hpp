// split_tiles.hpp — which tiles a launch of a prefilter scan over a derived copy visits, and which of them a block takes.  Host and device
// read the same arithmetic: the scan kernels (scan_split.hip, scan_i8copy.hip), their launchers and the regroup behind them
// (split_select.hip), and a host-only check (tools/split_tiles_check.cpp).  Nothing here needs the HIP runtime.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SPLIT_HD __host__ __device__
#else
#define SPLIT_HD
#endif

namespace qmx {

constexpr uint32_t SP_PHASE_STRIDE = 16;
// `phase` as the launchers take it: low byte 0 = every tile, 1 = tiles 0, S, 2 S, ... (the strided sample), 2 = all the others; the bytes above = S (0: 16)
SPLIT_HD inline uint32_t split_phase_stride(uint32_t phase) { const uint32_t st = phase >> 8; return st >= 2 ? st : SP_PHASE_STRIDE; }
SPLIT_HD inline uint64_t split_phase_tiles(uint64_t all_tiles, uint32_t phase) {
    const uint32_t st = split_phase_stride(phase), ph = phase & 0xFFu;
    const uint64_t first = (all_tiles + st - 1) / st;
    return ph == 0 ? all_tiles : ph == 1 ? first : all_tiles - first;
}
// the j-th tile of a launch: every tile | the strided S-th (0, S, 2 S, ...: a sample that sees the whole block, whatever its order) | the
// complement (j + j / (S - 1) + 1 skips the multiples of S)
struct SplitTileWalk {
    uint32_t ph, stride;
    SPLIT_HD explicit SplitTileWalk(uint32_t phase) : ph(phase & 0xFFu), stride(split_phase_stride(phase)) {}
    SPLIT_HD uint64_t tile(uint64_t j) const { return ph == 0 ? j : ph == 1 ? j * stride : j + j / (stride - 1) + 1; }
};
SPLIT_HD inline uint64_t split_phase_tile(uint64_t j, uint32_t phase) { return SplitTileWalk(phase).tile(j); }
// how many of a launch's n_tiles block b of a grid of g takes (its i-th is the launch's (b + i g)-th)
SPLIT_HD inline uint64_t split_block_tiles(uint64_t n_tiles, uint64_t b, uint64_t g) { return b < n_tiles ? (n_tiles - b + g - 1) / g : 0; }

// the launch of a scan over n_cand rows in tiles of rows_per_tile: its tiles and its grid (one block per CU at most; no tiles: no launch).  The scan
// and the regroup that reads its lists both ask here.
struct SplitGrid {
    uint64_t n_tiles;
    uint32_t grid;
};
inline SplitGrid split_scan_grid(uint64_t n_cand, uint32_t rows_per_tile, uint32_t phase, int num_cus) {
    const uint64_t n_tiles = split_phase_tiles((n_cand + rows_per_tile - 1) / rows_per_tile, phase);
    const uint64_t cus = num_cus > 1 ? (uint64_t)num_cus : 1;
    return SplitGrid{n_tiles, (uint32_t)(n_tiles < cus ? n_tiles : cus)};
}

}  // namespace qmx
