// matrix_plan.hpp — the parts of the distance matrix API (qmx_sample_points, qmx_search_matrix) that are plain integer logic, shared by the kernels of
// matrix.hip, the driver of api_matrix.hip and the stand-alone host check (tools/matrix_plan_check.cpp, built with the address and undefined-behaviour
// sanitizers): the sampler's key and its radix levels, the validation of a sample, the chunking of the queries and the clipping of the lists.
// No kernels and no runtime calls in here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QMX_MATRIX_HD __host__ __device__ __forceinline__
#else
#define QMX_MATRIX_HD inline
#endif

namespace qmx {

constexpr uint32_t MATRIX_MAX_SAMPLE = 65536;             // points per sample (qmx_sample_points' n, qmx_search_matrix' n_sample)
constexpr uint32_t MATRIX_MAX_CHUNK = 4096;               // queries searched per chunk, at most
constexpr uint64_t MATRIX_STAGE_BYTES = 256ull << 20;     // ... and the bytes their top-wide staging lists may take

// ---- the sampler's key: splitmix64 of the offset under `seed`.  The multiplier is odd and the finalizer a bijection of 64-bit words, so the keys of
// distinct offsets differ: "the n smallest (key, offset)" never needs the tie-break
QMX_MATRIX_HD uint64_t sample_key(uint64_t seed, uint32_t offset) {
    uint64_t z = seed + ((uint64_t)offset + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- the radix select over the keys: five levels of 12 bits from the top, then the last 4 bits
constexpr uint32_t SAMPLE_BINS = 4096;
constexpr uint32_t SAMPLE_LEVELS = 6;
QMX_MATRIX_HD uint32_t sample_level_bits(uint32_t level) { return level < 5 ? 12u : 4u; }
QMX_MATRIX_HD uint32_t sample_level_shift(uint32_t level) { return level < 5 ? 52u - 12u * level : 0u; }
// the key is still in the running at `level`: its bits above the level's digit are the boundary's
QMX_MATRIX_HD bool sample_in_prefix(uint64_t key, uint64_t prefix, uint32_t level) {
    if (level == 0) return true;
    const uint32_t above = sample_level_shift(level) + sample_level_bits(level);      // 52, 40, 28, 16, 4
    return (key >> above) == (prefix >> above);
}
QMX_MATRIX_HD uint32_t sample_bin(uint64_t key, uint32_t level) {
    return (uint32_t)(key >> sample_level_shift(level)) & ((1u << sample_level_bits(level)) - 1u);
}

// What the select knows between two levels (one device block; the host reads it back after each level).
struct SampleState {
    uint64_t prefix;         // the boundary key's digits found so far, the rest zero
    uint64_t threshold;      // done: the candidates with key <= threshold are the sample
    uint32_t need;           // candidates still to take among those in the prefix
    uint32_t done;
    uint32_t count;          // min(n, candidates), set by level 0
    uint32_t pad_;
};
// One level's decision from its histogram (bins of the candidates in the prefix; `groups`: the sums of 16 bins each, which the kernel's lanes form
// side by side): the boundary bin holds the need-th smallest key.  Everything in the bins below it is taken; when the boundary bin is taken whole the
// select is done, otherwise the next level splits it.
constexpr uint32_t SAMPLE_GROUP = 16;
QMX_MATRIX_HD void sample_level_step(SampleState &s, const uint32_t *hist, const uint32_t *groups, uint32_t level) {
    const uint32_t bins = 1u << sample_level_bits(level), shift = sample_level_shift(level), n_groups = bins / SAMPLE_GROUP;
    if (level == 0) {
        uint64_t total = 0;
        for (uint32_t g = 0; g < n_groups; ++g) total += groups[g];
        s.count = (uint32_t)(total < s.need ? total : s.need);
        if (total <= s.need) {      // every candidate
            s.threshold = ~0ull;
            s.done = 1;
            return;
        }
    }
    uint64_t below = 0;
    uint32_t g = 0;
    while (g + 1 < n_groups && below + groups[g] < s.need) below += groups[g++];
    uint32_t b = g * SAMPLE_GROUP;
    while (b + 1 < bins && below + hist[b] < s.need) below += hist[b++];
    s.prefix |= (uint64_t)b << shift;
    s.need -= (uint32_t)below;
    if (hist[b] <= s.need || shift == 0) {      // (shift 0: the prefix is a whole key, the bin holds that one candidate)
        s.threshold = s.prefix | (shift ? (1ull << shift) - 1 : 0ull);
        s.done = 1;
    }
}

// ---- qmx_search_matrix: the sample, the chunks, the lists
// 0: strictly ascending ids below n_rows;  1: not strictly ascending (unsorted or repeated);  2: an id past the rows.  *bad = the first offending position
inline int matrix_validate_sample(const uint32_t *ids, uint32_t n, uint64_t n_rows, uint32_t *bad) {
    for (uint32_t i = 0; i < n; ++i) {
        if (i && ids[i] <= ids[i - 1]) {
            *bad = i;
            return 1;
        }
        if (ids[i] >= n_rows) {
            *bad = i;
            return 2;
        }
    }
    return 0;
}
// entries searched per row: the limit best of the others and the row itself
QMX_MATRIX_HD uint32_t matrix_top(uint32_t n_sample, uint32_t limit) { return limit < n_sample ? limit + 1 : n_sample; }
// queries per chunk: their `top`-wide staging lists (8-byte entries) stay within MATRIX_STAGE_BYTES; whole 64-query tiles where that leaves any
inline uint32_t matrix_chunk(uint32_t n_sample, uint32_t limit) {
    const uint64_t top = matrix_top(n_sample, limit);
    uint64_t fit = top ? MATRIX_STAGE_BYTES / (top * 8) : MATRIX_MAX_CHUNK;
    if (fit > MATRIX_MAX_CHUNK) fit = MATRIX_MAX_CHUNK;
    if (fit >= 64) fit = fit / 64 * 64;
    if (fit < 1) fit = 1;
    return (uint32_t)(fit < n_sample ? fit : (n_sample ? n_sample : 1));
}
// A row's list after the scan: `count` entries in the contract's order, the row's own at `self_at` (count: not there).  The entries kept are those at
// positions != self_at, the first `limit` of them: entry k of the result is entry matrix_src(k, self_at) of the list.
QMX_MATRIX_HD uint32_t matrix_clip(uint32_t count, uint32_t self_at, uint32_t limit) {
    const uint32_t others = self_at < count ? count - 1 : count;
    return others < limit ? others : limit;
}
QMX_MATRIX_HD uint32_t matrix_src(uint32_t k, uint32_t self_at) { return k < self_at ? k : k + 1; }

// ---- f16 rows of 32 and more elements in the block of a qmx_search_matrix call (RowF16Avx, matrix_f16.hip)
// The reference's f16 AVX leaf (metric_f16/avx/dot.rs:13-69) keeps 4 registers x 8 SIMD lanes = 32 running sums, each fed once per iteration of 32
// elements, in order.  A lane of the scan owns one 16-byte piece of every 128-byte segment of a row, so a segment holds TWO iterations and a piece the
// two consecutive terms of four of the sums: piece 2 r + h = register r, SIMD lanes 4 h .. 4 h + 3, each as (iteration 2 s, iteration 2 s + 1).  An odd
// last iteration is paired with zeros, which change no sum.  The scalar tail (dim % 32 elements) follows the segments as it is.
constexpr uint32_t MATRIX_NO_SOURCE = 0xFFFFFFFFu;
QMX_MATRIX_HD uint32_t matrix_f16_avx_segments(uint32_t dim) { return (dim / 32 + 1) / 2; }
QMX_MATRIX_HD uint32_t matrix_f16_avx_dim(uint32_t dim) { return matrix_f16_avx_segments(dim) * 64 + dim % 32; }
// element `o` of a block row is element ... of the stored row (MATRIX_NO_SOURCE: a zero)
QMX_MATRIX_HD uint32_t matrix_f16_avx_source(uint32_t o, uint32_t dim) {
    const uint32_t iters = dim / 32, body = matrix_f16_avx_segments(dim) * 64;
    if (o >= body) return o - body < dim % 32 ? iters * 32 + (o - body) : MATRIX_NO_SOURCE;
    const uint32_t s = o / 64, piece = (o % 64) / 8, k = (o % 8) / 2, it = 2 * s + (o & 1);
    return it < iters ? 32 * it + 8 * (piece >> 1) + 4 * (piece & 1) + k : MATRIX_NO_SOURCE;
}

}  // namespace qmx
