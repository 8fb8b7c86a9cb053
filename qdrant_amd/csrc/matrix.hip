// matrix.hip — the kernels of the distance matrix API (qmx_sample_points, qmx_search_matrix; api_matrix.hip): "sample `sample` points under a filter and
// return, for each of them, its `limit` nearest among the other sampled points" (Collection::search_points_matrix,
// lib/collection/src/collection/distance_matrix.rs).  The scores themselves come from the exact top-k scans, unchanged; what is here:
//
//   sample_hist_kernel     : one level of the radix select over the sampler's keys - a pass over the liveness words, a 4 096-bin LDS histogram of the
//                            level's digit of every candidate still in the boundary's prefix, flushed to the global histogram by atomics
//   sample_boundary_kernel : one block takes the level's decision (matrix_plan.hpp sample_level_step) and clears the histogram for the next level
//   sample_count_kernel    : per block of 256 words, how many candidates lie at or below the threshold the select ended with;
//   sample_scan_kernel     : ... the exclusive prefix of those counts (one block);
//   sample_write_kernel    : ... and the ordered compaction: ascending offsets, nothing sorts ids
//   matrix_gather_kernel   : the sample's rows -> a transient block (one wave per row, 16-byte pieces), its deleted bitmap and the positions 0..S
//   matrix_gather_f16_avx_kernel : ... for f16 rows of 32 and more elements, in the layout whose scan (matrix_f16.hip) sums in the reference's order
//   matrix_finish_kernel   : one wave per row drops the row's own entry by POSITION, cuts to `limit`, writes hits, columns and counts
//
// The integer logic they share with the host (and with the sanitized host check) is matrix_plan.hpp.
#include "kernels.hpp"
#include "matrix_plan.hpp"

namespace qmx {

namespace {

constexpr int SAMPLE_BLOCK = 256;
constexpr int MATRIX_ROWS_PER_BLOCK = 4;      // waves of a gather / finish block, one row each

__device__ __forceinline__ uint64_t low_bits(uint64_t k) { return k >= 64 ? ~0ull : (1ull << k) - 1; }

// the candidates among offsets 64 w .. 64 w + 63, as DeletedView::live takes them one by one: below the rows, not deleted (past the point flags:
// deleted; past the vector flags: not), allowed (past the allow bits: not)
__device__ __forceinline__ uint64_t sample_word(const DeletedView &del, uint64_t w) {
    const uint64_t base = w * 64;
    uint64_t live = base < del.n_rows ? low_bits(del.n_rows - base) : 0ull;
    if (del.point_deleted) live &= base < del.n_point_bits ? ~del.point_deleted[w] & low_bits(del.n_point_bits - base) : 0ull;
    if (del.vec_deleted && base < del.n_vec_bits) live &= ~(del.vec_deleted[w] & low_bits(del.n_vec_bits - base));
    if (del.allowed) live &= base < del.n_allowed_bits ? del.allowed[w] & low_bits(del.n_allowed_bits - base) : 0ull;
    return live;
}

// ... those of them the finished select takes
__device__ __forceinline__ uint64_t sample_chosen_word(const DeletedView &del, uint64_t w, uint64_t seed, uint64_t threshold) {
    uint64_t m = sample_word(del, w), chosen = 0;
    while (m) {
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        if (sample_key(seed, (uint32_t)(w * 64 + b)) <= threshold) chosen |= 1ull << b;
    }
    return chosen;
}

// exclusive prefix of one value per lane over a block of SAMPLE_BLOCK lanes; *total: the block's sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *sh_waves, uint32_t *total) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, off, WAVE);
        if (lane >= off) incl += o;
    }
    __syncthreads();      // (the caller may still read sh_waves of an earlier call)
    if (lane == WAVE - 1) sh_waves[wave] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (int i = 0; i < SAMPLE_BLOCK / WAVE; ++i) {
        before += i < wave ? sh_waves[i] : 0u;
        sum += sh_waves[i];
    }
    *total = sum;
    return before + incl - v;
}

}  // namespace

// ---- the sampler ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_hist_kernel(DeletedView del, uint64_t n_words, uint64_t seed, uint32_t level, const SampleState *state,
                                                                   uint32_t *hist) {
    __shared__ uint32_t sh_hist[SAMPLE_BINS];
    for (uint32_t i = threadIdx.x; i < SAMPLE_BINS; i += SAMPLE_BLOCK) sh_hist[i] = 0;
    __syncthreads();
    const uint64_t prefix = level ? state->prefix : 0ull;
    for (uint64_t w = (uint64_t)blockIdx.x * SAMPLE_BLOCK + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * SAMPLE_BLOCK) {
        uint64_t m = sample_word(del, w);
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const uint64_t key = sample_key(seed, (uint32_t)(w * 64 + b));
            if (sample_in_prefix(key, prefix, level)) atomicAdd(&sh_hist[sample_bin(key, level)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < SAMPLE_BINS; i += SAMPLE_BLOCK)
        if (sh_hist[i]) atomicAdd(&hist[i], sh_hist[i]);
}

__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_boundary_kernel(uint32_t *hist, SampleState *state, uint32_t level) {
    __shared__ uint32_t sh_hist[SAMPLE_BINS], sh_groups[SAMPLE_BINS / SAMPLE_GROUP];
    for (uint32_t i = threadIdx.x; i < SAMPLE_BINS; i += SAMPLE_BLOCK) {
        sh_hist[i] = hist[i];
        hist[i] = 0;      // (the next level, or the next call, starts from zeros)
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < SAMPLE_BINS / SAMPLE_GROUP; g += SAMPLE_BLOCK) {
        uint32_t sum = 0;
        for (uint32_t j = 0; j < SAMPLE_GROUP; ++j) sum += sh_hist[g * SAMPLE_GROUP + j];
        sh_groups[g] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        SampleState s = *state;
        sample_level_step(s, sh_hist, sh_groups, level);
        *state = s;
    }
}

// block b counts the taken candidates of words 256 b .. 256 b + 255
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_count_kernel(DeletedView del, uint64_t n_words, uint64_t seed, const SampleState *state,
                                                                    uint32_t *block_counts) {
    __shared__ uint32_t sh_waves[SAMPLE_BLOCK / WAVE];
    const uint64_t w = (uint64_t)blockIdx.x * SAMPLE_BLOCK + threadIdx.x;
    const uint32_t mine = w < n_words ? (uint32_t)__popcll(sample_chosen_word(del, w, seed, state->threshold)) : 0u;
    uint32_t total = 0;
    (void)block_exclusive_scan(mine, sh_waves, &total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// in place: counts -> their exclusive prefix (one block, SAMPLE_BLOCK entries per step)
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_scan_kernel(uint32_t *block_counts, uint32_t n_blocks) {
    __shared__ uint32_t sh_waves[SAMPLE_BLOCK / WAVE];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += SAMPLE_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? block_counts[i] : 0u;
        uint32_t total = 0;
        const uint32_t before = block_exclusive_scan(v, sh_waves, &total);
        if (i < n_blocks) block_counts[i] = carry + before;
        carry += total;
    }
}

// the taken offsets in ascending order: a word's first goes to (the block's prefix) + (the taken of the block's earlier words); nothing is written past `cap`
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_write_kernel(DeletedView del, uint64_t n_words, uint64_t seed, const SampleState *state,
                                                                    const uint32_t *block_offsets, uint32_t *out, uint32_t cap) {
    __shared__ uint32_t sh_waves[SAMPLE_BLOCK / WAVE];
    const uint64_t w = (uint64_t)blockIdx.x * SAMPLE_BLOCK + threadIdx.x;
    uint64_t chosen = w < n_words ? sample_chosen_word(del, w, seed, state->threshold) : 0ull;
    uint32_t total = 0;
    uint32_t pos = block_offsets[blockIdx.x] + block_exclusive_scan((uint32_t)__popcll(chosen), sh_waves, &total);
    while (chosen) {
        const int b = __builtin_ctzll(chosen);
        chosen &= chosen - 1;
        if (pos < cap) out[pos] = (uint32_t)(w * 64 + b);
        ++pos;
    }
}

// ---- the matrix: gather and finish ------------------------------------------------------------------------------------------------------------------
// Row i of the block = stored row ids[i] (ids below n_rows: validated by the caller), in 16-byte pieces, the tail behind row_bytes zero; bit i of
// `deleted` (zeroed by the caller) is set when ids[i] is not live; positions[i] = i.  src16: base and stride of the stored rows are 16-byte multiples.
__global__ __launch_bounds__(MATRIX_ROWS_PER_BLOCK * WAVE) void matrix_gather_kernel(const char *rows, uint64_t row_stride, uint64_t row_bytes, int src16,
                                                                                     const uint32_t *ids, uint32_t n, DeletedView del, char *block,
                                                                                     uint64_t pitch, unsigned long long *deleted, uint32_t *positions) {
    const uint32_t i = blockIdx.x * MATRIX_ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    if (i >= n) return;
    const uint32_t id = ids[i];
    const char *src = rows + (uint64_t)id * row_stride;
    char *dst = block + (uint64_t)i * pitch;
    for (uint64_t o = (uint64_t)lane * 16; o < pitch; o += (uint64_t)WAVE * 16) {
        uint4 v;
        if (src16 && o + 16 <= row_bytes) {
            v = *reinterpret_cast<const uint4 *>(src + o);
        } else {
            uint32_t part[4] = {0u, 0u, 0u, 0u};
            for (uint32_t j = 0; j < 16; ++j)
                if (o + j < row_bytes) part[j >> 2] |= (uint32_t)(uint8_t)src[o + j] << (8 * (j & 3));
            v = make_uint4(part[0], part[1], part[2], part[3]);
        }
        *reinterpret_cast<uint4 *>(dst + o) = v;
    }
    if (lane == 0) {
        positions[i] = i;
        if (!del.live(id)) atomicOr(&deleted[i >> 6], 1ull << (i & 63));
    }
}

// The same for f16 rows of `dim` >= 32 elements, in the layout of RowF16Avx (matrix_plan.hpp matrix_f16_avx_source): a lane puts a 16-byte piece together
// from the two iterations it interleaves and stores it whole; the pitch covers block_dim elements.
__global__ __launch_bounds__(MATRIX_ROWS_PER_BLOCK * WAVE) void matrix_gather_f16_avx_kernel(const char *rows, uint64_t row_stride, uint32_t dim,
                                                                                             const uint32_t *ids, uint32_t n, DeletedView del, char *block,
                                                                                             uint64_t pitch, unsigned long long *deleted, uint32_t *positions) {
    const uint32_t i = blockIdx.x * MATRIX_ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    if (i >= n) return;
    const uint32_t id = ids[i];
    const uint16_t *src = reinterpret_cast<const uint16_t *>(rows + (uint64_t)id * row_stride);
    char *dst = block + (uint64_t)i * pitch;
    for (uint64_t o = (uint64_t)lane * 16; o < pitch; o += (uint64_t)WAVE * 16) {
        uint32_t part[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t from = matrix_f16_avx_source((uint32_t)(o / 2) + j, dim);
            if (from != MATRIX_NO_SOURCE) part[j >> 1] |= (uint32_t)src[from] << (16 * (j & 1));
        }
        *reinterpret_cast<uint4 *>(dst + o) = make_uint4(part[0], part[1], part[2], part[3]);
    }
    if (lane == 0) {
        positions[i] = i;
        if (!del.live(id)) atomicOr(&deleted[i >> 6], 1ull << (i & 63));
    }
}

// Row c0 + i of the matrix from list i of the chunk: `top` entries wide, idx = position in the sample, in the contract's order.
__global__ __launch_bounds__(MATRIX_ROWS_PER_BLOCK * WAVE) void matrix_finish_kernel(const qmx_scored_point *lists, const uint32_t *counts, uint32_t top,
                                                                                     uint32_t c0, uint32_t n_chunk, const uint32_t *sample_ids,
                                                                                     uint32_t n_sample, uint32_t limit, qmx_scored_point *out,
                                                                                     uint32_t *out_cols, uint32_t *out_counts) {
    const uint32_t i = blockIdx.x * MATRIX_ROWS_PER_BLOCK + threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    if (i >= n_chunk) return;
    const uint32_t p = c0 + i;
    const qmx_scored_point *list = lists + (uint64_t)i * top;
    const uint32_t count = counts[i] < top ? counts[i] : top;
    uint32_t self_at = count;
    for (uint32_t base = 0; base < count; base += WAVE) {
        const uint32_t k = base + lane;
        const uint64_t m = __ballot(k < count && list[k].idx == p);
        if (m) {
            self_at = base + (uint32_t)__builtin_ctzll(m);
            break;
        }
    }
    const uint32_t kept = matrix_clip(count, self_at, limit);
    qmx_scored_point *dst = out + (uint64_t)p * limit;
    uint32_t *cols = out_cols ? out_cols + (uint64_t)p * limit : nullptr;
    for (uint32_t k = lane; k < limit; k += WAVE) {
        qmx_scored_point e{0u, 0.0f};
        uint32_t col = 0;
        if (k < kept) {
            e = list[matrix_src(k, self_at)];
            col = e.idx;
            e.idx = col < n_sample ? sample_ids[col] : 0xFFFFFFFFu;
        }
        dst[k] = e;
        if (cols) cols[k] = col;
    }
    if (lane == 0) out_counts[p] = kept;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------------
uint32_t sample_count_blocks(uint64_t n_words) { return (uint32_t)((n_words + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK); }

int32_t launch_sample_level(hipStream_t st, const DeletedView &del, uint64_t n_words, uint64_t seed, uint32_t level, SampleState *state, uint32_t *hist) {
    // (a block flushes up to 4 096 bins: few blocks, several words per lane)
    const uint64_t want = (n_words + SAMPLE_BLOCK * 4 - 1) / (SAMPLE_BLOCK * 4);
    const uint32_t grid = (uint32_t)(want < 1 ? 1 : want > 512 ? 512 : want);
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sample_hist_kernel, dim3(grid), dim3(SAMPLE_BLOCK), 0, st, del, n_words, seed, level, state, hist);
    QMX_HIP(hipGetLastError());
    hipLaunchKernelGGL(sample_boundary_kernel, dim3(1), dim3(SAMPLE_BLOCK), 0, st, hist, state, level);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_sample_write(hipStream_t st, const DeletedView &del, uint64_t n_words, uint64_t seed, const SampleState *state, uint32_t *block_counts,
                            uint32_t *out, uint32_t cap) {
    const uint32_t blocks = sample_count_blocks(n_words);
    if (blocks == 0 || cap == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sample_count_kernel, dim3(blocks), dim3(SAMPLE_BLOCK), 0, st, del, n_words, seed, state, block_counts);
    QMX_HIP(hipGetLastError());
    hipLaunchKernelGGL(sample_scan_kernel, dim3(1), dim3(SAMPLE_BLOCK), 0, st, block_counts, blocks);
    QMX_HIP(hipGetLastError());
    hipLaunchKernelGGL(sample_write_kernel, dim3(blocks), dim3(SAMPLE_BLOCK), 0, st, del, n_words, seed, state, block_counts, out, cap);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_matrix_gather(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t row_bytes, const uint32_t *ids, uint32_t n, const DeletedView &del,
                             void *block, uint64_t pitch, uint64_t *deleted, uint32_t *positions) {
    if (n == 0) return QMX_OK;
    QMX_REQUIRE(pitch % 16 == 0 && pitch >= row_bytes && ((uintptr_t)block % 16) == 0, QMX_ERR_BAD_ARG, "matrix gather: a block of 16-byte pieces");
    const int src16 = row_stride % 16 == 0 && ((uintptr_t)rows % 16) == 0;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(matrix_gather_kernel, dim3((n + MATRIX_ROWS_PER_BLOCK - 1) / MATRIX_ROWS_PER_BLOCK), dim3(MATRIX_ROWS_PER_BLOCK * WAVE), 0, st,
                       (const char *)rows, row_stride, row_bytes, src16, ids, n, del, (char *)block, pitch, (unsigned long long *)deleted, positions);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_matrix_gather_f16_avx(hipStream_t st, const void *rows, uint64_t row_stride, uint32_t dim, const uint32_t *ids, uint32_t n, const DeletedView &del,
                                     void *block, uint64_t pitch, uint32_t block_dim, uint64_t *deleted, uint32_t *positions) {
    if (n == 0) return QMX_OK;
    QMX_REQUIRE(dim >= 32 && block_dim == matrix_f16_avx_dim(dim), QMX_ERR_BAD_ARG, "matrix gather: %u f16 elements do not make a block row of %u", dim, block_dim);
    QMX_REQUIRE(pitch % 16 == 0 && pitch >= (uint64_t)block_dim * 2 && ((uintptr_t)block % 16) == 0, QMX_ERR_BAD_ARG, "matrix gather: a block of 16-byte pieces");
    QMX_REQUIRE(row_stride % 2 == 0 && ((uintptr_t)rows % 2) == 0, QMX_ERR_NOT_SUPPORTED, "matrix gather: f16 rows at an odd address or stride");
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(matrix_gather_f16_avx_kernel, dim3((n + MATRIX_ROWS_PER_BLOCK - 1) / MATRIX_ROWS_PER_BLOCK), dim3(MATRIX_ROWS_PER_BLOCK * WAVE), 0, st,
                       (const char *)rows, row_stride, dim, ids, n, del, (char *)block, pitch, (unsigned long long *)deleted, positions);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_matrix_finish(hipStream_t st, const qmx_scored_point *lists, const uint32_t *counts, uint32_t top, uint32_t c0, uint32_t n_chunk,
                             const uint32_t *sample_ids, uint32_t n_sample, uint32_t limit, qmx_scored_point *out, uint32_t *out_cols, uint32_t *out_counts) {
    if (n_chunk == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(matrix_finish_kernel, dim3((n_chunk + MATRIX_ROWS_PER_BLOCK - 1) / MATRIX_ROWS_PER_BLOCK), dim3(MATRIX_ROWS_PER_BLOCK * WAVE), 0, st,
                       lists, counts, top, c0, n_chunk, sample_ids, n_sample, limit, out, out_cols, out_counts);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

}  // namespace qmx
