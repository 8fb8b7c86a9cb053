// sparse.hip — sparse vectors (QMX_DTYPE_SPARSE) on the device: the create-time preparation of a segment (row checks, row sort, remap,
// the dimension-major posting layout), the gather scorer of RawScorer (`score_vectors`, lib/sparse/src/common/sparse_vector.rs:66-90)
// the posting-list top-k of Nearest search (the GPU form of `advance_batch`, lib/sparse/src/index/search_context.rs:146-187), and the custom
// queries (recommend / discover / context / feedback) over the same rows and postings (`SparseCustomQueryScorer`).
//
// Every score is the reference's sum: the products of the shared dimensions, each rounded (`__fmul_rn`), added in ascending dimension
// order from 0.0, each add rounded (`__fadd_rn`).  No fused multiply-add, no atomics on scores.
#include "custom_combine.hpp"
#include "kernels.hpp"
#include "dev_mem.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

namespace qmx {

constexpr int SP_BLOCK = 256;
constexpr uint32_t SP_LDS_Q = 4096;           // query entries staged in LDS (32 KiB); longer queries are read from global memory
constexpr uint32_t SPT_SUB = 2048;            // point ids per wave in the posting top-k
constexpr uint32_t SPT_WAVES = SP_BLOCK / WAVE;
constexpr uint32_t SPT_TILE = SPT_SUB * SPT_WAVES;   // ids per work-group: 32 KiB of accumulators + 1 KiB overlap bitmap
constexpr uint32_t SPT_CHUNK = WAVE;          // query dimensions whose posting sub-ranges one wave finds at once (one per lane)

uint32_t sparse_tile_ids() { return SPT_TILE; }

// score_vectors: both lists ascending; *overlap = at least one shared dimension
__device__ __forceinline__ float sparse_dot(const uint32_t *ai, const float *av, uint32_t na, const uint32_t *bi, const float *bv, uint32_t nb,
                                            bool *overlap) {
    float s = 0.0f;
    bool ov = false;
    uint32_t i = 0, j = 0;
    while (i < na && j < nb) {
        const uint32_t x = ai[i], y = bi[j];
        if (x < y) {
            ++i;
        } else if (x > y) {
            ++j;
        } else {
            s = __fadd_rn(s, __fmul_rn(av[i], bv[j]));
            ov = true;
            ++i;
            ++j;
        }
    }
    *overlap = ov;
    return s;
}

// ---- create ----

// flags bit 0: a row is not strictly ascending; bit 1: a row holds an index twice
__global__ void sparse_check_rows_kernel(const uint64_t *offsets, const uint32_t *idx, uint64_t n, uint32_t *flags) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint64_t a = offsets[r], b = offsets[r + 1];
    uint32_t f = 0;
    for (uint64_t i = a + 1; i < b; ++i) {
        const uint32_t x = idx[i - 1], y = idx[i];
        if (x > y) f |= 1u;
        if (x == y) f |= 2u;
    }
    if (f) atomicOr(flags, f);
}

// insertion sort of each unsorted row by index, values along (rows are short: ~100 entries; a row of L entries costs O(L^2) on one thread)
__global__ void sparse_sort_rows_kernel(const uint64_t *offsets, uint32_t *idx, float *val, uint64_t n) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint64_t a = offsets[r], b = offsets[r + 1];
    bool sorted = true;
    for (uint64_t i = a + 1; i < b && sorted; ++i) sorted = idx[i - 1] <= idx[i];
    if (sorted) return;
    for (uint64_t i = a + 1; i < b; ++i) {
        const uint32_t k = idx[i];
        const float v = val[i];
        uint64_t j = i;
        while (j > a && idx[j - 1] > k) {
            idx[j] = idx[j - 1];
            val[j] = val[j - 1];
            --j;
        }
        idx[j] = k;
        val[j] = v;
    }
}

// IndicesTracker::remap_index over every stored index: keys sorted ascending; a key the map lacks sets *missing
__global__ void sparse_remap_kernel(uint32_t *idx, uint64_t nnz, const uint32_t *keys, const uint32_t *vals, uint64_t m, uint32_t *missing) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnz) return;
    const uint32_t k = idx[i];
    uint64_t lo = 0, hi = m;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    if (lo < m && keys[lo] == k) idx[i] = vals[lo];
    else atomicOr(missing, 1u);
}

// posting payload of every entry: (f32 bits of the weight << 32) | row id, in row order (the stable sort by dimension keeps ids ascending)
__global__ void sparse_post_payload_kernel(const uint64_t *offsets, const float *val, uint64_t n, uint64_t *out) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    for (uint64_t i = offsets[r]; i < offsets[r + 1]; ++i) out[i] = ((uint64_t)__float_as_uint(val[i]) << 32) | (uint32_t)r;
}

static uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + SP_BLOCK - 1) / SP_BLOCK); }

int32_t launch_sparse_check_rows(hipStream_t st, const uint64_t *offsets, const uint32_t *idx, uint64_t n, uint32_t *flags) {
    if (n == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sparse_check_rows_kernel, dim3(blocks_of(n)), dim3(SP_BLOCK), 0, st, offsets, idx, n, flags);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_sparse_sort_rows(hipStream_t st, const uint64_t *offsets, uint32_t *idx, float *val, uint64_t n) {
    if (n == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sparse_sort_rows_kernel, dim3(blocks_of(n)), dim3(SP_BLOCK), 0, st, offsets, idx, val, n);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_sparse_remap(hipStream_t st, uint32_t *idx, uint64_t nnz, const uint32_t *keys, const uint32_t *vals, uint64_t m, uint32_t *missing) {
    if (nnz == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sparse_remap_kernel, dim3(blocks_of(nnz)), dim3(SP_BLOCK), 0, st, idx, nnz, keys, vals, m, missing);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

// The dimension-major layout: post[] = the (id, weight) payloads grouped by dimension, ids ascending inside a group; dims[] / counts[] = the
// distinct dimensions ascending and their posting lengths, *n_dims of them.  Stable radix sort of the payloads by dimension, then a run-length
// encoding of the sorted dimensions.  Scratch is allocated and freed here.
int32_t sparse_build_postings(hipStream_t st, const uint64_t *offsets, const uint32_t *idx, const float *val, uint64_t n, uint64_t nnz, uint64_t *post,
                              uint32_t *dims, uint32_t *counts, uint32_t *n_dims_dev) {
    if (nnz == 0) {
        QMX_HIP(hipMemsetAsync(n_dims_dev, 0, 4, st));
        return QMX_OK;
    }
    QMX_REQUIRE(nnz <= 0xFFFFFFFFull, QMX_ERR_NOT_SUPPORTED, "a sparse segment holds at most 2^32 - 1 non-zeros (got %llu)", (unsigned long long)nnz);
    DevBuf b_payload, b_keys, tmp;
    QMX_TRY(b_payload.reserve(nnz * 8));
    QMX_TRY(b_keys.reserve(nnz * 4));
    uint64_t *payload = (uint64_t *)b_payload.p;
    uint32_t *keys_sorted = (uint32_t *)b_keys.p;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sparse_post_payload_kernel, dim3(blocks_of(n)), dim3(SP_BLOCK), 0, st, offsets, val, n, payload);
    QMX_HIP(hipGetLastError());
    size_t sort_bytes = 0, rle_bytes = 0;
    QMX_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, idx, keys_sorted, payload, post, (size_t)nnz, 0, 32, st));
    QMX_HIP(rocprim::run_length_encode(nullptr, rle_bytes, keys_sorted, (unsigned int)nnz, dims, counts, n_dims_dev, st));
    QMX_TRY(tmp.reserve(std::max(sort_bytes, rle_bytes)));
    QMX_HIP(rocprim::radix_sort_pairs(tmp.p, sort_bytes, idx, keys_sorted, payload, post, (size_t)nnz, 0, 32, st));
    QMX_HIP(rocprim::run_length_encode(tmp.p, rle_bytes, keys_sorted, (unsigned int)nnz, dims, counts, n_dims_dev, st));
    QMX_HIP(hipStreamSynchronize(st));
    return QMX_OK;
}

// ---- gather scoring (RawScorer) ----

// scores[(q - q0) * stride + i] = score_vectors(query q, row ids[i]) (0.0 without overlap); block (x, y) = a slice of the ids for query q0 + y,
// whose sorted list is staged in LDS
__global__ __launch_bounds__(SP_BLOCK) void sparse_score_matrix_kernel(SparseRows r, SparseQueries qs, uint32_t q0, const uint32_t *ids, uint64_t n,
                                                                       float *scores, uint64_t stride, int *err) {
    __shared__ uint32_t s_idx[SP_LDS_Q];
    __shared__ float s_val[SP_LDS_Q];
    const uint32_t qi = q0 + blockIdx.y;
    const uint64_t qo = qs.off[qi];
    const uint32_t qn = (uint32_t)(qs.off[qi + 1] - qo);
    const bool staged = qn <= SP_LDS_Q;
    if (staged)
        for (uint32_t k = threadIdx.x; k < qn; k += SP_BLOCK) {
            s_idx[k] = qs.idx[qo + k];
            s_val[k] = qs.val[qo + k];
        }
    __syncthreads();
    const uint32_t *qidx = staged ? s_idx : qs.idx + qo;
    const float *qval = staged ? s_val : qs.val + qo;
    for (uint64_t i = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SP_BLOCK) {
        const uint32_t id = ids ? ids[i] : (uint32_t)i;
        float s = 0.0f;
        if (id >= r.n) {
            *err = 1;
        } else {
            bool ov;
            const uint64_t ro = r.off[id];
            s = sparse_dot(r.idx + ro, r.val + ro, (uint32_t)(r.off[id + 1] - ro), qidx, qval, qn, &ov);
        }
        scores[(uint64_t)blockIdx.y * stride + i] = s;
    }
}

// one (query, row) item per thread: ragged score_points, rescoring
__global__ __launch_bounds__(SP_BLOCK) void sparse_score_pairs_kernel(SparseRows r, SparseQueries qs, PairSel sel, const uint32_t *ids, uint64_t n_items,
                                                                      float *scores, int *err) {
    const uint64_t i = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= n_items) return;
    const uint32_t qi = sel.query_of(i);
    if (!sel.live(i, qi)) {
        scores[i] = 0.0f;
        return;
    }
    const uint32_t id = ids[i];
    float s = 0.0f;
    if (id >= r.n) {
        *err = 1;
    } else {
        bool ov;
        const uint64_t ro = r.off[id], qo = qs.off[qi];
        s = sparse_dot(r.idx + ro, r.val + ro, (uint32_t)(r.off[id + 1] - ro), qs.idx + qo, qs.val + qo, (uint32_t)(qs.off[qi + 1] - qo), &ov);
    }
    scores[i] = s;
}

// score_internal: pair i = (stored row a[i], stored row b[i])
__global__ __launch_bounds__(SP_BLOCK) void sparse_score_internal_kernel(SparseRows r, const uint32_t *a, const uint32_t *b, uint64_t n, float *out, int *err) {
    const uint64_t i = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = a[i], y = b[i];
    float s = 0.0f;
    if (x >= r.n || y >= r.n) {
        *err = 1;
    } else {
        bool ov;
        const uint64_t xo = r.off[x], yo = r.off[y];
        s = sparse_dot(r.idx + xo, r.val + xo, (uint32_t)(r.off[x + 1] - xo), r.idx + yo, r.val + yo, (uint32_t)(r.off[y + 1] - yo), &ov);
    }
    out[i] = s;
}

int32_t launch_sparse_score_matrix(hipStream_t st, const SparseRows &r, const SparseQueries &qs, uint32_t q0, uint32_t nq, const uint32_t *ids, uint64_t n,
                                   float *scores, uint64_t stride, int *err) {
    if (n == 0 || nq == 0) return QMX_OK;
    const uint32_t gx = (uint32_t)std::min<uint64_t>(blocks_of(n), 4096);
    ::qmx::clear_stale_error();
    for (uint32_t y0 = 0; y0 < nq; y0 += 65535) {
        const uint32_t ny = std::min<uint32_t>(65535, nq - y0);
        hipLaunchKernelGGL(sparse_score_matrix_kernel, dim3(gx, ny), dim3(SP_BLOCK), 0, st, r, qs, q0 + y0, ids, n, scores + (uint64_t)y0 * stride, stride, err);
        QMX_NOTE_KERNEL(sparse_score_matrix_kernel);
    }
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_sparse_score_pairs(hipStream_t st, const SparseRows &r, const SparseQueries &qs, const PairSel &sel, const uint32_t *ids, uint64_t n_items,
                                  float *scores, int *err) {
    if (n_items == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sparse_score_pairs_kernel, dim3(blocks_of(n_items)), dim3(SP_BLOCK), 0, st, r, qs, sel, ids, n_items, scores, err);
    QMX_NOTE_KERNEL(sparse_score_pairs_kernel);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_sparse_score_internal(hipStream_t st, const SparseRows &r, const uint32_t *a, const uint32_t *b, uint64_t n, float *out, int *err) {
    if (n == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sparse_score_internal_kernel, dim3(blocks_of(n)), dim3(SP_BLOCK), 0, st, r, a, b, n, out, err);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
// ---- top-k ----

// the work-group's end of a pass: the four wave lists merged into the best `top` keys, written as list `list` of query ql
__device__ __forceinline__ void sparse_block_emit(uint64_t list, int top, uint32_t list_idx, uint32_t ql, uint32_t nq_tile, uint64_t *partial) {
    __shared__ uint64_t sh[SPT_WAVES][WAVE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    sh[wave][lane] = list;
    __syncthreads();
    if (wave == 0) {
        uint64_t merged = sh[0][lane];
        for (uint32_t w = 1; w < SPT_WAVES; ++w) wave_offer(merged, sh[w][lane], top, lane);
        if (lane < top) partial[((uint64_t)list_idx * nq_tile + ql) * top + lane] = merged;
    }
}

// The posting walk of one wave over one chunk of a plan: entries c .. c + nc (nc <= SPT_CHUNK) of `plan`, in that order.  The lanes first find the
// posting sub-range of their entry's dimension (one binary search per lane), then the wave adds weight x query weight of each dimension's entries that
// fall into [sub_lo, sub_hi) into the accumulators wacc[id - sub_lo], 64 entries per step; HIT: the overlap bit of every touched id is set in whit.
// Ids are distinct inside one posting list and a wave's LDS operations complete in order, so every accumulator sees the plan's dimensions one after
// the other.
template <bool HIT>
__device__ __forceinline__ void sparse_walk_chunk(const uint64_t *post, const SparsePlan &plan, uint32_t c, uint32_t nc, uint64_t sub_lo, uint64_t sub_hi,
                                                  float *wacc, uint32_t *whit, int lane) {
    uint64_t lo = 0, hi = 0;
    float w = 0.0f;
    if ((uint32_t)lane < nc) {   // lower_bound(sub_lo) in the dimension's posting list
        uint64_t a = plan.start[c + lane], b = plan.end[c + lane];
        hi = b;
        w = plan.w[c + lane];
        while (a < b) {
            const uint64_t m = (a + b) >> 1;
            if ((uint32_t)post[m] < sub_lo) a = m + 1;
            else b = m;
        }
        lo = a;
    }
    for (uint32_t j = 0; j < nc; ++j) {
        uint64_t p = readlane_u64(lo, (int)j);
        const uint64_t e = readlane_u64(hi, (int)j);
        const float qv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), (int)j));
        while (p < e) {
            const uint64_t i = p + lane;
            uint64_t ent = ~0ull;
            if (i < e) ent = post[i];
            const uint32_t id = (uint32_t)ent;
            const bool in = i < e && id < sub_hi;
            if (in) {
                const uint32_t k = id - (uint32_t)sub_lo;
                wacc[k] = __fadd_rn(wacc[k], __fmul_rn(__uint_as_float((uint32_t)(ent >> 32)), qv));
                if (HIT) atomicOr(&whit[k >> 5], 1u << (k & 31));
            }
            if (__ballot(in) != ~0ull) break;
            p += WAVE;
        }
    }
}

// Nearest over the posting layout.  Work-group (x, y): point ids [x * SPT_TILE, (x + 1) * SPT_TILE) for query q0 + y; wave w owns the
// SPT_SUB ids from x * SPT_TILE + w * SPT_SUB with its accumulators and overlap bits in LDS.  The query's dimensions are visited in ascending
// order; for each, the lanes of the wave first find the posting sub-range of their dimension (64 dimensions at a time, one binary search per
// lane), then the wave adds weight x query weight of the dimension's entries into the accumulators, 64 entries per step.  Ids are distinct inside
// one posting list and a wave's LDS operations complete in order, so every point's sum is score_vectors' sum, dimension after dimension.
// Then each wave offers its overlapping, live, allowed ids (below the bound of the previous pass) to a list of `top`, and the work-group
// writes the best `top` of its four lists as one key list of launch_merge_keys.
__global__ __launch_bounds__(SP_BLOCK) void sparse_topk_postings_kernel(const uint64_t *post, SparsePlan plan, uint32_t q0, uint32_t nq_tile, uint64_t n_scan,
                                                                        DeletedView del, uint32_t top, const uint64_t *key_bound, uint64_t *partial) {
    __shared__ float acc[SPT_TILE];
    __shared__ uint32_t hit[SPT_TILE / 32];
    const uint32_t tile = blockIdx.x, ql = blockIdx.y, qi = q0 + ql;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t bound = key_bound ? key_bound[ql] : 0;
    if (key_bound && bound == 0) {   // the query was exhausted by an earlier pass
        if (threadIdx.x < top) partial[((uint64_t)tile * nq_tile + ql) * top + threadIdx.x] = 0;
        return;
    }
    const uint64_t sub_lo = (uint64_t)tile * SPT_TILE + (uint64_t)wave * SPT_SUB;
    const uint64_t sub_hi = sub_lo + SPT_SUB < n_scan ? sub_lo + SPT_SUB : n_scan;
    float *wacc = acc + wave * SPT_SUB;
    uint32_t *whit = hit + wave * (SPT_SUB / 32);
    for (uint32_t k = lane; k < SPT_SUB; k += WAVE) wacc[k] = 0.0f;
    for (uint32_t k = lane; k < SPT_SUB / 32; k += WAVE) whit[k] = 0u;
    const uint32_t d0 = plan.off[qi], d1 = plan.off[qi + 1];
    for (uint32_t c = d0; c < d1 && sub_lo < sub_hi; c += SPT_CHUNK)
        sparse_walk_chunk<true>(post, plan, c, d1 - c < SPT_CHUNK ? d1 - c : SPT_CHUNK, sub_lo, sub_hi, wacc, whit, lane);
    uint64_t list = 0;
    for (uint32_t k0 = 0; k0 < SPT_SUB; k0 += WAVE) {
        const uint32_t k = k0 + lane;
        const uint64_t id = sub_lo + k;
        uint64_t key = 0;
        if (id < sub_hi && ((whit[k >> 5] >> (k & 31)) & 1u) && del.live((uint32_t)id)) key = make_key(wacc[k], (uint32_t)id);
        if (key_bound && key >= bound) key = 0;
        wave_offer(list, key, (int)top, lane);
    }
    sparse_block_emit(list, (int)top, tile, ql, nq_tile, partial);
}

// plain_search over an id list: block (x, y) scores a grid-strided slice of the ids against query q0 + y (staged in LDS) and keeps the
// overlapping, live, allowed ones
__global__ __launch_bounds__(SP_BLOCK) void sparse_topk_ids_kernel(SparseRows r, SparseQueries qs, uint32_t q0, uint32_t nq_tile, const uint32_t *ids,
                                                                   uint64_t n_ids, DeletedView del, uint32_t top, const uint64_t *key_bound, uint64_t *partial) {
    __shared__ uint32_t s_idx[SP_LDS_Q];
    __shared__ float s_val[SP_LDS_Q];
    const uint32_t ql = blockIdx.y, qi = q0 + ql;
    const int lane = threadIdx.x & 63;
    const uint64_t bound = key_bound ? key_bound[ql] : 0;
    if (key_bound && bound == 0) {
        if (threadIdx.x < top) partial[((uint64_t)blockIdx.x * nq_tile + ql) * top + threadIdx.x] = 0;
        return;
    }
    const uint64_t qo = qs.off[qi];
    const uint32_t qn = (uint32_t)(qs.off[qi + 1] - qo);
    const bool staged = qn <= SP_LDS_Q;
    if (staged)
        for (uint32_t k = threadIdx.x; k < qn; k += SP_BLOCK) {
            s_idx[k] = qs.idx[qo + k];
            s_val[k] = qs.val[qo + k];
        }
    __syncthreads();
    const uint32_t *qidx = staged ? s_idx : qs.idx + qo;
    const float *qval = staged ? s_val : qs.val + qo;
    uint64_t list = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * SP_BLOCK; base < n_ids; base += (uint64_t)gridDim.x * SP_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        uint64_t key = 0;
        if (i < n_ids) {
            const uint32_t id = ids[i];
            if (id < r.n && del.live(id)) {
                bool ov;
                const uint64_t ro = r.off[id];
                const float s = sparse_dot(r.idx + ro, r.val + ro, (uint32_t)(r.off[id + 1] - ro), qidx, qval, qn, &ov);
                if (ov) key = make_key(s, id);
            }
        }
        if (key_bound && key >= bound) key = 0;
        wave_offer(list, key, (int)top, lane);
    }
    sparse_block_emit(list, (int)top, blockIdx.x, ql, nq_tile, partial);
}

// ---- custom queries (SparseCustomQueryScorer, lib/segment/src/vector_storage/query_scorer/sparse_custom_query_scorer.rs) ----
// score(point) = query.score_by(|example| score_vectors(example, point).unwrap_or(0.0)): every live candidate has a score, overlap or not.  The
// scorer works on the vector STORAGE, not on the index: each example's sum runs in ascending ORIGINAL index order, whatever the IndicesTracker
// made of the ids.  The example batch therefore carries its lists and its posting plan a second time in that order (SparseQueries / SparsePlan
// handed to the kernels below are those).

// score_vectors of an example with a stored row, the example's dimensions in the order its list has them: `ei` holds the remapped ids, the row is
// sorted by remapped id, so each example dimension is looked up by binary search.  The sum starts at +0.0 and is never assigned: it cannot be -0.0.
__device__ __forceinline__ float sparse_dot_lookup(const uint32_t *ri, const float *rv, uint32_t rn, const uint32_t *ei, const float *ev, uint32_t en) {
    float s = 0.0f;
    for (uint32_t k = 0; k < en; ++k) {
        const uint32_t d = ei[k];
        uint32_t a = 0, b = rn;
        while (a < b) {
            const uint32_t m = (a + b) >> 1;
            if (ri[m] < d) a = m + 1;
            else b = m;
        }
        if (a < rn && ri[a] == d) s = __fadd_rn(s, __fmul_rn(rv[a], ev[k]));
    }
    return s;
}

// one custom query against one stored row (id < r.n)
__device__ __forceinline__ float sparse_custom_score(const SparseRows &r, const SparseQueries &ex, const qmx_custom_query &cq, const float *coefs, uint32_t id) {
    const uint64_t ro = r.off[id];
    const uint32_t rn = (uint32_t)(r.off[id + 1] - ro);
    return custom_score_by(cq.kind, cq.n_a, cq.n_b, coefs + cq.coef_first, [&](uint32_t e) {
        const uint64_t eo = ex.off[cq.first + e];
        return sparse_dot_lookup(r.idx + ro, r.val + ro, rn, ex.idx + eo, ex.val + eo, (uint32_t)(ex.off[cq.first + e + 1] - eo));
    });
}

// RawScorer::score_points: scores[qi * n + i] = custom query qi against row ids[i]; one thread per (query, id)
__global__ __launch_bounds__(SP_BLOCK) void sparse_custom_score_kernel(SparseRows r, SparseQueries ex, const qmx_custom_query *desc, const float *coefs,
                                                                       const uint32_t *ids, uint64_t n, float *scores, int *err) {
    const uint64_t i = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t qi = blockIdx.y, id = ids[i];
    float s = 0.0f;
    if (id >= r.n) *err = 1;
    else s = sparse_custom_score(r, ex, desc[qi], coefs, id);
    scores[(uint64_t)qi * n + i] = s;
}

// search_scored over an id list: block (x, y) scores a grid-strided slice of the ids against custom query q0 + y and keeps the live, allowed ones.
// ids == nullptr: the identity list (id = i), nothing materialised - the full scan of a segment whose postings hold no f32 weights
__global__ __launch_bounds__(SP_BLOCK) void sparse_custom_topk_ids_kernel(SparseRows r, SparseQueries ex, const qmx_custom_query *desc, const float *coefs,
                                                                          uint32_t q0, uint32_t nq_tile, const uint32_t *ids, uint64_t n_ids, DeletedView del,
                                                                          uint32_t top, const uint64_t *key_bound, uint64_t *partial) {
    const uint32_t ql = blockIdx.y, qi = q0 + ql;
    const int lane = threadIdx.x & 63;
    const uint64_t bound = key_bound ? key_bound[ql] : 0;
    if (key_bound && bound == 0) {
        if (threadIdx.x < top) partial[((uint64_t)blockIdx.x * nq_tile + ql) * top + threadIdx.x] = 0;
        return;
    }
    const qmx_custom_query cq = desc[qi];
    uint64_t list = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * SP_BLOCK; base < n_ids; base += (uint64_t)gridDim.x * SP_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        uint64_t key = 0;
        if (i < n_ids) {
            const uint32_t id = ids ? ids[i] : (uint32_t)i;
            if (id < r.n && del.live(id)) key = make_key(sparse_custom_score(r, ex, cq, coefs, id), id);
        }
        if (key_bound && key >= bound) key = 0;
        wave_offer(list, key, (int)top, lane);
    }
    sparse_block_emit(list, (int)top, blockIdx.x, ql, nq_tile, partial);
}

// search_scored over every point, fused on the posting layout.  Work-group (x, y) and its waves own point ids as in sparse_topk_postings_kernel
// (SPC_SUB ids per wave).  For each example of custom query q0 + y, in flat_iter() order: the wave zeroes its accumulators, walks the example's
// posting plan (sparse_walk_chunk: the similarity of the example with every point of the sub-range), and folds the finished similarities into the
// points' score_by states (custom_step).  Lane l folds the points l, l + 64, ... of the sub-range - a static mapping, so the SPC_SUB / 64 states of
// a lane stay in registers through fully unrolled loops and the LDS holds the accumulators only.  After the last example the scores are finished,
// and every live, allowed point (no overlap needed) below the pass's bound is offered to the wave's key list.
constexpr uint32_t SPC_SUB = 1024;                        // point ids per wave: half the Nearest kernel's (measured: DESIGN 3.9)
constexpr uint32_t SPC_TILE = SPC_SUB * SPT_WAVES;        // ids per work-group: 16 KiB of accumulators
constexpr uint32_t SPC_LANE_IDS = SPC_SUB / WAVE;
uint32_t sparse_custom_tile_ids() { return SPC_TILE; }
__global__ __launch_bounds__(SP_BLOCK) void sparse_custom_topk_postings_kernel(const uint64_t *post, SparsePlan plan, const qmx_custom_query *desc,
                                                                               const float *coefs, uint32_t q0, uint32_t nq_tile, uint64_t n_scan,
                                                                               DeletedView del, uint32_t top, const uint64_t *key_bound, uint64_t *partial) {
    __shared__ float acc[SPC_TILE];
    const uint32_t tile = blockIdx.x, ql = blockIdx.y, qi = q0 + ql;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t bound = key_bound ? key_bound[ql] : 0;
    if (key_bound && bound == 0) {   // the query was exhausted by an earlier pass
        if (threadIdx.x < top) partial[((uint64_t)tile * nq_tile + ql) * top + threadIdx.x] = 0;
        return;
    }
    const uint64_t sub_lo = (uint64_t)tile * SPC_TILE + (uint64_t)wave * SPC_SUB;
    const uint64_t sub_hi = sub_lo + SPC_SUB < n_scan ? sub_lo + SPC_SUB : n_scan;
    float *wacc = acc + wave * SPC_SUB;
    const qmx_custom_query cq = desc[qi];
    const float *cf = coefs + cq.coef_first;
    const uint32_t ne = custom_examples(cq.kind, cq.n_a, cq.n_b);
    CustomState st[SPC_LANE_IDS];
#pragma unroll
    for (uint32_t u = 0; u < SPC_LANE_IDS; ++u) st[u] = custom_init(cq.kind);
    for (uint32_t e = 0; e < ne && sub_lo < sub_hi; ++e) {
#pragma unroll
        for (uint32_t u = 0; u < SPC_LANE_IDS; ++u) wacc[u * WAVE + lane] = 0.0f;
        const uint32_t d0 = plan.off[cq.first + e], d1 = plan.off[cq.first + e + 1];
        for (uint32_t c = d0; c < d1; c += SPT_CHUNK)
            sparse_walk_chunk<false>(post, plan, c, d1 - c < SPT_CHUNK ? d1 - c : SPT_CHUNK, sub_lo, sub_hi, wacc, nullptr, lane);
#pragma unroll
        for (uint32_t u = 0; u < SPC_LANE_IDS; ++u) custom_step(cq.kind, cq.n_a, cf, st[u], e, wacc[u * WAVE + lane]);
    }
#pragma unroll
    for (uint32_t u = 0; u < SPC_LANE_IDS; ++u) wacc[u * WAVE + lane] = custom_finish(cq.kind, st[u]);
    uint64_t list = 0;
    for (uint32_t k0 = 0; k0 < SPC_SUB; k0 += WAVE) {
        const uint32_t k = k0 + lane;
        const uint64_t id = sub_lo + k;
        uint64_t key = 0;
        if (id < sub_hi && del.live((uint32_t)id)) key = make_key(wacc[k], (uint32_t)id);
        if (key_bound && key >= bound) key = 0;
        wave_offer(list, key, (int)top, lane);
    }
    sparse_block_emit(list, (int)top, tile, ql, nq_tile, partial);
}

int32_t launch_sparse_topk_postings(hipStream_t st, const uint64_t *post, const SparsePlan &plan, uint32_t q0, uint32_t nq_tile, uint64_t n_scan,
                                    const DeletedView &del, uint32_t top, const uint64_t *key_bound, uint64_t *partial, uint32_t *n_lists) {
    const uint64_t tiles = (n_scan + SPT_TILE - 1) / SPT_TILE;
    *n_lists = (uint32_t)tiles;
    if (tiles == 0 || nq_tile == 0) return QMX_OK;
    QMX_REQUIRE(nq_tile <= 65535, QMX_ERR_OTHER, "query tile too large");
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sparse_topk_postings_kernel, dim3((uint32_t)tiles, nq_tile), dim3(SP_BLOCK), 0, st, post, plan, q0, nq_tile, n_scan, del, top, key_bound,
                       partial);
    QMX_NOTE_KERNEL(sparse_topk_postings_kernel);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
uint32_t sparse_ids_lists(uint64_t n_ids) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n_ids + SP_BLOCK - 1) / SP_BLOCK, 1), 1024); }
int32_t launch_sparse_topk_ids(hipStream_t st, const SparseRows &r, const SparseQueries &qs, uint32_t q0, uint32_t nq_tile, const uint32_t *ids, uint64_t n_ids,
                               const DeletedView &del, uint32_t top, const uint64_t *key_bound, uint64_t *partial, uint32_t *n_lists) {
    *n_lists = sparse_ids_lists(n_ids);
    if (nq_tile == 0) return QMX_OK;
    QMX_REQUIRE(nq_tile <= 65535, QMX_ERR_OTHER, "query tile too large");
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sparse_topk_ids_kernel, dim3(*n_lists, nq_tile), dim3(SP_BLOCK), 0, st, r, qs, q0, nq_tile, ids, n_ids, del, top, key_bound, partial);
    QMX_NOTE_KERNEL(sparse_topk_ids_kernel);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_sparse_custom_score(hipStream_t st, const SparseRows &r, const SparseQueries &ex, const qmx_custom_query *desc, const float *coefs, uint32_t nq,
                                   const uint32_t *ids, uint64_t n, float *scores, int *err) {
    if (n == 0 || nq == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    for (uint32_t y0 = 0; y0 < nq; y0 += 65535) {
        const uint32_t ny = std::min<uint32_t>(65535, nq - y0);
        hipLaunchKernelGGL(sparse_custom_score_kernel, dim3(blocks_of(n), ny), dim3(SP_BLOCK), 0, st, r, ex, desc + y0, coefs, ids, n, scores + (uint64_t)y0 * n, err);
        QMX_NOTE_KERNEL(sparse_custom_score_kernel);
    }
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_sparse_custom_topk_postings(hipStream_t st, const uint64_t *post, const SparsePlan &plan, const qmx_custom_query *desc, const float *coefs,
                                           uint32_t q0, uint32_t nq_tile, uint64_t n_scan, const DeletedView &del, uint32_t top, const uint64_t *key_bound,
                                           uint64_t *partial, uint32_t *n_lists) {
    const uint64_t tiles = (n_scan + SPC_TILE - 1) / SPC_TILE;
    *n_lists = (uint32_t)tiles;
    if (tiles == 0 || nq_tile == 0) return QMX_OK;
    QMX_REQUIRE(nq_tile <= 65535, QMX_ERR_OTHER, "query tile too large");
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sparse_custom_topk_postings_kernel, dim3((uint32_t)tiles, nq_tile), dim3(SP_BLOCK), 0, st, post, plan, desc, coefs, q0, nq_tile, n_scan, del,
                       top, key_bound, partial);
    QMX_NOTE_KERNEL(sparse_custom_topk_postings_kernel);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_sparse_custom_topk_ids(hipStream_t st, const SparseRows &r, const SparseQueries &ex, const qmx_custom_query *desc, const float *coefs, uint32_t q0,
                                      uint32_t nq_tile, const uint32_t *ids, uint64_t n_ids, const DeletedView &del, uint32_t top, const uint64_t *key_bound,
                                      uint64_t *partial, uint32_t *n_lists) {
    *n_lists = sparse_ids_lists(n_ids);
    if (nq_tile == 0) return QMX_OK;
    QMX_REQUIRE(nq_tile <= 65535, QMX_ERR_OTHER, "query tile too large");
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sparse_custom_topk_ids_kernel, dim3(*n_lists, nq_tile), dim3(SP_BLOCK), 0, st, r, ex, desc, coefs, q0, nq_tile, ids, n_ids, del, top, key_bound,
                       partial);
    QMX_NOTE_KERNEL(sparse_custom_topk_ids_kernel);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

// ---- f16 / u8 index weights (SparseIndexConfig.datatype; lib/sparse/src/common/types.rs, compressed_posting_list.rs:361-407) ----
// The posting layout as a structure of arrays: post_id[nnz] and post_w[nnz] (u16 = the bits of half::f16, or u8 = QuantizedU8 with (min, diff256)
// per posting list).  The f32 kernels above are left as they are; the kernels below are their counterparts over the two arrays and score the
// DECODED weight, as SearchContext does over a CompressedPostingList<W>.

// Weight::to_f32: exact widening of f16; min + f32(code) * diff256 with the multiply and the add rounded separately
template <typename W>
__device__ __forceinline__ float sparse_decode(W c, float mn, float d256);
template <>
__device__ __forceinline__ float sparse_decode<uint16_t>(uint16_t c, float, float) { return __half2float(__ushort_as_half(c)); }
template <>
__device__ __forceinline__ float sparse_decode<uint8_t>(uint8_t c, float mn, float d256) { return __fadd_rn(mn, __fmul_rn((float)c, d256)); }

// Weight::from_f32: f16 rounds to nearest even and overflows to inf; u8 = ((v - min) / diff256).round().clamp(0, 255) as u8 - IEEE division, round
// half away from zero, NaN (0 / 0 of a list whose weights are all equal) becomes 0
template <typename W>
__device__ __forceinline__ W sparse_encode(float v, float mn, float d256);
template <>
__device__ __forceinline__ uint16_t sparse_encode<uint16_t>(float v, float, float) { return __half_as_ushort(__float2half_rn(v)); }
template <>
__device__ __forceinline__ uint8_t sparse_encode<uint8_t>(float v, float mn, float d256) {
    const float r = roundf(__fdiv_rn(__fsub_rn(v, mn), d256));
    return r >= 255.0f ? (uint8_t)255 : r > 0.0f ? (uint8_t)r : (uint8_t)0;      // (every comparison with NaN is false: 0)
}

// QuantizedU8::quantization_params_for of every posting list: work-group d (grid-strided) reduces the weights of dimension d
__global__ __launch_bounds__(SP_BLOCK) void sparse_post_params_kernel(const uint64_t *post, const uint64_t *dir_start, uint32_t n_dims, float *mn, float *d256) {
    __shared__ float s_lo[SP_BLOCK], s_hi[SP_BLOCK];
    for (uint32_t d = blockIdx.x; d < n_dims; d += gridDim.x) {
        const uint64_t a = dir_start[d], b = dir_start[d + 1];
        float lo = INFINITY, hi = -INFINITY;
        for (uint64_t i = a + threadIdx.x; i < b; i += SP_BLOCK) {
            const float v = __uint_as_float((uint32_t)(post[i] >> 32));
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
        s_lo[threadIdx.x] = lo;
        s_hi[threadIdx.x] = hi;
        __syncthreads();
        for (uint32_t s = SP_BLOCK / 2; s > 0; s >>= 1) {
            if (threadIdx.x < s) {
                s_lo[threadIdx.x] = fminf(s_lo[threadIdx.x], s_lo[threadIdx.x + s]);
                s_hi[threadIdx.x] = fmaxf(s_hi[threadIdx.x], s_hi[threadIdx.x + s]);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            mn[d] = s_lo[0];
            d256[d] = __fdiv_rn(__fsub_rn(s_hi[0], s_lo[0]), 255.0f);
        }
        __syncthreads();
    }
}

// the packed layout into the two arrays; work-group d (grid-strided) encodes the posting list of dimension d with its parameters
template <typename W>
__global__ __launch_bounds__(SP_BLOCK) void sparse_post_encode_kernel(const uint64_t *post, const uint64_t *dir_start, uint32_t n_dims, const float *mn,
                                                                      const float *d256, uint32_t *post_id, W *post_w) {
    for (uint32_t d = blockIdx.x; d < n_dims; d += gridDim.x) {
        const uint64_t a = dir_start[d], b = dir_start[d + 1];
        const float lo = mn ? mn[d] : 0.0f, dd = d256 ? d256[d] : 0.0f;
        for (uint64_t i = a + threadIdx.x; i < b; i += SP_BLOCK) {
            const uint64_t ent = post[i];
            post_id[i] = (uint32_t)ent;
            post_w[i] = sparse_encode<W>(__uint_as_float((uint32_t)(ent >> 32)), lo, dd);
        }
    }
}

// sparse_walk_chunk over the two arrays: the binary search runs over post_id, id and code come from their arrays, and the u8 parameters of a plan
// entry are broadcast with its query weight
template <typename W>
__device__ __forceinline__ void sparse_walk_chunk_q(const uint32_t *pid, const W *pw, const SparsePlanQ &plan, uint32_t c, uint32_t nc, uint64_t sub_lo,
                                                    uint64_t sub_hi, float *wacc, uint32_t *whit, int lane) {
    uint64_t lo = 0, hi = 0;
    float w = 0.0f, mn = 0.0f, dd = 0.0f;
    if ((uint32_t)lane < nc) {   // lower_bound(sub_lo) in the dimension's posting list
        uint64_t a = plan.start[c + lane], b = plan.end[c + lane];
        hi = b;
        w = plan.w[c + lane];
        if (sizeof(W) == 1) {
            mn = plan.mn[c + lane];
            dd = plan.d256[c + lane];
        }
        while (a < b) {
            const uint64_t m = (a + b) >> 1;
            if (pid[m] < sub_lo) a = m + 1;
            else b = m;
        }
        lo = a;
    }
    for (uint32_t j = 0; j < nc; ++j) {
        uint64_t p = readlane_u64(lo, (int)j);
        const uint64_t e = readlane_u64(hi, (int)j);
        const float qv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), (int)j));
        const float qmn = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mn), (int)j));
        const float qdd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dd), (int)j));
        while (p < e) {
            const uint64_t i = p + lane;
            uint32_t id = ~0u;
            W code = 0;
            if (i < e) {
                id = pid[i];
                code = pw[i];
            }
            const bool in = i < e && id < sub_hi;
            if (in) {
                const uint32_t k = id - (uint32_t)sub_lo;
                wacc[k] = __fadd_rn(wacc[k], __fmul_rn(sparse_decode<W>(code, qmn, qdd), qv));
                atomicOr(&whit[k >> 5], 1u << (k & 31));
            }
            if (__ballot(in) != ~0ull) break;
            p += WAVE;
        }
    }
}

// sparse_topk_postings_kernel over the two arrays: tiles, LDS, emit and merge are the f32 kernel's
template <typename W>
__global__ __launch_bounds__(SP_BLOCK) void sparse_topk_postings_q_kernel(const uint32_t *pid, const W *pw, SparsePlanQ plan, uint32_t q0, uint32_t nq_tile,
                                                                          uint64_t n_scan, DeletedView del, uint32_t top, const uint64_t *key_bound,
                                                                          uint64_t *partial) {
    __shared__ float acc[SPT_TILE];
    __shared__ uint32_t hit[SPT_TILE / 32];
    const uint32_t tile = blockIdx.x, ql = blockIdx.y, qi = q0 + ql;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t bound = key_bound ? key_bound[ql] : 0;
    if (key_bound && bound == 0) {   // the query was exhausted by an earlier pass
        if (threadIdx.x < top) partial[((uint64_t)tile * nq_tile + ql) * top + threadIdx.x] = 0;
        return;
    }
    const uint64_t sub_lo = (uint64_t)tile * SPT_TILE + (uint64_t)wave * SPT_SUB;
    const uint64_t sub_hi = sub_lo + SPT_SUB < n_scan ? sub_lo + SPT_SUB : n_scan;
    float *wacc = acc + wave * SPT_SUB;
    uint32_t *whit = hit + wave * (SPT_SUB / 32);
    for (uint32_t k = lane; k < SPT_SUB; k += WAVE) wacc[k] = 0.0f;
    for (uint32_t k = lane; k < SPT_SUB / 32; k += WAVE) whit[k] = 0u;
    const uint32_t d0 = plan.off[qi], d1 = plan.off[qi + 1];
    for (uint32_t c = d0; c < d1 && sub_lo < sub_hi; c += SPT_CHUNK)
        sparse_walk_chunk_q<W>(pid, pw, plan, c, d1 - c < SPT_CHUNK ? d1 - c : SPT_CHUNK, sub_lo, sub_hi, wacc, whit, lane);
    uint64_t list = 0;
    for (uint32_t k0 = 0; k0 < SPT_SUB; k0 += WAVE) {
        const uint32_t k = k0 + lane;
        const uint64_t id = sub_lo + k;
        uint64_t key = 0;
        if (id < sub_hi && ((whit[k >> 5] >> (k & 31)) & 1u) && del.live((uint32_t)id)) key = make_key(wacc[k], (uint32_t)id);
        if (key_bound && key >= bound) key = 0;
        wave_offer(list, key, (int)top, lane);
    }
    sparse_block_emit(list, (int)top, tile, ql, nq_tile, partial);
}

// plain_search over an id list on the index (search_context.rs:92-143): one thread per id; for each dimension of the query's plan, in ascending
// remapped order, the id is looked up in the dimension's posting ids (`skip_to`: a lower bound), and a hit adds decode(weight) x query weight.
// No decoded copy of the row exists.  Grid, key lists and passes as sparse_topk_ids_kernel.
template <typename W>
__global__ __launch_bounds__(SP_BLOCK) void sparse_topk_ids_q_kernel(const uint32_t *pid, const W *pw, SparsePlanQ plan, uint32_t q0, uint32_t nq_tile,
                                                                     const uint32_t *ids, uint64_t n_ids, uint64_t n_rows, DeletedView del, uint32_t top,
                                                                     const uint64_t *key_bound, uint64_t *partial) {
    const uint32_t ql = blockIdx.y, qi = q0 + ql;
    const int lane = threadIdx.x & 63;
    const uint64_t bound = key_bound ? key_bound[ql] : 0;
    if (key_bound && bound == 0) {
        if (threadIdx.x < top) partial[((uint64_t)blockIdx.x * nq_tile + ql) * top + threadIdx.x] = 0;
        return;
    }
    const uint32_t d0 = plan.off[qi], d1 = plan.off[qi + 1];
    uint64_t list = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * SP_BLOCK; base < n_ids; base += (uint64_t)gridDim.x * SP_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        uint64_t key = 0;
        if (i < n_ids) {
            const uint32_t id = ids[i];
            if (id < n_rows && del.live(id)) {
                float s = 0.0f;
                bool ov = false;
                for (uint32_t c = d0; c < d1; ++c) {
                    uint64_t a = plan.start[c], b = plan.end[c];
                    const uint64_t e = b;
                    while (a < b) {
                        const uint64_t m = (a + b) >> 1;
                        if (pid[m] < id) a = m + 1;
                        else b = m;
                    }
                    if (a < e && pid[a] == id) {
                        const float mn = sizeof(W) == 1 ? plan.mn[c] : 0.0f, dd = sizeof(W) == 1 ? plan.d256[c] : 0.0f;
                        s = __fadd_rn(s, __fmul_rn(sparse_decode<W>(pw[a], mn, dd), plan.w[c]));
                        ov = true;
                    }
                }
                if (ov) key = make_key(s, id);
            }
        }
        if (key_bound && key >= bound) key = 0;
        wave_offer(list, key, (int)top, lane);
    }
    sparse_block_emit(list, (int)top, blockIdx.x, ql, nq_tile, partial);
}

int32_t launch_sparse_post_params(hipStream_t st, const uint64_t *post, const uint64_t *dir_start, uint32_t n_dims, float *mn, float *d256) {
    if (n_dims == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sparse_post_params_kernel, dim3(std::min<uint32_t>(n_dims, 65535)), dim3(SP_BLOCK), 0, st, post, dir_start, n_dims, mn, d256);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_sparse_post_encode(hipStream_t st, const uint64_t *post, const uint64_t *dir_start, uint32_t n_dims, const float *mn, const float *d256,
                                  uint32_t wtype, uint32_t *post_id, void *post_w) {
    if (n_dims == 0) return QMX_OK;
    const dim3 grid(std::min<uint32_t>(n_dims, 65535));
    ::qmx::clear_stale_error();
    if (wtype == QMX_SPARSE_WEIGHT_U8)
        hipLaunchKernelGGL(sparse_post_encode_kernel<uint8_t>, grid, dim3(SP_BLOCK), 0, st, post, dir_start, n_dims, mn, d256, post_id, (uint8_t *)post_w);
    else
        hipLaunchKernelGGL(sparse_post_encode_kernel<uint16_t>, grid, dim3(SP_BLOCK), 0, st, post, dir_start, n_dims, nullptr, nullptr, post_id,
                           (uint16_t *)post_w);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_sparse_topk_postings_q(hipStream_t st, const SparsePostQ &post, const SparsePlanQ &plan, uint32_t q0, uint32_t nq_tile, uint64_t n_scan,
                                      const DeletedView &del, uint32_t top, const uint64_t *key_bound, uint64_t *partial, uint32_t *n_lists) {
    const uint64_t tiles = (n_scan + SPT_TILE - 1) / SPT_TILE;
    *n_lists = (uint32_t)tiles;
    if (tiles == 0 || nq_tile == 0) return QMX_OK;
    QMX_REQUIRE(nq_tile <= 65535, QMX_ERR_OTHER, "query tile too large");
    ::qmx::clear_stale_error();
    const dim3 grid((uint32_t)tiles, nq_tile);
    if (post.wtype == QMX_SPARSE_WEIGHT_U8) {
        hipLaunchKernelGGL(sparse_topk_postings_q_kernel<uint8_t>, grid, dim3(SP_BLOCK), 0, st, post.id, (const uint8_t *)post.w, plan, q0, nq_tile, n_scan, del,
                           top, key_bound, partial);
        QMX_NOTE_KERNEL(sparse_topk_postings_q_kernel<uint8_t>);
    } else {
        hipLaunchKernelGGL(sparse_topk_postings_q_kernel<uint16_t>, grid, dim3(SP_BLOCK), 0, st, post.id, (const uint16_t *)post.w, plan, q0, nq_tile, n_scan, del,
                           top, key_bound, partial);
        QMX_NOTE_KERNEL(sparse_topk_postings_q_kernel<uint16_t>);
    }
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_sparse_topk_ids_q(hipStream_t st, const SparsePostQ &post, const SparsePlanQ &plan, uint32_t q0, uint32_t nq_tile, const uint32_t *ids,
                                 uint64_t n_ids, uint64_t n_rows, const DeletedView &del, uint32_t top, const uint64_t *key_bound, uint64_t *partial,
                                 uint32_t *n_lists) {
    *n_lists = sparse_ids_lists(n_ids);
    if (nq_tile == 0) return QMX_OK;
    QMX_REQUIRE(nq_tile <= 65535, QMX_ERR_OTHER, "query tile too large");
    ::qmx::clear_stale_error();
    const dim3 grid(*n_lists, nq_tile);
    if (post.wtype == QMX_SPARSE_WEIGHT_U8) {
        hipLaunchKernelGGL(sparse_topk_ids_q_kernel<uint8_t>, grid, dim3(SP_BLOCK), 0, st, post.id, (const uint8_t *)post.w, plan, q0, nq_tile, ids, n_ids, n_rows,
                           del, top, key_bound, partial);
        QMX_NOTE_KERNEL(sparse_topk_ids_q_kernel<uint8_t>);
    } else {
        hipLaunchKernelGGL(sparse_topk_ids_q_kernel<uint16_t>, grid, dim3(SP_BLOCK), 0, st, post.id, (const uint16_t *)post.w, plan, q0, nq_tile, ids, n_ids,
                           n_rows, del, top, key_bound, partial);
        QMX_NOTE_KERNEL(sparse_topk_ids_q_kernel<uint16_t>);
    }
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

// ---- IDF corpus statistics (sparse_vector_index/read_view/idf.rs: the posting walk against a corpus mask) ----
// Work-groups (x, d) stride the posting ids of requested dimension d with coalesced loads; each wave counts the entries whose point the mask and
// the deleted flags let through by ballot + popcount and adds its count to df[d] once.
template <typename E>
__global__ __launch_bounds__(SP_BLOCK) void sparse_idf_corpus_kernel(const E *post, const uint64_t *start, const uint64_t *end, DeletedView del,
                                                                     unsigned long long *df) {
    const uint32_t d = blockIdx.y;
    const uint64_t a = start[d], e = end[d];
    uint32_t count = 0;      // wave-uniform
    for (uint64_t base = a + (uint64_t)blockIdx.x * SP_BLOCK; base < e; base += (uint64_t)gridDim.x * SP_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        const bool in = i < e && del.live((uint32_t)post[i]);
        count += (uint32_t)__popcll(__ballot(in));
    }
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(&df[d], (unsigned long long)count);
}
// the document count of a corpus: the points below n_scan that the mask and the deleted flags let through
__global__ __launch_bounds__(SP_BLOCK) void sparse_idf_docs_kernel(DeletedView del, uint64_t n_scan, unsigned long long *n_docs) {
    uint32_t count = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * SP_BLOCK; base < n_scan; base += (uint64_t)gridDim.x * SP_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        const bool in = i < n_scan && del.live((uint32_t)i);
        count += (uint32_t)__popcll(__ballot(in));
    }
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(n_docs, (unsigned long long)count);
}
int32_t launch_sparse_idf_corpus(hipStream_t st, const uint64_t *post, const uint32_t *post_id, const uint64_t *start, const uint64_t *end, uint32_t n_dims,
                                 uint64_t longest, const DeletedView &del, uint64_t n_scan, unsigned long long *df, unsigned long long *n_docs) {
    ::qmx::clear_stale_error();
    const uint32_t gx = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(blocks_of(longest), 1), 256);
    for (uint32_t y0 = 0; y0 < n_dims && longest; y0 += 65535) {
        const dim3 grid(gx, std::min<uint32_t>(65535, n_dims - y0));
        if (post) hipLaunchKernelGGL(sparse_idf_corpus_kernel<uint64_t>, grid, dim3(SP_BLOCK), 0, st, post, start + y0, end + y0, del, df + y0);
        else hipLaunchKernelGGL(sparse_idf_corpus_kernel<uint32_t>, grid, dim3(SP_BLOCK), 0, st, post_id, start + y0, end + y0, del, df + y0);
    }
    if (n_scan)
        hipLaunchKernelGGL(sparse_idf_docs_kernel, dim3((uint32_t)std::min<uint64_t>(blocks_of(n_scan), 1024)), dim3(SP_BLOCK), 0, st, del, n_scan, n_docs);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

}  // namespace qmx
