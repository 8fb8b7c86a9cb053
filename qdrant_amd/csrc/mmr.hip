// mmr.hip — maximal marginal relevance re-ranking of a candidate list, on device.
//
//  mmr_from_points_with_vector   lib/shard/src/query/mmr/mod.rs:42-100    (unique by id, < 2 candidates returned as they are)
//  maximal_marginal_relevance    lib/shard/src/query/mmr/mod.rs:198-279   (first pick by relevance, then lambda * rel - (1 - lambda) * max sim)
//  LazyMatrix::get_similarity    lib/shard/src/query/mmr/lazy_matrix.rs:56-67 (scorers[c].score_point(s): candidate c as the query, row s stored)
//
// (The selection machinery - unique by id, the order array, OrderedFloat keys, the arg-max, the pick - is mmr_common.hpp's, shared with sparse_mmr.hip.)
//
// One work-group per request, every selection step inside the one launch.  The reference only ever asks for (candidate, selected) pairs, so a step
// scores the remaining candidates against the ONE row selected last (staged in LDS as f32) and folds that column into a running maximum:
// limit x C row scores per request, no C x C matrix.  In LDS per candidate: its input position, its id, its relevance, max_sim_to_selected and its
// slot of the order array (the reference's `remaining_indices`, an IndexSet whose swap_remove moves the last element into the freed slot).
// Ties are the reference's: `max_by_key` returns the LAST maximal element of the iteration, i.e. "greatest score, then greatest position in the
// current order"; the running maximum takes a later equal similarity (>=); comparisons are OrderedFloat's (NaN greatest, -0.0 == 0.0).
//
// Pair scores are the f32 leaves of dense_policies.hpp (RowF32's accumulators and hsum order, small_f32_leaf below 32 elements): on an f32 segment
// the bits of qmx_query_create_internal([c]) + qmx_score_points([s]).  f16 / u8 rows are widened to f32 exactly first - the reference's temporary
// storage is always f32 (new_volatile_dense_vector_storage) - and the f32 metric applied.  The leaves are symmetric in their two vectors bit for bit
// (a * b, (a - b)^2 and |a - b| are), so the selected row serves as the LDS-resident side.
#include "dense_policies.hpp"
#include "mmr_common.hpp"

namespace qmx {

// element types of the stored block, widened to f32 (exact)
struct ElemF32 {
    static constexpr uint32_t BYTES = 4;
    static __device__ __forceinline__ float4 load4(const unsigned char *row, uint32_t e) { return *reinterpret_cast<const float4 *>(row + (uint64_t)e * 4); }
    static __device__ __forceinline__ float load1(const unsigned char *row, uint32_t e) { return reinterpret_cast<const float *>(row)[e]; }
};
struct ElemF16 {
    static constexpr uint32_t BYTES = 2;
    static __device__ __forceinline__ float4 load4(const unsigned char *row, uint32_t e) {
        const uint2 raw = *reinterpret_cast<const uint2 *>(row + (uint64_t)e * 2);
        const half2_t lo = *reinterpret_cast<const half2_t *>(&raw.x), hi = *reinterpret_cast<const half2_t *>(&raw.y);
        return make_float4((float)lo[0], (float)lo[1], (float)hi[0], (float)hi[1]);
    }
    static __device__ __forceinline__ float load1(const unsigned char *row, uint32_t e) { return (float)reinterpret_cast<const _Float16 *>(row)[e]; }
};
struct ElemU8 {
    static constexpr uint32_t BYTES = 1;
    static __device__ __forceinline__ float4 load4(const unsigned char *row, uint32_t e) {
        const uint32_t raw = *reinterpret_cast<const uint32_t *>(row + e);
        return make_float4((float)(raw & 255u), (float)((raw >> 8) & 255u), (float)((raw >> 16) & 255u), (float)(raw >> 24));
    }
    static __device__ __forceinline__ float load1(const unsigned char *row, uint32_t e) { return (float)row[e]; }
};

// rows of 32 elements and more: the AVX leaf (simple_avx.rs) by the 8 lanes of a group, candidate row `crow` as the query against the selected
// row `sel` (f32, LDS).  Accumulators, step order and hsum are group_score<RowF32>'s; U row pieces in flight per lane.
template <int METRIC, class E, int U = 12>
__device__ __forceinline__ float mmr_group_score(const float *sel, const unsigned char *crow, uint32_t dim, int t) {
    typedef RowF32<METRIC> P;
    const uint32_t piece = (uint32_t)lane_piece(t) * 4;
    const uint32_t nseg = dim / 32, tail_start = nseg * 32;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t s0 = 0; s0 < nseg; s0 += U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t s = s0 + (uint32_t)u < nseg ? s0 + (uint32_t)u : nseg - 1;
            v[u] = E::load4(crow, s * 32 + piece);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (s0 + (uint32_t)u < nseg) {
                const float4 r = *reinterpret_cast<const float4 *>(sel + (s0 + (uint32_t)u) * 32 + piece);
                P::mac1(acc[0], v[u].x, r.x);
                P::mac1(acc[1], v[u].y, r.y);
                P::mac1(acc[2], v[u].z, r.z);
                P::mac1(acc[3], v[u].w, r.w);
            }
        }
    }
    ScanArgs body;      // finish() reads the tail bounds only: none here, the tail below widens the stored elements itself
    body.dim = dim;
    body.tail_start = dim;
    float dummy[1] = {0.0f};
    float result = P::finish(acc, dummy, nullptr, nullptr, 0u, body);
    if (tail_start < dim) {      // the scalar tail adds to the positive sum (simple_avx.rs:208-211); negation is exact
        if (METRIC != M_DOT) result = -result;
        for (uint32_t i = tail_start; i < dim; ++i) result += term_f32<METRIC>(E::load1(crow, i), sel[i]);
        if (METRIC != M_DOT) result = -result;
    }
    return result;
}

template <int METRIC, class E>
__global__ __launch_bounds__(MMR_BLOCK) void mmr_select_kernel(const MmrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mmr_smem[];
    const uint32_t S = (a.stride + 3) & ~3u;
    MmrLists l;
    l.id = reinterpret_cast<uint32_t *>(mmr_smem);
    l.src = l.id + S;
    l.order = l.src + S;
    l.rel = reinterpret_cast<float *>(l.order + S);
    l.max = l.rel + S;
    float *s_row = l.max + S;      // [dim] the row selected last, as f32
    __shared__ uint64_t s_best[MMR_NW];
    __shared__ uint32_t s_bad, s_n, s_sel;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63;
    const qmx_scored_point *cand = a.cand + (uint64_t)q * a.stride;
    qmx_scored_point *out = a.out + (uint64_t)q * a.limit;
    const unsigned char *rows = reinterpret_cast<const unsigned char *>(a.rows);
    const uint32_t cnt = a.counts[q] < a.stride ? a.counts[q] : a.stride;

    if (!mmr_load_ids(l, cand, cnt, a.n_rows, a.limit, out, a.out_counts + q, a.err_flag, &s_bad)) return;
    const uint32_t C = mmr_unique(l, cnt, &s_n);
    for (uint32_t c = tid; c < C; c += MMR_BLOCK) {
        l.order[c] = c;
        l.rel[c] = a.rel[(uint64_t)q * a.stride + l.src[c]];
        l.max[c] = 0.0f;
    }
    __syncthreads();

    uint32_t n_sel = 0;
    if (C < 2) {      // "can't compute MMR for less than 2 points, return with original score" (mod.rs:77-80)
        if (tid == 0 && C == 1) out[0] = cand[l.src[0]];
        n_sel = C;
    } else {
        const uint32_t L = a.limit < C ? a.limit : C;
        uint32_t R = C;
        const float lambda = a.lambda, one_minus = 1.0f - a.lambda;
        const int t = lane & 7;
        const uint32_t g = tid >> 3;
        while (n_sel < L) {
            uint64_t best = 0;
            if (n_sel == 0) {      // the candidate of greatest relevance
                for (uint32_t p = tid; p < R; p += MMR_BLOCK) {
                    const uint64_t key = mmr_key(l.rel[l.order[p]], p);
                    best = key > best ? key : best;
                }
            } else {
                const uint32_t sel_id = l.id[l.src[s_sel]];
                const unsigned char *srow = rows + (uint64_t)sel_id * a.row_stride;
                for (uint32_t e = tid; e < a.dim; e += MMR_BLOCK) s_row[e] = E::load1(srow, e);
                __syncthreads();
                const bool first = n_sel == 1;
                if (a.dim >= 32) {
                    for (uint32_t base = 0; base < R; base += MMR_BLOCK / 8) {
                        const uint32_t p = base + g;
                        const bool valid = p < R;
                        const uint32_t c = l.order[valid ? p : 0];
                        const float sim = mmr_group_score<METRIC, E>(s_row, rows + (uint64_t)l.id[l.src[c]] * a.row_stride, a.dim, t);
                        if (valid && t == 0) {
                            const uint64_t key = mmr_fold(l, c, p, sim, first, lambda, one_minus);
                            best = key > best ? key : best;
                        }
                    }
                } else {      // below the AVX threshold: the SSE / scalar leaf, one lane per candidate
                    for (uint32_t p = tid; p < R; p += MMR_BLOCK) {
                        const uint32_t c = l.order[p];
                        const unsigned char *crow = rows + (uint64_t)l.id[l.src[c]] * a.row_stride;
                        const float sim = small_f32_leaf<METRIC>(a.dim, [&](uint32_t i) { return E::load1(crow, i); }, [&](uint32_t i) { return s_row[i]; });
                        const uint64_t key = mmr_fold(l, c, p, sim, first, lambda, one_minus);
                        best = key > best ? key : best;
                    }
                }
            }
            best = mmr_block_max(best, s_best);
            mmr_pick(l, best, R, cand, out, n_sel, &s_sel);
            --R;
            ++n_sel;
        }
    }
    if (tid == 0) a.out_counts[q] = n_sel;
    for (uint32_t i = n_sel + tid; i < a.limit; i += MMR_BLOCK) out[i] = qmx_scored_point{0u, 0.0f};
}

template <int METRIC, class E>
static int32_t launch_mmr_inst(hipStream_t st, const MmrArgs &a, uint32_t nq) {
    const size_t S = ((size_t)a.stride + 3) & ~(size_t)3;
    const size_t lds = S * MMR_CAND_BYTES + (((size_t)a.dim + 3) & ~(size_t)3) * 4;
    QMX_REQUIRE(lds <= 160 * 1024 - 256, QMX_ERR_NOT_SUPPORTED, "MMR over %u candidates of %u elements needs %zu B of LDS (> 160 KiB)", a.stride, a.dim, lds);
    auto kfn = mmr_select_kernel<METRIC, E>;
    static thread_local DeviceOnce attr_once;
    if (attr_once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
        attr_once.mark();
    }
    ::qmx::clear_stale_error();
    QMX_NOTE_KERNEL(kfn);
    hipLaunchKernelGGL(kfn, dim3(nq), dim3(MMR_BLOCK), lds, st, a);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

template <class E>
static int32_t launch_mmr_metric(hipStream_t st, int distance, const MmrArgs &a, uint32_t nq) {
    switch (distance) {
        case QMX_DISTANCE_COSINE:      // CosineMetric::similarity == DotProductMetric::similarity on the stored (preprocessed) rows (simple.rs:174-176)
        case QMX_DISTANCE_DOT: return launch_mmr_inst<M_DOT, E>(st, a, nq);
        case QMX_DISTANCE_EUCLID: return launch_mmr_inst<M_EUCLID, E>(st, a, nq);
        case QMX_DISTANCE_MANHATTAN: return launch_mmr_inst<M_MANHATTAN, E>(st, a, nq);
    }
    set_error("bad distance %d", distance);
    return QMX_ERR_BAD_ARG;
}

int32_t launch_mmr_select(hipStream_t st, int dtype, int distance, const MmrArgs &a, uint32_t nq) {
    if (nq == 0) return QMX_OK;
    switch (dtype) {
        case QMX_DTYPE_F32: return launch_mmr_metric<ElemF32>(st, distance, a, nq);
        case QMX_DTYPE_F16: return launch_mmr_metric<ElemF16>(st, distance, a, nq);
        case QMX_DTYPE_U8: return launch_mmr_metric<ElemU8>(st, distance, a, nq);
    }
    set_error("MMR: dtype %d not supported", dtype);
    return QMX_ERR_NOT_SUPPORTED;
}

}  // namespace qmx
