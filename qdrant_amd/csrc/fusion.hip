// fusion.hip — fusion of per-source top lists into one list per query, on device.
//
//  RRF   rrf_scoring + position_score      lib/segment/src/common/reciprocal_rank_fusion.rs:32-99
//  DBSF  score_fusion + distr_norm + norm   lib/segment/src/common/score_fusion.rs:46-164
//        welfords_mean_variance             lib/segment/src/common/score_fusion.rs:126-145
//
// One work-group per query.  Entry j = source * stride + position of the query's n_sources * stride slots gets the key (id << 32 | j); the keys are
// sorted in LDS (bitonic), so the entries of one id sit side by side in ascending j = the order in which the reference's hash-map fold meets them
// (sources in order, each list front to back).  The first entry of a run sums the run's contributions serially: a point's score STARTS at its first
// contribution and a duplicate id inside one list contributes twice, as `entry.score += ...` / `or_insert(point)` do.  The fused (score, id) keys -
// the total order of qmx_search_topk: score descending by OrderedFloat, the lower offset first among equal scores - are sorted once more and the
// best `top` written.  Every arithmetic step is one correctly rounded f32 operation in the reference's order (-ffp-contract=off; IEEE division and
// square root).
#include "kernels.hpp"
#include "sort_lds.hpp"

namespace qmx {

constexpr int FUSE_BLOCK = 256;
constexpr uint64_t FUSE_DEAD = ~0ull;      // a slot behind its list's count: sorts behind every live entry

// what list `s` of the query adds for its entry at position i (score `sc`)
struct FuseSource {
    float lo, span;      // DBSF: min and max - min of norm()
    uint32_t half;       // DBSF: every entry scores 0.5 (one entry, or min == max)
    uint32_t cnt;
};

__device__ __forceinline__ float fuse_contribution(const FuseArgs &a, const FuseSource &src, uint32_t s, uint32_t i, float sc) {
    if (a.kind == QMX_FUSION_RRF) {
        // position_score: 1.0 / ((position + 1) as f32 / weight + k as f32 - 1.0); 0.0 when weight <= 0
        const float w = a.n_weights ? a.weights[s] : 1.0f;
        if (w <= 0.0f) return 0.0f;
        return 1.0f / ((float)(i + 1) / w + (float)a.rrf_k - 1.0f);
    }
    const float normed = src.half ? 0.5f : (sc - src.lo) / src.span;
    return normed * (s < a.n_weights ? a.weights[s] : 1.0f);      // weights.chain(iter::repeat(1.0))
}

// the fused score of the run of entries that starts at sorted slot x (all of one id)
__device__ __forceinline__ float fuse_run_sum(const FuseArgs &a, const FuseSource *srcs, const uint64_t *keys, uint32_t n, uint32_t x, uint32_t q) {
    const uint32_t id = (uint32_t)(keys[x] >> 32);
    float sum = 0.0f;
    for (uint32_t y = x; y < n; ++y) {
        const uint64_t key = keys[y];
        if (key == FUSE_DEAD || (uint32_t)(key >> 32) != id) break;
        const uint32_t j = (uint32_t)key, s = j / a.stride, i = j - s * a.stride;
        const float sc = a.lists[((uint64_t)s * a.nq + q) * a.stride + i].score;
        const float c = fuse_contribution(a, srcs[s], s, i, sc);
        sum = y == x ? c : sum + c;
    }
    return sum;
}

// make_key's order puts -0.0 below 0.0, OrderedFloat holds them equal: the fused key of a zero sum is made from 0.0 whatever the sum's sign, so
// that the offset decides among zero sums (the result row gets the sum's own bits back, see below)
__device__ __forceinline__ float fuse_key_score(float s) { return s == 0.0f ? 0.0f : s; }

__global__ __launch_bounds__(FUSE_BLOCK) void fuse_topk_kernel(const FuseArgs a, uint32_t n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fuse_smem[];
    uint64_t *keys = reinterpret_cast<uint64_t *>(fuse_smem);      // [n] (id, slot), sorted ascending
    uint64_t *fused = keys + n;                                     // [n] (score, id) keys of the distinct ids, 0 elsewhere
    __shared__ FuseSource srcs[FUSE_MAX_SOURCES];
    __shared__ uint32_t n_distinct;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t total = a.n_sources * a.stride;

    // per-list statistics: one lane per (query, source); Welford's recurrence is serial by construction
    if (tid < a.n_sources) {
        const uint32_t s = tid;
        const uint32_t c = a.counts[(uint64_t)s * a.nq + q];
        FuseSource src;
        src.cnt = c < a.stride ? c : a.stride;
        src.lo = 0.0f;
        src.span = 0.0f;
        src.half = 1;
        if (a.kind == QMX_FUSION_DBSF && src.cnt >= 2) {
            const qmx_scored_point *list = a.lists + ((uint64_t)s * a.nq + q) * a.stride;
            float mean = 0.0f, aggregate = 0.0f;
            for (uint32_t k = 1; k <= src.cnt; ++k) {
                const float x = list[k - 1].score;
                const float old_delta = x - mean;
                mean += old_delta / (float)k;
                const float delta = x - mean;
                aggregate += old_delta * delta;
            }
            const float variance = aggregate / ((float)src.cnt - 1.0f);
            const float std_dev = __builtin_sqrtf(variance);
            const float lo = mean - 3.0f * std_dev, hi = mean + 3.0f * std_dev;
            src.half = lo == hi ? 1u : 0u;
            src.lo = lo;
            src.span = hi - lo;
        }
        srcs[s] = src;
    }
    if (tid == 0) n_distinct = 0;
    __syncthreads();

    for (uint32_t j = tid; j < n; j += FUSE_BLOCK) {
        uint64_t key = FUSE_DEAD;
        if (j < total) {
            const uint32_t s = j / a.stride, i = j - s * a.stride;
            if (i < srcs[s].cnt) key = ((uint64_t)a.lists[((uint64_t)s * a.nq + q) * a.stride + i].idx << 32) | j;
        }
        keys[j] = key;
    }
    __syncthreads();
    bitonic_sort_lds<FUSE_BLOCK>(keys, n);

    for (uint32_t x = tid; x < n; x += FUSE_BLOCK) {
        const uint64_t key = keys[x];
        uint64_t f = 0;
        if (key != FUSE_DEAD && (x == 0 || (uint32_t)(keys[x - 1] >> 32) != (uint32_t)(key >> 32))) {
            f = make_key(fuse_key_score(fuse_run_sum(a, srcs, keys, n, x, q)), (uint32_t)(key >> 32));
            atomicAdd(&n_distinct, 1u);
        }
        fused[x] = f;
    }
    __syncthreads();
    bitonic_sort_lds<FUSE_BLOCK>(fused, n);

    const uint32_t found = n_distinct < a.top ? n_distinct : a.top;
    for (uint32_t r = tid; r < a.top; r += FUSE_BLOCK) {
        qmx_scored_point p{0u, 0.0f};
        if (r < found) {
            const uint64_t f = fused[n - 1 - r];
            p.idx = key_idx(f);
            p.score = key_score(f);
            if (p.score == 0.0f) {
                // a zero sum (a zero weight, as a rule): the key carries 0.0, the result the sum's own bits - summed once more from the id's run
                uint32_t lo = 0, hi = n;      // first sorted slot of this id
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (keys[mid] < ((uint64_t)p.idx << 32)) lo = mid + 1; else hi = mid;
                }
                if (lo < n) p.score = fuse_run_sum(a, srcs, keys, n, lo, q);
            }
        }
        a.out[(uint64_t)q * a.top + r] = p;
    }
    if (tid == 0) a.out_counts[q] = found;
}

int32_t launch_fuse_topk(hipStream_t st, const FuseArgs &a) {
    if (a.nq == 0) return QMX_OK;
    const uint64_t total = (uint64_t)a.n_sources * a.stride;
    uint32_t n = 2;
    while (n < total) n <<= 1;
    const size_t lds = (size_t)n * 2 * sizeof(uint64_t);
    static thread_local DeviceOnce attr_once;
    if (attr_once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fuse_topk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(FUSE_MAX_ENTRIES * 2 * sizeof(uint64_t))));
        attr_once.mark();
    }
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(fuse_topk_kernel, dim3(a.nq), dim3(FUSE_BLOCK), lds, st, a, n);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

}  // namespace qmx
