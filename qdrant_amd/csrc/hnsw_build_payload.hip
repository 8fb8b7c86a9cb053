// hnsw_build_payload.hip — the payload-block build (hnsw_build_payload.hpp) instantiated for the dense lane policies, and the level-0 merge kernels.
#include "dense_policies.hpp"
#include "hnsw_build_payload.hpp"

namespace qmx {

int32_t launch_hnsw_payload_dense(hipStream_t st, int dtype, int distance, const ScanArgs &a, const HnswPayloadArgs &h, int phase, uint32_t grid, int *per_cu) {
    const HnswPayloadLauncher l{st, &h, phase, grid, per_cu};
    if (dtype == QMX_DTYPE_F32) return dispatch_metric<RowF32, SmallF32, true>(l, distance, a);
    if (dtype == QMX_DTYPE_F16) return dispatch_metric<RowF16, SmallF16, true>(l, distance, a);
    if (dtype == QMX_DTYPE_U8) {      // (as launch_hnsw_build_dense: the per-pair cosine takes the query's norm from the per-row norm column)
        QMX_REQUIRE(distance != QMX_DISTANCE_COSINE || a.dim < 32 || (a.row_norms_f && a.row_norms_i), QMX_ERR_BAD_ARG, "u8 cosine build without the row norms");
        return dispatch_metric<RowU8Internal, SmallU8, false>(l, distance, a);
    }
    set_error("payload links: dtype %d with distance %d not supported", dtype, distance);
    return QMX_ERR_NOT_SUPPORTED;
}

// ---- the merge ---------------------------------------------------------------------------------------------------------------------------------------
// cap[p] = cnt_main[p] + sum over p's memberships of cnt_block: one thread per point
__global__ __launch_bounds__(256) void hnsw_payload_merge_caps_kernel(const HnswPayloadMergeArgs m) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= m.n_points) return;
    uint64_t c = m.main_off ? m.main_off[p + 1] - m.main_off[p] : 0;
    for (uint64_t i = m.mem_off[p]; i < m.mem_off[p + 1]; ++i) {
        const uint32_t k = m.cnt[m.mem_slot[i]];
        c += k < m.pm0 ? k : m.pm0;
    }
    m.cap[p] = c;
}

// One wave per point: the main row, then per membership the links not yet in the row (a block row holds no id twice, so its links are tested against the
// row as it stood before that block row).  The row is written and re-read by the lanes of one wave through L2 (agent scope).
__global__ __launch_bounds__(64) void hnsw_payload_merge_rows_kernel(const HnswPayloadMergeArgs m) {
    const int lane = threadIdx.x;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    for (uint64_t p = blockIdx.x; p < m.n_points; p += gridDim.x) {
        uint32_t *row = m.tmp + m.cap[p];
        const uint64_t row_cap = m.cap[p + 1] - m.cap[p];
        uint64_t len = 0;
        if (m.main_off) {
            const uint64_t o0 = m.main_off[p], o1 = m.main_off[p + 1];
            for (uint64_t i = o0 + (uint64_t)lane; i < o1; i += 64) st_agent(row + (i - o0), m.main_nb[i]);
            len = o1 - o0;
        }
        for (uint64_t mi = m.mem_off[p]; mi < m.mem_off[p + 1]; ++mi) {
            const uint64_t slot = m.mem_slot[mi];
            const uint32_t *pts = m.points + m.mem_slot0[mi];
            uint32_t k = m.cnt[slot];
            k = k < m.pm0 ? k : m.pm0;
            const uint32_t *lst = m.links + slot * m.pm0;
            const uint64_t before = len;
            __threadfence();
            for (uint32_t base = 0; base < k; base += 64) {
                const bool on = base + (uint32_t)lane < k;
                const uint32_t id = on ? pts[lst[base + lane]] : 0;
                bool fresh = on;
                for (uint64_t j = 0; j < before && fresh; ++j) fresh = ld_agent(row + j) != id;
                const uint64_t mask = __ballot(fresh);
                if (fresh) {
                    const uint64_t at = len + (uint64_t)__popcll(mask & lt_mask);
                    if (at < row_cap) st_agent(row + at, id);
                }
                len += (uint64_t)__popcll(mask);
            }
        }
        if (lane == 0) m.len[p] = len < row_cap ? len : row_cap;
    }
}

__global__ __launch_bounds__(64) void hnsw_payload_merge_compact_kernel(const HnswPayloadMergeArgs m) {
    const int lane = threadIdx.x;
    for (uint64_t p = blockIdx.x; p < m.n_points; p += gridDim.x) {
        const uint32_t *row = m.tmp + m.cap[p];
        const uint64_t o0 = m.len[p], n = m.len[p + 1] - o0;
        for (uint64_t i = (uint64_t)lane; i < n; i += 64) m.out[o0 + i] = ld_agent(row + i);
    }
}

// exclusive prefix sum in place by one work-group: every thread owns a contiguous chunk (its sum, a scan of the 1024 sums in LDS, then its chunk again)
__global__ __launch_bounds__(1024) void exclusive_scan_u64_kernel(uint64_t *v, uint64_t n) {
    __shared__ uint64_t sums[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t chunk = (n + 1023) / 1024;
    const uint64_t lo = (uint64_t)t * chunk < n ? (uint64_t)t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    uint64_t s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += v[i];
    sums[t] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint64_t add = t >= off ? sums[t - off] : 0;
        __syncthreads();
        sums[t] += add;
        __syncthreads();
    }
    uint64_t run = sums[t] - s;      // exclusive
    for (uint64_t i = lo; i < hi; ++i) {
        const uint64_t x = v[i];
        v[i] = run;
        run += x;
    }
    if (t == 1023) v[n] = sums[1023];
}

// the original rows of a round's items, side by side (4-byte words; one wave per row)
__global__ __launch_bounds__(64) void gather_rows_kernel(const unsigned char *src, uint64_t src_stride, const uint32_t *ids, uint64_t n, uint32_t words,
                                                         unsigned char *dst, uint64_t dst_stride) {
    for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint32_t *s = reinterpret_cast<const uint32_t *>(src + (uint64_t)ids[r] * src_stride);
        uint32_t *d = reinterpret_cast<uint32_t *>(dst + r * dst_stride);
        for (uint32_t i = threadIdx.x; i < words; i += 64) d[i] = s[i];
    }
}
int32_t launch_gather_rows(hipStream_t st, const void *src, uint64_t src_stride, const uint32_t *ids, uint64_t n, uint32_t row_bytes, void *dst, uint64_t dst_stride) {
    if (!n) return QMX_OK;
    QMX_REQUIRE(row_bytes % 4 == 0 && src_stride % 4 == 0 && dst_stride % 4 == 0, QMX_ERR_BAD_ARG, "gather_rows: rows of whole 4-byte words");
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(gather_rows_kernel, dim3((uint32_t)(n < 65536 ? n : 65536)), dim3(64), 0, st, (const unsigned char *)src, src_stride, ids, n, row_bytes / 4,
                       (unsigned char *)dst, dst_stride);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

static uint32_t merge_grid(uint32_t n) { return n < 65536u * 8u ? (n ? n : 1u) : 65536u * 8u; }
int32_t launch_hnsw_payload_merge_caps(hipStream_t st, const HnswPayloadMergeArgs &m) {
    if (!m.n_points) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(hnsw_payload_merge_caps_kernel, dim3((m.n_points + 255) / 256), dim3(256), 0, st, m);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_hnsw_payload_merge_rows(hipStream_t st, const HnswPayloadMergeArgs &m) {
    if (!m.n_points) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(hnsw_payload_merge_rows_kernel, dim3(merge_grid(m.n_points)), dim3(64), 0, st, m);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_hnsw_payload_merge_compact(hipStream_t st, const HnswPayloadMergeArgs &m) {
    if (!m.n_points) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(hnsw_payload_merge_compact_kernel, dim3(merge_grid(m.n_points)), dim3(64), 0, st, m);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_exclusive_scan_u64(hipStream_t st, uint64_t *v, uint64_t n) {
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(exclusive_scan_u64_kernel, dim3(1), dim3(1024), 0, st, v, n);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

}  // namespace qmx
