// api_matrix.hip — the C-ABI of include/qdrant_amd.h, the distance matrix API: qmx_sample_points (Sample::Random on the device) and qmx_search_matrix (the
// nearest lists of a sample) over the kernels of matrix.hip and the unchanged exact scans.  (One of the api_*.hip translation units; what they share:
// api_internal.hpp.)
#include "api_internal.hpp"
#include "matrix_plan.hpp"

namespace {

// a count the caller reads: host memory or device memory
int32_t put_u32(uint32_t *dst, uint32_t v) {
    if (is_device_ptr(dst)) QMX_HIP(hipMemcpy(dst, &v, 4, hipMemcpyHostToDevice));
    else *dst = v;
    return QMX_OK;
}
int32_t zero_u32(uint32_t *dst, size_t n) {
    if (n == 0) return QMX_OK;
    if (is_device_ptr(dst)) QMX_HIP(hipMemset(dst, 0, n * 4));
    else memset(dst, 0, n * 4);
    return QMX_OK;
}

// the batch of a qmx_search_matrix call, destroyed with the call
struct QueryGuard {
    qmx_query *q = nullptr;
    ~QueryGuard() { (void)qmx_query_destroy(q); }
};

// The sample's rows as a segment of their own: the stored rows gathered in the segment's layout, "deleted" = not live in the segment.  No derived
// copies and no statistics, so a search over it takes the exact tiles.  The handle owns block and bitmap.
int32_t transient_block(const qmx_segment *seg, const uint32_t *d_ids, uint32_t n_sample, qmx_segment *t, uint32_t *d_positions) {
    t->device = seg->device;
    t->num_cus = seg->num_cus;
    t->dtype = seg->dtype;
    t->distance = seg->distance;
    t->dim = seg->dim;
    t->scan_dim = seg->scan_dim;
    t->flags = seg->flags & QMX_SEG_U8_SCALAR_ORDER;
    t->n = n_sample;
    t->row_bytes = seg->row_bytes;
    // f16 rows that take the reference's AVX leaf (32 elements and more; below, the small leaf has its order already): the block is laid out for the scan that
    // sums in that leaf's order (matrix_f16.hip) - the SIMD body in whole two-iteration segments, so the block's rows count a few elements more
    t->f16_avx_order = seg->dtype == QMX_DTYPE_F16 && seg->scan_dim >= 32;
    if (t->f16_avx_order) {
        t->dim = t->scan_dim = matrix_f16_avx_dim(seg->scan_dim);
        t->row_bytes = (uint64_t)t->scan_dim * 2;
    }
    t->row_stride = (t->row_bytes + 15) & ~15ull;
    const size_t words = ((size_t)n_sample + 63) / 64;
    DevBuf rows, bits;
    QMX_TRY(rows.reserve((size_t)n_sample * t->row_stride));
    QMX_TRY(bits.reserve(words * 8));
    QMX_HIP(hipMemsetAsync(bits.p, 0, words * 8, nullptr));
    if (t->f16_avx_order)
        QMX_TRY(launch_matrix_gather_f16_avx(nullptr, seg->d_rows, seg->row_stride, seg->scan_dim, d_ids, n_sample, seg->deleted_view(), rows.p, t->row_stride,
                                             t->scan_dim, (uint64_t *)bits.p, d_positions));
    else
        QMX_TRY(launch_matrix_gather(nullptr, seg->d_rows, seg->row_stride, seg->row_bytes, d_ids, n_sample, seg->deleted_view(), rows.p, t->row_stride,
                                     (uint64_t *)bits.p, d_positions));
    QMX_HIP(hipStreamSynchronize(nullptr));      // (the batch's stream does not wait for the null stream)
    t->d_rows = rows.detach();
    t->owns_rows = true;
    t->d_point_deleted = (uint64_t *)bits.detach();
    t->n_point_bits = n_sample;
    return QMX_OK;
}

}  // namespace

extern "C" {

int32_t qmx_sample_points(const qmx_segment *seg, const uint64_t *allowed, uint64_t n_allowed_bits, uint32_t n, uint64_t seed, uint32_t *out_ids,
                          uint32_t *out_count) {
    QMX_REQUIRE(seg && out_count && (n == 0 || out_ids), QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REFUSE_SPARSE(seg);
    QMX_REQUIRE(n <= MATRIX_MAX_SAMPLE, QMX_ERR_NOT_SUPPORTED, "a sample of %u points > %u", n, MATRIX_MAX_SAMPLE);
    QMX_HIP(hipSetDevice(seg->device));
    if (n == 0 || seg->n == 0) return put_u32(out_count, 0);
    Staging stage;
    DeletedView del = seg->deleted_view();
    if (allowed) {
        QMX_TRY(stage.in(allowed, (size_t)((n_allowed_bits + 63) / 64) * 8, &del.allowed));
        del.n_allowed_bits = n_allowed_bits;
        if (n_allowed_bits == 0) return put_u32(out_count, 0);      // (a bitmap without bits allows nothing)
    }
    uint32_t *d_out = nullptr;
    QMX_TRY(stage.out(out_ids, (size_t)n * 4, &d_out));
    const uint64_t n_words = (seg->n + 63) / 64;
    const size_t o_state = SAMPLE_BINS * 4, o_counts = o_state + 256;
    DevBuf work;      // histogram, state, the compaction's block counts
    QMX_TRY(work.reserve(o_counts + (size_t)sample_count_blocks(n_words) * 4));
    uint32_t *d_hist = (uint32_t *)work.p;
    SampleState *d_state = (SampleState *)((char *)work.p + o_state);
    SampleState h_state{};
    h_state.need = n;
    QMX_HIP(hipMemsetAsync(d_hist, 0, SAMPLE_BINS * 4, nullptr));
    QMX_HIP(hipMemcpyAsync(d_state, &h_state, sizeof(h_state), hipMemcpyHostToDevice, nullptr));
    // the select: a pass and a few words back per level, until the boundary bin is taken whole (the keys differ: at the latest when the key is complete)
    for (uint32_t level = 0; level < SAMPLE_LEVELS && !h_state.done; ++level) {
        QMX_TRY(launch_sample_level(nullptr, del, n_words, seed, level, d_state, d_hist));
        QMX_HIP(hipMemcpy(&h_state, d_state, sizeof(h_state), hipMemcpyDeviceToHost));
    }
    QMX_REQUIRE(h_state.done && h_state.count <= n, QMX_ERR_OTHER, "the sampler's select did not end");
    QMX_TRY(launch_sample_write(nullptr, del, n_words, seed, d_state, (uint32_t *)((char *)work.p + o_counts), d_out, h_state.count));
    QMX_HIP(hipStreamSynchronize(nullptr));
    QMX_TRY(stage.back());
    return put_u32(out_count, h_state.count);
}

int32_t qmx_search_matrix(const qmx_segment *seg, const uint32_t *sample_ids, uint32_t n_sample, uint32_t limit, qmx_scored_point *out, uint32_t *out_cols,
                          uint32_t *out_counts, qmx_counters *counters) {
    QMX_REQUIRE(seg && (n_sample == 0 || (sample_ids && out_counts)), QMX_ERR_BAD_ARG, "NULL argument");
    if (counters) memset(counters, 0, sizeof(*counters));
    QMX_REFUSE_SPARSE(seg);
    QMX_REQUIRE(seg->dtype <= QMX_DTYPE_U8, QMX_ERR_NOT_SUPPORTED,
                "dtype %u: the matrix is scored with the original vectors (the reference rescored a quantized search with them): hand over the original storage",
                seg->dtype);
    QMX_REQUIRE(n_sample <= MATRIX_MAX_SAMPLE, QMX_ERR_NOT_SUPPORTED, "a sample of %u points > %u", n_sample, MATRIX_MAX_SAMPLE);
    QMX_HIP(hipSetDevice(seg->device));
    // the ids are validated on the host, whichever side they live on: the gather indexes the rows with them unchecked, and the order of the lists rests on theirs
    std::vector<uint32_t> h_ids(n_sample);
    if (n_sample) QMX_HIP(hipMemcpy(h_ids.data(), sample_ids, (size_t)n_sample * 4, hipMemcpyDefault));
    uint32_t bad = 0;
    const int verdict = matrix_validate_sample(h_ids.data(), n_sample, seg->n, &bad);
    QMX_REQUIRE(verdict != 1, QMX_ERR_BAD_ARG, "sample_ids must be strictly ascending: sample_ids[%u] = %u follows %u", bad, h_ids[bad], h_ids[bad - 1]);
    QMX_REQUIRE(verdict != 2, QMX_ERR_OUT_OF_BOUNDS, "sample_ids[%u] = %u: the segment holds %llu rows", bad, h_ids[bad], (unsigned long long)seg->n);
    if (n_sample < 2 || limit == 0) return zero_u32(out_counts, n_sample);      // the reference's empty response
    QMX_REQUIRE(out, QMX_ERR_BAD_ARG, "NULL output");

    Staging stage;
    const uint32_t *d_ids = nullptr;
    qmx_scored_point *d_out = nullptr;
    uint32_t *d_cols = nullptr, *d_counts = nullptr;
    QMX_TRY(stage.in(sample_ids, (size_t)n_sample * 4, &d_ids));
    QMX_TRY(stage.out(out, (size_t)n_sample * limit * sizeof(qmx_scored_point), &d_out));
    QMX_TRY(stage.out(out_cols, (size_t)n_sample * limit * 4, &d_cols));
    QMX_TRY(stage.out(out_counts, (size_t)n_sample * 4, &d_counts));

    // ---- gather: the sample's rows as a block of their own ----
    DevBuf positions;
    QMX_TRY(positions.reserve((size_t)n_sample * 4));
    qmx_segment block;
    QMX_TRY(transient_block(seg, d_ids, n_sample, &block, (uint32_t *)positions.p));

    // ---- score and finish, chunk by chunk: an internal batch over the block, the exact scans, one wave per row ----
    const uint32_t top = matrix_top(n_sample, limit), chunk = matrix_chunk(n_sample, limit);
    DevBuf lists;
    QMX_TRY(lists.reserve((size_t)chunk * top * sizeof(qmx_scored_point) + (size_t)chunk * 4));
    qmx_scored_point *d_lists = (qmx_scored_point *)lists.p;
    uint32_t *d_list_counts = (uint32_t *)(d_lists + (size_t)chunk * top);
    QueryGuard g;
    QMX_TRY(qmx_query_create_internal(&block, (const uint32_t *)positions.p, chunk, &g.q));
    qmx_query *q = g.q;
    qmx_counters total{};
    const bool timed = (seg->flags & QMX_SEG_TIME_KERNELS) != 0;      // event pairs around the scans: counters->kernel_ms
    for (uint32_t c0 = 0; c0 < n_sample; c0 += chunk) {
        const uint32_t n_chunk = std::min<uint32_t>(chunk, n_sample - c0);
        if (c0) {      // (chunk 0 was encoded at create)
            if (n_chunk < chunk) QMX_HIP(hipMemsetAsync(q->d_queries, 0, (size_t)q->nq_padded * q->q_stride, q->stream));
            q->nq = n_chunk;
            QMX_TRY(query_encode_internal(q, (const uint32_t *)positions.p + c0));
        }
        qmx_counters c{};
        QMX_TRY(search_enqueue(q, top, nullptr, 0, d_lists, d_list_counts, nullptr, &c, timed));
        QMX_TRY(launch_matrix_finish(q->stream, d_lists, d_list_counts, top, c0, n_chunk, d_ids, n_sample, limit, d_out, d_cols, d_counts));
        total.vectors_scored += c.vectors_scored;
        total.bytes_read += c.bytes_read;
        total.kernel_launches += c.kernel_launches + 1;
    }
    QMX_TRY(check_err_flag(q));      // synchronises the stream
    if (timed) {
        QMX_TRY(timing_fold(q));
        total.kernel_ms = q->timing_ms;
    }
    QMX_TRY(stage.back());
    total.kernel_launches += 1;      // the gather
    total.bytes_read += (uint64_t)n_sample * seg->row_bytes;
    if (counters) *counters = total;
    return QMX_OK;
}

}  // extern "C"
