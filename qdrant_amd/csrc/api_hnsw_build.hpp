// api_hnsw_build.hpp — what the two device builds share on the host: qmx_hnsw_build* (api_hnsw_build.hip: an id range under the 1/32 rule and a moving
// entry point) and qmx_hnsw_build_payload_links (api_hnsw_payload.hip: precomputed rounds of every block).  Their insertion loops are their own; the
// argument checks, the host's view of the deleted flags, the ScanArgs of a build, the query entries made from original vectors, the per-slot scratch
// and the hand-over of the finished plain arrays are here.
#pragma once
#include "api_internal.hpp"
#include "hnsw_payload_args.hpp"

// the plain arrays in `host` become a graph handle (qmx_hnsw_create's path, like every built graph), which takes them over for qmx_hnsw_export_plain
// (api_hnsw.hip)
extern "C" int32_t hnsw_finish_graph(qmx_hnsw &host, uint32_t m, uint32_t m0, uint32_t n, uint32_t n_levels, int device, qmx_hnsw **out);

// PQ: whether the build recomputes its entries from the codebook (pq.hip HopPQDirectBuild + HopPQInternalDirect; the default where the codebook allows,
// option hnsw_pq_table_build for the other) instead of reading LUTs and the centroid pair table
static inline bool pq_table_free_build(const qmx_segment *seg) {
    return !option(OPT_HNSW_PQ_TABLE_BUILD) && pq_direct_walk_ok(seg->dim, seg->pq_m, seg->pq.chunk_size, seg->pq.n_centroids);
}

// The segment a build can run over.  what = the caller's name in the texts, original_hint = how its text on a missing `original` ends;
// table_free_ok: the caller can build a PQ segment without the pair table.
static int32_t build_check_segment(const qmx_segment *seg, const qmx_segment *original, const char *what, const char *original_hint, bool table_free_ok) {
    QMX_REQUIRE(seg->dtype <= QMX_DTYPE_BQ || seg->dtype == QMX_DTYPE_TQ, QMX_ERR_NOT_SUPPORTED, "%s: dtype %u not supported", what, seg->dtype);
    if (seg->dtype == QMX_DTYPE_PQ || seg->dtype == QMX_DTYPE_TQ) {   // point_scorer.rs:197-212: the insertion searches score through the query (PQ: LUT) of the ORIGINAL vector
        QMX_REQUIRE(original, QMX_ERR_NOT_SUPPORTED,
                    "a PQ / TurboQuant segment cannot score a stored row as a query (encode_internal_vector -> None): pass the original f32 segment%s", original_hint);
        QMX_REQUIRE(original->dtype == QMX_DTYPE_F32 && original->dim == seg->dim && original->n >= seg->n && original->device == seg->device,
                    QMX_ERR_BAD_ARG, "the original segment must be f32, of the same dim, on the same device and hold every row of the quantized segment");
        QMX_REQUIRE(seg->dtype != QMX_DTYPE_PQ || seg->d_pq_pair || (table_free_ok && pq_table_free_build(seg)), QMX_ERR_NOT_SUPPORTED,
                    "PQ build: the centroid pair table (m x n_centroids^2 floats) exceeds 256 MB");
    }
    QMX_REQUIRE(seg->dtype == QMX_DTYPE_SQ_U8 || seg->dtype == QMX_DTYPE_PQ || seg->fast_layout(), QMX_ERR_NOT_SUPPORTED,
                "adopted device block is not 16-byte aligned");
    return QMX_OK;
}

// The deleted flags on the host, copied once: deleted points are never indexed and never entry points.
struct HostLiveness {
    std::vector<uint64_t> pdel, vdel;
    uint64_t n_point_bits = 0, n_vec_bits = 0;
    int32_t load(const qmx_segment *seg) {
        n_point_bits = seg->n_point_bits;
        n_vec_bits = seg->n_vec_bits;
        if (seg->d_point_deleted) { pdel.resize((n_point_bits + 63) / 64); QMX_HIP(hipMemcpy(pdel.data(), seg->d_point_deleted, pdel.size() * 8, hipMemcpyDeviceToHost)); }
        if (seg->d_vec_deleted) { vdel.resize((n_vec_bits + 63) / 64); QMX_HIP(hipMemcpy(vdel.data(), seg->d_vec_deleted, vdel.size() * 8, hipMemcpyDeviceToHost)); }
        return QMX_OK;
    }
    void load(const MultiBuild &mb) {      // multi-vector points: flags per POINT, given on the host
        n_point_bits = mb.n_deleted_bits;
        if (mb.h_deleted) pdel.assign(mb.h_deleted, mb.h_deleted + (mb.n_deleted_bits + 63) / 64);
    }
    bool live(uint32_t id) const {
        const bool vd = (!vdel.empty() && id < n_vec_bits) ? ((vdel[id >> 6] >> (id & 63)) & 1) : false;
        const bool pd = !pdel.empty() ? (id < n_point_bits ? ((pdel[id >> 6] >> (id & 63)) & 1) : true) : false;
        return !vd && !pd;
    }
};

// The ScanArgs of a build: no query batch (nq, queries, err_flag stay zero) - stored rows are the queries; stored <-> stored BQ scores are one-bit; for
// TurboQuant the layout of the entries the build makes per batch, and score_symmetric's inputs.
static void fill_build_args(const qmx_segment *s, ScanArgs &a) {
    fill_args_storage(s, a);
    if (s->dtype == QMX_DTYPE_SQ_U8) {
        // get_shift (encoded_vectors_u8.rs:116-134)
        float shift = (s->distance == QMX_DISTANCE_DOT || s->distance == QMX_DISTANCE_COSINE)
                          ? (float)s->sq.actual_dim * s->sq.offset * s->sq.offset : 0.0f;
        a.sq_shift = s->sq.invert ? -shift : shift;
    }
    if (s->dtype == QMX_DTYPE_BQ) {
        a.bq_dim = s->dim;
        a.bq_flip = (s->flags & QMX_SEG_BQ_TOGGLE_INVERT) ? 1 : 0;
        a.bq_qbits = 1;
    }
    if (s->dtype == QMX_DTYPE_TQ) {
        uint32_t pieces;
        a.tq_planes = (s->tq_value_bits == 1 && s->d_tq_shift) ? 16 : 8;
        tq_entry_layout(s, &pieces, &a.tq_qbytes_off, &a.aux_off);
        a.q_stride = lds_tile_stride(a.aux_off + QUERY_AUX_BYTES);
        a.bq_qbits = pieces;
        a.tq_code_bytes = s->tq_code_bytes;
        a.tq_ec = TqEc{s->d_tq_weights, s->d_tq_xm, s->tq_weight_scale, s->tq_mm_const};
    }
}

// The new point's own stored row as its query entry: bytes of a row as it lies in HBM (the SQ block holds the codes only, the vector_offset column is
// separate), staged in whole 128-byte steps.  Returns the row bytes, for check_row_query_slot.
template <class Args>
static uint64_t stage_stored_rows(const qmx_segment *seg, Args &h) {
    const uint64_t dev_row_bytes = seg->dtype == QMX_DTYPE_SQ_U8 ? (uint64_t)seg->sq.actual_dim : seg->row_bytes;
    h.row_bytes = (uint32_t)dev_row_bytes;
    h.lds_query_bytes = (uint32_t)((dev_row_bytes + 127) / 128 * 128 + 128);
    return dev_row_bytes;
}
static int32_t check_row_query_slot(uint32_t lds_query_bytes, uint64_t dev_row_bytes) {
    QMX_REQUIRE(lds_query_bytes <= HNSW_LDS_QUERY_MAX, QMX_ERR_NOT_SUPPORTED, "rows of %llu bytes do not fit the LDS query slot", (unsigned long long)dev_row_bytes);
    return QMX_OK;
}

// u8 cosine: the per-pair cosine's query norm of a stored row, one column per point
struct U8RowNorms {
    DevBuf f, i;
    int32_t attach(const qmx_segment *seg, uint32_t n, ScanArgs &a) {
        if (!(seg->dtype == QMX_DTYPE_U8 && seg->distance == QMX_DISTANCE_COSINE && seg->dim >= 32)) return QMX_OK;
        const size_t nn = std::max<uint32_t>(n, 1);
        QMX_TRY(f.reserve(nn * 4)); QMX_TRY(i.reserve(nn * 4));
        QMX_TRY(launch_u8_row_norms(nullptr, seg->d_rows, seg->row_stride, n, seg->dim, seg->flags, (float *)f.p, (int32_t *)i.p));
        a.row_norms_f = (const float *)f.p;
        a.row_norms_i = (const int32_t *)i.p;
        return QMX_OK;
    }
};

// PQ / TurboQuant segments: the query entries of a batch's new points, made from their ORIGINAL vectors before phase 1 (quantized_vectors.raw_scorer(original
// vector): Metric::preprocess - quantized_query_scorer.rs:39-41; identity for a row normalised at insert, up to the reference's 1e-6 rule -, then
// EncodedVectorsPQ::encode_query, or the rotation and TurboQuantizer::precompute_query).
struct BuildQueryEntries {
    DevBuf b_bq, b_bqsrc, b_rot;      // the entries; the original vectors of the batch; their rotations (TurboQuant)
    bool pq_table_free = false;       // PQ: the entries are the preprocessed original vectors themselves, staged in LDS per insertion - no LUTs are made, and none are
                                      // reserved (max_entries x lut_stride is 1.6 GB at m = 96: several builds on one device would multiply it for nothing)
    static uint64_t pq_lut_stride(const qmx_segment *seg) { return ((uint64_t)seg->pq_m * seg->pq.n_centroids * sizeof(float) + 15) & ~15ull; }

    // room for max_entries entries; where phase 1 finds entry bi, and what of it is staged in LDS: into h
    template <class Args>
    int32_t reserve(const qmx_segment *seg, const ScanArgs &a, Args &h, uint64_t max_entries, bool table_free_ok) {
        QMX_TRY(b_bqsrc.reserve((size_t)max_entries * seg->dim * sizeof(float)));
        if (seg->dtype == QMX_DTYPE_PQ) {   // LUTs, read through L2 (as the PQ walk does)
            pq_table_free = table_free_ok && pq_table_free_build(seg);
            if (!pq_table_free) QMX_TRY(b_bq.reserve((size_t)max_entries * pq_lut_stride(seg)));
            h.batch_queries = (const unsigned char *)(pq_table_free ? b_bqsrc.p : b_bq.p);
            h.batch_q_stride = pq_table_free ? (uint64_t)seg->dim * 4 : pq_lut_stride(seg);
            h.lds_query_bytes = pq_table_free ? seg->dim * 4 : 0;
            // (round 5 tried an 8-bit LUT image per new point behind its vector, to prefilter the hops of the insertion searches: the same graph,
            // 25.6 s against 24.9 s at 2 M x 1536 points - gone from the code since round 6, profiles/r5_walk_variants_pq_hop_prefilter.jsonl)
        } else {                            // precompute_query entries, staged in LDS per insertion
            QMX_TRY(b_bq.reserve((size_t)max_entries * a.q_stride));
            QMX_TRY(b_rot.reserve((size_t)max_entries * seg->tq_padded_dim * sizeof(double)));
            h.batch_queries = (const unsigned char *)b_bq.p;
            h.batch_q_stride = a.q_stride;
            h.lds_query_bytes = a.q_stride;
        }
        return QMX_OK;
    }

    // the entries of nr new points: rows r0 .. r0 + nr of the original segment, or - d_ids - its rows d_ids[0 .. nr)
    int32_t make(const qmx_segment *seg, const qmx_segment *original, const ScanArgs &a, uint64_t r0, const uint32_t *d_ids, uint64_t nr) {
        if (!nr) return QMX_OK;
        float *src = (float *)b_bqsrc.p;
        if (d_ids) QMX_TRY(launch_gather_rows(nullptr, original->d_rows, original->row_stride, d_ids, nr, seg->dim * 4, src, (uint64_t)seg->dim * 4));
        else QMX_HIP(hipMemcpy2DAsync(src, (size_t)seg->dim * 4, (const char *)original->d_rows + r0 * original->row_stride, original->row_stride,
                                      (size_t)seg->dim * 4, nr, hipMemcpyDeviceToDevice, nullptr));
        if (seg->distance == QMX_DISTANCE_COSINE) QMX_TRY(launch_cosine_preprocess_f32(nullptr, src, src, nr, seg->dim));
        if (seg->dtype == QMX_DTYPE_PQ) {
            if (!pq_table_free) QMX_TRY(launch_pq_lut(nullptr, seg->distance, seg->dim, seg->pq, seg->d_centroids, src, (uint32_t)nr, (float *)b_bq.p));
            return QMX_OK;
        }
        QMX_TRY(launch_tq_rotate(nullptr, src, (uint32_t)nr, tq_rotation(seg), (double *)b_rot.p));
        QMX_TRY(launch_tq_query_encode(nullptr, (double *)b_rot.p, (uint32_t)nr, seg->tq_padded_dim, seg->tq_value_bits, seg->distance == QMX_DISTANCE_EUCLID ? 1 : 0,
                                       b_bq.p, a.q_stride, a.aux_off, seg->d_tq_shift, seg->d_tq_scale, a.tq_qbytes_off));
        return QMX_OK;
    }
};

// The scratch of the launches: how many insertions run side by side in each phase (the occupancy of the kernels that `launch(phase, grid, &per_cu)` would
// start, the slot cap, the visited budget, `most` = the largest batch), a visited bitmap of vis_bits bits and its log per phase-1 slot, and the two counters
// the slots draw their next insertion from.
struct InsertSlots {
    DevBuf b_vis, b_log, b_next;
    uint64_t slots1 = 1, slots2 = 1;
    template <class Args, class Launch>
    int32_t reserve(const qmx_segment *seg, Args &h, uint64_t vis_bits, uint64_t most, const Launch &launch) {
        h.log_cap = 16384;
        h.vis_words = std::max<uint64_t>(1, (vis_bits + 31) / 32);
        int per_cu1 = 1, per_cu2 = 1;
        QMX_TRY(launch(1, 0u, &per_cu1));
        QMX_TRY(launch(2, 0u, &per_cu2));
        slots1 = std::min<uint64_t>({(uint64_t)seg->num_cus * per_cu1, (uint64_t)HNSW_SLOT_CAP, most});
        slots1 = std::max<uint64_t>(1, std::min<uint64_t>(slots1, HNSW_VIS_BUDGET / (h.vis_words * 4)));
        slots2 = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)seg->num_cus * per_cu2, most));
        QMX_TRY(b_next.reserve(8));
        h.next = (uint32_t *)b_next.p;
        QMX_TRY(b_vis.reserve((size_t)slots1 * h.vis_words * 4));
        QMX_TRY(b_log.reserve((size_t)slots1 * h.log_cap * 4));
        QMX_HIP(hipMemset(b_vis.p, 0, (size_t)slots1 * h.vis_words * 4));
        h.visited = (uint32_t *)b_vis.p;
        h.vis_log = (uint32_t *)b_log.p;
        return QMX_OK;
    }
    // the grids of a batch of `count` insertions; the counters start at them
    int32_t begin_batch(uint32_t count, uint32_t *grid1, uint32_t *grid2) {
        *grid1 = (uint32_t)std::min<uint64_t>(slots1, count);
        *grid2 = (uint32_t)std::min<uint64_t>(slots2, count);
        const uint32_t start[2] = {*grid1, *grid2};
        QMX_HIP(hipMemcpyAsync(b_next.p, start, sizeof(start), hipMemcpyHostToDevice, nullptr));      // (pageable source: the copy is staged before the call returns)
        return QMX_OK;
    }
};
