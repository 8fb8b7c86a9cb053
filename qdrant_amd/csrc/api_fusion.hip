// api_fusion.hip — the C-ABI of include/qdrant_amd.h, hybrid queries: fusion of prefetch lists (qmx_fuse_topk*, kernel in fusion.hip) and MMR
// re-ranking (qmx_mmr_select*, kernel in mmr.hip).
// (One of the api_*.hip translation units; what they share: api_internal.hpp.)
#include "api_internal.hpp"

static int32_t fuse_args(const qmx_scored_point *lists, const uint32_t *counts, uint32_t n_sources, uint32_t nq, uint32_t stride, const qmx_fusion_params *p,
                         qmx_scored_point *out, uint32_t *out_counts, FuseArgs &a) {
    QMX_REQUIRE(p && out && out_counts && (nq == 0 || n_sources == 0 || (lists && counts)), QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(p->kind == QMX_FUSION_RRF || p->kind == QMX_FUSION_DBSF, QMX_ERR_BAD_ARG, "fusion kind %u is neither RRF nor DBSF", p->kind);
    QMX_REQUIRE(p->n_weights == 0 || p->weights, QMX_ERR_BAD_ARG, "weights is NULL");
    QMX_REQUIRE(p->kind != QMX_FUSION_RRF || p->n_weights == 0 || p->n_weights == n_sources, QMX_ERR_BAD_ARG,
                "Number of weights in RRF should match number of pre-fetches: got %u, expected %u", p->n_weights, n_sources);
    QMX_REQUIRE(p->top >= 1 && p->top <= MAX_TOP, QMX_ERR_NOT_SUPPORTED, "top %u not in 1..%u", p->top, MAX_TOP);
    QMX_REQUIRE(n_sources <= FUSE_MAX_SOURCES, QMX_ERR_NOT_SUPPORTED, "fusion of %u sources (at most %u)", n_sources, FUSE_MAX_SOURCES);
    QMX_REQUIRE((uint64_t)n_sources * stride <= FUSE_MAX_ENTRIES, QMX_ERR_NOT_SUPPORTED, "fusion of %u lists x %u entries exceeds %u entries per query",
                n_sources, stride, FUSE_MAX_ENTRIES);
    memset(&a, 0, sizeof(a));
    a.lists = lists;
    a.counts = counts;
    a.n_sources = n_sources;
    a.nq = nq;
    a.stride = stride;
    a.kind = p->kind;
    a.rrf_k = p->rrf_k;
    a.n_weights = std::min(p->n_weights, n_sources);
    for (uint32_t i = 0; i < a.n_weights; ++i) a.weights[i] = p->weights[i];
    a.top = p->top;
    a.out = out;
    a.out_counts = out_counts;
    return QMX_OK;
}

// relevance of every candidate on the query's stream, then the selection kernel
static int32_t mmr_enqueue(qmx_query *q, const qmx_scored_point *d_cand, const uint32_t *d_counts, uint32_t stride, float lambda, uint32_t limit,
                           qmx_scored_point *d_out, uint32_t *d_oc) {
    const qmx_segment *s = q->seg;
    const uint64_t total = (uint64_t)q->nq * stride;
    QMX_TRY(q->mmr_ids.reserve((size_t)total * 4));
    QMX_TRY(q->mmr_rel.reserve((size_t)total * 4));
    QMX_TRY(launch_split_candidates(q->stream, d_cand, d_counts, stride, q->nq, (uint32_t *)q->mmr_ids.p, 0, nullptr, nullptr));
    const PairSel sel{nullptr, stride, d_counts, nullptr};
    QMX_TRY(score_pairs_device(q, sel, (const uint32_t *)q->mmr_ids.p, total, (float *)q->mmr_rel.p, false));
    MmrArgs a;
    a.rows = s->d_rows;
    a.n_rows = s->n;
    a.row_stride = s->row_stride;
    a.dim = s->dim;
    a.cand = d_cand;
    a.counts = d_counts;
    a.stride = stride;
    a.rel = (const float *)q->mmr_rel.p;
    a.lambda = lambda;
    a.limit = limit;
    a.out = d_out;
    a.out_counts = d_oc;
    a.err_flag = q->d_err;
    QMX_TRY(launch_mmr_select(q->stream, (int)s->dtype, (int)s->distance, a, q->nq));
    q->last_kernel = last_noted_kernel();
    return QMX_OK;
}

static int32_t mmr_check(const qmx_query *q, const void *cand, const void *counts, uint32_t stride, uint32_t limit, const void *out, const void *oc) {
    QMX_REQUIRE(q && out && oc && (q->nq == 0 || (counts && (stride == 0 || cand))), QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(!is_sparse(q) && q->seg->dtype <= QMX_DTYPE_U8, QMX_ERR_NOT_SUPPORTED,
                "MMR is built for dense f32 / f16 / u8 segments (dtype %u: sparse, quantized and multi-vector storages are not)", q->seg->dtype);
    QMX_REQUIRE(q->seg->fast_layout(), QMX_ERR_NOT_SUPPORTED, "adopted device block is not 16-byte aligned");
    QMX_REQUIRE(limit >= 1, QMX_ERR_BAD_ARG, "limit must be > 0");
    QMX_REQUIRE(limit <= MAX_TOP, QMX_ERR_NOT_SUPPORTED, "limit %u > %u", limit, MAX_TOP);
    QMX_REQUIRE(stride <= MMR_MAX_CANDIDATES, QMX_ERR_NOT_SUPPORTED, "MMR over %u candidates per request (at most %u)", stride, MMR_MAX_CANDIDATES);
    return QMX_OK;
}

extern "C" {

int32_t qmx_fuse_topk(int32_t device_id, const qmx_scored_point *lists, const uint32_t *counts, uint32_t n_sources, uint32_t nq, uint32_t stride,
                      const qmx_fusion_params *params, qmx_scored_point *out, uint32_t *out_counts) {
    FuseArgs a;
    QMX_TRY(fuse_args(lists, counts, n_sources, nq, stride, params, out, out_counts, a));
    QMX_TRY(check_device(device_id, nullptr));
    if (nq == 0) return QMX_OK;
    const size_t lbytes = (size_t)n_sources * nq * stride * sizeof(qmx_scored_point);
    const size_t cbytes = (size_t)n_sources * nq * sizeof(uint32_t);
    const size_t obytes = (size_t)nq * a.top * sizeof(qmx_scored_point);
    Staging st;
    QMX_TRY(st.in(lists, lbytes, &a.lists));
    QMX_TRY(st.in(counts, cbytes, &a.counts));
    QMX_TRY(st.out(out, obytes, &a.out));
    QMX_TRY(st.out(out_counts, (size_t)nq * 4, &a.out_counts));
    QMX_TRY(launch_fuse_topk(nullptr, a));
    QMX_TRY(st.back());
    QMX_HIP(hipDeviceSynchronize());
    return QMX_OK;
}

int32_t qmx_fuse_topk_async(int32_t device_id, void *hip_stream, const qmx_scored_point *lists_dev, const uint32_t *counts_dev, uint32_t n_sources,
                            uint32_t nq, uint32_t stride, const qmx_fusion_params *params, qmx_scored_point *out_dev, uint32_t *out_counts_dev) {
    FuseArgs a;
    QMX_TRY(fuse_args(lists_dev, counts_dev, n_sources, nq, stride, params, out_dev, out_counts_dev, a));
    QMX_HIP(hipSetDevice(device_id));
    return launch_fuse_topk((hipStream_t)hip_stream, a);
}

int32_t qmx_mmr_select(qmx_query *q, const qmx_scored_point *candidates, const uint32_t *counts, uint32_t stride, float lambda, uint32_t limit,
                       qmx_scored_point *out, uint32_t *out_counts) {
    QMX_TRY(mmr_check(q, candidates, counts, stride, limit, out, out_counts));
    QMX_HIP(hipSetDevice(q->device));
    if (q->nq == 0) return QMX_OK;
    const void *d_cand = nullptr, *d_counts = nullptr;
    QMX_TRY(stage_in(q, q->cand, candidates, (size_t)q->nq * stride * sizeof(qmx_scored_point), &d_cand));
    QMX_TRY(stage_in(q, q->cand_cnt, counts, (size_t)q->nq * 4, &d_counts));
    const bool out_dev = is_device_ptr(out), cnt_dev = is_device_ptr(out_counts);
    qmx_scored_point *d_out = out;
    uint32_t *d_oc = out_counts;
    if (!out_dev) { QMX_TRY(q->out.reserve((size_t)q->nq * limit * sizeof(qmx_scored_point))); d_out = (qmx_scored_point *)q->out.p; }
    if (!cnt_dev) { QMX_TRY(q->counts.reserve((size_t)q->nq * 4)); d_oc = (uint32_t *)q->counts.p; }
    QMX_TRY(mmr_enqueue(q, (const qmx_scored_point *)d_cand, (const uint32_t *)d_counts, stride, lambda, limit, d_out, d_oc));
    if (!out_dev) QMX_TRY(copy_out(q->stream, out, d_out, (size_t)q->nq * limit * sizeof(qmx_scored_point)));
    if (!cnt_dev) QMX_TRY(copy_out(q->stream, out_counts, d_oc, (size_t)q->nq * 4));
    return check_err_flag(q);      // synchronises
}

int32_t qmx_mmr_select_async(qmx_query *q, const qmx_scored_point *candidates_dev, const uint32_t *counts_dev, uint32_t stride, float lambda,
                             uint32_t limit, qmx_scored_point *out_dev, uint32_t *out_counts_dev) {
    QMX_TRY(mmr_check(q, candidates_dev, counts_dev, stride, limit, out_dev, out_counts_dev));
    QMX_HIP(hipSetDevice(q->device));
    if (q->nq == 0) return QMX_OK;
    QMX_REQUIRE(stride == 0 || is_device_ptr(candidates_dev), QMX_ERR_BAD_ARG, "async MMR needs device candidates");
    return mmr_enqueue(q, candidates_dev, counts_dev, stride, lambda, limit, out_dev, out_counts_dev);
}

}  // extern "C"
