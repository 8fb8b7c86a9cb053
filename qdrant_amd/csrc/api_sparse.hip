// api_sparse.hip — the C-ABI of include/qdrant_amd.h, sparse vectors (QMX_DTYPE_SPARSE): segment and query creation, the sparse arms of
// score_points / score_internal / search_topk that api_query.hip and api_search.hip dispatch to, and the custom queries over sparse vectors
// (qmx_sparse_custom_*), and MMR re-ranking over them (qmx_sparse_mmr_select*).  The kernels are in sparse.hip and sparse_mmr.hip.
// (One of the api_*.hip translation units; what they share: api_internal.hpp.)
#include "api_internal.hpp"

// the segment: CSR rows sorted by (remapped) index, the dimension-major posting layout, and on the host the row offsets, the directory of the
// posting layout (distinct dimensions ascending, where each one's postings start) and the IndicesTracker map
struct SparseSeg {
    uint64_t nnz = 0;
    uint64_t n_nonempty = 0;                 // rows with at least one entry: InvertedIndex::vector_count
    uint64_t *d_off = nullptr;
    uint32_t *d_idx = nullptr;
    float *d_val = nullptr;
    uint64_t *d_post = nullptr;              // [nnz]: (f32 weight bits << 32) | point id, grouped by dimension, ids ascending (f32 index weights)
    uint32_t wtype = QMX_SPARSE_WEIGHT_F32;  // f16 / u8 index weights: the two arrays below instead of d_post
    uint32_t *d_post_id = nullptr;           // [nnz]
    void *d_post_w = nullptr;                // [nnz] u16 (f16 bits) / u8 (QuantizedU8 codes)
    std::vector<float> dir_min, dir_d256;    // [D]: QuantizedU8Params of every posting list (u8 only)
    std::vector<uint64_t> h_off;             // [n + 1]
    std::vector<uint32_t> dir_dims;          // [D]
    std::vector<uint64_t> dir_start;         // [D + 1]
    std::vector<uint32_t> map_keys, map_vals;   // sorted by key; empty = identity
    bool has_map = false;
    uint64_t longest_row = 0;                // entries of the longest row
    // a map under which ascending remapped id is NOT ascending original index: its remapped ids ascending and the original index of each, for the
    // pair scores of qmx_sparse_mmr_select (sparse_mmr.hip); null under no map or a monotone one
    uint32_t *d_inv_vals = nullptr, *d_inv_keys = nullptr;
    uint32_t n_inv = 0;
    ~SparseSeg() {
        dev_free(d_off); dev_free(d_idx); dev_free(d_val); dev_free(d_post); dev_free(d_post_id); dev_free(d_post_w);
        dev_free(d_inv_vals); dev_free(d_inv_keys);
    }
};

// a query batch: CSR lists sorted by (remapped) index, and the posting plan of every query (its dimensions that have postings, ascending)
struct SparseQuery {
    uint64_t *d_off = nullptr;
    uint32_t *d_idx = nullptr;
    float *d_val = nullptr;
    uint32_t *d_poff = nullptr;
    uint64_t *d_pstart = nullptr, *d_pend = nullptr;
    float *d_pw = nullptr;
    float *d_pmn = nullptr, *d_pd256 = nullptr;   // u8 index weights: the QuantizedU8Params of every plan entry's posting list
    uint64_t posting_entries = 0;            // sum over the queries of the posting lengths of their dimensions
    // the custom queries (SparseCustomQueryScorer) sum each example in ascending ORIGINAL index order: the lists (remapped ids, weights) and the
    // posting plan once more in that order, under the same offsets.  Without a map they ARE the arrays above (not owned twice).
    uint32_t *d_oidx = nullptr;
    float *d_oval = nullptr;
    uint64_t *d_opstart = nullptr, *d_opend = nullptr;
    float *d_opw = nullptr;
    bool own_original = false;
    bool internal = false;                   // made by qmx_query_create_internal: stored rows, whose original order is not known
    std::vector<uint64_t> h_entries;         // [nq]: posting entries of each query
    uint64_t longest = 0;                    // entries of the longest list
    ~SparseQuery() {
        dev_free(d_off); dev_free(d_idx); dev_free(d_val); dev_free(d_poff); dev_free(d_pstart); dev_free(d_pend); dev_free(d_pw);
        dev_free(d_pmn); dev_free(d_pd256);
        if (!own_original) return;
        dev_free(d_oidx); dev_free(d_oval); dev_free(d_opstart); dev_free(d_opend); dev_free(d_opw);
    }
};

static SparseRows rows_of(const qmx_segment *s) {
    const SparseSeg *sp = s->sparse;
    return SparseRows{sp->d_off, sp->d_idx, sp->d_val, s->n};
}
static SparseQueries queries_of(const qmx_query *q) {
    const SparseQuery *sq = q->sparse;
    return SparseQueries{sq->d_off, sq->d_idx, sq->d_val};
}

// what the destructors of qmx_segment / qmx_query call: the structs above are complete in this file only
void sparse_delete(SparseSeg *sp) { delete sp; }
void sparse_delete(SparseQuery *sq) { delete sq; }

// (index, value) pairs of one vector sorted by index; false on a duplicate index (validate_sparse_vector_impl, sparse_vector.rs:302-323)
static bool sort_pairs(std::vector<std::pair<uint32_t, float>> &v) {
    std::sort(v.begin(), v.end(), [](const std::pair<uint32_t, float> &a, const std::pair<uint32_t, float> &b) { return a.first < b.first; });
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i - 1].first == v[i].first) return false;
    return true;
}

// the posting plan of lists `idx` / `val` under offsets `off`: per list, its dimensions that have postings, in the list's order
static void posting_plan(const SparseSeg *sp, uint32_t nq, const std::vector<uint64_t> &off, const std::vector<uint32_t> &idx, const std::vector<float> &val,
                         std::vector<uint32_t> &poff, std::vector<uint64_t> &pstart, std::vector<uint64_t> &pend, std::vector<float> &pw,
                         std::vector<uint64_t> *entries, std::vector<float> *pmn = nullptr, std::vector<float> *pd256 = nullptr) {
    poff.assign(nq + 1, 0);
    for (uint32_t qi = 0; qi < nq; ++qi) {
        uint64_t sum = 0;
        for (uint64_t k = off[qi]; k < off[qi + 1]; ++k) {
            auto it = std::lower_bound(sp->dir_dims.begin(), sp->dir_dims.end(), idx[k]);
            if (it == sp->dir_dims.end() || *it != idx[k]) continue;      // no stored point has this dimension
            const size_t d = (size_t)(it - sp->dir_dims.begin());
            pstart.push_back(sp->dir_start[d]);
            pend.push_back(sp->dir_start[d + 1]);
            pw.push_back(val[k]);
            if (pmn) {
                pmn->push_back(sp->dir_min[d]);
                pd256->push_back(sp->dir_d256[d]);
            }
            sum += sp->dir_start[d + 1] - sp->dir_start[d];
        }
        poff[qi + 1] = (uint32_t)pstart.size();
        if (entries) entries->push_back(sum);
    }
}

// the batch's device arrays from host CSR lists that are sorted and remapped already, and the posting plan from the segment's directory.
// oidx / oval: the same lists (remapped ids, weights) in ascending original index order, or null where that is the order of idx / val
static int32_t query_finish(qmx_query *q, const std::vector<uint64_t> &off, const std::vector<uint32_t> &idx, const std::vector<float> &val,
                            const std::vector<uint32_t> *oidx = nullptr, const std::vector<float> *oval = nullptr) {
    const SparseSeg *sp = q->seg->sparse;
    SparseQuery *sq = q->sparse;
    std::vector<uint32_t> poff;
    std::vector<uint64_t> pstart, pend;
    std::vector<float> pw, pmn, pd256;
    const bool u8 = sp->wtype == QMX_SPARSE_WEIGHT_U8;
    posting_plan(sp, q->nq, off, idx, val, poff, pstart, pend, pw, &sq->h_entries, u8 ? &pmn : nullptr, u8 ? &pd256 : nullptr);
    for (uint64_t e : sq->h_entries) sq->posting_entries += e;
    for (uint32_t qi = 0; qi < q->nq; ++qi) sq->longest = std::max(sq->longest, off[qi + 1] - off[qi]);
    QMX_TRY(dev_upload(&sq->d_off, off.data(), off.size()));
    QMX_TRY(dev_upload(&sq->d_idx, idx.data(), idx.size()));
    QMX_TRY(dev_upload(&sq->d_val, val.data(), val.size()));
    QMX_TRY(dev_upload(&sq->d_poff, poff.data(), poff.size()));
    QMX_TRY(dev_upload(&sq->d_pstart, pstart.data(), pstart.size()));
    QMX_TRY(dev_upload(&sq->d_pend, pend.data(), pend.size()));
    QMX_TRY(dev_upload(&sq->d_pw, pw.data(), pw.size()));
    if (u8) {
        QMX_TRY(dev_upload(&sq->d_pmn, pmn.data(), pmn.size()));
        QMX_TRY(dev_upload(&sq->d_pd256, pd256.data(), pd256.size()));
    }
    if (!oidx) {
        sq->d_oidx = sq->d_idx;
        sq->d_oval = sq->d_val;
        sq->d_opstart = sq->d_pstart;
        sq->d_opend = sq->d_pend;
        sq->d_opw = sq->d_pw;
        return QMX_OK;
    }
    // (the same dimensions in another order: the plan's offsets are those above)
    std::vector<uint32_t> opoff;
    std::vector<uint64_t> opstart, opend;
    std::vector<float> opw;
    posting_plan(sp, q->nq, off, *oidx, *oval, opoff, opstart, opend, opw, nullptr);
    sq->own_original = true;
    QMX_TRY(dev_upload(&sq->d_oidx, oidx->data(), oidx->size()));
    QMX_TRY(dev_upload(&sq->d_oval, oval->data(), oval->size()));
    QMX_TRY(dev_upload(&sq->d_opstart, opstart.data(), opstart.size()));
    QMX_TRY(dev_upload(&sq->d_opend, opend.data(), opend.size()));
    QMX_TRY(dev_upload(&sq->d_opw, opw.data(), opw.size()));
    return QMX_OK;
}

static int32_t sparse_query_alloc(const qmx_segment *seg, uint32_t nq, qmx_query **out) {
    qmx_query *q = new (std::nothrow) qmx_query();
    QMX_REQUIRE(q, QMX_ERR_OUT_OF_MEMORY, "host allocation failed");
    q->seg = seg;
    q->device = seg->device;
    q->nq = nq;
    q->nq_padded = nq;
    q->sparse = new (std::nothrow) SparseQuery();
    hipError_t e = q->sparse ? hipStreamCreateWithFlags(&q->own_stream, hipStreamNonBlocking) : hipErrorOutOfMemory;
    if (e == hipSuccess) {
        q->stream = q->own_stream;
        e = hipMalloc((void **)&q->d_err, sizeof(int));
    }
    if (e == hipSuccess) e = hipMemset(q->d_err, 0, sizeof(int));
    if (e != hipSuccess) {
        const int32_t rc = hip_status(e, "sparse query allocation", __FILE__, __LINE__);
        qmx_query_destroy(q);
        return rc;
    }
    *out = q;
    return QMX_OK;
}

// ---------------------------------------------------------------------------------------------
// the sparse arms of the shared entry points
// ---------------------------------------------------------------------------------------------
int32_t sparse_query_create_internal(const qmx_segment *seg, const uint32_t *point_ids, uint32_t nq, qmx_query **out) {
    const SparseSeg *sp = seg->sparse;
    std::vector<uint32_t> ids(nq);
    if (nq) QMX_HIP(hipMemcpy(ids.data(), point_ids, (size_t)nq * 4, hipMemcpyDefault));
    std::vector<uint64_t> off(nq + 1, 0);
    for (uint32_t i = 0; i < nq; ++i) {
        QMX_REQUIRE(ids[i] < seg->n, QMX_ERR_OUT_OF_BOUNDS, "point offset %u out of range for this segment (the reference panics here)", ids[i]);
        off[i + 1] = off[i] + sp->h_off[ids[i] + 1] - sp->h_off[ids[i]];
    }
    // the stored rows ARE the queries (FilteredScorer::new_internal): already sorted and remapped
    std::vector<uint32_t> idx(off[nq]);
    std::vector<float> val(off[nq]);
    for (uint32_t i = 0; i < nq; ++i) {
        const uint64_t len = off[i + 1] - off[i], src = sp->h_off[ids[i]];
        if (!len) continue;
        QMX_HIP(hipMemcpy(idx.data() + off[i], sp->d_idx + src, len * 4, hipMemcpyDeviceToHost));
        QMX_HIP(hipMemcpy(val.data() + off[i], sp->d_val + src, len * 4, hipMemcpyDeviceToHost));
    }
    qmx_query *q = nullptr;
    QMX_TRY(sparse_query_alloc(seg, nq, &q));
    q->sparse->internal = true;
    const int32_t rc = query_finish(q, off, idx, val);
    if (rc != QMX_OK) {
        qmx_query_destroy(q);
        return rc;
    }
    *out = q;
    return QMX_OK;
}

int32_t sparse_score_matrix(const qmx_query *q, uint32_t tile0, uint32_t nq_tile, const uint32_t *d_ids, uint64_t n, float *d_scores, uint64_t stride) {
    QMX_REQUIRE(q->sparse, QMX_ERR_NOT_SUPPORTED, "a sparse segment is scored with a sparse query batch (qmx_sparse_query_create)");
    QMX_TRY(launch_sparse_score_matrix(q->stream, rows_of(q->seg), queries_of(q), tile0, nq_tile, d_ids, n, d_scores, stride, q->d_err));
    const_cast<qmx_query *>(q)->last_kernel = last_noted_kernel();
    return QMX_OK;
}

int32_t sparse_score_pairs(qmx_query *q, const PairSel &sel, const uint32_t *d_ids, uint64_t n_items, float *d_scores) {
    QMX_REQUIRE(q->sparse, QMX_ERR_NOT_SUPPORTED, "a sparse segment is scored with a sparse query batch (qmx_sparse_query_create)");
    QMX_TRY(launch_sparse_score_pairs(q->stream, rows_of(q->seg), queries_of(q), sel, d_ids, n_items, d_scores, q->d_err));
    q->last_kernel = last_noted_kernel();
    return QMX_OK;
}

int32_t sparse_score_internal(const qmx_segment *seg, const uint32_t *a_ids, const uint32_t *b_ids, uint32_t n, float *out) {
    QMX_HIP(hipSetDevice(seg->device));
    Staging st;
    DevBuf be;
    const uint32_t *d_a = nullptr, *d_b = nullptr;
    float *d_out = nullptr;
    QMX_TRY(st.in(a_ids, (size_t)n * 4, &d_a));
    QMX_TRY(st.in(b_ids, (size_t)n * 4, &d_b));
    QMX_TRY(st.out(out, (size_t)n * 4, &d_out));
    QMX_TRY(be.reserve(4));
    QMX_HIP(hipMemset(be.p, 0, 4));
    QMX_TRY(launch_sparse_score_internal(nullptr, rows_of(seg), d_a, d_b, n, d_out, (int *)be.p));
    int flag = 0;
    QMX_HIP(hipMemcpy(&flag, be.p, 4, hipMemcpyDeviceToHost));
    QMX_TRY(st.back());
    QMX_REQUIRE(!flag, QMX_ERR_OUT_OF_BOUNDS, "point offset out of range for this segment");
    return QMX_OK;
}

// Nearest: the posting top-k over every point (sparse_topk_postings_kernel), or plain_search over an id list (sparse_topk_ids_kernel); over f16 / u8
// index weights their counterparts on the two-array layout (sparse_topk_postings_q_kernel, sparse_topk_ids_q_kernel).  All write
// one key list of `top` (<= 64) per work-group and query, merged by launch_merge_keys.  top > 64 runs in passes of 64, each below the last key of
// the pass before.  Queries go in tiles of 128 (the key lists of a tile: lists x 128 x 64 keys).
int32_t sparse_search_enqueue(qmx_query *q, uint32_t top, const uint32_t *d_ids, uint64_t n_ids, qmx_scored_point *d_out, uint32_t *d_counts,
                              const volatile uint8_t *is_stopped, qmx_counters *counters, bool timed) {
    const qmx_segment *s = q->seg;
    QMX_REQUIRE(q->sparse, QMX_ERR_NOT_SUPPORTED, "a sparse segment is searched with a sparse query batch (qmx_sparse_query_create)");
    const SparseQuery *sq = q->sparse;
    DeletedView del = s->deleted_view();
    if (q->has_filter) {
        del.allowed = (const uint64_t *)q->filter.p;
        del.n_allowed_bits = q->n_filter_bits;
    }
    const uint64_t n_scan = s->scan_rows();
    const uint32_t n_lists_max = d_ids ? sparse_ids_lists(n_ids) : (uint32_t)((n_scan + sparse_tile_ids() - 1) / sparse_tile_ids());
    q->last_counters = qmx_counters{};
    q->last_split = false;
    if (n_lists_max == 0) {      // no rows: every list is empty
        QMX_HIP(hipMemsetAsync(d_counts, 0, (size_t)q->nq * 4, q->stream));
        if (counters) *counters = q->last_counters;
        return QMX_OK;
    }
    const uint32_t QT = 128;
    const uint32_t ptop_max = std::min<uint32_t>(top, MAX_TOP_FAST);
    const uint32_t n_pass = (top + MAX_TOP_FAST - 1) / MAX_TOP_FAST;
    QMX_TRY(q->partial.reserve((size_t)n_lists_max * std::min<uint32_t>(q->nq, QT) * ptop_max * sizeof(uint64_t)));
    if (n_pass > 1) QMX_TRY(q->bounds.reserve((size_t)QT * sizeof(uint64_t)));
    const SparsePlan plan{sq->d_poff, sq->d_pstart, sq->d_pend, sq->d_pw};
    const SparseSeg *sp = s->sparse;
    const bool quantized = sp->wtype != QMX_SPARSE_WEIGHT_F32;
    const SparsePlanQ plan_q{sq->d_poff, sq->d_pstart, sq->d_pend, sq->d_pw, sq->d_pmn, sq->d_pd256};
    const SparsePostQ post_q{sp->d_post_id, sp->d_post_w, sp->wtype};
    uint32_t launches = 0;
    for (uint32_t tile0 = 0; tile0 < q->nq; tile0 += QT) {
        const uint32_t nq_tile = std::min<uint32_t>(QT, q->nq - tile0);
        for (uint32_t pass = 0; pass < n_pass; ++pass) {
            QMX_CHECK_CANCELLED(is_stopped);
            const uint32_t off = pass * MAX_TOP_FAST;
            const uint32_t ptop = std::min<uint32_t>(MAX_TOP_FAST, top - off);
            const uint64_t *bound = pass ? (const uint64_t *)q->bounds.p : nullptr;
            uint32_t n_lists = 0;
            size_t slot = 0;
            if (timed) QMX_TRY(timing_begin(q, &slot));
            if (quantized && d_ids)
                QMX_TRY(launch_sparse_topk_ids_q(q->stream, post_q, plan_q, tile0, nq_tile, d_ids, n_ids, s->n, del, ptop, bound, (uint64_t *)q->partial.p,
                                                 &n_lists));
            else if (quantized)
                QMX_TRY(launch_sparse_topk_postings_q(q->stream, post_q, plan_q, tile0, nq_tile, n_scan, del, ptop, bound, (uint64_t *)q->partial.p, &n_lists));
            else if (d_ids)
                QMX_TRY(launch_sparse_topk_ids(q->stream, rows_of(s), queries_of(q), tile0, nq_tile, d_ids, n_ids, del, ptop, bound, (uint64_t *)q->partial.p,
                                               &n_lists));
            else
                QMX_TRY(launch_sparse_topk_postings(q->stream, s->sparse->d_post, plan, tile0, nq_tile, n_scan, del, ptop, bound, (uint64_t *)q->partial.p,
                                                    &n_lists));
            q->last_kernel = last_noted_kernel();
            if (timed) QMX_TRY(timing_end(q, slot));
            QMX_TRY(launch_merge_keys(q->stream, (const uint64_t *)q->partial.p, n_lists, nq_tile, nq_tile, ptop, d_out + (size_t)tile0 * top,
                                      d_counts + tile0, top, off, n_pass > 1 ? (uint64_t *)q->bounds.p : nullptr));
            launches += 2;
        }
    }
    qmx_counters &c = q->last_counters;
    const uint64_t entries = d_ids ? (uint64_t)q->nq * n_ids : sq->posting_entries;
    c.vectors_scored = entries * n_pass;
    // posting entries (id, weight): 8 / 6 / 5 bytes each; the id-list paths read rows, or probe postings, of unknown length
    c.bytes_read = d_ids ? 0 : entries * (sp->wtype == QMX_SPARSE_WEIGHT_U8 ? 5 : sp->wtype == QMX_SPARSE_WEIGHT_F16 ? 6 : 8) * n_pass;
    c.kernel_launches = launches;
    if (counters) *counters = c;
    return QMX_OK;
}

extern "C" {

// the device arrays of a new sparse segment `s` from its descriptor: rows (remapped and sorted), the posting layout and its directory
static int32_t sparse_segment_build(qmx_segment *s, const qmx_sparse_segment_desc *d, std::vector<uint64_t> &&h_off) {
    SparseSeg *sp = s->sparse;
    QMX_REQUIRE(sp, QMX_ERR_OUT_OF_MEMORY, "host allocation failed");
    const uint64_t nnz = h_off[d->n];
    sp->nnz = nnz;
    sp->h_off = std::move(h_off);
    for (uint64_t r = 0; r < d->n; ++r) {
        sp->n_nonempty += sp->h_off[r + 1] > sp->h_off[r];
        sp->longest_row = std::max(sp->longest_row, sp->h_off[r + 1] - sp->h_off[r]);
    }
    QMX_TRY(dev_upload(&sp->d_off, sp->h_off.data(), sp->h_off.size()));
    QMX_TRY(dev_upload(&sp->d_idx, d->indices, nnz));
    QMX_TRY(dev_upload(&sp->d_val, d->values, nnz));
    DevBuf flag, keys, vals, dims, counts_dev, dir, mn, d256;
    QMX_TRY(flag.reserve(4));
    uint32_t *d_flag = (uint32_t *)flag.p;
    QMX_HIP(hipMemset(d_flag, 0, 4));
    if (d->map_keys) {      // IndicesTracker: every stored index is remapped, then every row re-sorted
        std::vector<std::pair<uint32_t, uint32_t>> m(d->n_map);
        std::vector<uint32_t> k(d->n_map), v(d->n_map);
        if (d->n_map) {
            QMX_HIP(hipMemcpy(k.data(), d->map_keys, d->n_map * 4, hipMemcpyDefault));
            QMX_HIP(hipMemcpy(v.data(), d->map_values, d->n_map * 4, hipMemcpyDefault));
        }
        for (uint64_t i = 0; i < d->n_map; ++i) m[i] = {k[i], v[i]};
        std::sort(m.begin(), m.end());
        bool dup = false;
        for (uint64_t i = 1; i < d->n_map; ++i) dup = dup || m[i - 1].first == m[i].first;
        QMX_REQUIRE(!dup, QMX_ERR_BAD_ARG, "the dimension map holds a key twice");
        sp->has_map = true;
        for (auto &p : m) {
            sp->map_keys.push_back(p.first);
            sp->map_vals.push_back(p.second);
        }
        QMX_TRY(dev_upload(keys, sp->map_keys.data(), sp->map_keys.size()));
        QMX_TRY(dev_upload(vals, sp->map_vals.data(), sp->map_vals.size()));
        QMX_TRY(launch_sparse_remap(nullptr, sp->d_idx, nnz, (const uint32_t *)keys.p, (const uint32_t *)vals.p, d->n_map, d_flag));
        uint32_t missing = 0;
        QMX_HIP(hipMemcpy(&missing, d_flag, 4, hipMemcpyDeviceToHost));
        QMX_REQUIRE(!missing, QMX_ERR_BAD_ARG, "a stored index is not in the dimension map");
        // the map by remapped id, kept where it changes the order (the first original index of a remapped id two of them share)
        bool monotone = true;
        for (size_t i = 1; i < sp->map_vals.size(); ++i) monotone = monotone && sp->map_vals[i - 1] < sp->map_vals[i];
        if (!monotone) {
            std::vector<std::pair<uint32_t, uint32_t>> inv;
            for (size_t i = 0; i < sp->map_keys.size(); ++i) inv.push_back({sp->map_vals[i], sp->map_keys[i]});
            std::sort(inv.begin(), inv.end());
            std::vector<uint32_t> iv, ik;
            for (size_t i = 0; i < inv.size(); ++i)
                if (i == 0 || inv[i].first != inv[i - 1].first) {
                    iv.push_back(inv[i].first);
                    ik.push_back(inv[i].second);
                }
            sp->n_inv = (uint32_t)iv.size();
            QMX_TRY(dev_upload(&sp->d_inv_vals, iv.data(), iv.size()));
            QMX_TRY(dev_upload(&sp->d_inv_keys, ik.data(), ik.size()));
        }
    }
    // sorted by index on the way in; duplicates refused
    QMX_TRY(launch_sparse_check_rows(nullptr, sp->d_off, sp->d_idx, s->n, d_flag));
    uint32_t flags = 0;
    QMX_HIP(hipMemcpy(&flags, d_flag, 4, hipMemcpyDeviceToHost));
    if (flags & 1u) {
        QMX_TRY(launch_sparse_sort_rows(nullptr, sp->d_off, sp->d_idx, sp->d_val, s->n));
        QMX_HIP(hipMemset(d_flag, 0, 4));
        QMX_TRY(launch_sparse_check_rows(nullptr, sp->d_off, sp->d_idx, s->n, d_flag));
        QMX_HIP(hipMemcpy(&flags, d_flag, 4, hipMemcpyDeviceToHost));
    }
    QMX_REQUIRE(!(flags & 2u), QMX_ERR_BAD_ARG, "a sparse vector holds an index twice");
    // the posting layout and its directory
    QMX_HIP(hipMalloc((void **)&sp->d_post, std::max<uint64_t>(nnz, 1) * 8));
    QMX_TRY(dims.reserve(std::max<uint64_t>(nnz, 1) * 4));
    QMX_TRY(counts_dev.reserve(std::max<uint64_t>(nnz, 1) * 4));
    QMX_TRY(sparse_build_postings(nullptr, sp->d_off, sp->d_idx, sp->d_val, s->n, nnz, sp->d_post, (uint32_t *)dims.p, (uint32_t *)counts_dev.p, d_flag));
    uint32_t n_dims = 0;
    QMX_HIP(hipMemcpy(&n_dims, d_flag, 4, hipMemcpyDeviceToHost));
    sp->dir_dims.resize(n_dims);
    std::vector<uint32_t> counts(n_dims);
    if (n_dims) {
        QMX_HIP(hipMemcpy(sp->dir_dims.data(), dims.p, (size_t)n_dims * 4, hipMemcpyDeviceToHost));
        QMX_HIP(hipMemcpy(counts.data(), counts_dev.p, (size_t)n_dims * 4, hipMemcpyDeviceToHost));
    }
    sp->dir_start.assign(n_dims + 1, 0);
    for (uint32_t i = 0; i < n_dims; ++i) sp->dir_start[i + 1] = sp->dir_start[i] + counts[i];
    sp->wtype = d->flags & QMX_SPARSE_WEIGHT_MASK;
    if (sp->wtype == QMX_SPARSE_WEIGHT_F32) return QMX_OK;
    // f16 / u8 index weights: the packed layout is encoded into (post_id, post_w) and freed - 8 B per entry become 6 B / 5 B.  The u8
    // parameters of every posting list stay on the host beside the directory.
    const bool u8 = sp->wtype == QMX_SPARSE_WEIGHT_U8;
    QMX_TRY(dev_upload(dir, sp->dir_start.data(), sp->dir_start.size()));
    QMX_HIP(hipMalloc((void **)&sp->d_post_id, std::max<uint64_t>(nnz, 1) * 4));
    QMX_HIP(hipMalloc(&sp->d_post_w, std::max<uint64_t>(nnz, 1) * (u8 ? 1 : 2)));
    float *d_mn = nullptr, *d_d256 = nullptr;
    if (u8) {
        QMX_TRY(mn.reserve(std::max<size_t>(n_dims, 1) * 4));
        QMX_TRY(d256.reserve(std::max<size_t>(n_dims, 1) * 4));
        d_mn = (float *)mn.p;
        d_d256 = (float *)d256.p;
        QMX_TRY(launch_sparse_post_params(nullptr, sp->d_post, (const uint64_t *)dir.p, n_dims, d_mn, d_d256));
    }
    QMX_TRY(launch_sparse_post_encode(nullptr, sp->d_post, (const uint64_t *)dir.p, n_dims, d_mn, d_d256, sp->wtype, sp->d_post_id, sp->d_post_w));
    if (u8) {
        sp->dir_min.resize(n_dims);
        sp->dir_d256.resize(n_dims);
        if (n_dims) {
            QMX_HIP(hipMemcpy(sp->dir_min.data(), d_mn, (size_t)n_dims * 4, hipMemcpyDeviceToHost));
            QMX_HIP(hipMemcpy(sp->dir_d256.data(), d_d256, (size_t)n_dims * 4, hipMemcpyDeviceToHost));
        }
    }
    QMX_HIP(hipDeviceSynchronize());
    dev_free(sp->d_post);
    return QMX_OK;
}

int32_t qmx_sparse_segment_create(const qmx_sparse_segment_desc *d, qmx_segment **out) {
    QMX_REQUIRE(d && out, QMX_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    QMX_REQUIRE(d->n <= 0xFFFFFFFFull, QMX_ERR_BAD_ARG, "PointOffsetType is u32: n=%llu too large", (unsigned long long)d->n);
    QMX_REQUIRE(d->offsets || d->n == 0, QMX_ERR_BAD_ARG, "offsets is NULL");
    QMX_REQUIRE((d->map_keys == nullptr) == (d->map_values == nullptr), QMX_ERR_BAD_ARG, "map_keys and map_values go together");
    QMX_REQUIRE((d->flags & ~QMX_SPARSE_WEIGHT_MASK) == 0 && d->flags <= QMX_SPARSE_WEIGHT_U8, QMX_ERR_BAD_ARG,
                "flags 0x%x: QMX_SPARSE_WEIGHT_F32 / _F16 / _U8 only", d->flags);
    hipDeviceProp_t prop;
    QMX_TRY(check_device(d->device_id, &prop));
    std::vector<uint64_t> h_off(d->n + 1, 0);
    if (d->offsets) QMX_HIP(hipMemcpy(h_off.data(), d->offsets, h_off.size() * 8, hipMemcpyDefault));
    QMX_REQUIRE(h_off[0] == 0, QMX_ERR_BAD_ARG, "offsets[0] must be 0");
    for (uint64_t i = 0; i < d->n; ++i)
        QMX_REQUIRE(h_off[i] <= h_off[i + 1], QMX_ERR_BAD_ARG, "offsets must be non-decreasing (row %llu)", (unsigned long long)i);
    const uint64_t nnz = h_off[d->n];
    QMX_REQUIRE(nnz == 0 || (d->indices && d->values), QMX_ERR_BAD_ARG, "indices / values are NULL");
    QMX_REQUIRE(nnz <= 0xFFFFFFFFull, QMX_ERR_NOT_SUPPORTED, "a sparse segment holds at most 2^32 - 1 non-zeros (got %llu)", (unsigned long long)nnz);

    qmx_segment *s = new (std::nothrow) qmx_segment();
    QMX_REQUIRE(s, QMX_ERR_OUT_OF_MEMORY, "host allocation failed");
    s->device = d->device_id;
    s->num_cus = prop.multiProcessorCount;
    s->dtype = QMX_DTYPE_SPARSE;
    s->distance = QMX_DISTANCE_DOT;
    s->n = d->n;
    s->sparse = new (std::nothrow) SparseSeg();
    const int32_t rc = sparse_segment_build(s, d, std::move(h_off));
    if (rc != QMX_OK) {
        qmx_segment_destroy(s);
        return rc;
    }
    *out = s;
    return QMX_OK;
}

int32_t qmx_sparse_query_create(const qmx_segment *seg, const uint64_t *offsets, const uint32_t *indices, const float *values, uint32_t nq, qmx_query **out) {
    QMX_REQUIRE(seg && out && (nq == 0 || offsets), QMX_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    QMX_REQUIRE(is_sparse(seg), QMX_ERR_NOT_SUPPORTED, "qmx_sparse_query_create needs a sparse segment (qmx_sparse_segment_create)");
    QMX_HIP(hipSetDevice(seg->device));
    const SparseSeg *sp = seg->sparse;
    std::vector<uint64_t> in_off(nq + 1, 0);
    if (nq) QMX_HIP(hipMemcpy(in_off.data(), offsets, in_off.size() * 8, hipMemcpyDefault));
    QMX_REQUIRE(in_off[0] == 0, QMX_ERR_BAD_ARG, "offsets[0] must be 0");
    for (uint32_t i = 0; i < nq; ++i) QMX_REQUIRE(in_off[i] <= in_off[i + 1], QMX_ERR_BAD_ARG, "offsets must be non-decreasing (query %u)", i);
    const uint64_t total = in_off[nq];
    QMX_REQUIRE(total == 0 || (indices && values), QMX_ERR_BAD_ARG, "indices / values are NULL");
    std::vector<uint32_t> in_idx(total);
    std::vector<float> in_val(total);
    if (total) {
        QMX_HIP(hipMemcpy(in_idx.data(), indices, total * 4, hipMemcpyDefault));
        QMX_HIP(hipMemcpy(in_val.data(), values, total * 4, hipMemcpyDefault));
    }
    std::vector<uint64_t> off(nq + 1, 0);
    std::vector<uint32_t> idx, oidx;
    std::vector<float> val, oval;
    std::vector<std::pair<uint32_t, float>> v;
    for (uint32_t qi = 0; qi < nq; ++qi) {
        v.clear();
        for (uint64_t k = in_off[qi]; k < in_off[qi + 1]; ++k) v.push_back({in_idx[k], in_val[k]});
        QMX_REQUIRE(sort_pairs(v), QMX_ERR_BAD_ARG, "query %u holds an index twice", qi);
        if (sp->has_map) {      // remap_vector: dimensions the tracker does not know are dropped, the rest re-sorted
            std::vector<std::pair<uint32_t, float>> r;
            for (auto &p : v) {
                auto it = std::lower_bound(sp->map_keys.begin(), sp->map_keys.end(), p.first);
                if (it != sp->map_keys.end() && *it == p.first) r.push_back({sp->map_vals[(size_t)(it - sp->map_keys.begin())], p.second});
            }
            for (auto &p : r) {      // still in ascending original index: the order of the custom queries' sums
                oidx.push_back(p.first);
                oval.push_back(p.second);
            }
            QMX_REQUIRE(sort_pairs(r), QMX_ERR_BAD_ARG, "query %u maps two indices to one", qi);
            v.swap(r);
        }
        for (auto &p : v) {
            idx.push_back(p.first);
            val.push_back(p.second);
        }
        off[qi + 1] = idx.size();
    }
    qmx_query *q = nullptr;
    QMX_TRY(sparse_query_alloc(seg, nq, &q));
    const int32_t rc = sp->has_map ? query_finish(q, off, idx, val, &oidx, &oval) : query_finish(q, off, idx, val);
    if (rc != QMX_OK) {
        qmx_query_destroy(q);
        return rc;
    }
    *out = q;
    return QMX_OK;
}

// fill_idf_statistics (sparse_vector_index/read_view/idf.rs:51-140)
int32_t qmx_sparse_idf_statistics(const qmx_segment *seg, const uint32_t *dims, uint32_t n, const uint64_t *corpus_words, uint64_t n_corpus_bits,
                                  uint64_t *df_out, uint64_t *n_docs_out) {
    QMX_REQUIRE(seg && n_docs_out && (n == 0 || (dims && df_out)), QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(is_sparse(seg), QMX_ERR_NOT_SUPPORTED, "qmx_sparse_idf_statistics needs a sparse segment (qmx_sparse_segment_create)");
    QMX_HIP(hipSetDevice(seg->device));
    const SparseSeg *sp = seg->sparse;
    // the posting range of every requested dimension: remap_index, then the directory; none = df 0
    std::vector<uint32_t> h_dims(n);
    if (n) QMX_HIP(hipMemcpy(h_dims.data(), dims, (size_t)n * 4, hipMemcpyDefault));
    std::vector<uint64_t> start(n, 0), end(n, 0);
    uint64_t longest = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t d = h_dims[i];
        if (sp->has_map) {
            auto it = std::lower_bound(sp->map_keys.begin(), sp->map_keys.end(), d);
            if (it == sp->map_keys.end() || *it != d) continue;
            d = sp->map_vals[(size_t)(it - sp->map_keys.begin())];
        }
        auto it = std::lower_bound(sp->dir_dims.begin(), sp->dir_dims.end(), d);
        if (it == sp->dir_dims.end() || *it != d) continue;
        const size_t k = (size_t)(it - sp->dir_dims.begin());
        start[i] = sp->dir_start[k];
        end[i] = sp->dir_start[k + 1];
        longest = std::max(longest, end[i] - start[i]);
    }
    if (!corpus_words) {      // global: whole posting lengths (deleted points included) and InvertedIndex::vector_count, the non-empty vectors
        for (uint32_t i = 0; i < n; ++i) df_out[i] = end[i] - start[i];
        *n_docs_out = sp->n_nonempty;
        return QMX_OK;
    }
    const uint64_t n_words = (n_corpus_bits + 63) / 64;
    DevBuf mask, ranges, cnt;
    QMX_TRY(mask.reserve(std::max<size_t>(n_words, 1) * 8));
    QMX_TRY(ranges.reserve(std::max<size_t>(n, 1) * 16));
    QMX_TRY(cnt.reserve(((size_t)n + 1) * 8));
    uint64_t *d_start = (uint64_t *)ranges.p, *d_end = d_start + n;
    unsigned long long *d_cnt = (unsigned long long *)cnt.p;
    if (n_words) QMX_HIP(hipMemcpy(mask.p, corpus_words, n_words * 8, hipMemcpyDefault));
    if (n) QMX_HIP(hipMemcpy(d_start, start.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    if (n) QMX_HIP(hipMemcpy(d_end, end.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    QMX_HIP(hipMemset(d_cnt, 0, ((size_t)n + 1) * 8));
    DeletedView del = seg->deleted_view();
    del.allowed = (const uint64_t *)mask.p;
    del.n_allowed_bits = n_corpus_bits;
    QMX_TRY(launch_sparse_idf_corpus(nullptr, sp->d_post, sp->d_post_id, d_start, d_end, n, longest, del, seg->scan_rows(), d_cnt, d_cnt + n));
    std::vector<unsigned long long> h_cnt((size_t)n + 1);
    QMX_HIP(hipMemcpy(h_cnt.data(), d_cnt, h_cnt.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) df_out[i] = h_cnt[i];
    *n_docs_out = h_cnt[n];
    return QMX_OK;
}

// VectorQueryContext::fancy_idf: f32 throughout, f32::ln = libm logf (computed here on the host: the device's logf rounds differently)
static float fancy_idf(float n, float df) { return logf((n - df + 0.5f) / (df + 0.5f) + 1.0f); }

int32_t qmx_sparse_query_create_idf(const qmx_segment *seg, const uint64_t *offsets, const uint32_t *indices, const float *values, uint32_t nq,
                                    const uint32_t *stat_dims, const uint64_t *stat_df, uint32_t n_stats, uint64_t n_docs, qmx_query **out) {
    QMX_REQUIRE(seg && out && (nq == 0 || offsets) && (n_stats == 0 || (stat_dims && stat_df)), QMX_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    QMX_REQUIRE(is_sparse(seg), QMX_ERR_NOT_SUPPORTED, "qmx_sparse_query_create_idf needs a sparse segment (qmx_sparse_segment_create)");
    QMX_HIP(hipSetDevice(seg->device));
    std::vector<uint64_t> off(nq + 1, 0);
    if (nq) QMX_HIP(hipMemcpy(off.data(), offsets, off.size() * 8, hipMemcpyDefault));
    QMX_REQUIRE(off[0] == 0, QMX_ERR_BAD_ARG, "offsets[0] must be 0");
    for (uint32_t i = 0; i < nq; ++i) QMX_REQUIRE(off[i] <= off[i + 1], QMX_ERR_BAD_ARG, "offsets must be non-decreasing (query %u)", i);
    const uint64_t total = off[nq];
    QMX_REQUIRE(total == 0 || (indices && values), QMX_ERR_BAD_ARG, "indices / values are NULL");
    std::vector<uint32_t> idx(total);
    std::vector<float> val(total);
    if (total) {
        QMX_HIP(hipMemcpy(idx.data(), indices, total * 4, hipMemcpyDefault));
        QMX_HIP(hipMemcpy(val.data(), values, total * 4, hipMemcpyDefault));
    }
    std::vector<std::pair<uint32_t, uint64_t>> stats(n_stats);
    for (uint32_t i = 0; i < n_stats; ++i) stats[i] = {stat_dims[i], stat_df[i]};
    std::sort(stats.begin(), stats.end());
    const float n = (float)n_docs;
    for (uint64_t k = 0; k < total; ++k) {      // remap_idf_weights: by ORIGINAL index, before any remap
        auto it = std::lower_bound(stats.begin(), stats.end(), std::make_pair(idx[k], (uint64_t)0));
        const uint64_t df = it != stats.end() && it->first == idx[k] ? it->second : 0;
        val[k] *= fancy_idf(n, (float)df);
    }
    return qmx_sparse_query_create(seg, off.data(), idx.data(), val.data(), nq, out);
}

// ---------------------------------------------------------------------------------------------
// custom queries over sparse vectors (SparseCustomQueryScorer; sparse_custom_*_kernel in sparse.hip)
// ---------------------------------------------------------------------------------------------
// the example batch of a sparse custom query: made by qmx_sparse_query_create over a sparse segment
static int32_t sparse_custom_check(const qmx_query *ex, const char *fn) {
    if (!is_sparse(ex) || !ex->sparse || ex->sparse->internal) {
        set_error("%s needs an example batch made by qmx_sparse_query_create over a sparse segment", fn);
        return QMX_ERR_NOT_SUPPORTED;
    }
    return QMX_OK;
}

// descriptors to the device; *n_examples_total = the examples of all queries, *entries = their posting entries
static int32_t sparse_custom_stage(qmx_query *ex, const qmx_custom_query *queries, uint32_t n_queries, uint64_t *n_examples_total, uint64_t *entries) {
    QMX_TRY(custom_validate(ex, queries, n_queries, ex->nq, nullptr));
    *n_examples_total = *entries = 0;
    for (uint32_t i = 0; i < n_queries; ++i) {
        const qmx_custom_query &c = queries[i];
        const uint32_t ne = c.kind <= QMX_CUSTOM_RECO_SUM_SCORES ? c.n_a + c.n_b : c.n_a + 2 * c.n_b;
        *n_examples_total += ne;
        for (uint32_t e = 0; e < ne; ++e) *entries += ex->sparse->h_entries[c.first + e];
    }
    QMX_TRY(ex->cq_desc.reserve((size_t)n_queries * sizeof(qmx_custom_query)));
    QMX_HIP(hipMemcpyAsync(ex->cq_desc.p, queries, (size_t)n_queries * sizeof(qmx_custom_query), hipMemcpyHostToDevice, ex->stream));
    return QMX_OK;
}

int32_t qmx_sparse_custom_score_points(qmx_query *ex, const qmx_custom_query *queries, uint32_t n_queries, const uint32_t *ids, uint32_t n, float *scores) {
    QMX_REQUIRE(ex && (n_queries == 0 || queries) && (n == 0 || (ids && scores)), QMX_ERR_BAD_ARG, "NULL argument");
    QMX_TRY(sparse_custom_check(ex, __func__));
    QMX_HIP(hipSetDevice(ex->device));
    if (n == 0 || n_queries == 0) return QMX_OK;
    const SparseQuery *sq = ex->sparse;
    uint64_t n_examples = 0, entries = 0;
    QMX_TRY(sparse_custom_stage(ex, queries, n_queries, &n_examples, &entries));
    const void *d_ids = nullptr;
    QMX_TRY(stage_in(ex, ex->ids, ids, (size_t)n * 4, &d_ids));
    QMX_TRY(ex->cq_scores.reserve((size_t)n_queries * n * 4));
    QMX_TRY(launch_sparse_custom_score(ex->stream, rows_of(ex->seg), SparseQueries{sq->d_off, sq->d_oidx, sq->d_oval}, (const qmx_custom_query *)ex->cq_desc.p,
                                       (const float *)ex->cq_coefs.p, n_queries, (const uint32_t *)d_ids, n, (float *)ex->cq_scores.p, ex->d_err));
    ex->last_kernel = last_noted_kernel();
    QMX_TRY(copy_out(ex->stream, scores, ex->cq_scores.p, (size_t)n_queries * n * 4));
    return check_err_flag(ex);      // synchronises (the caller's descriptors may go away)
}

// search_scored: the fused posting scan over every point (sparse_custom_topk_postings_kernel) or the id list (sparse_custom_topk_ids_kernel); key lists,
// passes of 64 and query tiles of 128 as sparse_search_enqueue
int32_t qmx_sparse_custom_search_topk(qmx_query *ex, const qmx_custom_query *queries, uint32_t n_queries, uint32_t top, const uint32_t *ids, uint64_t n_ids,
                                      qmx_scored_point *out, uint32_t *out_counts, const volatile uint8_t *is_stopped, qmx_counters *counters) {
    QMX_REQUIRE(ex && (n_queries == 0 || queries) && out && out_counts, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_TRY(sparse_custom_check(ex, __func__));
    QMX_REFUSE_FILTERS(ex);
    QMX_REQUIRE(top >= 1 && top <= MAX_TOP, QMX_ERR_NOT_SUPPORTED, "top %u not in 1..%u", top, MAX_TOP);
    QMX_HIP(hipSetDevice(ex->device));
    if (counters) memset(counters, 0, sizeof(*counters));
    if (n_queries == 0) return QMX_OK;
    const qmx_segment *s = ex->seg;
    const SparseQuery *sq = ex->sparse;
    uint64_t n_examples = 0, entries = 0;
    QMX_TRY(sparse_custom_stage(ex, queries, n_queries, &n_examples, &entries));
    const void *d_ids = nullptr;
    if (ids && n_ids) QMX_TRY(stage_in(ex, ex->ids, ids, (size_t)n_ids * 4, &d_ids));
    const bool out_dev = is_device_ptr(out), cnt_dev = is_device_ptr(out_counts);
    qmx_scored_point *d_out = out;
    uint32_t *d_counts = out_counts;
    if (!out_dev) { QMX_TRY(ex->out.reserve((size_t)n_queries * top * sizeof(qmx_scored_point))); d_out = (qmx_scored_point *)ex->out.p; }
    if (!cnt_dev) { QMX_TRY(ex->counts.reserve((size_t)n_queries * 4)); d_counts = (uint32_t *)ex->counts.p; }
    DeletedView del = s->deleted_view();
    if (ex->has_filter) {
        del.allowed = (const uint64_t *)ex->filter.p;
        del.n_allowed_bits = ex->n_filter_bits;
    }
    const uint64_t n_scan = s->scan_rows();
    // over f16 / u8 index weights no f32 postings exist and the custom scorer reads the vector storage: the full scan is the row kernel over the
    // implicit identity id list
    const bool rows_scan = !ids && s->sparse->wtype != QMX_SPARSE_WEIGHT_F32;
    const uint32_t n_lists_max = ids        ? (n_ids ? sparse_ids_lists(n_ids) : 0)
                                 : rows_scan ? (n_scan ? sparse_ids_lists(n_scan) : 0)
                                             : (uint32_t)((n_scan + sparse_custom_tile_ids() - 1) / sparse_custom_tile_ids());
    const bool timed = ex->timing || (s->flags & QMX_SEG_TIME_KERNELS) != 0;
    ex->last_counters = qmx_counters{};
    ex->last_split = false;
    uint32_t launches = 0;
    const uint32_t n_pass = (top + MAX_TOP_FAST - 1) / MAX_TOP_FAST;
    if (n_lists_max == 0) {      // no candidates: every list is empty
        QMX_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_queries * 4, ex->stream));
    } else {
        const uint32_t QT = 128;
        const uint32_t ptop_max = std::min<uint32_t>(top, MAX_TOP_FAST);
        QMX_TRY(ex->partial.reserve((size_t)n_lists_max * std::min<uint32_t>(n_queries, QT) * ptop_max * sizeof(uint64_t)));
        if (n_pass > 1) QMX_TRY(ex->bounds.reserve((size_t)QT * sizeof(uint64_t)));
        const SparsePlan plan{sq->d_poff, sq->d_opstart, sq->d_opend, sq->d_opw};
        const SparseQueries exq{sq->d_off, sq->d_oidx, sq->d_oval};
        const qmx_custom_query *d_desc = (const qmx_custom_query *)ex->cq_desc.p;
        const float *d_coefs = (const float *)ex->cq_coefs.p;
        for (uint32_t tile0 = 0; tile0 < n_queries; tile0 += QT) {
            const uint32_t nq_tile = std::min<uint32_t>(QT, n_queries - tile0);
            for (uint32_t pass = 0; pass < n_pass; ++pass) {
                if (is_stopped && *is_stopped) {
                    QMX_HIP(hipStreamSynchronize(ex->stream));      // (the caller's descriptors may go away)
                    set_error("search cancelled");
                    return QMX_ERR_CANCELLED;
                }
                const uint32_t off = pass * MAX_TOP_FAST;
                const uint32_t ptop = std::min<uint32_t>(MAX_TOP_FAST, top - off);
                const uint64_t *bound = pass ? (const uint64_t *)ex->bounds.p : nullptr;
                uint32_t n_lists = 0;
                size_t slot = 0;
                if (timed) QMX_TRY(timing_begin(ex, &slot));
                if (d_ids || rows_scan)
                    QMX_TRY(launch_sparse_custom_topk_ids(ex->stream, rows_of(s), exq, d_desc, d_coefs, tile0, nq_tile, (const uint32_t *)d_ids,
                                                          d_ids ? n_ids : n_scan, del, ptop, bound, (uint64_t *)ex->partial.p, &n_lists));
                else
                    QMX_TRY(launch_sparse_custom_topk_postings(ex->stream, s->sparse->d_post, plan, d_desc, d_coefs, tile0, nq_tile, n_scan, del, ptop, bound,
                                                               (uint64_t *)ex->partial.p, &n_lists));
                ex->last_kernel = last_noted_kernel();
                if (timed) QMX_TRY(timing_end(ex, slot));
                QMX_TRY(launch_merge_keys(ex->stream, (const uint64_t *)ex->partial.p, n_lists, nq_tile, nq_tile, ptop, d_out + (size_t)tile0 * top,
                                          d_counts + tile0, top, off, n_pass > 1 ? (uint64_t *)ex->bounds.p : nullptr));
                launches += 2;
            }
        }
    }
    qmx_counters &c = ex->last_counters;
    c.vectors_scored = (d_ids ? n_examples * n_ids : rows_scan ? n_examples * n_scan : entries) * n_pass;
    c.bytes_read = d_ids || rows_scan ? 0 : entries * 8 * n_pass;      // posting entries (id, weight) of every example; the id-list path reads rows of unknown length
    c.kernel_launches = launches;
    if (!out_dev) QMX_TRY(copy_out(ex->stream, out, d_out, (size_t)n_queries * top * sizeof(qmx_scored_point)));
    if (!cnt_dev) QMX_TRY(copy_out(ex->stream, out_counts, d_counts, (size_t)n_queries * 4));
    QMX_TRY(check_err_flag(ex));      // synchronises
    if (counters) *counters = c;
    if (timed) {
        const float before = ex->timing_ms;
        QMX_TRY(timing_fold(ex));
        if (counters) counters->kernel_ms = ex->timing_ms - before;
    }
    return QMX_OK;
}

// ---------------------------------------------------------------------------------------------
// MMR re-ranking over sparse vectors (sparse_mmr_select_kernel in sparse_mmr.hip)
// ---------------------------------------------------------------------------------------------
static int32_t sparse_mmr_check(const qmx_query *q, const void *cand, const void *counts, uint32_t stride, uint32_t limit, const void *out, const void *oc,
                                const char *fn) {
    QMX_REQUIRE(q && out && oc && (q->nq == 0 || (counts && (stride == 0 || cand))), QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(is_sparse(q) && q->sparse, QMX_ERR_BAD_ARG, "%s needs a batch made by qmx_sparse_query_create over a sparse segment (dense segments: qmx_mmr_select)", fn);
    // a batch of stored rows carries no original order under a map: the status of the sparse custom calls
    QMX_REQUIRE(!(q->sparse->internal && q->seg->sparse->has_map), QMX_ERR_NOT_SUPPORTED,
                "%s over a mapped segment needs a batch made by qmx_sparse_query_create (stored rows have lost their original order)", fn);
    QMX_REQUIRE(limit >= 1, QMX_ERR_BAD_ARG, "limit must be > 0");
    QMX_REQUIRE(limit <= MAX_TOP, QMX_ERR_NOT_SUPPORTED, "limit %u > %u", limit, MAX_TOP);
    QMX_REQUIRE(stride <= MMR_MAX_CANDIDATES, QMX_ERR_NOT_SUPPORTED, "MMR over %u candidates per request (at most %u)", stride, MMR_MAX_CANDIDATES);
    return QMX_OK;
}

static int32_t sparse_mmr_enqueue(qmx_query *q, const qmx_scored_point *d_cand, const uint32_t *d_counts, uint32_t stride, float lambda, uint32_t limit,
                                  qmx_scored_point *d_out, uint32_t *d_oc) {
    const SparseSeg *sp = q->seg->sparse;
    const SparseQuery *sq = q->sparse;
    SparseMmrArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = rows_of(q->seg);
    a.qs = SparseQueries{sq->d_off, sq->d_oidx, sq->d_oval};
    a.inv_vals = sp->d_inv_vals;
    a.inv_keys = sp->d_inv_keys;
    a.n_inv = sp->n_inv;
    a.stage_cap = (uint32_t)std::min<uint64_t>(SPARSE_MMR_STAGE_CAP, std::max(sp->longest_row, sq->longest));
    if (sp->d_inv_vals && sp->longest_row > SPARSE_MMR_STAGE_CAP) {      // a picked row that outgrows LDS is ranked into the request's slice
        a.spill_stride = sp->longest_row;
        QMX_TRY(q->mmr_spill.reserve((size_t)q->nq * 3 * a.spill_stride * 4));
        a.spill = (uint32_t *)q->mmr_spill.p;
    }
    a.cand = d_cand;
    a.counts = d_counts;
    a.stride = stride;
    a.lambda = lambda;
    a.limit = limit;
    a.out = d_out;
    a.out_counts = d_oc;
    a.err_flag = q->d_err;
    QMX_TRY(launch_sparse_mmr_select(q->stream, a, q->nq));
    q->last_kernel = last_noted_kernel();
    return QMX_OK;
}

int32_t qmx_sparse_mmr_select(qmx_query *q, const qmx_scored_point *candidates, const uint32_t *counts, uint32_t stride, float lambda, uint32_t limit,
                              qmx_scored_point *out, uint32_t *out_counts) {
    QMX_TRY(sparse_mmr_check(q, candidates, counts, stride, limit, out, out_counts, __func__));
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
    QMX_TRY(sparse_mmr_enqueue(q, (const qmx_scored_point *)d_cand, (const uint32_t *)d_counts, stride, lambda, limit, d_out, d_oc));
    if (!out_dev) QMX_TRY(copy_out(q->stream, out, d_out, (size_t)q->nq * limit * sizeof(qmx_scored_point)));
    if (!cnt_dev) QMX_TRY(copy_out(q->stream, out_counts, d_oc, (size_t)q->nq * 4));
    return check_err_flag(q);      // synchronises
}

int32_t qmx_sparse_mmr_select_async(qmx_query *q, const qmx_scored_point *candidates_dev, const uint32_t *counts_dev, uint32_t stride, float lambda,
                                    uint32_t limit, qmx_scored_point *out_dev, uint32_t *out_counts_dev) {
    QMX_TRY(sparse_mmr_check(q, candidates_dev, counts_dev, stride, limit, out_dev, out_counts_dev, __func__));
    QMX_HIP(hipSetDevice(q->device));
    if (q->nq == 0) return QMX_OK;
    QMX_REQUIRE(stride == 0 || is_device_ptr(candidates_dev), QMX_ERR_BAD_ARG, "async MMR needs device candidates");
    return sparse_mmr_enqueue(q, candidates_dev, counts_dev, stride, lambda, limit, out_dev, out_counts_dev);
}

}  // extern "C"
