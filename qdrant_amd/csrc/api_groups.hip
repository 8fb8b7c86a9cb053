// api_groups.hip — the C-ABI of include/qdrant_amd.h, grouped search: the key column (qmx_group_keys_*) and the driver of qmx_group_search over the
// kernels of groups.hip.  (One of the api_*.hip translation units; what they share: api_internal.hpp.)
#include "api_internal.hpp"
#include "group_logic.hpp"

struct qmx_group_keys {
    int device = 0;
    uint64_t n_points = 0, n_keys = 0;
    uint32_t n_distinct = 0;
    uint32_t *d_keys = nullptr;        // padded to a multiple of 4 entries with QMX_GROUP_NONE
    uint64_t *d_offsets = nullptr;     // CSR only
    qmx_group_keys() = default;
    qmx_group_keys(const qmx_group_keys &) = delete;
    qmx_group_keys &operator=(const qmx_group_keys &) = delete;
    ~qmx_group_keys() {
        dev_free(d_keys);
        dev_free(d_offsets);
    }
};

namespace {

constexpr uint64_t GROUP_MATRIX_BYTES = 1ull << 30;      // default budget of the fallback's score matrix (option group_matrix_bytes)

int32_t keys_create(qmx_group_keys *h, const uint32_t *keys, const uint64_t *offsets, uint32_t n_distinct) {
    const uint64_t n = h->n_points;
    h->n_keys = n;
    if (offsets) {
        QMX_TRY(dev_upload(&h->d_offsets, offsets, (size_t)(n + 1)));
        uint64_t ends[2] = {0, 0};      // first and last offset
        QMX_HIP(hipMemcpy(&ends[0], h->d_offsets, 8, hipMemcpyDeviceToHost));
        QMX_HIP(hipMemcpy(&ends[1], h->d_offsets + n, 8, hipMemcpyDeviceToHost));
        QMX_REQUIRE(ends[0] == 0, QMX_ERR_BAD_ARG, "group key offsets must start at 0 (got %llu)", (unsigned long long)ends[0]);
        QMX_REQUIRE(ends[1] <= (1ull << 36), QMX_ERR_NOT_SUPPORTED, "%llu group key values", (unsigned long long)ends[1]);
        h->n_keys = ends[1];
    }
    const uint64_t padded = (h->n_keys + 3) / 4 * 4 + 4;
    QMX_HIP(hipMalloc((void **)&h->d_keys, (size_t)padded * 4));
    QMX_HIP(hipMemset(h->d_keys, 0xFF, (size_t)padded * 4));
    if (h->n_keys) QMX_REQUIRE(keys, QMX_ERR_BAD_ARG, "NULL keys");
    // offsets that decrease are found below, before anything reads keys through them; the copy trusts only the LAST offset, as the caller's array must hold that many
    if (h->n_keys) QMX_HIP(hipMemcpy(h->d_keys, keys, (size_t)h->n_keys * 4, hipMemcpyDefault));
    DevBuf flag;
    uint32_t bad = 0;
    QMX_TRY(flag.reserve(4));
    QMX_HIP(hipMemset(flag.p, 0, 4));
    QMX_TRY(launch_group_keys_check(nullptr, h->d_keys, h->n_keys, n_distinct, h->d_offsets, n, (uint32_t *)flag.p));
    QMX_HIP(hipMemcpy(&bad, flag.p, 4, hipMemcpyDeviceToHost));
    QMX_REQUIRE(!(bad & 2u), QMX_ERR_BAD_ARG, "group key offsets must not decrease");
    QMX_REQUIRE(!(bad & 1u), QMX_ERR_OUT_OF_BOUNDS, "a group key is >= n_distinct (%u) and not QMX_GROUP_NONE", n_distinct);
    return QMX_OK;
}

// a possibly-host output: written on the device into `buf` at `*off`, copied back after the last kernel.  Not a Staging (dev_mem.hpp): the four
// outputs share ONE long-lived buffer of the query (grp_out, no allocation in steady state) and go back by stream-ordered copies on its stream.
struct GroupOut {
    void *host = nullptr, *dev = nullptr;
    size_t bytes = 0;
};
void *place_out(GroupOut &o, void *user, size_t bytes, char *stage, size_t *off) {
    o.bytes = bytes;
    if (is_device_ptr(user)) {
        o.dev = user;
        return user;
    }
    o.host = user;
    o.dev = stage + *off;
    *off += (bytes + 255) / 256 * 256;
    return o.dev;
}

int32_t zero_counts(qmx_query *q, uint32_t *out_n_groups) {
    if (q->nq == 0) return QMX_OK;
    if (is_device_ptr(out_n_groups)) {
        QMX_HIP(hipMemsetAsync(out_n_groups, 0, (size_t)q->nq * 4, q->stream));
        QMX_HIP(hipStreamSynchronize(q->stream));
    } else {
        for (uint32_t i = 0; i < q->nq; ++i) out_n_groups[i] = 0;
    }
    return QMX_OK;
}

}  // namespace

extern "C" {

int32_t qmx_group_keys_create(int32_t device_id, uint64_t n_points, const uint32_t *keys, const uint64_t *offsets, uint32_t n_distinct,
                              qmx_group_keys **out) {
    QMX_REQUIRE(out && (n_points == 0 || keys || offsets), QMX_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    QMX_REQUIRE(n_points <= 0xFFFFFFFEull, QMX_ERR_NOT_SUPPORTED, "point offsets are 32-bit (%llu points)", (unsigned long long)n_points);
    QMX_TRY(check_device(device_id, nullptr));
    qmx_group_keys *h = new (std::nothrow) qmx_group_keys();
    QMX_REQUIRE(h, QMX_ERR_OUT_OF_MEMORY, "host allocation failed");
    h->device = device_id;
    h->n_points = n_points;
    h->n_distinct = n_distinct;
    const int32_t rc = keys_create(h, keys, offsets, n_distinct);
    if (rc != QMX_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return QMX_OK;
}

int32_t qmx_group_keys_destroy(qmx_group_keys *keys) {
    if (!keys) return QMX_OK;
    (void)hipSetDevice(keys->device);
    delete keys;
    return QMX_OK;
}

int32_t qmx_group_search(qmx_query *q, const qmx_group_keys *keys, uint32_t limit, uint32_t group_size, const uint32_t *ids, uint64_t n_ids,
                         const float *score_threshold, uint32_t *out_group_keys, uint32_t *out_group_sizes, qmx_scored_point *out_hits,
                         uint32_t *out_n_groups, qmx_group_counters *counters) {
    QMX_REQUIRE(q && keys && out_n_groups, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REFUSE_SPARSE(q);
    QMX_REFUSE_FILTERS(q);
    if (counters) memset(counters, 0, sizeof(*counters));
    const qmx_segment *s = q->seg;
    QMX_REQUIRE(keys->device == s->device, QMX_ERR_BAD_ARG, "the group keys live on device %d, the segment on device %d", keys->device, s->device);
    QMX_REQUIRE(keys->n_points >= s->n, QMX_ERR_BAD_ARG, "group keys over %llu points, the segment holds %llu", (unsigned long long)keys->n_points,
                (unsigned long long)s->n);
    QMX_HIP(hipSetDevice(s->device));
    // the driver's State::Done for a zero limit or group size (driver.rs): no groups; so does an empty candidate list
    if (limit == 0 || group_size == 0 || (ids && n_ids == 0)) return zero_counts(q, out_n_groups);
    QMX_REQUIRE(limit <= GROUP_MAX_LIMIT, QMX_ERR_NOT_SUPPORTED, "limit %u > %u groups", limit, GROUP_MAX_LIMIT);
    QMX_REQUIRE((uint64_t)limit * group_size <= GROUP_MAX_HITS, QMX_ERR_NOT_SUPPORTED, "limit %u x group_size %u > %u hits per query", limit, group_size,
                GROUP_MAX_HITS);
    QMX_REQUIRE(out_group_keys && out_group_sizes && out_hits, QMX_ERR_BAD_ARG, "NULL output");
    const uint32_t nq = q->nq;
    if (nq == 0) return QMX_OK;
    const void *d_ids = nullptr;
    if (ids) QMX_TRY(stage_in(q, q->ids, ids, (size_t)n_ids * 4, &d_ids));
    const uint64_t n_cand = ids ? n_ids : s->scan_rows();
    hipStream_t st = q->stream;

    // ---- per-query state: slots, counters, bounds; pages ----
    const size_t slots = (size_t)nq * limit;
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) / 256 * 256;
        return at;
    };
    const size_t o_stats = take(sizeof(GroupStats)), o_nslots = take((size_t)nq * 4), o_nfull = take((size_t)nq * 4), o_zero_end = off;
    const size_t o_bound = take((size_t)nq * 8), o_key = take(slots * 4), o_cnt = take(slots * 4), o_hits = take(slots * group_size * 8),
                 o_list = take((size_t)nq * 4);
    QMX_TRY(q->grp_state.reserve(off));
    char *base = (char *)q->grp_state.p;
    GroupState gs;
    gs.stats = (GroupStats *)(base + o_stats);
    gs.n_slots = (uint32_t *)(base + o_nslots);
    gs.n_full = (uint32_t *)(base + o_nfull);
    gs.bound = (uint64_t *)(base + o_bound);
    gs.slot_key = (uint32_t *)(base + o_key);
    gs.slot_cnt = (uint32_t *)(base + o_cnt);
    gs.slot_hits = (uint64_t *)(base + o_hits);
    gs.limit = limit;
    gs.group_size = group_size;
    uint32_t *d_list = (uint32_t *)(base + o_list);
    QMX_HIP(hipMemsetAsync(base, 0, o_zero_end, st));
    QMX_HIP(hipMemsetAsync(gs.bound, 0xFF, (size_t)nq * 8, st));
    QMX_TRY(q->grp_pages.reserve((size_t)nq * GROUP_PAGE * sizeof(qmx_scored_point) + (size_t)nq * 4));
    qmx_scored_point *d_pages = (qmx_scored_point *)q->grp_pages.p;
    uint32_t *d_page_counts = (uint32_t *)(d_pages + (size_t)nq * GROUP_PAGE);
    GroupKeysDev gk{keys->d_keys, keys->d_offsets, keys->n_points};

    // ---- outputs: on the device, host buffers staged ----
    const size_t b_keys = slots * 4, b_hits = slots * group_size * sizeof(qmx_scored_point), b_n = (size_t)nq * 4;
    QMX_TRY(q->grp_out.reserve(2 * b_keys + b_hits + b_n + 4 * 256));
    GroupOut ok, os, oh, on;
    size_t out_off = 0;
    uint32_t *d_out_keys = (uint32_t *)place_out(ok, out_group_keys, b_keys, (char *)q->grp_out.p, &out_off);
    uint32_t *d_out_sizes = (uint32_t *)place_out(os, out_group_sizes, b_keys, (char *)q->grp_out.p, &out_off);
    qmx_scored_point *d_out_hits = (qmx_scored_point *)place_out(oh, out_hits, b_hits, (char *)q->grp_out.p, &out_off);
    uint32_t *d_out_n = (uint32_t *)place_out(on, out_n_groups, b_n, (char *)q->grp_out.p, &out_off);

    // ---- stage 0: the search as it is, 64 hits per query, on whichever path the dispatch picks; one aggregate launch ----
    qmx_counters c0{};
    QMX_TRY(search_enqueue(q, GROUP_PAGE, (const uint32_t *)d_ids, n_ids, d_pages, d_page_counts, nullptr, &c0, false));
    QMX_TRY(launch_group_aggregate(st, gk, gs, d_pages, d_page_counts, nullptr, nq, score_threshold));
    uint32_t launches = c0.kernel_launches + 1, score_passes = 0, n_unfinished = 0;
    std::vector<uint64_t> h_bound(nq);
    std::vector<uint32_t> h_list(nq);
    GroupStats h_stats{};
    QMX_HIP(hipMemcpyAsync(h_bound.data(), gs.bound, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
    QMX_TRY(check_err_flag(q));      // synchronises the stream; an id past the segment's rows ends the call here, before any selection
    n_unfinished = group_pack_unfinished(h_bound.data(), nq, h_list.data());

    // ---- the fallback: score rows of the unfinished queries, tile by tile; pages by selection until no query of the tile is unfinished ----
    if (n_unfinished) {
        ScanArgs fa;
        fill_args(q, 0, 1, fa);      // (the deleted view with the batch's filter)
        const uint64_t stride = group_score_stride(n_cand);
        const int64_t opt = option(OPT_GROUP_MATRIX_BYTES);
        const uint32_t tile = group_tile_queries(n_unfinished, n_cand, opt > 0 ? (uint64_t)opt : GROUP_MATRIX_BYTES);
        const uint64_t page_bound = group_page_bound(limit, group_size);
        QMX_HIP(hipMemcpyAsync(d_list, h_list.data(), (size_t)n_unfinished * 4, hipMemcpyHostToDevice, st));
        QMX_TRY(q->grp_scores.reserve((size_t)tile * stride * sizeof(float)));
        const size_t packed_entries = ((size_t)tile + 63) / 64 * 64 + 64;      // (the scan kernels read whole query tiles)
        const bool l1 = tq_l1(s);
        if (!l1) {
            QMX_TRY(q->grp_queries.reserve(packed_entries * q->q_stride));
            QMX_HIP(hipMemsetAsync(q->grp_queries.p, 0, packed_entries * q->q_stride, st));
        }
        float *d_scores = (float *)q->grp_scores.p;
        for (uint32_t t0 = 0; t0 < n_unfinished; t0 += tile) {
            const uint32_t nt = std::min<uint32_t>(tile, n_unfinished - t0);
            if (l1) {      // TurboQuant over Manhattan scores from the f32 queries of the batch (tq_l1.hip): one query at a time where it sits
                for (uint32_t u = 0; u < nt; ++u)
                    QMX_TRY(score_matrix_enqueue(q, h_list[t0 + u], 1, (const uint32_t *)d_ids, n_cand, d_scores + (size_t)u * stride, stride, &launches));
                score_passes += nt;
            } else {
                // the unfinished queries' entries packed (as the split path packs its overflowed queries), then score_matrix_enqueue's loop over them
                QMX_TRY(launch_gather_rows(st, q->d_queries, q->q_stride, q->q_stride, d_list + t0, nt, nq, q->grp_queries.p, q->d_err));
                const uint32_t SQT = tile_qt(s, q);
                const bool loops = s->dtype == QMX_DTYPE_F32 && SQT >= 8 && mfma_scan_ok(s);
                const uint32_t step = loops ? nt : SQT;
                for (uint32_t st0 = 0; st0 < nt; st0 += step) {
                    const uint32_t nq_sub = std::min<uint32_t>(step, nt - st0);
                    ScanArgs pre;
                    fill_args(q, 0, nq_sub, pre);
                    pre.queries = (const char *)q->grp_queries.p + (size_t)st0 * q->q_stride;
                    pre.ids = (const uint32_t *)d_ids;
                    pre.n_cand = n_cand;
                    pre.top = 1;
                    pre.scores = d_scores + (size_t)st0 * stride;
                    pre.scores_stride = stride;
                    uint32_t pgrid = 0;
                    QMX_TRY(launch_scan(q, (int)std::min<uint32_t>(pow2_ceil(nq_sub), std::max<uint32_t>(SQT, 8)), SCAN_SCORES, pre, &pgrid));
                    ++score_passes;
                    ++launches;
                }
                ++launches;
            }
            const uint32_t blocks = group_select_blocks(n_cand, nt);
            QMX_TRY(q->grp_partial.reserve((size_t)blocks * nt * GROUP_PAGE * sizeof(uint64_t)));
            for (uint64_t page = 0;; ++page) {
                // (every page's first row is eligible by construction: each page adds a hit to every unfinished query)
                QMX_REQUIRE(page <= page_bound, QMX_ERR_OTHER, "grouped search: a query is unfinished after %llu pages (limit %u x group_size %u)",
                            (unsigned long long)page, limit, group_size);
                QMX_TRY(launch_group_select(st, gk, gs, d_scores, stride, n_cand, (const uint32_t *)d_ids, fa.del, d_list + t0, nt, blocks,
                                            (uint64_t *)q->grp_partial.p));
                q->last_kernel = last_noted_kernel();
                QMX_TRY(launch_merge_keys(st, (const uint64_t *)q->grp_partial.p, blocks, nt, nt, GROUP_PAGE, d_pages, d_page_counts, GROUP_PAGE, 0, nullptr,
                                          nullptr, d_list + t0));
                QMX_HIP(hipMemsetAsync(&gs.stats->unfinished, 0, 4, st));
                QMX_TRY(launch_group_aggregate(st, gk, gs, d_pages, d_page_counts, d_list + t0, nt, score_threshold));
                launches += 3;
                QMX_HIP(hipMemcpyAsync(&h_stats, gs.stats, sizeof(h_stats), hipMemcpyDeviceToHost, st));
                QMX_TRY(check_err_flag(q));
                if (h_stats.unfinished == 0) break;
            }
        }
    }

    // ---- the result ----
    QMX_TRY(launch_group_final(st, gs, nq, d_out_keys, d_out_sizes, d_out_hits, d_out_n));
    ++launches;
    for (GroupOut *o : {&ok, &os, &oh, &on})
        if (o->host) QMX_HIP(hipMemcpyAsync(o->host, o->dev, o->bytes, hipMemcpyDeviceToHost, st));
    QMX_HIP(hipMemcpyAsync(&h_stats, gs.stats, sizeof(h_stats), hipMemcpyDeviceToHost, st));
    QMX_TRY(check_err_flag(q));
    if (counters) {
        counters->pages = h_stats.pages;
        counters->fallback_queries = n_unfinished;
        counters->score_passes = score_passes;
        counters->kernel_launches = launches;
    }
    return QMX_OK;
}

}  // extern "C"
