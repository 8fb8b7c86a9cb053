// api_hnsw.hip — the C-ABI of include/qdrant_amd.h, HNSW graphs: create / import / export, the walks.  (The device builds: api_hnsw_build.hip,
// api_hnsw_payload.hip.)  (One of the api_*.hip translation units; what they share: api_internal.hpp.)
#include "api_hnsw_build.hpp"
#include "hnsw_layout.hpp"
#include <algorithm>

extern "C" {


int32_t qmx_hnsw_destroy(qmx_hnsw *g) {
    if (!g) return QMX_OK;
    (void)hipSetDevice(g->device);
    delete g;
    return QMX_OK;
}

// the graph's arrays on the device, and where every level-0 list fits it the packed level-0 table
static int32_t hnsw_upload(qmx_hnsw *g, const qmx_hnsw_desc *d) {
    QMX_TRY(dev_upload(&g->d_reindex, d->reindex, d->n_points));
    QMX_TRY(dev_upload(&g->d_level_offsets, d->level_offsets, d->n_points ? (size_t)d->n_levels + 1 : 0));
    QMX_TRY(dev_upload(&g->d_offsets, d->offsets, d->n_points ? d->n_offsets : 0));
    QMX_TRY(dev_upload(&g->d_neighbors, d->neighbors, d->n_neighbors));
    QMX_TRY(dev_upload(&g->d_ep_ids, d->entry_point_ids, d->n_entry_points));
    QMX_TRY(dev_upload(&g->d_ep_levels, d->entry_point_levels, d->n_entry_points));
    QMX_TRY(dev_upload(&g->d_xp_ids, d->extra_entry_point_ids, d->n_extra_entry_points));
    QMX_TRY(dev_upload(&g->d_xp_levels, d->extra_entry_point_levels, d->n_extra_entry_points));
    // the longest level-0 list: m0 is the reference's per-hop limit, not a capacity (merge_from_other appends past it), so whatever holds a whole list
    // is sized by this
    if (d->n_points) {
        std::vector<uint64_t> copy;
        const uint64_t *off = d->offsets;
        if (is_device_ptr(d->offsets)) {
            copy.resize((size_t)d->n_points + 1);
            QMX_HIP(hipMemcpy(copy.data(), d->offsets, copy.size() * 8, hipMemcpyDeviceToHost));
            off = copy.data();
        }
        uint64_t longest = 0;
        for (uint64_t i = 0; i < d->n_points; ++i) longest = std::max<uint64_t>(longest, off[i + 1] >= off[i] ? off[i + 1] - off[i] : 0);
        g->max_row0 = (uint32_t)std::min<uint64_t>(longest, 0xFFFFFFFFull);
    }
    // packed level-0 table (one round trip per hop instead of two); lists longer than m0 or 63 keep the CSR path
    if (!d->n_points || d->m0 > 63) return QMX_OK;
    const uint32_t stride = d->m0 + 1;
    bool fits = true;
    if (!is_device_ptr(d->offsets))
        for (uint64_t i = 0; i < d->n_points && fits; ++i) fits = d->offsets[i + 1] - d->offsets[i] <= d->m0;
    else fits = false;   // device-side arrays are not inspected
    if (fits && hipMalloc((void **)&g->d_l0, (size_t)d->n_points * stride * 4) == hipSuccess) {
        g->l0_stride = stride;
        QMX_TRY(launch_hnsw_pack_level0(nullptr, g->d_offsets, g->d_neighbors, d->n_points, stride, g->d_l0));
        QMX_HIP(hipDeviceSynchronize());
    } else {
        (void)hipGetLastError();
        g->d_l0 = nullptr;
    }
    return QMX_OK;
}

// flat_ok: a graph of level 0 alone may carry m = 0 (the reference's m = 0 index of payload links only, qmx_hnsw_build_payload_links: built, exported and
// loaded again); the file loaders keep m >= 1
static int32_t hnsw_create_checked(const qmx_hnsw_desc *d, qmx_hnsw **out, bool flat_ok);
int32_t qmx_hnsw_create(const qmx_hnsw_desc *d, qmx_hnsw **out) { return hnsw_create_checked(d, out, true); }
static int32_t hnsw_create_checked(const qmx_hnsw_desc *d, qmx_hnsw **out, bool flat_ok) {
    QMX_REQUIRE(d && out, QMX_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    QMX_REQUIRE((d->m >= 1 || (flat_ok && d->n_levels <= 1)) && d->m0 >= 1, QMX_ERR_BAD_ARG, "m / m0 must be > 0");
    QMX_REQUIRE(d->n_points == 0 || (d->n_levels >= 1 && d->reindex && d->level_offsets && d->offsets), QMX_ERR_BAD_ARG,
                "graph arrays missing");
    QMX_REQUIRE(d->n_neighbors == 0 || d->neighbors, QMX_ERR_BAD_ARG, "neighbors missing");
    QMX_REQUIRE(d->n_entry_points == 0 || (d->entry_point_ids && d->entry_point_levels), QMX_ERR_BAD_ARG, "entry points missing");
    QMX_REQUIRE(d->n_extra_entry_points == 0 || (d->extra_entry_point_ids && d->extra_entry_point_levels), QMX_ERR_BAD_ARG,
                "extra entry points missing");
    QMX_REQUIRE(d->n_points == 0 || d->n_offsets >= (uint64_t)d->n_points + 1, QMX_ERR_BAD_ARG,
                "offsets must hold n_points + 1 entries at least (level 0 has a slot per point)");
    // structural checks on host-visible arrays (a corrupt links file must not crash the GPU); they run before the device is
    // touched, so a bad file is reported as such on any host
    if (d->n_points && !is_device_ptr(d->level_offsets)) {
        QMX_REQUIRE(d->level_offsets[0] == 0 && d->level_offsets[d->n_levels] + 1 == d->n_offsets, QMX_ERR_BAD_ARG,
                    "level_offsets do not span the offsets array");
        for (uint32_t l = 0; l < d->n_levels; ++l)
            QMX_REQUIRE(d->level_offsets[l] <= d->level_offsets[l + 1], QMX_ERR_BAD_ARG, "level_offsets must be non-decreasing");
        QMX_REQUIRE(d->level_offsets[d->n_levels > 1 ? 1 : d->n_levels] == d->n_points, QMX_ERR_BAD_ARG,
                    "level 0 must have one slot per point");
    }
    if (d->n_points && !is_device_ptr(d->offsets)) {
        for (uint64_t i = 0; i + 1 < d->n_offsets; ++i)
            QMX_REQUIRE(d->offsets[i] <= d->offsets[i + 1], QMX_ERR_BAD_ARG, "offsets must be non-decreasing");
        QMX_REQUIRE(d->offsets[d->n_offsets - 1] <= d->n_neighbors, QMX_ERR_BAD_ARG, "offsets run past the neighbors array");
    }
    // every link stored on level l >= 1 must point at a node that HAS a slot on level l (the walk indexes offsets[] with
    // level_offsets[l] + reindex[id]); the same for an entry point and the level it claims.  The kernel bounds the slot as well.
    const bool host_graph = d->n_points && !is_device_ptr(d->level_offsets) && !is_device_ptr(d->offsets) && !is_device_ptr(d->reindex) &&
                            (d->n_neighbors == 0 || !is_device_ptr(d->neighbors));
    if (host_graph) {
        for (uint32_t i = 0; i < d->n_points; ++i)
            QMX_REQUIRE(d->reindex[i] < d->n_points, QMX_ERR_OUT_OF_BOUNDS, "reindex entry out of range");
        for (uint32_t l = 1; l < d->n_levels; ++l) {
            const uint64_t size_l = d->level_offsets[l + 1] - d->level_offsets[l];
            for (uint64_t slot = d->level_offsets[l]; slot < d->level_offsets[l + 1]; ++slot)
                for (uint64_t j = d->offsets[slot]; j < d->offsets[slot + 1]; ++j) {
                    const uint32_t id = d->neighbors[j];
                    QMX_REQUIRE(id < d->n_points && d->reindex[id] < size_l, QMX_ERR_OUT_OF_BOUNDS,
                                "link %u on level %u points at a node that is not on that level", id, l);
                }
        }
        auto ep_ok = [&](uint32_t id, uint32_t lv) {
            if (id >= d->n_points) return false;
            const uint32_t l = std::min<uint32_t>(lv, d->n_levels - 1);
            return l == 0 || (uint64_t)d->reindex[id] < d->level_offsets[l + 1] - d->level_offsets[l];
        };
        for (uint32_t i = 0; i < d->n_entry_points && !is_device_ptr(d->entry_point_ids) && !is_device_ptr(d->entry_point_levels); ++i)
            QMX_REQUIRE(ep_ok(d->entry_point_ids[i], d->entry_point_levels[i]), QMX_ERR_OUT_OF_BOUNDS, "entry point %u is not on its level %u",
                        d->entry_point_ids[i], d->entry_point_levels[i]);
        for (uint32_t i = 0; i < d->n_extra_entry_points && !is_device_ptr(d->extra_entry_point_ids) && !is_device_ptr(d->extra_entry_point_levels); ++i)
            QMX_REQUIRE(ep_ok(d->extra_entry_point_ids[i], d->extra_entry_point_levels[i]), QMX_ERR_OUT_OF_BOUNDS,
                        "extra entry point %u is not on its level %u", d->extra_entry_point_ids[i], d->extra_entry_point_levels[i]);
    }
    for (uint32_t i = 0; i < d->n_entry_points && !is_device_ptr(d->entry_point_ids); ++i)
        QMX_REQUIRE(d->entry_point_ids[i] < d->n_points, QMX_ERR_OUT_OF_BOUNDS, "entry point %u out of range", d->entry_point_ids[i]);
    for (uint32_t i = 0; i < d->n_extra_entry_points && !is_device_ptr(d->extra_entry_point_ids); ++i)
        QMX_REQUIRE(d->extra_entry_point_ids[i] < d->n_points, QMX_ERR_OUT_OF_BOUNDS, "extra entry point out of range");
    QMX_TRY(check_device(d->device_id, nullptr));
    qmx_hnsw *g = new (std::nothrow) qmx_hnsw();
    QMX_REQUIRE(g, QMX_ERR_OUT_OF_MEMORY, "host allocation failed");
    g->device = d->device_id;
    g->m = d->m; g->m0 = d->m0; g->n_points = d->n_points; g->n_levels = d->n_levels;
    g->n_ep = d->n_entry_points; g->n_xp = d->n_extra_entry_points;
    g->n_offsets = d->n_offsets; g->n_neighbors = d->n_neighbors;
    const int32_t rc = hnsw_upload(g, d);
    if (rc != QMX_OK) {
        qmx_hnsw_destroy(g);
        return rc;
    }
    *out = g;
    return QMX_OK;
}

int32_t qmx_hnsw_create_from_plain_file(const void *bytes, uint64_t n_bytes, const qmx_hnsw_desc *desc, qmx_hnsw **out) {
    QMX_REQUIRE(bytes && desc && out, QMX_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    QMX_REQUIRE(!is_device_ptr(bytes), QMX_ERR_BAD_ARG, "the links file must be host memory (mmap it)");
    QMX_REQUIRE(n_bytes >= 64, QMX_ERR_BAD_ARG, "links file shorter than its 64-byte header");
    const uint8_t *b = (const uint8_t *)bytes;
    uint64_t hdr[5];
    memcpy(hdr, b, sizeof(hdr));
    const uint64_t point_count = hdr[0], levels_count = hdr[1], total_neighbors = hdr[2], total_offsets = hdr[3], pad = hdr[4];
    QMX_REQUIRE(levels_count != 0xFFFFFFFFFFFFFF01ull && levels_count != 0xFFFFFFFFFFFFFF02ull, QMX_ERR_NOT_SUPPORTED,
                "compressed graph links (header version %llx): re-serialize as Plain first", (unsigned long long)levels_count);
    QMX_REQUIRE(point_count <= 0xFFFFFFFFull && levels_count <= 64 && (pad == 0 || pad == 4), QMX_ERR_BAD_ARG, "not a plain links header");
    // section sizes, with overflow-safe bounds (every count is checked against the file size first)
    QMX_REQUIRE(total_neighbors <= n_bytes / 4 && total_offsets <= n_bytes / 8, QMX_ERR_BAD_ARG, "links header counts exceed the file size");
    const uint64_t off_levels = 64, off_reindex = off_levels + levels_count * 8, off_neigh = off_reindex + point_count * 4,
                   off_offsets = off_neigh + total_neighbors * 4 + pad, end = off_offsets + total_offsets * 8;
    QMX_REQUIRE(end <= n_bytes && off_offsets % 8 == 0, QMX_ERR_BAD_ARG, "links file truncated or misaligned (%llu > %llu)",
                (unsigned long long)end, (unsigned long long)n_bytes);
    QMX_REQUIRE(point_count == 0 || total_offsets >= 1, QMX_ERR_BAD_ARG, "empty offsets section");
    std::vector<uint64_t> level_offsets((size_t)levels_count + 1);
    memcpy(level_offsets.data(), b + off_levels, (size_t)levels_count * 8);
    level_offsets[(size_t)levels_count] = total_offsets ? total_offsets - 1 : 0;
    // the sections are only 4-byte aligned inside an arbitrary buffer: copy what needs 8
    std::vector<uint64_t> offsets((size_t)total_offsets);
    memcpy(offsets.data(), b + off_offsets, (size_t)total_offsets * 8);
    std::vector<uint32_t> reindex((size_t)point_count), neighbors((size_t)total_neighbors);
    memcpy(reindex.data(), b + off_reindex, (size_t)point_count * 4);
    memcpy(neighbors.data(), b + off_neigh, (size_t)total_neighbors * 4);
    qmx_hnsw_desc d = *desc;
    d.n_points = (uint32_t)point_count;
    d.n_levels = (uint32_t)levels_count;
    d.reindex = reindex.data();
    d.level_offsets = level_offsets.data();
    d.offsets = offsets.data();
    d.n_offsets = total_offsets;
    d.neighbors = neighbors.data();
    d.n_neighbors = total_neighbors;
    for (uint64_t i = 0; i < total_neighbors; ++i)
        QMX_REQUIRE(neighbors[i] < point_count, QMX_ERR_OUT_OF_BOUNDS, "link %u out of range", neighbors[i]);
    for (uint64_t i = 0; i < point_count; ++i)
        QMX_REQUIRE(reindex[i] < point_count, QMX_ERR_OUT_OF_BOUNDS, "reindex entry out of range");
    return hnsw_create_checked(&d, out, false);
}

int32_t hnsw_finish_graph(qmx_hnsw &g, uint32_t m, uint32_t m0, uint32_t n, uint32_t n_levels, int device, qmx_hnsw **out) {
    qmx_hnsw_desc d;
    memset(&d, 0, sizeof(d));
    d.m = m; d.m0 = m0; d.n_points = n; d.n_levels = n_levels;
    d.reindex = g.h_reindex.data(); d.level_offsets = g.h_level_offsets.data(); d.offsets = g.h_offsets.data();
    d.n_offsets = g.h_offsets.size(); d.neighbors = g.h_neighbors.data(); d.n_neighbors = g.h_neighbors.size();
    d.entry_point_ids = g.h_ep_ids.data(); d.entry_point_levels = g.h_ep_levels.data(); d.n_entry_points = (uint32_t)g.h_ep_ids.size();
    d.extra_entry_point_ids = g.h_xp_ids.data(); d.extra_entry_point_levels = g.h_xp_levels.data();
    d.n_extra_entry_points = (uint32_t)g.h_xp_ids.size();
    d.device_id = device;
    QMX_TRY(qmx_hnsw_create(&d, out));
    qmx_hnsw *dev = *out;
    dev->h_reindex = std::move(g.h_reindex); dev->h_neighbors = std::move(g.h_neighbors);
    dev->h_ep_ids = std::move(g.h_ep_ids); dev->h_ep_levels = std::move(g.h_ep_levels);
    dev->h_xp_ids = std::move(g.h_xp_ids); dev->h_xp_levels = std::move(g.h_xp_levels);
    dev->h_level_offsets = std::move(g.h_level_offsets); dev->h_offsets = std::move(g.h_offsets);
    return QMX_OK;
}

int32_t qmx_hnsw_get_info(const qmx_hnsw *g, qmx_hnsw_info *out) {
    QMX_REQUIRE(g && out, QMX_ERR_BAD_ARG, "NULL argument");
    out->m = g->m; out->m0 = g->m0; out->n_points = g->n_points; out->n_levels = g->n_levels;
    out->n_offsets = g->n_offsets; out->n_neighbors = g->n_neighbors;
    out->n_entry_points = g->n_ep; out->n_extra_entry_points = g->n_xp;
    return QMX_OK;
}

int32_t qmx_hnsw_export_plain(const qmx_hnsw *g, uint32_t *reindex, uint64_t *level_offsets, uint64_t *offsets, uint32_t *neighbors,
                              uint32_t *ep_ids, uint32_t *ep_levels, uint32_t *xp_ids, uint32_t *xp_levels) {
    QMX_REQUIRE(g, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(g->n_points == 0 || !g->h_offsets.empty(), QMX_ERR_NOT_SUPPORTED, "only graphs built by qmx_hnsw_build keep a host copy to export");
    auto cp = [](void *dst, const void *src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
    cp(reindex, g->h_reindex.data(), g->h_reindex.size() * 4);
    cp(level_offsets, g->h_level_offsets.data(), g->h_level_offsets.size() * 8);
    cp(offsets, g->h_offsets.data(), g->h_offsets.size() * 8);
    cp(neighbors, g->h_neighbors.data(), g->h_neighbors.size() * 4);
    cp(ep_ids, g->h_ep_ids.data(), g->h_ep_ids.size() * 4);
    cp(ep_levels, g->h_ep_levels.data(), g->h_ep_levels.size() * 4);
    cp(xp_ids, g->h_xp_ids.data(), g->h_xp_ids.size() * 4);
    cp(xp_levels, g->h_xp_levels.data(), g->h_xp_levels.size() * 4);
    return QMX_OK;
}

static int32_t launch_hnsw(const qmx_query *q, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu) {
    const qmx_segment *s = q->seg;
    if (a.cq_desc && a.mv_offsets) {
        if (s->dtype <= QMX_DTYPE_U8) {
            QMX_REQUIRE(s->fast_layout(), QMX_ERR_NOT_SUPPORTED, "adopted device block is not 16-byte aligned");
            return launch_hnsw_custom_maxsim_dense(q->stream, (int)s->dtype, (int)s->distance, a, h, grid, per_cu);
        }
        if (s->dtype == QMX_DTYPE_SQ_U8) return launch_hnsw_custom_maxsim_sq(q->stream, (int)s->distance, a, h, grid, per_cu);
        set_error("custom walk over multi-vector points: inner rows of dtype %u are not built (dense and SQ are)", s->dtype);
        return QMX_ERR_NOT_SUPPORTED;
    }
    if (a.cq_desc) {
        if (s->dtype <= QMX_DTYPE_U8) {
            QMX_REQUIRE(s->fast_layout(), QMX_ERR_NOT_SUPPORTED, "adopted device block is not 16-byte aligned");
            return launch_hnsw_custom_dense(q->stream, (int)s->dtype, (int)s->distance, a, h, grid, per_cu);
        }
        if (s->dtype == QMX_DTYPE_SQ_U8) return launch_hnsw_custom_sq(q->stream, (int)s->distance, a, h, grid, per_cu);
        if (s->dtype == QMX_DTYPE_PQ) return launch_hnsw_custom_pq(q->stream, a, h, grid, per_cu);
        if (s->dtype == QMX_DTYPE_BQ) return launch_hnsw_custom_bq(q->stream, a, h, grid, per_cu);
        if (tq_l1(s)) return launch_hnsw_custom_tq_l1(q->stream, a, h, grid, per_cu, s->tq_rot_dim);
        if (s->dtype == QMX_DTYPE_TQ) return launch_hnsw_custom_tq(q->stream, a, h, grid, per_cu);
        set_error("dtype %u not built yet", s->dtype);
        return QMX_ERR_NOT_SUPPORTED;
    }
    if (a.mv_offsets) {
        if (s->dtype <= QMX_DTYPE_U8) {
            QMX_REQUIRE(s->fast_layout(), QMX_ERR_NOT_SUPPORTED, "adopted device block is not 16-byte aligned");
            return launch_hnsw_maxsim_dense(q->stream, (int)s->dtype, (int)s->distance, a, h, grid, per_cu);
        }
        if (s->dtype == QMX_DTYPE_SQ_U8) return launch_hnsw_maxsim_sq(q->stream, (int)s->distance, a, h, grid, per_cu);
        if (s->dtype == QMX_DTYPE_BQ) return launch_hnsw_maxsim_bq(q->stream, a, h, grid, per_cu);
        if (s->dtype == QMX_DTYPE_PQ) return launch_hnsw_maxsim_pq(q->stream, a, h, grid, per_cu);
        if (s->dtype == QMX_DTYPE_TQ) return launch_hnsw_maxsim_tq(q->stream, a, h, grid, per_cu);      // (over Manhattan: refused by hnsw_enqueue)
        set_error("MaxSim walk: inner rows of dtype %u are not built", s->dtype);
        return QMX_ERR_NOT_SUPPORTED;
    }
    if (s->dtype <= QMX_DTYPE_U8) {
        QMX_REQUIRE(s->fast_layout(), QMX_ERR_NOT_SUPPORTED, "adopted device block is not 16-byte aligned");
        return launch_hnsw_dense(q->stream, (int)s->dtype, (int)s->distance, a, h, grid, per_cu);
    }
    if (s->dtype == QMX_DTYPE_SQ_U8) return launch_hnsw_sq(q->stream, (int)s->distance, a, h, grid, per_cu);
    if (s->dtype == QMX_DTYPE_PQ && a.queries == q->enc.p && !a.cq_desc && !a.mv_offsets) return launch_hnsw_pq_direct(q->stream, a, h, grid, per_cu);
    if (s->dtype == QMX_DTYPE_PQ) {
        return launch_hnsw_pq(q->stream, a, h, grid, per_cu);
    }
    if (s->dtype == QMX_DTYPE_BQ) return launch_hnsw_bq(q->stream, a, h, grid, per_cu);
    if (tq_l1(s)) return launch_hnsw_tq_l1(q->stream, a, h, grid, per_cu, s->tq_rot_dim);
    if (s->dtype == QMX_DTYPE_TQ) return launch_hnsw_tq(q->stream, a, h, grid, per_cu);
    set_error("dtype %u not built yet", s->dtype);
    return QMX_ERR_NOT_SUPPORTED;
}


int32_t hnsw_enqueue(const qmx_hnsw *g, qmx_query *q, uint32_t top, uint32_t ef, qmx_scored_point *d_out,
                            uint32_t *d_counts, uint32_t *d_scored, bool timed, bool acorn, const MultiWalk *mw,
                            const ExpandedOut *xo, const CustomWalk *cw, const PopTrace *pt) {
    const qmx_segment *s = q->seg;
    QMX_REQUIRE(!tq_l1(s) || !mw, QMX_ERR_NOT_SUPPORTED, "multi-vector walks through a TurboQuant storage over Manhattan are not built");
    // (per-request filters index the walk's searches as the batch's queries: custom and multi-vector walks, whose searches are not the batch's entries, and
    // the expanded-candidates walk of search_with_vectors refuse at their entry points - this is the backstop)
    QMX_REQUIRE(!q->has_filters || (!mw && !cw && !xo), QMX_ERR_NOT_SUPPORTED, "this walk does not serve per-request filters (qmx_query_set_filters)");
    ScanArgs a;
    fill_args(q, 0, q->nq, a);
    if (tq_l1(s)) {   // the walk scores against the query as given (tq_l1_policy.hpp): f32 entries of dim floats, 16-byte padded
        const uint32_t qs = tq_l1_query_bytes(s->dim);
        QMX_TRY(q->tq_rot.reserve((size_t)q->nq * qs));
        QMX_HIP(hipMemsetAsync(q->tq_rot.p, 0, (size_t)q->nq * qs, q->stream));
        QMX_HIP(hipMemcpy2DAsync(q->tq_rot.p, qs, q->enc.p, (size_t)s->dim * 4, (size_t)s->dim * 4, q->nq, hipMemcpyDeviceToDevice, q->stream));
        a.queries = q->tq_rot.p;
        a.q_stride = qs;
    }
    // PQ: the LUT-free walk (pq.hip HopPQDirect) - the entry of a search is its preprocessed vector (q->enc keeps them), staged in LDS
    const bool pq_direct = s->dtype == QMX_DTYPE_PQ && !cw && !mw && option(OPT_HNSW_PQ_DIRECT_WALK) > 0 &&
                           s->d_centroids &&
                           pq_direct_walk_ok(s->dim, s->pq_m, s->pq.chunk_size, s->pq.n_centroids);
    if (pq_direct) {
        a.queries = q->enc.p;
        a.q_stride = s->dim * 4;
    }
    const uint32_t n_searches = cw ? cw->n_queries : mw ? mw->n_queries : q->nq;
    if (cw) {
        a.cq_desc = cw->d_desc;
        a.cq_coefs = cw->d_coefs;
    }
    if (mw) {
        a.mv_offsets = mw->d_offsets;
        a.mv_qfirst = mw->d_qfirst;
        a.del = mw->del;
    }
    HnswArgs h;
    memset(&h, 0, sizeof(h));
    h.reindex = g->d_reindex; h.level_offsets = g->d_level_offsets; h.offsets = g->d_offsets; h.neighbors = g->d_neighbors;
    h.l0 = g->d_l0; h.l0_stride = g->l0_stride;
    // SQ segments, plain walk over a packed level 0: the link rows bring the linked rows' vector_offset along (scan_quant.hip RowSQX): the table is made once
    // per (graph, segment) - 10 M points x 64 dwords = 2.56 GB, one gather pass - and costs the walk one more line per hop instead of a random request per row
    if (s->dtype == QMX_DTYPE_SQ_U8 && g->d_l0 && !acorn && !xo && !mw && !cw && !(option(OPT_HNSW_REFERENCE_HEAP_ORDER) > 0) && s->d_row_offsets && g->n_points <= s->n) {
        std::lock_guard<std::mutex> lock(g->l0x_mu);
        // (the table belongs to the first SQ segment walked over this graph: another segment - another quantization of the same points - keeps the column;
        // nothing is ever freed under a running kernel)
        if (!g->d_l0x && !g->l0x_failed) {
            const size_t bytes = (size_t)g->n_points * (2 * (g->l0_stride - 1)) * 4;
            if (hipMalloc((void **)&g->d_l0x, bytes) != hipSuccess) {
                (void)hipGetLastError();
                g->d_l0x = nullptr;
                g->l0x_failed = true;
            } else {
                QMX_TRY(launch_hnsw_pack_level0_aux(q->stream, g->d_l0, g->n_points, g->l0_stride, s->d_row_offsets, s->n, g->d_l0x));
                QMX_HIP(hipStreamSynchronize(q->stream));      // (other threads' streams read it once the lock is gone)
                g->l0x_segment_uid = s->uid;
            }
        }
        if (g->d_l0x && g->l0x_segment_uid == s->uid) {
            h.l0 = g->d_l0x;
            h.l0_aux_off = g->l0_stride - 1;               // = m0: the row is [m0 link slots][m0 offsets]
            h.l0_stride = 2 * (g->l0_stride - 1);
        }
    }
    h.n_offsets = g->n_offsets; h.n_neighbors = g->n_neighbors;
    h.n_points = g->n_points; h.n_levels = g->n_levels; h.m = g->m; h.m0 = g->m0;
    h.ep_ids = g->d_ep_ids; h.ep_levels = g->d_ep_levels; h.n_ep = g->n_ep;
    h.xp_ids = g->d_xp_ids; h.xp_levels = g->d_xp_levels; h.n_xp = g->n_xp;
    h.ef = ef; h.top = top; h.nq = n_searches;
    h.out = d_out; h.out_counts = d_counts; h.out_scored = d_scored;
    if (xo) { h.expanded = xo->d_ids; h.expanded_cnt = xo->d_cnt; h.xcap = xo->xcap; }
    if (pt) {
        QMX_REQUIRE(!xo && !acorn && !mw && !cw, QMX_ERR_NOT_SUPPORTED, "the pop trace is the plain walk's");
        h.pops = pt->d_pops; h.pop_cnt = pt->d_cnt; h.pop_cap = pt->cap;
    }
    // option hnsw_reference_heap_order: the plain walk keeps the reference's two binary heaps (hnsw.hpp RefHeaps); other walks are unaffected
    h.ref_heaps = (option(OPT_HNSW_REFERENCE_HEAP_ORDER) > 0 && !acorn && !xo && !mw && !cw && !tq_l1(s)) ? 1 : 0;
    h.ref_cap = HNSW_REF_CAND_CAP;
    h.lds_query_bytes = q->q_stride <= HNSW_LDS_QUERY_MAX ? q->q_stride : 0;
    if (tq_l1(s)) {
        h.lds_query_bytes = tq_l1_lds_bytes(s->dim, s->tq_rot_dim);
        QMX_REQUIRE(h.lds_query_bytes <= HNSW_LDS_QUERY_MAX, QMX_ERR_NOT_SUPPORTED, "TurboQuant over Manhattan, the walk: %u bytes of LDS per search", h.lds_query_bytes);
    }
    if (mw) {   // [16-byte header][the multi-query's inner vectors, when the longest fits a modest share of the LDS; else every search reads its own through L2]
        const uint64_t need = 16 + (uint64_t)std::max<uint32_t>(mw->max_tokens, 1) * q->q_stride;
        h.lds_query_bytes = need <= 64 * 1024 ? (uint32_t)need : 16;
    }
    // A PQ LUT of more than half the LDS leaves one search per CU; the walk is a chain of dependent memory round trips,
    // so many searches per CU with the LUT read through L2 win (measured: tools/bench_hnsw.py)
    if (s->dtype == QMX_DTYPE_PQ && q->q_stride > 16 * 1024 && !mw) h.lds_query_bytes = 0;      // (a multi-query's LUTs are always staged)
    if (pq_direct) h.lds_query_bytes = a.q_stride;
    if (cw) {   // [32-byte header][the examples' entries]: staged when they fit a modest share of the LDS, read through L2 otherwise (PQ LUTs always)
        const uint64_t need = 32 + (uint64_t)std::max<uint32_t>(cw->max_examples, 1) * q->q_stride;
        h.lds_query_bytes = (need <= 48 * 1024 && h.lds_query_bytes != 0) ? (uint32_t)need : 32;
        if (tq_l1(s)) {   // TurboQuant over Manhattan: [header][the examples, always staged][the hop scratch][64 scores per example] (hnsw.hpp HopCustom::hop)
            const uint64_t ne = std::max<uint32_t>(cw->max_examples, 1);
            const uint64_t need_l1 = 32 + ne * a.q_stride + (tq_l1_lds_bytes(s->dim, s->tq_rot_dim) - tq_l1_query_bytes(s->dim)) + ne * 256;
            QMX_REQUIRE(need_l1 <= HNSW_LDS_QUERY_MAX, QMX_ERR_NOT_SUPPORTED, "a custom query of %u examples over TurboQuant / Manhattan needs %llu bytes of LDS",
                        cw->max_examples, (unsigned long long)need_l1);
            h.lds_query_bytes = (uint32_t)need_l1;
        }
        if (cw->lds_bytes) {      // multi-vector examples: always staged (the MaxSim policy reads its tokens from LDS)
            QMX_REQUIRE(cw->lds_bytes <= HNSW_LDS_QUERY_MAX, QMX_ERR_NOT_SUPPORTED, "a custom query of %u bytes of example tokens does not fit the LDS", cw->lds_bytes);
            h.lds_query_bytes = cw->lds_bytes;
        }
    }
    if (std::max(top, ef) > HNSW_MAX_EF_REG && !mw && !cw && !tq_l1(s)) {   // a list this long lives in LDS behind the query entry, which is then always staged (a PQ LUT too)
        const size_t beam = hnsw_beam_lds(std::max(top, ef));
        QMX_REQUIRE((size_t)a.q_stride + beam + 2048 <= 160 * 1024, QMX_ERR_NOT_SUPPORTED,
                    "hnsw max(top, ef) = %u: the query entry (%u bytes) and the list do not fit the LDS together", std::max(top, ef), a.q_stride);
        h.lds_query_bytes = a.q_stride;
    }
    // the visited set in LDS (hnsw.hpp LdsVisited) where the search has room for it beside its query entry; the bitmap below stays allocated for what the
    // table's buckets cannot hold
    h.vis_lds = (!acorn && !h.ref_heaps && !option(OPT_HNSW_NO_LDS_VISITED) && g->n_points <= HNSW_VIS_LDS_MAX_POINTS && h.lds_query_bytes <= 32 * 1024) ? HNSW_VIS_LDS_BYTES : 0;
    // the PQ walk through per-search LUTs (HopPQ, not the LUT-free walk): the LUTs' 8-bit images for the hop prefilter (pq.hip HopPQ::prefilter), built
    // here from the batch's f32 LUTs.  Its 24 KiB per search take the LDS the visited table would: that walk keeps the bitmap
    if (s->dtype == QMX_DTYPE_PQ && !pq_direct && !acorn && !mw && !cw && !h.ref_heaps && !option(OPT_HNSW_NO_PQ_PREFILTER) && a.queries == q->d_queries &&
        s->pq_m <= 128 && s->pq.n_centroids <= 256 && q->q_stride > 16 * 1024 && h.lds_query_bytes == 0) {
        const uint32_t st8 = pq_walk_lut8_stride(s->pq_m);
        QMX_TRY(q->hnsw_pq8.reserve((size_t)n_searches * st8));
        QMX_TRY(launch_pq_walk_lut8(q->stream, q->d_queries, q->q_stride, n_searches, s->pq_m, s->pq.n_centroids, q->hnsw_pq8.p));
        h.pq8 = (const unsigned char *)q->hnsw_pq8.p;
        h.pq8_stride = st8;
        h.vis_lds = 0;
    }
    // ... and the LUT-free walk (HopPQDirect) prefilters its hops on the image of the EXACT-ORDER LUT - the entries it recomputes; a batch whose LUTs came
    // from the matrix cores (<= 1e-5 off that order) gets exact-order LUTs made for the image alone
    if (pq_direct && !acorn && !xo && !h.ref_heaps && !option(OPT_HNSW_NO_PQ_PREFILTER) && s->pq_m <= 128 && s->pq.n_centroids <= 256) {
        const uint32_t st8 = pq_walk_lut8_stride(s->pq_m);
        const size_t lut_bytes = (size_t)s->pq_m * s->pq.n_centroids * sizeof(float);
        const void *luts = q->d_queries;
        uint32_t lstride = q->q_stride;
        const bool dotlike = s->distance == QMX_DISTANCE_DOT || s->distance == QMX_DISTANCE_COSINE;
        if (s->pq.lut_mfma && dotlike) {
            qmx_pq_params exact = s->pq;
            exact.lut_mfma = 0;
            QMX_TRY(q->hnsw_lutx.reserve((size_t)n_searches * lut_bytes));
            QMX_TRY(launch_pq_lut(q->stream, s->distance, s->dim, exact, s->d_centroids, (const float *)q->enc.p, n_searches, (float *)q->hnsw_lutx.p));
            luts = q->hnsw_lutx.p;
            lstride = (uint32_t)lut_bytes;
        }
        QMX_TRY(q->hnsw_pq8.reserve((size_t)n_searches * st8));
        QMX_TRY(launch_pq_walk_lut8(q->stream, luts, lstride, n_searches, s->pq_m, s->pq.n_centroids, q->hnsw_pq8.p));
        h.pq8 = (const unsigned char *)q->hnsw_pq8.p;
        h.pq8_stride = st8;
        h.vis_lds = 0;
    }
    h.log_cap = HNSW_LOG_CAP;
    {   // tests: force the whole-bitmap clear path
        const int64_t v = option(OPT_HNSW_LOG_CAP);
        if (v >= 1 && v <= (int64_t)HNSW_LOG_CAP) h.log_cap = (uint32_t)v;
    }
    h.vis_words = ((uint64_t)g->n_points + 31) / 32;
    if (h.vis_words == 0) h.vis_words = 1;
    h.acorn = acorn ? 1 : 0;
    h.hop_cap = 64;
    if (acorn) {   // two visited lists; every explored node may add m0 points to one scoring batch
        QMX_REQUIRE(g->m0 >= 1 && g->m0 <= 128, QMX_ERR_NOT_SUPPORTED, "ACORN walk: m0 = %u not in 1..128", g->m0);
        h.vis_words *= 2;
        // every unvisited link of the popped candidate that fails the filter is explored: a list as long as the candidate's, which m0 does not bound
        QMX_REQUIRE(g->max_row0 <= 8192, QMX_ERR_NOT_SUPPORTED, "ACORN walk: a level-0 list of %u links does not fit the LDS", g->max_row0);
        h.explore_cap = std::max<uint32_t>(g->m0, g->max_row0);
        h.hop_cap = std::min<uint32_t>((g->m0 * (g->m0 + 1) + 63) / 64 * 64, 4160);    // (m0 > 64: the kernel scores what it holds before the buffer could overflow)
    }
    int per_cu = 1;
    QMX_TRY(launch_hnsw(q, a, h, 0, &per_cu));
    if (s->dtype == QMX_DTYPE_PQ && h.lds_query_bytes == 0 && option(OPT_HNSW_PQ_PER_CU) > 0) per_cu = (int)std::min<int64_t>(per_cu, option(OPT_HNSW_PQ_PER_CU));
    // whole waves per SIMD: with 9 searches per CU one SIMD carries three waves and the others two, and the slowest SIMD sets the pace
    // (measured on the SQ walk at 10 M points: 5.76 ms with 8 per CU, 6.09 with 9, 6.23 with 7: profiles/r5_sq_walk_visited.md)
    if (per_cu >= 8) per_cu -= per_cu % 4;
    if (option(OPT_HNSW_PER_CU) > 0) per_cu = (int)std::min<int64_t>(per_cu, option(OPT_HNSW_PER_CU));
    uint64_t slots = std::min<uint64_t>({(uint64_t)n_searches, (uint64_t)s->num_cus * per_cu, (uint64_t)HNSW_SLOT_CAP});
    const uint64_t by_budget = std::max<uint64_t>(1, HNSW_VIS_BUDGET / (h.vis_words * 4));
    slots = std::max<uint64_t>(1, std::min(slots, by_budget));
    if (xo) {      // search_with_vectors: a slot's stack of evicted candidates that tie with the bound (hnsw.hpp; the reference keeps every one of them in `candidates`)
        h.ev_cap = HNSW_EV_SPILL_CAP;
        QMX_TRY(q->hnsw_refc.reserve((size_t)slots * h.ev_cap * sizeof(uint64_t)));
        h.ev_spill = (uint64_t *)q->hnsw_refc.p;
    }
    if (h.ref_heaps) {
        slots = std::min<uint64_t>(slots, HNSW_REF_SLOT_CAP);
        QMX_TRY(q->hnsw_refc.reserve((size_t)slots * h.ref_cap * sizeof(uint2)));
        h.ref_cands = (uint2 *)q->hnsw_refc.p;
    }
    if (q->hnsw_slots < slots || q->hnsw_vis_words != h.vis_words) {
        // (re)allocate for the largest slot count this handle can use, zero once: the kernel returns the bitmaps all-zero
        const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)std::max<uint32_t>(std::max(q->nq, n_searches), 1), (uint64_t)s->num_cus * per_cu,
                                                                       (uint64_t)HNSW_SLOT_CAP, by_budget}));
        QMX_HIP(hipStreamSynchronize(q->stream));
        q->hnsw_slots = 0;
        QMX_TRY(q->hnsw_vis.reserve((size_t)want * h.vis_words * 4));
        QMX_TRY(q->hnsw_log.reserve((size_t)want * HNSW_LOG_CAP * 4));
        QMX_HIP(hipMemsetAsync(q->hnsw_vis.p, 0, (size_t)want * h.vis_words * 4, q->stream));
        q->hnsw_slots = (uint32_t)want;
        q->hnsw_vis_words = h.vis_words;
    }
    h.visited = (uint32_t *)q->hnsw_vis.p;
    h.vis_log = (uint32_t *)q->hnsw_log.p;
    // the slots draw their searches from a counter that starts behind the first `slots` (hnsw.hpp)
    QMX_TRY(q->hnsw_next.reserve(32));         // [u32 next search][pad][u64 hop candidates offered to the PQ prefilter][u64 scored exactly]
    QMX_HIP(hipMemsetD32Async((hipDeviceptr_t)q->hnsw_next.p, (int)slots, 1, q->stream));
    QMX_HIP(hipMemsetAsync((char *)q->hnsw_next.p + 8, 0, 16, q->stream));
    h.next_query = (uint32_t *)q->hnsw_next.p;
    h.pq_stats = h.pq8 ? (unsigned long long *)((char *)q->hnsw_next.p + 8) : nullptr;
    size_t slot = 0;
    if (timed) QMX_TRY(timing_begin(q, &slot));
    QMX_TRY(launch_hnsw(q, a, h, (uint32_t)slots, &per_cu));
    q->last_kernel = last_noted_kernel();
    if (timed) QMX_TRY(timing_end(q, slot));
    return QMX_OK;
}

int32_t hnsw_check(const qmx_hnsw *g, const qmx_query *q, uint32_t top, uint32_t ef) {
    QMX_REQUIRE(g->device == q->seg->device, QMX_ERR_BAD_ARG, "graph lives on device %d, the segment on %d", g->device, q->seg->device);
    QMX_REQUIRE((uint64_t)g->n_points <= q->seg->n, QMX_ERR_OUT_OF_BOUNDS, "graph has %u points, the segment %llu rows", g->n_points,
                (unsigned long long)q->seg->n);
    QMX_REQUIRE(top >= 1, QMX_ERR_BAD_ARG, "top must be > 0");
    QMX_REQUIRE(std::max(top, ef) <= HNSW_MAX_EF, QMX_ERR_NOT_SUPPORTED, "max(top, ef) = %u > %u not supported yet", std::max(top, ef),
                HNSW_MAX_EF);
    return QMX_OK;
}

int32_t hnsw_search_sync(const qmx_hnsw *g, qmx_query *q, uint32_t top, uint32_t ef, qmx_scored_point *out, uint32_t *out_counts,
                                const volatile uint8_t *is_stopped, qmx_counters *counters, bool acorn) {
    QMX_REQUIRE(g && q && out && out_counts, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_TRY(hnsw_check(g, q, top, ef));
    QMX_HIP(hipSetDevice(q->device));
    if (counters) memset(counters, 0, sizeof(*counters));
    if (q->nq == 0) return QMX_OK;
    QMX_CHECK_CANCELLED(is_stopped);
    if (g->n_points == 0) {   // get_entry_point() -> None -> empty result (graph_layers.rs:539-542)
        if (is_device_ptr(out_counts)) QMX_HIP(hipMemset(out_counts, 0, (size_t)q->nq * 4));
        else memset(out_counts, 0, (size_t)q->nq * 4);
        return QMX_OK;
    }
    const bool out_dev = is_device_ptr(out), cnt_dev = is_device_ptr(out_counts);
    qmx_scored_point *d_out = out;
    uint32_t *d_counts = out_counts;
    if (!out_dev) { QMX_TRY(q->out.reserve((size_t)q->nq * top * sizeof(qmx_scored_point))); d_out = (qmx_scored_point *)q->out.p; }
    if (!cnt_dev) { QMX_TRY(q->counts.reserve((size_t)q->nq * 4)); d_counts = (uint32_t *)q->counts.p; }
    QMX_TRY(q->hnsw_scored.reserve((size_t)q->nq * 4));
    const bool timed = q->timing || (q->seg->flags & QMX_SEG_TIME_KERNELS) != 0;
    QMX_TRY(hnsw_enqueue(g, q, top, ef, d_out, d_counts, (uint32_t *)q->hnsw_scored.p, timed, acorn));
    if (!out_dev) QMX_TRY(copy_out(q->stream, out, d_out, (size_t)q->nq * top * sizeof(qmx_scored_point)));
    if (!cnt_dev) QMX_TRY(copy_out(q->stream, out_counts, d_counts, (size_t)q->nq * 4));
    std::vector<uint32_t> scored(counters ? q->nq : 0);
    unsigned long long pq_stats[2] = {0, 0};
    if (counters) QMX_HIP(hipMemcpyAsync(scored.data(), q->hnsw_scored.p, (size_t)q->nq * 4, hipMemcpyDeviceToHost, q->stream));
    if (counters && q->hnsw_next.p) QMX_HIP(hipMemcpyAsync(pq_stats, (char *)q->hnsw_next.p + 8, 16, hipMemcpyDeviceToHost, q->stream));
    QMX_TRY(check_err_flag(q));   // synchronises the stream
    if (counters) {
        uint64_t total = 0;
        for (uint32_t v : scored) total += v;
        counters->vectors_scored = total;
        // the PQ walk's hop prefilter (hnsw.hpp HopPQ::prefilter): level-0 hop candidates that met the 8-bit bound / those that survived it and were scored exactly
        counters->prefilter_candidates = pq_stats[0];
        counters->verified_rows = pq_stats[1];
        counters->bytes_read = total * q->seg->row_bytes;
        counters->kernel_launches = 1;
    }
    if (timed) {
        const float before = q->timing_ms;
        QMX_TRY(timing_fold(q));
        if (counters) counters->kernel_ms = q->timing_ms - before;
    }
    return QMX_OK;
}

int32_t qmx_hnsw_search(const qmx_hnsw *g, qmx_query *q, uint32_t top, uint32_t ef, qmx_scored_point *out, uint32_t *out_counts,
                        const volatile uint8_t *is_stopped, qmx_counters *counters) {
    QMX_REFUSE_SPARSE(q);
    return hnsw_search_sync(g, q, top, ef, out, out_counts, is_stopped, counters, false);
}
int32_t qmx_hnsw_search_acorn(const qmx_hnsw *g, qmx_query *q, uint32_t top, uint32_t ef, qmx_scored_point *out, uint32_t *out_counts,
                              const volatile uint8_t *is_stopped, qmx_counters *counters) {
    QMX_REFUSE_SPARSE(q);
    return hnsw_search_sync(g, q, top, ef, out, out_counts, is_stopped, counters, true);
}

int32_t qmx_hnsw_search_traced(const qmx_hnsw *g, qmx_query *q, uint32_t top, uint32_t ef, qmx_scored_point *out, uint32_t *out_counts,
                               qmx_scored_point *pops, uint32_t pop_cap, uint32_t *pop_counts) {
    QMX_REFUSE_SPARSE(q);
    QMX_REQUIRE(g && q && out && out_counts && pops && pop_counts && pop_cap >= 1, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(!is_device_ptr(out) && !is_device_ptr(out_counts) && !is_device_ptr(pops) && !is_device_ptr(pop_counts), QMX_ERR_BAD_ARG,
                "qmx_hnsw_search_traced writes host arrays");
    QMX_TRY(hnsw_check(g, q, top, ef));
    QMX_HIP(hipSetDevice(q->device));
    if (q->nq == 0) return QMX_OK;
    memset(out_counts, 0, (size_t)q->nq * 4);
    memset(pop_counts, 0, (size_t)q->nq * 4);
    if (g->n_points == 0) return QMX_OK;
    QMX_TRY(q->out.reserve((size_t)q->nq * top * sizeof(qmx_scored_point)));
    QMX_TRY(q->counts.reserve((size_t)q->nq * 4));
    QMX_TRY(q->cand.reserve((size_t)q->nq * pop_cap * sizeof(qmx_scored_point)));
    QMX_TRY(q->xcnt.reserve((size_t)q->nq * 4));
    PopTrace pt{(qmx_scored_point *)q->cand.p, (uint32_t *)q->xcnt.p, pop_cap};
    // (a search without a live entry point - every point deleted, or rejected by the search's own filter - returns before it counts its pops)
    QMX_HIP(hipMemsetAsync(q->xcnt.p, 0, (size_t)q->nq * 4, q->stream));
    QMX_TRY(hnsw_enqueue(g, q, top, ef, (qmx_scored_point *)q->out.p, (uint32_t *)q->counts.p, nullptr, false, false, nullptr, nullptr, nullptr, &pt));
    QMX_TRY(copy_out(q->stream, out, q->out.p, (size_t)q->nq * top * sizeof(qmx_scored_point)));
    QMX_TRY(copy_out(q->stream, out_counts, q->counts.p, (size_t)q->nq * 4));
    QMX_TRY(copy_out(q->stream, pops, q->cand.p, (size_t)q->nq * pop_cap * sizeof(qmx_scored_point)));
    QMX_TRY(copy_out(q->stream, pop_counts, q->xcnt.p, (size_t)q->nq * 4));
    return check_err_flag(q);   // synchronises the stream
}

int32_t qmx_hnsw_search_async(const qmx_hnsw *g, qmx_query *q, uint32_t top, uint32_t ef, qmx_scored_point *out_dev,
                              uint32_t *out_counts_dev, uint32_t *out_scored_dev) {
    QMX_REFUSE_SPARSE(q);
    QMX_REQUIRE(g && q && out_dev && out_counts_dev, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_TRY(hnsw_check(g, q, top, ef));
    QMX_HIP(hipSetDevice(q->device));
    if (q->nq == 0) return QMX_OK;
    if (g->n_points == 0) {
        QMX_HIP(hipMemsetAsync(out_counts_dev, 0, (size_t)q->nq * 4, q->stream));
        return QMX_OK;
    }
    const bool timed = q->timing || (q->seg->flags & QMX_SEG_TIME_KERNELS) != 0;
    return hnsw_enqueue(g, q, top, ef, out_dev, out_counts_dev, out_scored_dev, timed);
}

int32_t qmx_hnsw_search_with_vectors(const qmx_hnsw *g, qmx_query *links, qmx_query *base, uint32_t top, uint32_t ef, qmx_scored_point *out,
                                     uint32_t *out_counts, const volatile uint8_t *is_stopped, qmx_counters *counters) {
    QMX_REFUSE_SPARSE(links);
    QMX_REFUSE_SPARSE(base);
    QMX_REFUSE_FILTERS(links);
    QMX_REFUSE_FILTERS(base);
    QMX_REQUIRE(g && links && base && out && out_counts, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(base->nq == links->nq && base->device == links->device, QMX_ERR_BAD_ARG, "the two query batches must match");
    QMX_REQUIRE(base->seg->n >= g->n_points, QMX_ERR_OUT_OF_BOUNDS, "graph has %u points, the base-vector segment %llu rows", g->n_points,
                (unsigned long long)base->seg->n);
    QMX_TRY(hnsw_check(g, links, top, ef));
    QMX_REQUIRE(top <= MAX_TOP, QMX_ERR_NOT_SUPPORTED, "top %u > %u", top, MAX_TOP);
    QMX_HIP(hipSetDevice(links->device));
    if (counters) memset(counters, 0, sizeof(*counters));
    const uint32_t nq = links->nq;
    if (nq == 0) return QMX_OK;
    QMX_CHECK_CANCELLED(is_stopped);
    if (g->n_points == 0) {
        if (is_device_ptr(out_counts)) QMX_HIP(hipMemset(out_counts, 0, (size_t)nq * 4));
        else memset(out_counts, 0, (size_t)nq * 4);
        return QMX_OK;
    }
    const uint32_t beam_ef = std::max(top, ef);
    // a search pops about ef..2 ef candidates: the list is sized for 32 ef (or every point); a search that pops more (a graph the walk wanders through:
    // a filter that leaves few points, a bad entry) makes the batch run again with a list as long as the largest count it reported - every point at most
    uint32_t xcap = (uint32_t)std::min<uint64_t>(g->n_points, (uint64_t)32 * beam_ef + 256);
    QMX_TRY(links->cand.reserve((size_t)nq * beam_ef * sizeof(qmx_scored_point)));
    QMX_TRY(links->cand_cnt.reserve((size_t)nq * 4));
    QMX_TRY(links->hnsw_scored.reserve((size_t)nq * 4));
    QMX_TRY(links->xcnt.reserve((size_t)nq * 4));
    const bool timed = links->timing || (links->seg->flags & QMX_SEG_TIME_KERNELS) != 0;
    std::vector<uint32_t> cnt(nq), sc(nq);
    uint64_t popped = 0, scored = 0;
    uint32_t walks = 0;
    while (true) {
        QMX_TRY(links->cand_ids.reserve((size_t)nq * xcap * 4));
        ExpandedOut xo{(uint32_t *)links->cand_ids.p, (uint32_t *)links->xcnt.p, xcap};
        QMX_TRY(hnsw_enqueue(g, links, std::min(top, beam_ef), ef, (qmx_scored_point *)links->cand.p, (uint32_t *)links->cand_cnt.p,
                             (uint32_t *)links->hnsw_scored.p, timed, false, nullptr, &xo));
        ++walks;
        QMX_HIP(hipMemcpyAsync(cnt.data(), links->xcnt.p, (size_t)nq * 4, hipMemcpyDeviceToHost, links->stream));
        QMX_HIP(hipMemcpyAsync(sc.data(), links->hnsw_scored.p, (size_t)nq * 4, hipMemcpyDeviceToHost, links->stream));
        QMX_TRY(check_err_flag(links));     // synchronises
        uint32_t worst = 0;
        popped = scored = 0;
        for (uint32_t i = 0; i < nq; ++i) {
            worst = std::max(worst, cnt[i]);
            popped += cnt[i];
            scored += sc[i];
        }
        if (worst <= xcap) break;
        // (the walk is deterministic: the second run pops the same candidates, now all listed; a count above n_points + 1 cannot be)
        QMX_REQUIRE(xcap < g->n_points + 1u, QMX_ERR_OTHER, "a search popped %u candidates of a graph of %u points", worst, g->n_points);
        xcap = (uint32_t)std::min<uint64_t>((uint64_t)g->n_points + 1, worst);
        QMX_CHECK_CANCELLED(is_stopped);
    }
    // base_search_context: FixedLengthPriorityQueue(ef) over the base scores of the popped candidates, into_iter_sorted().take(top)
    QMX_TRY(qmx_rescore(base, (const uint32_t *)links->cand_ids.p, (const uint32_t *)links->xcnt.p, xcap, top, out, out_counts));
    if (counters) {
        counters->vectors_scored = scored + popped;
        counters->bytes_read = scored * links->seg->row_bytes + popped * base->seg->row_bytes;
        counters->kernel_launches = 2 + walks;
        if (timed) { const float before = links->timing_ms; QMX_TRY(timing_fold(links)); counters->kernel_ms = links->timing_ms - before; }
    }
    return QMX_OK;
}

int32_t qmx_multi_hnsw_search(const qmx_hnsw *g, qmx_query *inner, const uint32_t *query_first, uint32_t n_queries, const uint64_t *point_offsets,
                              uint32_t n_points, const uint64_t *point_deleted, uint64_t n_deleted_bits, uint32_t top, uint32_t ef,
                              qmx_scored_point *out, uint32_t *out_counts, qmx_counters *counters) {
    QMX_REFUSE_SPARSE(inner);
    QMX_REFUSE_FILTERS(inner);
    QMX_REQUIRE(g && inner && query_first && point_offsets && out && out_counts, QMX_ERR_BAD_ARG, "NULL argument");
    const qmx_segment *s = inner->seg;
    QMX_REQUIRE(g->device == s->device, QMX_ERR_BAD_ARG, "graph lives on device %d, the segment on %d", g->device, s->device);
    QMX_REQUIRE(g->n_points <= n_points, QMX_ERR_OUT_OF_BOUNDS, "graph has %u points, the multi-vector storage %u", g->n_points, n_points);
    QMX_REQUIRE(top >= 1, QMX_ERR_BAD_ARG, "top must be > 0");
    QMX_REQUIRE(std::max(top, ef) <= HNSW_MAX_EF, QMX_ERR_NOT_SUPPORTED, "max(top, ef) = %u > %u not supported yet", std::max(top, ef), HNSW_MAX_EF);
    QMX_REQUIRE(!is_device_ptr(query_first) && !is_device_ptr(point_offsets), QMX_ERR_BAD_ARG, "query_first and point_offsets are host arrays");
    QMX_HIP(hipSetDevice(inner->device));
    if (counters) memset(counters, 0, sizeof(*counters));
    if (n_queries == 0) return QMX_OK;
    QMX_REQUIRE(query_first[n_queries] <= inner->nq, QMX_ERR_OUT_OF_BOUNDS, "multi-queries reach past the %u inner query vectors of the batch", inner->nq);
    uint32_t max_tokens = 0;
    for (uint32_t j = 0; j < n_queries; ++j) {
        QMX_REQUIRE(query_first[j] <= query_first[j + 1], QMX_ERR_BAD_ARG, "query_first is not ascending at %u", j);
        max_tokens = std::max(max_tokens, query_first[j + 1] - query_first[j]);
    }
    for (uint32_t p = 0; p < n_points; ++p)
        QMX_REQUIRE(point_offsets[p] <= point_offsets[p + 1], QMX_ERR_BAD_ARG, "point_offsets is not ascending at %u", p);
    QMX_REQUIRE(point_offsets[n_points] <= s->n, QMX_ERR_OUT_OF_BOUNDS, "point_offsets reach past the %llu inner rows of the segment",
                (unsigned long long)s->n);
    const bool out_dev = is_device_ptr(out), cnt_dev = is_device_ptr(out_counts);
    if (g->n_points == 0) {   // get_entry_point() -> None
        if (cnt_dev) QMX_HIP(hipMemset(out_counts, 0, (size_t)n_queries * 4));
        else memset(out_counts, 0, (size_t)n_queries * 4);
        return QMX_OK;
    }
    QMX_TRY(inner->mv_qfirst.reserve((size_t)(n_queries + 1) * 4));
    QMX_TRY(inner->mv_offsets.reserve((size_t)(n_points + 1) * 8));
    QMX_HIP(hipMemcpyAsync(inner->mv_qfirst.p, query_first, (size_t)(n_queries + 1) * 4, hipMemcpyHostToDevice, inner->stream));
    QMX_HIP(hipMemcpyAsync(inner->mv_offsets.p, point_offsets, (size_t)(n_points + 1) * 8, hipMemcpyHostToDevice, inner->stream));
    MultiWalk mw;
    memset(&mw, 0, sizeof(mw));
    mw.d_qfirst = (const uint32_t *)inner->mv_qfirst.p;
    mw.d_offsets = (const uint64_t *)inner->mv_offsets.p;
    mw.n_queries = n_queries;
    mw.max_tokens = max_tokens;
    mw.del.n_rows = n_points;      // deletion is per POINT (the id tracker's bitslice over multi-vector points), not per inner row
    if (point_deleted && n_deleted_bits) {
        const void *d_bits = nullptr;
        QMX_TRY(stage_in(inner, inner->mv_deleted, point_deleted, (size_t)((n_deleted_bits + 63) / 64) * 8, &d_bits));
        mw.del.point_deleted = (const uint64_t *)d_bits;
        mw.del.n_point_bits = n_deleted_bits;
    }
    if (inner->has_filter) { mw.del.allowed = (const uint64_t *)inner->filter.p; mw.del.n_allowed_bits = inner->n_filter_bits; }
    qmx_scored_point *d_out = out;
    uint32_t *d_counts = out_counts;
    if (!out_dev) { QMX_TRY(inner->out.reserve((size_t)n_queries * top * sizeof(qmx_scored_point))); d_out = (qmx_scored_point *)inner->out.p; }
    if (!cnt_dev) { QMX_TRY(inner->counts.reserve((size_t)n_queries * 4)); d_counts = (uint32_t *)inner->counts.p; }
    QMX_TRY(inner->hnsw_scored.reserve((size_t)n_queries * 4));
    const bool timed = inner->timing || (s->flags & QMX_SEG_TIME_KERNELS) != 0;
    QMX_TRY(hnsw_enqueue(g, inner, top, ef, d_out, d_counts, (uint32_t *)inner->hnsw_scored.p, timed, false, &mw));
    if (!out_dev) QMX_TRY(copy_out(inner->stream, out, d_out, (size_t)n_queries * top * sizeof(qmx_scored_point)));
    if (!cnt_dev) QMX_TRY(copy_out(inner->stream, out_counts, d_counts, (size_t)n_queries * 4));
    QMX_TRY(check_err_flag(inner));    // synchronises (the staged partitions may go away)
    if (counters) {
        std::vector<uint32_t> sc(n_queries);
        QMX_HIP(hipMemcpy(sc.data(), inner->hnsw_scored.p, (size_t)n_queries * 4, hipMemcpyDeviceToHost));
        uint64_t total = 0;
        for (uint32_t v : sc) total += v;
        counters->vectors_scored = total;            // POINTS scored (each costs |query| x |point| inner scores)
        counters->kernel_launches = 1;
        if (timed) { const float before = inner->timing_ms; QMX_TRY(timing_fold(inner)); counters->kernel_ms = inner->timing_ms - before; }
    }
    return QMX_OK;
}

}  // extern "C"
