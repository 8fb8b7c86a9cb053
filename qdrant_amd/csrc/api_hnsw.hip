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


// ---- one walk (hnsw_enqueue): describe it, plan it (hnsw_walk_plan.hpp), set up what the plan names, launch ----
static WalkShape walk_shape(const qmx_hnsw *g, const qmx_query *q, const WalkRequest &r, const ScanArgs &a) {
    const qmx_segment *s = q->seg;
    WalkShape w;
    w.acorn = r.acorn; w.expanded = r.expanded != nullptr; w.multi = r.multi != nullptr; w.custom = r.custom != nullptr; w.traced = r.trace != nullptr;
    w.filters = q->has_filters;
    w.storage = s->dtype == QMX_DTYPE_PQ ? WalkStorage::PQ : tq_l1(s) ? WalkStorage::TqL1 : WalkStorage::Other;
    w.dim = s->dim;
    if (w.storage == WalkStorage::PQ) {
        w.pq_m = s->pq_m;
        w.n_centroids = s->pq.n_centroids;
        w.pq_direct_ok = s->d_centroids && pq_direct_walk_ok(s->dim, s->pq_m, s->pq.chunk_size, s->pq.n_centroids);
    }
    if (w.storage == WalkStorage::TqL1) {
        w.tq_l1_entry_bytes = tq_l1_query_bytes(s->dim);
        w.tq_l1_lds_bytes = tq_l1_lds_bytes(s->dim, s->tq_rot_dim);
    }
    w.q_stride = q->q_stride; w.top = r.top; w.ef = r.ef;
    w.batch_entries = a.queries == q->d_queries;
    w.n_points = g->n_points; w.m0 = g->m0; w.max_row0 = g->max_row0;
    if (r.multi) w.max_tokens = r.multi->max_tokens;
    if (r.custom) { w.max_examples = r.custom->max_examples; w.custom_lds_bytes = r.custom->lds_bytes; }
    w.opt_pq_direct_walk = option(OPT_HNSW_PQ_DIRECT_WALK) > 0;
    w.opt_reference_heap_order = option(OPT_HNSW_REFERENCE_HEAP_ORDER) > 0;
    w.opt_no_lds_visited = option(OPT_HNSW_NO_LDS_VISITED) != 0;
    w.opt_no_pq_prefilter = option(OPT_HNSW_NO_PQ_PREFILTER) != 0;
    w.opt_log_cap = option(OPT_HNSW_LOG_CAP);
    return w;
}

static int32_t walk_refused(const WalkPlan &p, const WalkShape &w) {
    const unsigned long long bytes = p.refused_bytes;
    switch (p.refusal) {
    case WalkRefusal::None: return QMX_OK;
    case WalkRefusal::TqL1Multi: set_error("multi-vector walks through a TurboQuant storage over Manhattan are not built"); break;
    // (custom and multi-vector walks, whose searches are not the batch's entries, and the expanded-candidates walk of search_with_vectors refuse a batch
    // with per-request filters at their entry points - this is the backstop)
    case WalkRefusal::Filters: set_error("this walk does not serve per-request filters (qmx_query_set_filters)"); break;
    case WalkRefusal::Trace: set_error("the pop trace is the plain walk's"); break;
    case WalkRefusal::TqL1Lds: set_error("TurboQuant over Manhattan, the walk: %u bytes of LDS per search", (uint32_t)bytes); break;
    case WalkRefusal::CustomTqL1Lds: set_error("a custom query of %u examples over TurboQuant / Manhattan needs %llu bytes of LDS", w.max_examples, bytes); break;
    case WalkRefusal::CustomTokensLds: set_error("a custom query of %u bytes of example tokens does not fit the LDS", (uint32_t)bytes); break;
    case WalkRefusal::BeamLds:
        set_error("hnsw max(top, ef) = %u: the query entry (%u bytes) and the list do not fit the LDS together", std::max(w.top, w.ef), p.entry_stride);
        break;
    case WalkRefusal::AcornM0: set_error("ACORN walk: m0 = %u not in 1..128", w.m0); break;
    case WalkRefusal::AcornRow: set_error("ACORN walk: a level-0 list of %u links does not fit the LDS", w.max_row0); break;
    }
    return QMX_ERR_NOT_SUPPORTED;
}

// the query entries as the walk reads them, where they are not the batch's
static int32_t stage_walk_entries(qmx_query *q, const WalkPlan &p, ScanArgs &a) {
    const qmx_segment *s = q->seg;
    if (tq_l1(s)) {   // the walk scores against the query as given (tq_l1_policy.hpp): f32 entries of dim floats, 16-byte padded
        const size_t qs = p.entry_stride;
        QMX_TRY(q->tq_rot.reserve((size_t)q->nq * qs));
        QMX_HIP(hipMemsetAsync(q->tq_rot.p, 0, (size_t)q->nq * qs, q->stream));
        QMX_HIP(hipMemcpy2DAsync(q->tq_rot.p, qs, q->enc.p, (size_t)s->dim * 4, (size_t)s->dim * 4, q->nq, hipMemcpyDeviceToDevice, q->stream));
        a.queries = q->tq_rot.p;
    }
    // PQ: the LUT-free walk (pq.hip HopPQDirect) - the entry of a search is its preprocessed vector (q->enc keeps them)
    if (p.pq_direct) a.queries = q->enc.p;
    a.q_stride = p.entry_stride;
    return QMX_OK;
}

static int32_t fill_sq_level0(const qmx_segment *s, const uint32_t *d_l0, uint32_t n_points, uint32_t l0_stride, hipStream_t st, uint32_t *table) {
    QMX_TRY(launch_hnsw_pack_level0_aux(st, d_l0, n_points, l0_stride, s->d_row_offsets, s->n, table));
    QMX_HIP(hipStreamSynchronize(st));      // (other threads' streams read it once the lock is gone)
    return QMX_OK;
}
int32_t SqLevel0Table::for_segment(const qmx_segment *s, const uint32_t *d_l0, uint32_t n_points, uint32_t l0_stride, hipStream_t st, const uint32_t **table) {
    *table = nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!d_table && !failed) {      // the first SQ segment walked over this graph
        uint32_t *fresh = nullptr;
        if (hipMalloc((void **)&fresh, (size_t)n_points * (2 * (l0_stride - 1)) * 4) != hipSuccess) {
            (void)hipGetLastError();
            failed = true;
            return QMX_OK;
        }
        const int32_t rc = fill_sq_level0(s, d_l0, n_points, l0_stride, st, fresh);
        if (rc != QMX_OK) {         // (a table that was not completed is nobody's)
            (void)hipFree(fresh);
            failed = true;
            return rc;
        }
        d_table = fresh;
        owner_uid = s->uid;
    }
    if (d_table && owner_uid == s->uid) *table = d_table;
    return QMX_OK;
}

// the graph's tables, its shape, and the capacities the plan chose
static int32_t bind_graph(const qmx_hnsw *g, const qmx_query *q, const WalkRequest &r, const WalkPlan &p, HnswArgs &h) {
    const qmx_segment *s = q->seg;
    h.reindex = g->d_reindex; h.level_offsets = g->d_level_offsets; h.offsets = g->d_offsets; h.neighbors = g->d_neighbors;
    h.l0 = g->d_l0; h.l0_stride = g->l0_stride;
    // SQ segments, plain walk over a packed level 0: the link rows bring the linked rows' vector_offset along, where the graph's table is this segment's
    const bool plain = !r.acorn && !r.expanded && !r.multi && !r.custom && !p.ref_heaps;
    if (s->dtype == QMX_DTYPE_SQ_U8 && g->d_l0 && plain && s->d_row_offsets && g->n_points <= s->n) {
        const uint32_t *l0x = nullptr;
        QMX_TRY(g->l0x.for_segment(s, g->d_l0, g->n_points, g->l0_stride, q->stream, &l0x));
        if (l0x) {
            h.l0 = l0x;
            h.l0_aux_off = g->l0_stride - 1;               // = m0: the row is [m0 link slots][m0 offsets]
            h.l0_stride = 2 * (g->l0_stride - 1);
        }
    }
    h.n_offsets = g->n_offsets; h.n_neighbors = g->n_neighbors;
    h.n_points = g->n_points; h.n_levels = g->n_levels; h.m = g->m; h.m0 = g->m0;
    h.ep_ids = g->d_ep_ids; h.ep_levels = g->d_ep_levels; h.n_ep = g->n_ep;
    h.xp_ids = g->d_xp_ids; h.xp_levels = g->d_xp_levels; h.n_xp = g->n_xp;
    h.acorn = r.acorn ? 1 : 0;
    h.ref_heaps = p.ref_heaps ? 1 : 0;      // option hnsw_reference_heap_order: the plain walk keeps the reference's two binary heaps (hnsw.hpp RefHeaps)
    h.ref_cap = HNSW_REF_CAND_CAP;
    h.lds_query_bytes = p.lds_query_bytes;
    h.vis_lds = p.vis_lds;                  // the visited set in LDS (hnsw.hpp LdsVisited)
    h.vis_words = p.vis_words; h.log_cap = p.log_cap; h.hop_cap = p.hop_cap; h.explore_cap = p.explore_cap; h.ev_cap = p.ev_cap;
    return QMX_OK;
}

// the 8-bit images of the searches' LUTs for the PQ walk's hop prefilter (pq.hip HopPQ::prefilter); their 24 KiB per search take the LDS the visited table
// would.  The LUT-free walk (HopPQDirect) prefilters on the image of the EXACT-ORDER LUT - the entries it recomputes: a batch whose LUTs came from the
// matrix cores (<= 1e-5 off that order) gets exact-order LUTs made for the image alone
static int32_t build_pq_image(qmx_query *q, const WalkPlan &p, uint32_t n_searches, HnswArgs &h) {
    if (p.pq_image == PqImage::None) return QMX_OK;
    const qmx_segment *s = q->seg;
    const void *luts = q->d_queries;
    uint32_t lstride = q->q_stride;
    const bool dotlike = s->distance == QMX_DISTANCE_DOT || s->distance == QMX_DISTANCE_COSINE;
    if (p.pq_image == PqImage::ExactOrderLuts && s->pq.lut_mfma && dotlike) {
        const size_t lut_bytes = (size_t)s->pq_m * s->pq.n_centroids * sizeof(float);
        qmx_pq_params exact = s->pq;
        exact.lut_mfma = 0;
        QMX_TRY(q->hnsw_lutx.reserve((size_t)n_searches * lut_bytes));
        QMX_TRY(launch_pq_lut(q->stream, s->distance, s->dim, exact, s->d_centroids, (const float *)q->enc.p, n_searches, (float *)q->hnsw_lutx.p));
        luts = q->hnsw_lutx.p;
        lstride = (uint32_t)lut_bytes;
    }
    const uint32_t st8 = pq_walk_lut8_stride(s->pq_m);
    QMX_TRY(q->hnsw_pq8.reserve((size_t)n_searches * st8));
    QMX_TRY(launch_pq_walk_lut8(q->stream, luts, lstride, n_searches, s->pq_m, s->pq.n_centroids, q->hnsw_pq8.p));
    h.pq8 = (const unsigned char *)q->hnsw_pq8.p;
    h.pq8_stride = st8;
    return QMX_OK;
}

// the handle's scratch for `ws.slots` searches in flight: visited bitmaps and logs, the spill / reference candidates, the work counter
static int32_t bind_walk_scratch(qmx_query *q, const WalkSlots &ws, HnswArgs &h) {
    if (h.ev_cap) {      // search_with_vectors: a slot's stack of evicted candidates that tie with the bound (hnsw.hpp; the reference keeps every one of them in `candidates`)
        QMX_TRY(q->hnsw_refc.reserve((size_t)ws.slots * h.ev_cap * sizeof(uint64_t)));
        h.ev_spill = (uint64_t *)q->hnsw_refc.p;
    }
    if (h.ref_heaps) {
        QMX_TRY(q->hnsw_refc.reserve((size_t)ws.slots * h.ref_cap * sizeof(uint2)));
        h.ref_cands = (uint2 *)q->hnsw_refc.p;
    }
    if (q->hnsw_slots < ws.slots || q->hnsw_vis_words != h.vis_words) {
        // (re)allocate for the largest slot count this handle can use, zero once: the kernel returns the bitmaps all-zero
        QMX_HIP(hipStreamSynchronize(q->stream));
        q->hnsw_slots = 0;
        QMX_TRY(q->hnsw_vis.reserve((size_t)ws.want * h.vis_words * 4));
        QMX_TRY(q->hnsw_log.reserve((size_t)ws.want * HNSW_LOG_CAP * 4));
        QMX_HIP(hipMemsetAsync(q->hnsw_vis.p, 0, (size_t)ws.want * h.vis_words * 4, q->stream));
        q->hnsw_slots = (uint32_t)ws.want;
        q->hnsw_vis_words = h.vis_words;
    }
    h.visited = (uint32_t *)q->hnsw_vis.p;
    h.vis_log = (uint32_t *)q->hnsw_log.p;
    // the slots draw their searches from a counter that starts behind the first `slots` (hnsw.hpp)
    QMX_TRY(q->hnsw_next.reserve(32));         // [u32 next search][pad][u64 hop candidates offered to the PQ prefilter][u64 scored exactly]
    QMX_HIP(hipMemsetD32Async((hipDeviceptr_t)q->hnsw_next.p, (int)ws.slots, 1, q->stream));
    QMX_HIP(hipMemsetAsync((char *)q->hnsw_next.p + 8, 0, 16, q->stream));
    h.next_query = (uint32_t *)q->hnsw_next.p;
    h.pq_stats = h.pq8 ? (unsigned long long *)((char *)q->hnsw_next.p + 8) : nullptr;
    return QMX_OK;
}

int32_t hnsw_enqueue(const qmx_hnsw *g, qmx_query *q, const WalkRequest &r) {
    const qmx_segment *s = q->seg;
    ScanArgs a;
    fill_args(q, 0, q->nq, a);
    const WalkShape shape = walk_shape(g, q, r, a);
    const WalkPlan plan = hnsw_walk_plan(shape);
    QMX_TRY(walk_refused(plan, shape));
    QMX_TRY(stage_walk_entries(q, plan, a));
    const uint32_t n_searches = r.custom ? r.custom->n_queries : r.multi ? r.multi->n_queries : q->nq;
    if (r.custom) {
        a.cq_desc = r.custom->d_desc;
        a.cq_coefs = r.custom->d_coefs;
    }
    if (r.multi) {
        a.mv_offsets = r.multi->d_offsets;
        a.mv_qfirst = r.multi->d_qfirst;
        a.del = r.multi->del;
    }
    HnswArgs h;
    memset(&h, 0, sizeof(h));
    QMX_TRY(bind_graph(g, q, r, plan, h));
    h.ef = r.ef; h.top = r.top; h.nq = n_searches;
    h.out = r.d_out; h.out_counts = r.d_counts; h.out_scored = r.d_scored;
    if (r.expanded) { h.expanded = r.expanded->d_ids; h.expanded_cnt = r.expanded->d_cnt; h.xcap = r.expanded->xcap; }
    if (r.trace) { h.pops = r.trace->d_pops; h.pop_cnt = r.trace->d_cnt; h.pop_cap = r.trace->cap; }
    QMX_TRY(build_pq_image(q, plan, n_searches, h));
    int per_cu = 1;
    QMX_TRY(launch_hnsw(q, a, h, 0, &per_cu));      // (grid 0: the occupancy of the kernel this launch takes)
    WalkSlotOptions so;
    so.pq_per_cu = option(OPT_HNSW_PQ_PER_CU);
    so.per_cu = option(OPT_HNSW_PER_CU);
    const WalkSlots ws = hnsw_walk_slots(plan, per_cu, n_searches, q->nq, s->num_cus, so);
    per_cu = ws.per_cu;
    QMX_TRY(bind_walk_scratch(q, ws, h));
    size_t slot = 0;
    if (r.timed) QMX_TRY(timing_begin(q, &slot));
    QMX_TRY(launch_hnsw(q, a, h, (uint32_t)ws.slots, &per_cu));
    q->last_kernel = last_noted_kernel();
    if (r.timed) QMX_TRY(timing_end(q, slot));
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

int32_t hnsw_walk_to_caller(const qmx_hnsw *g, qmx_query *q, WalkRequest r, uint32_t n_searches, qmx_scored_point *out, uint32_t *out_counts,
                            qmx_counters *counters, bool plain) {
    const bool out_dev = is_device_ptr(out), cnt_dev = is_device_ptr(out_counts);
    const size_t out_bytes = (size_t)n_searches * r.top * sizeof(qmx_scored_point), cnt_bytes = (size_t)n_searches * 4;
    if (g->n_points == 0) {   // get_entry_point() -> None -> empty result (graph_layers.rs:539-542)
        if (cnt_dev) QMX_HIP(hipMemset(out_counts, 0, cnt_bytes));
        else memset(out_counts, 0, cnt_bytes);
        QMX_HIP(hipStreamSynchronize(q->stream));      // (what the caller staged for the walk may go away)
        return QMX_OK;
    }
    r.d_out = out;
    r.d_counts = out_counts;
    if (!out_dev) { QMX_TRY(q->out.reserve(out_bytes)); r.d_out = (qmx_scored_point *)q->out.p; }
    if (!cnt_dev) { QMX_TRY(q->counts.reserve(cnt_bytes)); r.d_counts = (uint32_t *)q->counts.p; }
    QMX_TRY(q->hnsw_scored.reserve(cnt_bytes));
    r.d_scored = (uint32_t *)q->hnsw_scored.p;
    r.timed = q->timing || (q->seg->flags & QMX_SEG_TIME_KERNELS) != 0;
    QMX_TRY(hnsw_enqueue(g, q, r));
    if (!out_dev) QMX_TRY(copy_out(q->stream, out, r.d_out, out_bytes));
    if (!cnt_dev) QMX_TRY(copy_out(q->stream, out_counts, r.d_counts, cnt_bytes));
    std::vector<uint32_t> scored(counters ? n_searches : 0);
    unsigned long long pq_stats[2] = {0, 0};
    if (counters) QMX_HIP(hipMemcpyAsync(scored.data(), r.d_scored, cnt_bytes, hipMemcpyDeviceToHost, q->stream));
    if (counters && plain) QMX_HIP(hipMemcpyAsync(pq_stats, (char *)q->hnsw_next.p + 8, 16, hipMemcpyDeviceToHost, q->stream));
    QMX_TRY(check_err_flag(q));   // synchronises the stream (what the caller staged for the walk may go away)
    if (counters) {
        uint64_t total = 0;
        for (uint32_t v : scored) total += v;
        counters->vectors_scored = total;      // custom / MaxSim walks: POINTS scored (each costs one similarity per example, |query| x |point| inner scores)
        counters->kernel_launches = 1;
        if (plain) {
            // the PQ walk's hop prefilter (hnsw.hpp HopPQ::prefilter): level-0 hop candidates that met the 8-bit bound / those that survived it and were scored exactly
            counters->prefilter_candidates = pq_stats[0];
            counters->verified_rows = pq_stats[1];
            counters->bytes_read = total * q->seg->row_bytes;
        }
    }
    if (r.timed && (counters || plain)) {      // (the plain walk folds its time into the batch's at once; the others leave it to the next fold when nobody asks)
        const float before = q->timing_ms;
        QMX_TRY(timing_fold(q));
        if (counters) counters->kernel_ms = q->timing_ms - before;
    }
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
    WalkRequest r;
    r.top = top; r.ef = ef; r.acorn = acorn;
    return hnsw_walk_to_caller(g, q, r, q->nq, out, out_counts, counters, true);
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
    WalkRequest r;
    r.d_out = (qmx_scored_point *)q->out.p; r.d_counts = (uint32_t *)q->counts.p;
    r.top = top; r.ef = ef; r.trace = &pt;
    QMX_TRY(hnsw_enqueue(g, q, r));
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
    WalkRequest r;
    r.d_out = out_dev; r.d_counts = out_counts_dev; r.d_scored = out_scored_dev;
    r.top = top; r.ef = ef;
    r.timed = q->timing || (q->seg->flags & QMX_SEG_TIME_KERNELS) != 0;
    return hnsw_enqueue(g, q, r);
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
        WalkRequest r;
        r.d_out = (qmx_scored_point *)links->cand.p; r.d_counts = (uint32_t *)links->cand_cnt.p; r.d_scored = (uint32_t *)links->hnsw_scored.p;
        r.top = std::min(top, beam_ef); r.ef = ef; r.timed = timed; r.expanded = &xo;
        QMX_TRY(hnsw_enqueue(g, links, r));
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

int32_t stage_multi_walk(qmx_query *inner, const uint32_t *first, uint32_t n_first, const uint64_t *point_offsets, uint32_t n_points,
                         const uint64_t *point_deleted, uint64_t n_deleted_bits, MultiWalk *mw) {
    for (uint32_t p = 0; p < n_points; ++p)
        QMX_REQUIRE(point_offsets[p] <= point_offsets[p + 1], QMX_ERR_BAD_ARG, "point_offsets is not ascending at %u", p);
    QMX_REQUIRE(point_offsets[n_points] <= inner->seg->n, QMX_ERR_OUT_OF_BOUNDS, "point_offsets reach past the %llu inner rows of the segment",
                (unsigned long long)inner->seg->n);
    QMX_TRY(inner->mv_qfirst.reserve((size_t)(n_first + 1) * 4));
    QMX_TRY(inner->mv_offsets.reserve((size_t)(n_points + 1) * 8));
    QMX_HIP(hipMemcpyAsync(inner->mv_qfirst.p, first, (size_t)(n_first + 1) * 4, hipMemcpyHostToDevice, inner->stream));
    QMX_HIP(hipMemcpyAsync(inner->mv_offsets.p, point_offsets, (size_t)(n_points + 1) * 8, hipMemcpyHostToDevice, inner->stream));
    memset(mw, 0, sizeof(*mw));
    mw->d_qfirst = (const uint32_t *)inner->mv_qfirst.p;
    mw->d_offsets = (const uint64_t *)inner->mv_offsets.p;
    mw->del.n_rows = n_points;      // deletion is per POINT (the id tracker's bitslice over multi-vector points), not per inner row
    if (point_deleted && n_deleted_bits) {
        const void *d_bits = nullptr;
        QMX_TRY(stage_in(inner, inner->mv_deleted, point_deleted, (size_t)((n_deleted_bits + 63) / 64) * 8, &d_bits));
        mw->del.point_deleted = (const uint64_t *)d_bits;
        mw->del.n_point_bits = n_deleted_bits;
    }
    if (inner->has_filter) { mw->del.allowed = (const uint64_t *)inner->filter.p; mw->del.n_allowed_bits = inner->n_filter_bits; }
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
    MultiWalk mw;
    uint32_t max_tokens = 0;
    for (uint32_t j = 0; j < n_queries; ++j) {
        QMX_REQUIRE(query_first[j] <= query_first[j + 1], QMX_ERR_BAD_ARG, "query_first is not ascending at %u", j);
        max_tokens = std::max(max_tokens, query_first[j + 1] - query_first[j]);
    }
    QMX_TRY(stage_multi_walk(inner, query_first, n_queries, point_offsets, n_points, point_deleted, n_deleted_bits, &mw));
    mw.n_queries = n_queries;
    mw.max_tokens = max_tokens;
    WalkRequest r;
    r.top = top; r.ef = ef; r.multi = &mw;
    return hnsw_walk_to_caller(g, inner, r, n_queries, out, out_counts, counters, false);
}

}  // extern "C"
