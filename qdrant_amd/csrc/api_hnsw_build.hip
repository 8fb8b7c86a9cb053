// api_hnsw_build.hip — the C-ABI of include/qdrant_amd.h, the HNSW build on the device (hnsw_build.hpp): one segment, segments side by side, multi-vector points.
// (One of the api_*.hip translation units; what it shares with the payload-block build: api_hnsw_build.hpp.)
#include "api_hnsw_build.hpp"
#include <algorithm>
#include <atomic>

extern "C" {

static inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static int32_t launch_hnsw_build_any(const qmx_segment *seg, const ScanArgs &a, const HnswBuildArgs &h, int phase, uint32_t grid, int *per_cu) {
    if (a.mv_offsets) {   // multi-vector points (qmx_multi_hnsw_build)
        if (seg->dtype == QMX_DTYPE_SQ_U8) return launch_hnsw_build_maxsim_sq(nullptr, (int)seg->distance, a, h, phase, grid, per_cu);
        if (seg->dtype == QMX_DTYPE_BQ) return launch_hnsw_build_maxsim_bq(nullptr, a, h, phase, grid, per_cu);
        if (seg->dtype == QMX_DTYPE_PQ) return launch_hnsw_build_maxsim_pq(nullptr, a, h, phase, grid, per_cu);
        if (seg->dtype == QMX_DTYPE_TQ) return launch_hnsw_build_maxsim_tq(nullptr, a, h, phase, grid, per_cu);
        return launch_hnsw_build_maxsim_dense(nullptr, (int)seg->dtype, (int)seg->distance, a, h, phase, grid, per_cu);
    }
    if (seg->dtype == QMX_DTYPE_SQ_U8) return launch_hnsw_build_sq(nullptr, (int)seg->distance, a, h, phase, grid, per_cu);
    if (seg->dtype == QMX_DTYPE_BQ) return launch_hnsw_build_bq(nullptr, a, h, phase, grid, per_cu);
    if (seg->dtype == QMX_DTYPE_PQ) return launch_hnsw_build_pq(nullptr, a, h, phase, grid, per_cu);
    if (tq_l1(seg)) return launch_hnsw_build_tq_l1(nullptr, a, h, phase, grid, per_cu, seg->tq_rot_dim, seg->tq_padded_dim);
    if (seg->dtype == QMX_DTYPE_TQ) return launch_hnsw_build_tq(nullptr, a, h, phase, grid, per_cu);
    return launch_hnsw_build_dense(nullptr, (int)seg->dtype, (int)seg->distance, a, h, phase, grid, per_cu);
}

int32_t qmx_hnsw_build(const qmx_segment *seg, const qmx_hnsw_build_params *bp, qmx_hnsw **out) {
    QMX_REFUSE_SPARSE(seg);
    return qmx_hnsw_build_quantized(seg, nullptr, bp, out);
}

static int32_t hnsw_build_impl(const qmx_segment *seg, const qmx_segment *original, const qmx_hnsw_build_params *bp, qmx_hnsw **out, const MultiBuild *mb);

int32_t qmx_hnsw_build_quantized(const qmx_segment *seg, const qmx_segment *original, const qmx_hnsw_build_params *bp, qmx_hnsw **out) {
    QMX_REFUSE_SPARSE(seg);
    QMX_REFUSE_SPARSE(original);
    return hnsw_build_impl(seg, original, bp, out, nullptr);
}

// Build fan-out over independent segments (gpu_devices_manager.rs:120-143 + hnsw/build.rs:53: one device locked per segment build, builds share nothing):
// one host thread per segment, each driving its segment's device; the thread's own error text travels back with its status.
static int32_t sharded_hnsw_build_body(const qmx_segment *const *segments, const qmx_segment *const *originals, uint32_t n_segments,
                                       const qmx_hnsw_build_params *bp, qmx_hnsw **out_graphs, int32_t *out_status);
int32_t qmx_sharded_hnsw_build(const qmx_segment *const *segments, const qmx_segment *const *originals, uint32_t n_segments,
                               const qmx_hnsw_build_params *bp, qmx_hnsw **out_graphs, int32_t *out_status) {
    for (uint32_t i = 0; segments && i < n_segments; ++i) {
        QMX_REFUSE_SPARSE(segments[i]);
        if (originals) QMX_REFUSE_SPARSE(originals[i]);
    }
    try {
        return sharded_hnsw_build_body(segments, originals, n_segments, bp, out_graphs, out_status);
    } catch (...) {         // nothing C++ crosses the C ABI
        set_error("qmx_sharded_hnsw_build: out of host memory");
        return QMX_ERR_OUT_OF_MEMORY;
    }
}
static int32_t sharded_hnsw_build_body(const qmx_segment *const *segments, const qmx_segment *const *originals, uint32_t n_segments,
                                       const qmx_hnsw_build_params *bp, qmx_hnsw **out_graphs, int32_t *out_status) {
    QMX_REQUIRE(segments && bp && out_graphs && n_segments >= 1, QMX_ERR_BAD_ARG, "NULL argument");
    for (uint32_t i = 0; i < n_segments; ++i) {
        out_graphs[i] = nullptr;
        if (out_status) out_status[i] = QMX_OK;
    }
    for (uint32_t i = 0; i < n_segments; ++i) QMX_REQUIRE(segments[i], QMX_ERR_BAD_ARG, "segment %u: NULL", i);
    std::vector<int32_t> rcs(n_segments, QMX_OK);
    std::vector<std::string> errs(n_segments);
    auto work = [&](uint32_t i) {
        try {
            rcs[i] = hnsw_build_impl(segments[i], originals ? originals[i] : nullptr, bp, &out_graphs[i], nullptr);
            if (rcs[i] != QMX_OK) errs[i] = last_error_text();          // (thread-local: copied out before the thread ends)
        } catch (...) {     // (bad_alloc of a host vector inside the build: a status, not a terminate)
            rcs[i] = QMX_ERR_OUT_OF_MEMORY;
        }
    };
    if (n_segments == 1) {
        work(0);
    } else {
        // One worker thread per DEVICE x QMX_BUILDS_PER_DEVICE (the reference locks one GPU of its pool per segment build, gpu_devices_manager.rs:120-143;
        // here a device takes up to two builds at once: each holds its full scratch - visited bitmaps, selection buffers - so the count is bounded).
        // Workers draw segments of their device from a shared cursor.  No C++ exception leaves this extern "C" function: a thread that cannot be
        // started leaves its share to the calling thread, which runs whatever is left inline after joining the rest.
        constexpr uint32_t QMX_BUILDS_PER_DEVICE = 2;
        std::vector<int> devs;
        for (uint32_t i = 0; i < n_segments; ++i)
            if (std::find(devs.begin(), devs.end(), segments[i]->device) == devs.end()) devs.push_back(segments[i]->device);
        std::vector<std::atomic<uint32_t>> cursor(devs.size());
        for (auto &c : cursor) c.store(0);
        auto drain = [&](size_t d) {      // the next unbuilt segment of device d, until none is left
            for (;;) {
                const uint32_t start = cursor[d].fetch_add(1);
                uint32_t seen = 0, pick = n_segments;
                for (uint32_t i = 0; i < n_segments; ++i)
                    if (segments[i]->device == devs[d] && seen++ == start) { pick = i; break; }
                if (pick == n_segments) return;
                work(pick);
            }
        };
        std::vector<std::thread> pool;
        try {
            pool.reserve(devs.size() * QMX_BUILDS_PER_DEVICE);
            for (size_t d = 0; d < devs.size(); ++d)
                for (uint32_t k = 0; k < QMX_BUILDS_PER_DEVICE; ++k) pool.emplace_back(drain, d);
        } catch (...) {
            // (std::system_error from the thread constructor, bad_alloc: keep what started)
        }
        for (auto &t : pool)
            if (t.joinable()) t.join();
        for (size_t d = 0; d < devs.size(); ++d) drain(d);      // whatever no worker took (all of it if no thread could be started)
    }
    int32_t first = QMX_OK;
    for (uint32_t i = 0; i < n_segments; ++i) {
        if (out_status) out_status[i] = rcs[i];
        if (rcs[i] != QMX_OK && first == QMX_OK) {
            first = rcs[i];
            set_error("segment %u: %s", i, errs[i].c_str());
        }
    }
    return first;
}

int32_t qmx_multi_hnsw_build_quantized(const qmx_segment *inner, const qmx_segment *original_inner, const uint64_t *point_offsets, uint32_t n_points,
                                       const uint64_t *point_deleted, uint64_t n_deleted_bits, const qmx_hnsw_build_params *bp, qmx_hnsw **out) {
    QMX_REFUSE_SPARSE(inner);
    QMX_REFUSE_SPARSE(original_inner);
    QMX_REQUIRE(inner && point_offsets && bp && out, QMX_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    QMX_REQUIRE(inner->dtype == QMX_DTYPE_F32 || inner->dtype == QMX_DTYPE_F16 || inner->dtype == QMX_DTYPE_SQ_U8 || inner->dtype == QMX_DTYPE_BQ ||
                    inner->dtype == QMX_DTYPE_PQ || (inner->dtype == QMX_DTYPE_TQ && !tq_l1(inner)),
                QMX_ERR_NOT_SUPPORTED, "device HNSW build over multi-vectors: inner dtype %u not supported (f32, f16, SQ, BQ, PQ, TurboQuant except over Manhattan)",
                inner->dtype);
    QMX_REQUIRE(!is_device_ptr(point_offsets) && !is_device_ptr(point_deleted), QMX_ERR_BAD_ARG, "point_offsets and point_deleted are host arrays");
    for (uint32_t p = 0; p < n_points; ++p)
        QMX_REQUIRE(point_offsets[p] <= point_offsets[p + 1], QMX_ERR_BAD_ARG, "point_offsets is not ascending at %u", p);
    QMX_REQUIRE(point_offsets[n_points] <= inner->n, QMX_ERR_OUT_OF_BOUNDS, "point_offsets reach past the %llu inner rows of the segment",
                (unsigned long long)inner->n);
    const MultiBuild mb{point_offsets, n_points, (point_deleted && n_deleted_bits) ? point_deleted : nullptr, point_deleted ? n_deleted_bits : 0};
    return hnsw_build_impl(inner, (inner->dtype == QMX_DTYPE_PQ || inner->dtype == QMX_DTYPE_TQ) ? original_inner : nullptr, bp, out, &mb);
}
int32_t qmx_multi_hnsw_build(const qmx_segment *inner, const uint64_t *point_offsets, uint32_t n_points, const uint64_t *point_deleted,
                             uint64_t n_deleted_bits, const qmx_hnsw_build_params *bp, qmx_hnsw **out) {
    QMX_REFUSE_SPARSE(inner);
    return qmx_multi_hnsw_build_quantized(inner, nullptr, point_offsets, n_points, point_deleted, n_deleted_bits, bp, out);
}

// what the device phase of a build leaves on the host: the fixed-capacity link lists and the entry points
struct BuiltLinks {
    std::vector<uint32_t> links0, cnt0, linksU, cntU;
    bool have_ep = false;
    uint32_t ep_id = 0, ep_level = 0;
    std::vector<std::pair<uint32_t, uint32_t>> extra;   // (level, id)
};

// the insertions of a build on the device; its scratch lives as long as this call
static int32_t hnsw_build_links(const qmx_segment *seg, const qmx_segment *original, const qmx_hnsw_build_params *bp, const MultiBuild *mb, uint32_t n,
                                uint32_t max_batch, const std::vector<uint8_t> &level, const std::vector<uint32_t> &up_off, uint64_t n_up,
                                const HostLiveness &alive, BuiltLinks &r) {
    const uint32_t m = bp->m, m0 = bp->m0;
    const bool from_original = seg->dtype == QMX_DTYPE_PQ || seg->dtype == QMX_DTYPE_TQ;
    DevBuf b_level, b_upoff, b_links0, b_cnt0, b_linksU, b_cntU, b_lock, b_sel, b_sels, b_selc, b_mvoff, b_mvdel;
    U8RowNorms norms;
    BuildQueryEntries entries;
    InsertSlots slots;
    const size_t nn = std::max<uint32_t>(n, 1);
    QMX_TRY(b_level.reserve(nn)); QMX_TRY(b_upoff.reserve(nn * 4));
    QMX_TRY(b_links0.reserve(nn * m0 * 4)); QMX_TRY(b_cnt0.reserve(nn * 4));
    QMX_TRY(b_linksU.reserve(std::max<uint64_t>(n_up, 1) * m * 4)); QMX_TRY(b_cntU.reserve(std::max<uint64_t>(n_up, 1) * 4));
    QMX_TRY(b_lock.reserve(nn * 4));
    QMX_HIP(hipMemcpy(b_level.p, level.data(), nn, hipMemcpyHostToDevice));
    QMX_HIP(hipMemcpy(b_upoff.p, up_off.data(), nn * 4, hipMemcpyHostToDevice));
    QMX_HIP(hipMemset(b_cnt0.p, 0, nn * 4));
    QMX_HIP(hipMemset(b_cntU.p, 0, std::max<uint64_t>(n_up, 1) * 4));
    QMX_HIP(hipMemset(b_lock.p, 0, nn * 4));
    QMX_TRY(b_sel.reserve((size_t)max_batch * HNSW_BUILD_MAX_LEVELS * m0 * 4));
    QMX_TRY(b_sels.reserve((size_t)max_batch * HNSW_BUILD_MAX_LEVELS * m0 * 4));
    QMX_TRY(b_selc.reserve((size_t)max_batch * HNSW_BUILD_MAX_LEVELS * 4));

    ScanArgs a;
    fill_build_args(seg, a);
    if (mb) {   // the graph's points are multi-vectors: offsets into the inner rows, deletion per POINT (the inner rows carry no flags of their own)
        QMX_TRY(b_mvoff.reserve((size_t)(n + 1) * 8));
        QMX_HIP(hipMemcpy(b_mvoff.p, mb->h_offsets, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
        a.mv_offsets = (const uint64_t *)b_mvoff.p;
        DeletedView dv;
        memset(&dv, 0, sizeof(dv));
        dv.n_rows = n;
        if (!alive.pdel.empty()) {
            QMX_TRY(b_mvdel.reserve(alive.pdel.size() * 8));
            QMX_HIP(hipMemcpy(b_mvdel.p, alive.pdel.data(), alive.pdel.size() * 8, hipMemcpyHostToDevice));
            dv.point_deleted = (const uint64_t *)b_mvdel.p;
            dv.n_point_bits = mb->n_deleted_bits;
        }
        a.del = dv;
    }
    HnswBuildArgs h;
    memset(&h, 0, sizeof(h));
    h.g.links0 = (uint32_t *)b_links0.p; h.g.cnt0 = (uint32_t *)b_cnt0.p; h.g.linksU = (uint32_t *)b_linksU.p; h.g.cntU = (uint32_t *)b_cntU.p;
    h.g.up_off = (const uint32_t *)b_upoff.p; h.g.m = m; h.g.m0 = m0;
    h.level = (const uint8_t *)b_level.p;
    h.n_points = n;
    h.ef_construct = bp->ef_construct;
    h.sel_ids = (uint32_t *)b_sel.p; h.sel_scores = (float *)b_sels.p; h.sel_cnt = (uint32_t *)b_selc.p;
    h.lock = (uint32_t *)b_lock.p;
    const uint64_t dev_row_bytes = stage_stored_rows(seg, h);
    uint64_t max_entries = max_batch;      // query entries a batch may need: one per point - or, multi-vector points, one per inner vector
    if (from_original) {
        if (mb) {   // at least the longest point, at most 1 GiB of LUTs / 256 MiB of rotated vectors (the insertion loop shortens a batch that would need more)
            const uint64_t entry_bytes = seg->dtype == QMX_DTYPE_PQ ? BuildQueryEntries::pq_lut_stride(seg) : (uint64_t)seg->tq_padded_dim * sizeof(double);
            const uint64_t budget = seg->dtype == QMX_DTYPE_PQ ? 1ull << 30 : 1ull << 28;
            uint64_t longest = 1;
            for (uint32_t p = 0; p < n; ++p) longest = std::max<uint64_t>(longest, mb->h_offsets[p + 1] - mb->h_offsets[p]);
            max_entries = std::max<uint64_t>(longest, std::min<uint64_t>(mb->h_offsets[n] ? mb->h_offsets[n] : 1, budget / entry_bytes));
            if (seg->dtype == QMX_DTYPE_PQ) a.q_stride = (uint32_t)BuildQueryEntries::pq_lut_stride(seg);
        }
        QMX_TRY(entries.reserve(seg, a, h, max_entries, !mb));
        if (tq_l1(seg)) {   // over Manhattan the entry is the original vector as given (quantization.rs:532-535), its hop scratch behind it in LDS (tq_l1_policy.hpp)
            a.tq_l1 = seg->d_tq_l1;
            a.q_stride = tq_l1_query_bytes(seg->dim);
            QMX_TRY(entries.b_bq.reserve((size_t)max_batch * a.q_stride));
            h.batch_queries = (const unsigned char *)entries.b_bq.p;
            h.batch_q_stride = a.q_stride;
            h.lds_query_bytes = tq_l1_lds_bytes(seg->dim, seg->tq_rot_dim);
        }
    }
    if (mb) h.lds_query_bytes = 0;      // nothing staged: the inner rows of the new point are read where they lie
    QMX_TRY(norms.attach(seg, n, a));
    QMX_TRY(check_row_query_slot(h.lds_query_bytes, dev_row_bytes));
    QMX_TRY(slots.reserve(seg, h, n, max_batch, [&](int phase, uint32_t grid, int *per_cu) { return launch_hnsw_build_any(seg, a, h, phase, grid, per_cu); }));

    // ---- insertion loop ----
    // EntryPoints (entry_points.rs:46-94) kept on the host: the live point of the highest level seen first is the
    // entry; the `entry_points_num` highest others are the extra entries
    bool &have_ep = r.have_ep;
    uint32_t &ep_id = r.ep_id, &ep_level = r.ep_level, inserted = 0;
    std::vector<std::pair<uint32_t, uint32_t>> &extra = r.extra;
    auto note_point = [&](uint32_t id) {
        const uint32_t lv = level[id];
        if (!have_ep) { have_ep = true; ep_id = id; ep_level = lv; return; }
        std::pair<uint32_t, uint32_t> other(lv, id);
        if (lv > ep_level) { other = {ep_level, ep_id}; ep_id = id; ep_level = lv; }
        if (bp->entry_points_num == 0) return;
        if (extra.size() < bp->entry_points_num) { extra.push_back(other); return; }
        size_t lo = 0;
        for (size_t i = 1; i < extra.size(); ++i) if (extra[i].first < extra[lo].first) lo = i;
        if (extra[lo].first < other.first) extra[lo] = other;
    };
    uint32_t next = 0;
    while (next < n) {
        if (!have_ep) {                      // the first live point: nothing to link to
            if (alive.live(next)) { note_point(next); ++inserted; }
            ++next;
            continue;
        }
        uint32_t count = std::min<uint32_t>({max_batch, std::max<uint32_t>(1, inserted / 32), n - next});
        // a point above the current top level ends its batch: the next batch starts from it
        for (uint32_t i = 0; i < count; ++i)
            if (level[next + i] > ep_level && alive.live(next + i)) { count = i + 1; break; }
        if (mb && from_original)      // the batch's inner vectors must fit the entries (a single point always does)
            while (count > 1 && mb->h_offsets[next + count] - mb->h_offsets[next] > max_entries) --count;
        h.first = next; h.count = count; h.ep_id = ep_id; h.ep_level = ep_level;
        if (tq_l1(seg)) {   // EncodedVectorsTQ over Manhattan: no preprocessing, no rotation - the rows themselves, zero padded to whole 16 bytes
            QMX_HIP(hipMemsetAsync(entries.b_bq.p, 0, (size_t)count * a.q_stride, nullptr));
            QMX_HIP(hipMemcpy2DAsync(entries.b_bq.p, a.q_stride, (const char *)original->d_rows + (uint64_t)next * original->row_stride, original->row_stride,
                                (size_t)seg->dim * 4, count, hipMemcpyDeviceToDevice, nullptr));
        } else if (from_original) {      // one entry per point of the batch (multi-vector points: per inner vector of the batch's points, in storage order)
            const uint64_t r0 = mb ? mb->h_offsets[next] : next, nr = mb ? mb->h_offsets[next + count] - r0 : count;
            QMX_TRY(entries.make(seg, original, a, r0, nullptr, nr));
        }
        uint32_t grid1, grid2;
        QMX_TRY(slots.begin_batch(count, &grid1, &grid2));
        int per_cu = 1;
        QMX_TRY(launch_hnsw_build_any(seg, a, h, 1, grid1, &per_cu));
        QMX_TRY(launch_hnsw_build_any(seg, a, h, 2, grid2, &per_cu));
        for (uint32_t i = 0; i < count; ++i)
            if (alive.live(next + i)) { note_point(next + i); ++inserted; }
        next += count;
    }
    QMX_HIP(hipDeviceSynchronize());

    r.links0.resize((size_t)nn * m0);
    r.cnt0.resize(nn);
    r.linksU.resize(std::max<uint64_t>(n_up, 1) * m);
    r.cntU.resize(std::max<uint64_t>(n_up, 1));
    QMX_HIP(hipMemcpy(r.links0.data(), b_links0.p, r.links0.size() * 4, hipMemcpyDeviceToHost));
    QMX_HIP(hipMemcpy(r.cnt0.data(), b_cnt0.p, r.cnt0.size() * 4, hipMemcpyDeviceToHost));
    QMX_HIP(hipMemcpy(r.linksU.data(), b_linksU.p, r.linksU.size() * 4, hipMemcpyDeviceToHost));
    QMX_HIP(hipMemcpy(r.cntU.data(), b_cntU.p, r.cntU.size() * 4, hipMemcpyDeviceToHost));
    return QMX_OK;
}

static int32_t hnsw_build_impl(const qmx_segment *seg, const qmx_segment *original, const qmx_hnsw_build_params *bp, qmx_hnsw **out, const MultiBuild *mb) {
    QMX_REQUIRE(seg && bp && out, QMX_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    QMX_TRY(build_check_segment(seg, original, "device HNSW build", " to qmx_hnsw_build_quantized", !mb));
    QMX_REQUIRE(bp->m >= 1 && bp->m0 >= bp->m && bp->m0 <= HNSW_BUILD_MAX_M0, QMX_ERR_BAD_ARG, "need 1 <= m <= m0 <= %u", HNSW_BUILD_MAX_M0);
    QMX_REQUIRE(bp->ef_construct >= 1 && bp->ef_construct <= HNSW_MAX_EF, QMX_ERR_NOT_SUPPORTED, "ef_construct %u not in 1..%u",
                bp->ef_construct, HNSW_MAX_EF);
    QMX_REQUIRE(seg->n <= 0xFFFFFFFFull, QMX_ERR_BAD_ARG, "too many rows");
    QMX_HIP(hipSetDevice(seg->device));
    const uint32_t n = mb ? mb->n_points : (uint32_t)seg->n, m = bp->m, m0 = bp->m0;
    const uint32_t max_batch = bp->max_batch ? bp->max_batch : 16384;

    // ---- levels (graph_layers_builder.rs:388-396), the same draw as the CPU oracle ----
    std::vector<uint8_t> level(std::max<uint32_t>(n, 1));
    std::vector<uint32_t> up_off(std::max<uint32_t>(n, 1));
    const double level_factor = 1.0 / log((double)(m > 2 ? m : 2));
    uint64_t n_up = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t r = splitmix64(bp->seed ^ (0xA0761D6478BD642Full * ((uint64_t)i + 1)));
        const double u = ((double)(r >> 11) + 0.5) * (1.0 / 9007199254740992.0);
        double lv = round(-log(u) * level_factor);
        if (lv > (double)(HNSW_BUILD_MAX_LEVELS - 1)) lv = HNSW_BUILD_MAX_LEVELS - 1;
        level[i] = (uint8_t)lv;
        up_off[i] = (uint32_t)n_up;
        n_up += level[i];
    }
    QMX_REQUIRE(n_up <= 0xFFFFFFFFull, QMX_ERR_BAD_ARG, "too many upper-level lists");
    // deleted flags on the host: deleted points are never indexed and never entry points
    HostLiveness alive;
    if (mb) alive.load(*mb);
    else QMX_TRY(alive.load(seg));

    // ---- device state and the insertion loop ----
    BuiltLinks r;
    QMX_TRY(hnsw_build_links(seg, original, bp, mb, n, max_batch, level, up_off, n_up, alive, r));
    const std::vector<uint32_t> &links0 = r.links0, &cnt0 = r.cnt0, &linksU = r.linksU, &cntU = r.cntU;
    const bool have_ep = r.have_ep;
    const uint32_t ep_id = r.ep_id, ep_level = r.ep_level;
    const std::vector<std::pair<uint32_t, uint32_t>> &extra = r.extra;
    const size_t nn = std::max<uint32_t>(n, 1);

    // ---- export: fixed-capacity lists -> plain GraphLinks arrays (graph_links/serializer.rs:52-209) ----
    uint32_t maxl = 0;
    for (uint32_t i = 0; i < n; ++i) maxl = std::max<uint32_t>(maxl, level[i]);
    const uint32_t L = n ? maxl + 1 : 0;
    qmx_hnsw host;      // (the plain arrays only: hnsw_finish_graph makes the handle)
    qmx_hnsw *g = &host;
    std::vector<uint64_t> count_ge(L + 1, 0);
    for (uint32_t i = 0; i < n; ++i) for (uint32_t l = 0; l <= level[i]; ++l) count_ge[l]++;
    // back_index: points by descending level, ties by id
    std::vector<uint32_t> back(nn);
    {
        std::vector<uint64_t> start(L + 1, 0);
        uint64_t acc = 0;
        for (int32_t l = (int32_t)L - 1; l >= 0; --l) { start[l] = acc; acc += count_ge[l] - (l + 1 < (int32_t)L ? count_ge[l + 1] : 0); }
        for (uint32_t i = 0; i < n; ++i) back[start[level[i]]++] = i;
    }
    g->h_reindex.resize(n);
    for (uint32_t i = 0; i < n; ++i) g->h_reindex[back[i]] = i;
    uint64_t total_slots = 0;
    for (uint32_t l = 0; l < L; ++l) total_slots += count_ge[l];
    g->h_level_offsets.assign(L + 1, 0);
    g->h_offsets.assign(total_slots + 1, 0);
    uint64_t nnb = 0;
    for (uint32_t i = 0; i < n; ++i) { nnb += cnt0[i]; for (uint32_t l = 1; l <= level[i]; ++l) nnb += cntU[up_off[i] + l - 1]; }
    g->h_neighbors.resize(nnb);
    uint64_t off = 0, slot = 0;
    for (uint32_t l = 0; l < L; ++l) {
        g->h_level_offsets[l] = slot;
        for (uint64_t j = 0; j < count_ge[l]; ++j) {
            const uint32_t id = l == 0 ? (uint32_t)j : back[j];
            g->h_offsets[slot++] = off;
            const uint32_t len = l == 0 ? cnt0[id] : cntU[up_off[id] + l - 1];
            const uint32_t *src = l == 0 ? &links0[(size_t)id * m0] : &linksU[((size_t)up_off[id] + l - 1) * m];
            memcpy(g->h_neighbors.data() + off, src, (size_t)len * 4);
            off += len;
        }
    }
    g->h_level_offsets[L] = slot;
    g->h_offsets[slot] = off;
    if (have_ep) { g->h_ep_ids.push_back(ep_id); g->h_ep_levels.push_back(ep_level); }
    for (auto &e : extra) { g->h_xp_ids.push_back(e.second); g->h_xp_levels.push_back(e.first); }
    return hnsw_finish_graph(host, m, m0, n, L, seg->device, out);
}

}  // extern "C"
