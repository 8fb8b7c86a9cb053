// api_hnsw_payload.hip — the C-ABI of include/qdrant_amd.h, payload-block sub-graphs merged into the graph (hnsw_build_payload.hpp).
// (One of the api_*.hip translation units; what it shares with the main build: api_hnsw_build.hpp.)
#include "api_hnsw_build.hpp"
#include <algorithm>

extern "C" {

static int32_t launch_hnsw_payload_any(const qmx_segment *seg, const ScanArgs &a, const HnswPayloadArgs &h, int phase, uint32_t grid, int *per_cu) {
    if (seg->dtype == QMX_DTYPE_SQ_U8) return launch_hnsw_payload_sq(nullptr, (int)seg->distance, a, h, phase, grid, per_cu);
    if (seg->dtype == QMX_DTYPE_BQ) return launch_hnsw_payload_bq(nullptr, a, h, phase, grid, per_cu);
    if (seg->dtype == QMX_DTYPE_PQ) return launch_hnsw_payload_pq(nullptr, a, h, phase, grid, per_cu);
    if (seg->dtype == QMX_DTYPE_TQ) return launch_hnsw_payload_tq(nullptr, a, h, phase, grid, per_cu);
    return launch_hnsw_payload_dense(nullptr, (int)seg->dtype, (int)seg->distance, a, h, phase, grid, per_cu);
}

static int32_t hnsw_payload_links_body(const qmx_segment *seg, const qmx_segment *original, const qmx_hnsw *main_graph, const qmx_hnsw_payload_blocks *bl, qmx_hnsw **out,
                                       qmx_hnsw_payload_info *info) {
    // (over Manhattan a TurboQuant segment is a supported dtype: refusing it first changes no other refusal)
    QMX_REQUIRE(!tq_l1(seg), QMX_ERR_NOT_SUPPORTED, "payload links through a TurboQuant storage over Manhattan are not built");
    QMX_TRY(build_check_segment(seg, original, "payload links", "", true));
    const bool from_original = seg->dtype == QMX_DTYPE_PQ || seg->dtype == QMX_DTYPE_TQ;
    QMX_REQUIRE(bl->payload_m0 >= 1 && bl->payload_m0 <= HNSW_BUILD_MAX_M0, QMX_ERR_BAD_ARG, "payload_m0 %u not in 1..%u", bl->payload_m0, HNSW_BUILD_MAX_M0);
    QMX_REQUIRE(bl->ef_construct >= 1 && bl->ef_construct <= HNSW_MAX_EF, QMX_ERR_BAD_ARG, "ef_construct %u not in 1..%u", bl->ef_construct, HNSW_MAX_EF);
    QMX_REQUIRE(seg->n <= 0xFFFFFFFFull, QMX_ERR_BAD_ARG, "too many rows");
    QMX_REQUIRE(bl->n_blocks == 0 || bl->offsets, QMX_ERR_BAD_ARG, "block offsets missing");
    QMX_REQUIRE(bl->n_blocks < 0xFFFFFFFFu, QMX_ERR_BAD_ARG, "too many blocks");
    QMX_REQUIRE(!is_device_ptr(bl->offsets) && !is_device_ptr(bl->points), QMX_ERR_BAD_ARG, "block offsets and points are host arrays");
    const uint32_t n = (uint32_t)seg->n, n_blocks = bl->n_blocks, pm0 = bl->payload_m0;
    const uint32_t max_batch = bl->max_batch ? bl->max_batch : 16384;
    if (n_blocks) {
        QMX_REQUIRE(bl->offsets[0] == 0, QMX_ERR_BAD_ARG, "block offsets must start at 0");
        for (uint32_t b = 0; b < n_blocks; ++b)
            QMX_REQUIRE(bl->offsets[b] <= bl->offsets[b + 1], QMX_ERR_BAD_ARG, "block offsets decrease at block %u", b);
        QMX_REQUIRE(bl->offsets[n_blocks] == 0 || bl->points, QMX_ERR_BAD_ARG, "block points missing");
    }
    if (main_graph) {
        QMX_REQUIRE(main_graph->n_points == n && main_graph->device == seg->device, QMX_ERR_BAD_ARG,
                    "the main graph must hold the segment's %u points on its device (it has %u)", n, main_graph->n_points);
        QMX_REQUIRE(n == 0 || (!main_graph->h_offsets.empty() && main_graph->h_offsets.size() > n), QMX_ERR_NOT_SUPPORTED,
                    "payload links: the main graph keeps no host copy of its plain arrays (graphs built by qmx_hnsw_build do)");
    }
    QMX_HIP(hipSetDevice(seg->device));

    HostLiveness alive;
    QMX_TRY(alive.load(seg));

    // ---- the membership slots: the live points of every block, block after block ----
    std::vector<uint32_t> pts;
    std::vector<uint64_t> blk_off(n_blocks + 1, 0);
    {
        std::vector<uint32_t> stamp(n, 0);      // block + 1 that listed the point last
        for (uint32_t b = 0; b < n_blocks; ++b) {
            for (uint64_t i = bl->offsets[b]; i < bl->offsets[b + 1]; ++i) {
                const uint32_t p = bl->points[i];
                QMX_REQUIRE(p < n, QMX_ERR_BAD_ARG, "block %u lists point %u of %u", b, p, n);
                QMX_REQUIRE(stamp[p] != b + 1, QMX_ERR_BAD_ARG, "block %u lists point %u twice", b, p);
                stamp[p] = b + 1;
                if (alive.live(p)) pts.push_back(p);
            }
            blk_off[b + 1] = pts.size();
        }
    }
    const uint64_t n_slots = pts.size();
    uint32_t largest = 0, blocks_built = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint64_t len = blk_off[b + 1] - blk_off[b];
        largest = (uint32_t)std::max<uint64_t>(largest, len);
        blocks_built += len ? 1 : 0;
    }

    // ---- the schedule: a round holds the next batch of every block that still has points (batch rule per block: <= max(1, inserted / 32), <= max_batch);
    // position 0 of a block is its entry point and needs no search.  The rounds of a block depend on its size alone, so there are as many rounds as
    // the largest block needs by itself
    std::vector<uint32_t> item_block, item_pos;
    std::vector<uint64_t> round_first(1, 0);
    {
        item_block.reserve(n_slots);
        item_pos.reserve(n_slots);
        std::vector<uint32_t> active, done_pos(n_blocks, 1);
        for (uint32_t b = 0; b < n_blocks; ++b) if (blk_off[b + 1] - blk_off[b] > 1) active.push_back(b);
        while (!active.empty()) {
            size_t keep = 0;
            for (size_t k = 0; k < active.size(); ++k) {
                const uint32_t b = active[k], len = (uint32_t)(blk_off[b + 1] - blk_off[b]);
                const uint32_t count = std::min<uint32_t>({max_batch, std::max<uint32_t>(1, done_pos[b] / 32), len - done_pos[b]});
                for (uint32_t i = 0; i < count; ++i) { item_block.push_back(b); item_pos.push_back(done_pos[b] + i); }
                done_pos[b] += count;
                if (done_pos[b] < len) active[keep++] = b;
            }
            active.resize(keep);
            round_first.push_back(item_block.size());
        }
    }
    const size_t n_rounds = round_first.size() - 1;
    uint64_t max_round = 1;
    for (size_t r = 0; r < n_rounds; ++r) max_round = std::max<uint64_t>(max_round, round_first[r + 1] - round_first[r]);
    QMX_REQUIRE(max_round <= 0xFFFFFFFFull, QMX_ERR_BAD_ARG, "too many insertions in one round");

    // ---- device state ----
    DevBuf b_pts, b_blk, b_iblk, b_ipos, b_links, b_cnt, b_lock, b_sel, b_sels, b_selc, b_ipt;
    U8RowNorms norms;
    BuildQueryEntries entries;
    InsertSlots slots;
    QMX_TRY(dev_upload(b_pts, pts.data(), pts.size()));
    QMX_TRY(dev_upload(b_blk, blk_off.data(), blk_off.size()));
    QMX_TRY(dev_upload(b_iblk, item_block.data(), item_block.size()));
    QMX_TRY(dev_upload(b_ipos, item_pos.data(), item_pos.size()));
    const size_t ns1 = std::max<uint64_t>(n_slots, 1);
    QMX_TRY(b_links.reserve(ns1 * pm0 * 4)); QMX_TRY(b_cnt.reserve(ns1 * 4)); QMX_TRY(b_lock.reserve(ns1 * 4));
    QMX_HIP(hipMemset(b_cnt.p, 0, ns1 * 4));
    QMX_HIP(hipMemset(b_lock.p, 0, ns1 * 4));
    uint32_t launches = 0;
    if (n_rounds) {
        QMX_TRY(b_sel.reserve((size_t)max_round * pm0 * 4)); QMX_TRY(b_sels.reserve((size_t)max_round * pm0 * 4)); QMX_TRY(b_selc.reserve((size_t)max_round * 4));
        ScanArgs a;
        fill_build_args(seg, a);
        HnswPayloadArgs h;
        memset(&h, 0, sizeof(h));
        h.points = (const uint32_t *)b_pts.p; h.blk_off = (const uint64_t *)b_blk.p;
        h.item_block = (const uint32_t *)b_iblk.p; h.item_pos = (const uint32_t *)b_ipos.p;
        h.pm0 = pm0; h.links = (uint32_t *)b_links.p; h.cnt = (uint32_t *)b_cnt.p; h.lock = (uint32_t *)b_lock.p;
        h.ef_construct = bl->ef_construct;
        h.sel_pos = (uint32_t *)b_sel.p; h.sel_scores = (float *)b_sels.p; h.sel_cnt = (uint32_t *)b_selc.p;
        const uint64_t dev_row_bytes = stage_stored_rows(seg, h);
        QMX_TRY(check_row_query_slot(h.lds_query_bytes, dev_row_bytes));
        QMX_TRY(norms.attach(seg, n, a));
        if (from_original) {      // the query entries of a round's items: their original vectors are gathered by id
            std::vector<uint32_t> item_point(item_block.size());
            for (size_t i = 0; i < item_point.size(); ++i) item_point[i] = pts[blk_off[item_block[i]] + item_pos[i]];
            QMX_TRY(dev_upload(b_ipt, item_point.data(), item_point.size()));
            QMX_TRY(entries.reserve(seg, a, h, max_round, true));
        }
        QMX_REQUIRE(h.lds_query_bytes <= HNSW_LDS_QUERY_MAX, QMX_ERR_NOT_SUPPORTED, "query entries of %u bytes do not fit the LDS query slot", h.lds_query_bytes);
        // (the visited set of an insertion search: one bit per position of the largest BLOCK)
        QMX_TRY(slots.reserve(seg, h, largest, max_round, [&](int phase, uint32_t grid, int *per_cu) { return launch_hnsw_payload_any(seg, a, h, phase, grid, per_cu); }));
        for (size_t r = 0; r < n_rounds; ++r) {
            h.first_item = round_first[r];
            h.count = (uint32_t)(round_first[r + 1] - round_first[r]);
            uint32_t grid1, grid2;
            QMX_TRY(slots.begin_batch(h.count, &grid1, &grid2));
            if (from_original) QMX_TRY(entries.make(seg, original, a, 0, (const uint32_t *)b_ipt.p + h.first_item, h.count));
            int per_cu = 1;
            QMX_TRY(launch_hnsw_payload_any(seg, a, h, 1, grid1, &per_cu));
            QMX_TRY(launch_hnsw_payload_any(seg, a, h, 2, grid2, &per_cu));
            launches += 2;
        }
    }

    // ---- merge_from_other on level 0, every point at once ----
    // the memberships of every point in block order (a counting sort of the slots by point: slots ascend with their blocks)
    std::vector<uint64_t> mem_off((size_t)n + 1, 0), mem_slot(n_slots), mem_slot0(n_slots);
    for (uint64_t s = 0; s < n_slots; ++s) mem_off[pts[s] + 1]++;
    for (uint32_t p = 0; p < n; ++p) mem_off[p + 1] += mem_off[p];
    {
        std::vector<uint64_t> fill(mem_off.begin(), mem_off.end() - 1);
        for (uint32_t b = 0; b < n_blocks; ++b)
            for (uint64_t s = blk_off[b]; s < blk_off[b + 1]; ++s) {
                const uint64_t at = fill[pts[s]]++;
                mem_slot[at] = s;
                mem_slot0[at] = blk_off[b];
            }
    }
    DevBuf b_moff, b_mslot, b_mslot0, b_cap, b_len, b_tmp, b_out;
    QMX_TRY(dev_upload(b_moff, mem_off.data(), mem_off.size()));
    QMX_TRY(dev_upload(b_mslot, mem_slot.data(), mem_slot.size()));
    QMX_TRY(dev_upload(b_mslot0, mem_slot0.data(), mem_slot0.size()));
    QMX_TRY(b_cap.reserve(((size_t)n + 1) * 8)); QMX_TRY(b_len.reserve(((size_t)n + 1) * 8));
    HnswPayloadMergeArgs mg;
    memset(&mg, 0, sizeof(mg));
    mg.n_points = n;
    if (main_graph && n) { mg.main_off = main_graph->d_offsets; mg.main_nb = main_graph->d_neighbors; }
    mg.mem_off = (const uint64_t *)b_moff.p; mg.mem_slot = (const uint64_t *)b_mslot.p; mg.mem_slot0 = (const uint64_t *)b_mslot0.p;
    mg.points = (const uint32_t *)b_pts.p; mg.links = (const uint32_t *)b_links.p; mg.cnt = (const uint32_t *)b_cnt.p; mg.pm0 = pm0;
    mg.cap = (uint64_t *)b_cap.p; mg.len = (uint64_t *)b_len.p;
    uint64_t cap_total = 0, l0_total = 0;
    std::vector<uint64_t> l0_off((size_t)n + 1, 0);
    std::vector<uint32_t> l0_nb;
    if (n) {
        QMX_TRY(launch_hnsw_payload_merge_caps(nullptr, mg));
        QMX_TRY(launch_exclusive_scan_u64(nullptr, mg.cap, n));
        QMX_HIP(hipMemcpy(&cap_total, mg.cap + n, 8, hipMemcpyDeviceToHost));
        QMX_TRY(b_tmp.reserve(std::max<uint64_t>(cap_total, 1) * 4));
        mg.tmp = (uint32_t *)b_tmp.p;
        QMX_TRY(launch_hnsw_payload_merge_rows(nullptr, mg));
        QMX_TRY(launch_exclusive_scan_u64(nullptr, mg.len, n));
        QMX_HIP(hipMemcpy(l0_off.data(), mg.len, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
        l0_total = l0_off[n];
        QMX_REQUIRE(l0_total <= cap_total, QMX_ERR_OTHER, "payload links: the merge wrote %llu links into %llu slots", (unsigned long long)l0_total,
                    (unsigned long long)cap_total);
        QMX_TRY(b_out.reserve(std::max<uint64_t>(l0_total, 1) * 4));
        mg.out = (uint32_t *)b_out.p;
        QMX_TRY(launch_hnsw_payload_merge_compact(nullptr, mg));
        l0_nb.resize(l0_total);
        if (l0_total) QMX_HIP(hipMemcpy(l0_nb.data(), mg.out, l0_total * 4, hipMemcpyDeviceToHost));
    }
    QMX_HIP(hipDeviceSynchronize());

    // ---- the plain arrays of the result: the merged level 0, the main graph's upper levels behind it ----
    qmx_hnsw host;
    qmx_hnsw *g = &host;
    const uint32_t L = main_graph ? main_graph->n_levels : (n ? 1u : 0u);
    uint64_t main_l0 = 0;
    if (main_graph && n) {
        main_l0 = main_graph->h_offsets[n];
        g->h_reindex = main_graph->h_reindex;
        g->h_level_offsets = main_graph->h_level_offsets;
        g->h_offsets.resize(main_graph->h_offsets.size());
        std::copy(l0_off.begin(), l0_off.end(), g->h_offsets.begin());
        for (size_t s = (size_t)n + 1; s < g->h_offsets.size(); ++s) g->h_offsets[s] = main_graph->h_offsets[s] - main_l0 + l0_total;
        g->h_neighbors = std::move(l0_nb);
        g->h_neighbors.insert(g->h_neighbors.end(), main_graph->h_neighbors.begin() + (ptrdiff_t)main_l0, main_graph->h_neighbors.end());
        g->h_ep_ids = main_graph->h_ep_ids; g->h_ep_levels = main_graph->h_ep_levels;
        g->h_xp_ids = main_graph->h_xp_ids; g->h_xp_levels = main_graph->h_xp_levels;
    } else if (n) {
        g->h_reindex.resize(n);
        for (uint32_t i = 0; i < n; ++i) g->h_reindex[i] = i;
        g->h_level_offsets = {0, n};
        g->h_offsets = std::move(l0_off);
        g->h_neighbors = std::move(l0_nb);
    }
    for (uint32_t b = 0; b < n_blocks; ++b)      // EntryPoints::merge_from_other: the block graphs' entry points behind the main graph's, in block order
        if (blk_off[b + 1] > blk_off[b]) { g->h_ep_ids.push_back(pts[blk_off[b]]); g->h_ep_levels.push_back(0); }
    uint64_t longest = 0;
    for (uint32_t p = 0; p < n; ++p) longest = std::max<uint64_t>(longest, g->h_offsets[p + 1] - g->h_offsets[p]);
    QMX_TRY(hnsw_finish_graph(host, main_graph ? main_graph->m : 0, main_graph ? main_graph->m0 : pm0, n, L, seg->device, out));
    if (info) {
        info->blocks_built = blocks_built;
        info->launches = launches;
        info->links_added = l0_total - main_l0;
        info->longest_row = longest;
    }
    return QMX_OK;
}

int32_t qmx_hnsw_build_payload_links(const qmx_segment *seg, const qmx_segment *original, const qmx_hnsw *main_graph, const qmx_hnsw_payload_blocks *blocks,
                                     qmx_hnsw **out, qmx_hnsw_payload_info *info) {
    if (out) *out = nullptr;
    if (info) memset(info, 0, sizeof(*info));
    QMX_REFUSE_SPARSE(seg);
    QMX_REFUSE_SPARSE(original);
    QMX_REQUIRE(seg && blocks && out, QMX_ERR_BAD_ARG, "NULL argument");
    try {
        const int32_t rc = hnsw_payload_links_body(seg, original, main_graph, blocks, out, info);
        if (rc != QMX_OK && *out) { qmx_hnsw_destroy(*out); *out = nullptr; }
        return rc;
    } catch (...) {         // nothing C++ crosses the C ABI
        set_error("qmx_hnsw_build_payload_links: out of host memory");
        return QMX_ERR_OUT_OF_MEMORY;
    }
}

}  // extern "C"
