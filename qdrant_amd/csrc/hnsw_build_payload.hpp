// hnsw_build_payload.hpp — the payload-block sub-graphs of an HNSW build on the device (qmx_hnsw_build_payload_links).
//
// For every payload block of an indexed field the reference builds a second, FLAT graph over the block's points only
// (hnsw/build.rs:408-531, build_filtered_graph :631-716: GraphLayersBuilder::new_with_params(total, payload_m, ef_construct, 1, ..) - every point on
// level 0, capacity payload_m0, the block's first point its entry point) and appends its links to the main graph's level 0 (merge_from_other,
// graph_layers_builder.rs:346-381).  Blocks share nothing, so all of them are built here side by side: the per-point work is the main build's
// (hnsw_build.hpp: phase 1 = search_on_level(ef_construct) + heuristic, phase 2 = publish + back links under the neighbour's lock), over a WORK LIST
// instead of an id range.  An item = (block, position in block); one launch pair inserts the next batch of every block that still has points.
//
// Storage is block-local: a block's points occupy the membership slots blk_off[b] .. blk_off[b + 1] (live points only, insertion order); link rows,
// counts and locks are indexed by slot, links are POSITIONS within the block (the id of position i of block b = points[blk_off[b] + i]), and the
// visited bitmap of an insertion search has one bit per position of the largest block.  The insertion is hnsw_build.hpp's, instantiated over BlockView
// (nodes = positions, id_of = the block's point list); what is written here is the work list: item decode, the block's entry point, the launch.
#pragma once
#include "hnsw_build.hpp"
#include "hnsw_payload_args.hpp"

namespace qmx {

// one block's flat graph: nodes are positions within the block, rows / counts / locks those of its membership slots
// (indexed through the arguments: a row, a count and a lock pointer kept per block cost the SQ search kernel a register and, with it, a wave)
struct BlockView {
    static constexpr bool IDENTITY = false;
    const HnswPayloadArgs &h;
    uint64_t slot0;              // the block's first slot
    const uint32_t *pts;         // [blk_n] the block's points
    uint32_t blk_n;
    __device__ __forceinline__ BlockView(const HnswPayloadArgs &args, uint32_t blk)
        : h(args), slot0(args.blk_off[blk]), pts(args.points + slot0), blk_n((uint32_t)(args.blk_off[blk + 1] - slot0)) {}
    __device__ __forceinline__ uint32_t id_of(uint32_t node) const { return pts[node]; }
    __device__ __forceinline__ uint32_t *list(uint32_t node) const { return h.links + (slot0 + node) * h.pm0; }
    __device__ __forceinline__ uint32_t *count(uint32_t node) const { return h.cnt + slot0 + node; }
    __device__ __forceinline__ uint32_t *lock(uint32_t node) const { return h.lock + slot0 + node; }
    __device__ __forceinline__ uint32_t n_nodes() const { return blk_n; }
    __device__ __forceinline__ uint32_t cap() const { return h.pm0; }
    __device__ __forceinline__ uint32_t row_len(uint32_t len) const { return len < h.pm0 ? len : h.pm0; }
};

// ---- phase 1: one wavefront per item, every block graph READ-ONLY ---------------------------------------------------------------------------------------
template <class H, class HI, int E>
__global__ __launch_bounds__(64) void hnsw_payload_search_kernel(const ScanArgs a0, const HnswPayloadArgs h) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const InsertLds s = insert_lds<HNSW_BUILD_LDS_HEAD_NODES>(smem, hnsw_build_cand_cap(E, h.ef_construct), h.lds_query_bytes);
    const VisitedSlot vs = visited_slot(h);

    auto next_item = [&](uint32_t bi) -> uint32_t {      // (as the main build: the items of a round are handed out one at a time)
        uint32_t v = 0;
        if (lane == 0) v = atomicAdd(&h.next[0], 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    };
    for (uint32_t bi = blockIdx.x; bi < h.count; bi = next_item(bi)) {
        const BlockView v(h, h.item_block[h.first_item + bi]);
        const uint32_t p = v.id_of(h.item_pos[h.first_item + bi]);
        const ScanArgs a = query_args<H>(a0, p);     // the new point is the query of every score below
        if (lane == 0) h.sel_cnt[bi] = 0;
        const unsigned char *qp = stage_query_entry<H>(a0, h, bi, p, s.q_lds, lane);

        // ---- the block's entry point: its first point, on level 0 like every point (graph_layers_builder.rs:441-447: score_internal(p, entry)) ----
        if (lane == 0) s.hop_ids[0] = v.id_of(0);
        if (is_asymmetric<HI>::value)
            hop_score<HI>(query_args<HI>(a0, p), stored_query<HI>(a0, p), s.hop_ids, s.hop_scores, 1, lane);
        else
            hop_score<H>(a, qp, s.hop_ids, s.hop_scores, 1, lane);
        const float entry_score = s.hop_scores[0];

        // ---- search_on_level(ef_construct) on level 0 of the block graph -> heuristic -> sel ----
        const uint32_t n_cand = search_on_level<H, E>(a, qp, v, h.ef_construct, s, vs, 0u, entry_score, lane);
        const uint32_t n_sel = heuristic_fill<HI>(a0, v, s.cand, s.cand_scores, n_cand, h.pm0, s.sel, s.sel_scores, s.hop_ids, s.hop_scores, lane);
        const uint64_t so = (uint64_t)bi * h.pm0;
        for (uint32_t i = (uint32_t)lane; i < n_sel; i += 64) {
            h.sel_pos[so + i] = s.sel[i];
            h.sel_scores[so + i] = s.sel_scores[i];
        }
        if (lane == 0) h.sel_cnt[bi] = n_sel;
        __syncthreads();
    }
}

// ---- phase 2: publish the item's links, then connect_with_heuristic(p, q) under q's lock for every selected neighbour q of its block ------------------
template <class H>
__global__ __launch_bounds__(64) void hnsw_payload_link_kernel(const ScanArgs a, const HnswPayloadArgs h) {
    __shared__ LinkLds s;
    const int lane = threadIdx.x;
    auto next_item = [&](uint32_t bi) -> uint32_t {
        uint32_t v = 0;
        if (lane == 0) v = atomicAdd(&h.next[1], 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    };
    for (uint32_t bi = blockIdx.x; bi < h.count; bi = next_item(bi)) {
        uint32_t n_sel = h.sel_cnt[bi];
        n_sel = n_sel < h.pm0 ? n_sel : h.pm0;
        if (n_sel == 0) continue;
        const uint64_t so = (uint64_t)bi * h.pm0;
        link_new_node<H>(a, BlockView(h, h.item_block[h.first_item + bi]), h.item_pos[h.first_item + bi], h.sel_pos + so, h.sel_scores + so, n_sel, s, lane);
    }
}

template <class H, class HI = H>
int32_t launch_hnsw_payload_hop(hipStream_t st, const ScanArgs &a, const HnswPayloadArgs &h, int phase, uint32_t grid, int *per_cu) {
    QMX_REQUIRE(h.ef_construct >= 1 && h.ef_construct <= HNSW_MAX_EF, QMX_ERR_BAD_ARG, "ef_construct %u not in 1..%u", h.ef_construct, HNSW_MAX_EF);
    QMX_REQUIRE(h.pm0 >= 1 && h.pm0 <= HNSW_BUILD_MAX_M0, QMX_ERR_BAD_ARG, "payload_m0 %u not in 1..%u", h.pm0, HNSW_BUILD_MAX_M0);
    return launch_hnsw_insert_hop<hnsw_payload_search_kernel<H, HI, 2>, hnsw_payload_search_kernel<H, HI, 8>, hnsw_payload_search_kernel<H, HI, 0>,
                                  hnsw_payload_link_kernel<HI>, HNSW_BUILD_LDS_HEAD_NODES>(st, a, h, phase, grid, per_cu, "payload links");
}

struct HnswPayloadLauncher {
    hipStream_t st;
    const HnswPayloadArgs *h;
    int phase;
    uint32_t grid;
    int *per_cu;
    template <class P> int32_t row(const ScanArgs &a) const { return launch_hnsw_payload_hop<HopRow<P>>(st, a, *h, phase, grid, per_cu); }
    template <class S> int32_t small(const ScanArgs &a) const { return launch_hnsw_payload_hop<HopSmall<S>>(st, a, *h, phase, grid, per_cu); }
};

}  // namespace qmx
