// hnsw_payload_args.hpp — arguments and launchers of the payload-block build (hnsw_build_payload.hpp, hnsw_build_payload.hip): what api_hnsw_payload.hip sees of it.
#pragma once
#include "kernels.hpp"

namespace qmx {

// Every block graph at once.  Membership slot s = blk_off[b] + i is position i of block b; `points[s]` its point id.
struct HnswPayloadArgs {
    const uint32_t *points;      // [n_slots] the live points of every block, block after block, in insertion order
    const uint64_t *blk_off;     // [n_blocks + 1] first slot of each block
    // the schedule: the items of every round, round after round; a round holds the next batch of every block that still has points
    const uint32_t *item_block;  // [n_items]
    const uint32_t *item_pos;    // [n_items] position within the block
    uint64_t first_item;         // this round: items first_item .. first_item + count
    uint32_t count;
    uint32_t pm0;                // capacity of a block-graph row (payload_m0)
    uint32_t *links;             // [n_slots][pm0] positions within the block
    uint32_t *cnt;               // [n_slots]
    uint32_t *lock;              // [n_slots]
    uint32_t ef_construct;
    uint32_t *visited;           // [slots][vis_words]: one bit per position of the largest block
    uint64_t vis_words;
    uint32_t *vis_log;           // [slots][log_cap]
    uint32_t log_cap;
    // phase 1 -> phase 2: sel[bi * pm0 + k] (positions), bi = item index within the round
    uint32_t *sel_pos;
    float *sel_scores;
    uint32_t *sel_cnt;           // [count]
    uint32_t lds_query_bytes, row_bytes;     // as HnswBuildArgs
    const unsigned char *batch_queries;      // as HnswBuildArgs: entry bi of the round (nullptr = stage the stored row)
    uint64_t batch_q_stride;
    uint32_t *next;              // [2] the counters the slots of phase 1 / phase 2 draw their next item from
};
// phase 1 = insertion searches + heuristic selection, phase 2 = linking; grid == 0: report occupancy only
int32_t launch_hnsw_payload_dense(hipStream_t st, int dtype, int distance, const ScanArgs &a, const HnswPayloadArgs &h, int phase, uint32_t grid, int *per_cu);
int32_t launch_hnsw_payload_sq(hipStream_t st, int distance, const ScanArgs &a, const HnswPayloadArgs &h, int phase, uint32_t grid, int *per_cu);
int32_t launch_hnsw_payload_bq(hipStream_t st, const ScanArgs &a, const HnswPayloadArgs &h, int phase, uint32_t grid, int *per_cu);
int32_t launch_hnsw_payload_pq(hipStream_t st, const ScanArgs &a, const HnswPayloadArgs &h, int phase, uint32_t grid, int *per_cu);      // (pq.hip)
int32_t launch_hnsw_payload_tq(hipStream_t st, const ScanArgs &a, const HnswPayloadArgs &h, int phase, uint32_t grid, int *per_cu);      // (hnsw_build_tq.hip)
// dst row r (dst_stride bytes apart, row_bytes copied) = src row ids[r]: the original vectors of a round's items
int32_t launch_gather_rows(hipStream_t st, const void *src, uint64_t src_stride, const uint32_t *ids, uint64_t n, uint32_t row_bytes, void *dst, uint64_t dst_stride);

// merge_from_other on level 0 for every point at once (graph_layers_builder.rs:346-381): row p = the main row, then for each membership of p in block order the
// block-graph links of p that are not yet in the row, as ids.
struct HnswPayloadMergeArgs {
    uint32_t n_points;
    const uint64_t *main_off;    // [n_points + 1] level-0 offsets of the main graph, or nullptr (no main graph: empty rows)
    const uint32_t *main_nb;
    const uint64_t *mem_off;     // [n_points + 1] the memberships of every point, in block order
    const uint64_t *mem_slot;    // the membership's slot
    const uint64_t *mem_slot0;   // ... and the first slot of its block
    const uint32_t *points;
    const uint32_t *links;       // [n_slots][pm0]
    const uint32_t *cnt;
    uint32_t pm0;
    uint64_t *cap;               // [n_points + 1] before the scan: upper bound of row p = cnt_main[p] + sum cnt_block[p]; after: its exclusive prefix sum
    uint32_t *tmp;               // rows of `cap` entries each
    uint64_t *len;               // [n_points + 1] before the scan: merged length; after: the plain arrays' level-0 offsets
    uint32_t *out;               // merged level 0, compact
};
int32_t launch_hnsw_payload_merge_caps(hipStream_t st, const HnswPayloadMergeArgs &m);
int32_t launch_hnsw_payload_merge_rows(hipStream_t st, const HnswPayloadMergeArgs &m);
int32_t launch_hnsw_payload_merge_compact(hipStream_t st, const HnswPayloadMergeArgs &m);
// in place exclusive prefix sum of v[0 .. n) with the total in v[n]
int32_t launch_exclusive_scan_u64(hipStream_t st, uint64_t *v, uint64_t n);

}  // namespace qmx
