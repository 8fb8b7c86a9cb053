// group_logic.hpp — the parts of grouped search (qmx_group_search) that are plain integer logic, shared by the kernels of groups.hip, the driver of
// api_groups.hip and the stand-alone host check (tools/group_logic_check.cpp, built with the address and undefined-behaviour sanitizers): the key
// table of the selection, one aggregation step over a query's slots, the termination bound and the tiling of the fallback.  No kernels and no runtime calls in here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QMX_GROUP_HD __host__ __device__ __forceinline__
#else
#define QMX_GROUP_HD inline
#endif

namespace qmx {

constexpr uint32_t GROUP_NONE = 0xFFFFFFFFu;      // QMX_GROUP_NONE: no key; also the empty entry of the key table (never a slot's key)
constexpr uint32_t GROUP_TABLE = 2048;            // entries of the key table: twice the most slots a query has, so a probe sequence always ends at an empty entry

// open addressing, linear probing; multiplicative hash (Knuth), the top 11 bits
QMX_GROUP_HD uint32_t group_hash(uint32_t key) { return (key * 2654435761u) >> 21; }
QMX_GROUP_HD bool group_table_has(const uint32_t *table, uint32_t key) {
    uint32_t h = group_hash(key);
    for (uint32_t probes = 0; probes < GROUP_TABLE; ++probes) {
        const uint32_t t = table[h];
        if (t == key) return true;
        if (t == GROUP_NONE) return false;
        h = (h + 1) & (GROUP_TABLE - 1);
    }
    return false;
}
// (the kernel inserts with an atomic compare-and-swap on the same probe sequence)
inline void group_table_insert_host(uint32_t *table, uint32_t key) {
    uint32_t h = group_hash(key);
    while (table[h] != GROUP_NONE && table[h] != key) h = (h + 1) & (GROUP_TABLE - 1);
    table[h] = key;
}

// Which keys the table of a selection pass holds, and what a hit in it means (the reference's two filters in <= limit keys of state):
//   fewer than `limit` slots in use : the table holds the keys of the FULL slots, a row is eligible when one of its keys is NOT in it (`except_on`);
//   `limit` slots in use            : the table holds the keys of the UNFILLED slots, a row is eligible when one of its keys IS in it (`match_on`).
QMX_GROUP_HD bool group_filling(uint32_t n_slots, uint32_t limit) { return n_slots >= limit; }
QMX_GROUP_HD bool group_slot_in_table(uint32_t cnt, uint32_t group_size, bool filling) { return (cnt >= group_size) != filling; }
QMX_GROUP_HD bool group_key_eligible(const uint32_t *table, uint32_t key, bool filling) {
    return key != GROUP_NONE && group_table_has(table, key) == filling;
}

// One step of the aggregator: the ranked stream hands over point `idx` (as `hit`, its key in the project's order) carrying group key `key`.
// `found` = the slot that holds `key` or -1.  Returns the slot the hit goes to, or -1 when it is skipped:
//   a slot exists and is not full -> append (the stream is ranked: appending keeps the order), unless its last hit is this very point;
//   no slot and fewer than `limit` in use -> open one; otherwise skip.
struct GroupStep {
    int32_t slot;        // where the hit goes, -1: nowhere
    uint32_t pos;        // its position in the slot
    bool opened;         // a new slot
    bool filled;         // the slot is full after it
};
QMX_GROUP_HD GroupStep group_step(int32_t found, uint32_t found_cnt, uint32_t found_last_idx, uint32_t idx, uint32_t n_slots, uint32_t limit,
                                  uint32_t group_size) {
    GroupStep s{-1, 0u, false, false};
    if (found >= 0) {
        if (found_cnt >= group_size || found_last_idx == idx) return s;
        s.slot = found;
        s.pos = found_cnt;
    } else {
        if (n_slots >= limit) return s;
        s.slot = (int32_t)n_slots;
        s.opened = true;
    }
    s.filled = s.pos + 1 == group_size;
    return s;
}
// after a page: the query needs no further page
QMX_GROUP_HD bool group_done(uint32_t n_full, uint32_t limit, uint32_t page_hits, uint32_t page_len, bool below_threshold) {
    return n_full >= limit || page_hits < page_len || below_threshold;
}

// Every fallback page's first row is eligible by construction, so each page adds at least one hit: a query is done after at most this many pages.
inline uint64_t group_page_bound(uint32_t limit, uint32_t group_size) { return (uint64_t)limit * group_size + 1; }
// elements between the score rows of the fallback's matrix: whole 16-byte pieces
inline uint64_t group_score_stride(uint64_t n_cand) { return (n_cand + 3) / 4 * 4; }
// unfinished queries scored per tile of the fallback: as many score rows as the byte budget holds, at least one
inline uint32_t group_tile_queries(uint32_t unfinished, uint64_t n_cand, uint64_t budget_bytes) {
    const uint64_t row = group_score_stride(n_cand) * sizeof(float);
    uint64_t fit = row ? budget_bytes / row : unfinished;
    if (fit < 1) fit = 1;
    return (uint32_t)(fit < unfinished ? fit : unfinished);
}
// blocks per query of a selection launch: ~8 k rows per block, at most ~1024 blocks per launch
inline uint32_t group_select_blocks(uint64_t n_cand, uint32_t tile_queries) {
    uint64_t by_rows = (n_cand + 8191) / 8192;
    const uint64_t by_grid = tile_queries ? (1024 + tile_queries - 1) / tile_queries : 1;
    if (by_rows > by_grid) by_rows = by_grid;
    return (uint32_t)(by_rows < 1 ? 1 : by_rows);
}
// the queries whose bound says "unfinished", in batch order
inline uint32_t group_pack_unfinished(const uint64_t *bound, uint32_t nq, uint32_t *list) {
    uint32_t n = 0;
    for (uint32_t q = 0; q < nq; ++q)
        if (bound[q] != 0) list[n++] = q;
    return n;
}

}  // namespace qmx
