// hnsw_layout.hpp — the dynamic LDS of one walk (hnsw.hpp hnsw_search_kernel): where each region starts, and the total.  The kernel carves its LDS by it,
// the launcher and the occupancy query ask it for the bytes: a region exists in one place only.  Integer logic a host compiler reads without HIP
// (tools/hnsw_layout_check.cpp sweeps it under the sanitizers).  The integer limits of a walk's launch live here too: the kernels (through kernels.hpp),
// the host code and hnsw_walk_plan.hpp read the one definition.
//
//   [hop ids][hop scores][ACORN explore list][query entry, padded to 16][LDS beam / `nearest`][reference candidates][visited table][PQ 8-bit image]
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QMX_LAYOUT_HD __host__ __device__ static inline
#else
#define QMX_LAYOUT_HD static inline
#endif

namespace qmx {

constexpr int HNSW_E_REF = -1;                     // the template value of the walk's E that selects option hnsw_reference_heap_order (hnsw.hpp RefHeaps)
constexpr uint32_t HNSW_REF_CAND_LDS = 1024;       // ... entries of its `candidates` heap kept in LDS (8 KiB per search): the ten levels every sift touches
constexpr uint32_t HNSW_REF_CAND_CAP = 1u << 16;   // ... entries of one search's whole `candidates` heap (512 KiB per slot)
constexpr uint32_t HNSW_REF_SLOT_CAP = 4096;       // ... searches in flight in that mode (1 024 until round 5: fewer than the default walk keeps in flight)
constexpr uint32_t HNSW_EV_SPILL_CAP = 4096;       // search_with_vectors: evicted candidates of ONE score a slot can hold beyond four (32 KiB per slot; more raises err_flag = 2)
constexpr uint32_t HNSW_MAX_EF = 4096;             // max(top, ef) of a walk: up to HNSW_MAX_EF_REG in a register beam, beyond it in an LDS beam (hnsw.hpp Beam<0>)
constexpr uint32_t HNSW_MAX_EF_REG = 512;          // ... the register beam's; and the largest ef_construct (the build keeps its beam in registers)
constexpr uint32_t HNSW_LDS_QUERY_MAX = 150 * 1024;            // bytes of query entry a search stages at most
constexpr uint32_t HNSW_VIS_LDS_BYTES = 16384;                 // the walk's visited table in LDS (hnsw.hpp LdsVisited): 1024 buckets x 8 tags of 16 bits
constexpr uint32_t HNSW_VIS_LDS_MAX_POINTS = 65534u * 1024u;   // ... graphs whose (id >> 10) + 1 fits a tag below the "taken back" mark 0xFFFF
constexpr uint32_t HNSW_SLOT_CAP = 4096;                       // searches in flight per launch
constexpr uint32_t HNSW_LOG_CAP = 16384;                       // visited words logged per search before falling back to a full clear
constexpr uint64_t HNSW_VIS_BUDGET = 8ull << 30;               // bytes of visited bitmaps per query handle

// bytes of the ACORN walk's list of nodes to explore (one per link of the popped candidate: HnswArgs::explore_cap ids - the graph's longest level-0 list -, 64 at least)
QMX_LAYOUT_HD uint32_t hnsw_acorn_lds(uint32_t acorn, uint32_t m0) { return acorn ? 4u * (((m0 < 64u ? 64u : m0) + 63u) / 64u * 64u) : 0u; }
// bytes of the LDS beam of a walk with max(top, ef) = ef > HNSW_MAX_EF_REG: keys + expanded flags
QMX_LAYOUT_HD size_t hnsw_beam_lds(uint32_t ef) { return ((size_t)ef * 9 + 15) / 16 * 16; }

// bytes of the two hop arrays (hop_cap ids, hop_cap scores): what lies in front of the ACORN explore list
QMX_LAYOUT_HD size_t hnsw_hop_lds(uint32_t hop_cap) { return 8 * (size_t)hop_cap; }

// byte offsets into the walk's dynamic LDS; a region that the launch does not have is empty (it starts where the next one does)
struct HnswLds {
    size_t hop_ids, hop_scores;     // hop_cap u32 / f32 each
    size_t explore;                 // ACORN: the nodes to explore
    size_t query;                   // QLDS: the query entry (lds_query_bytes, padded to 16)
    size_t beam;                    // E == 0: the LDS beam; E == HNSW_E_REF: `nearest`
    size_t ref_cands;               // E == HNSW_E_REF: the first HNSW_REF_CAND_LDS entries of `candidates`
    size_t visited;                 // LdsVisited's table (vis_lds bytes)
    size_t pq8;                     // HopPQ's 8-bit LUT image of the search (pq8_stride bytes when the launch carries one)
    size_t total;
};

// E, QLDS: the template parameters of the kernel; the others are HnswArgs' fields of the same names (ef = max(ef, top); has_pq8 = pq8 != nullptr)
QMX_LAYOUT_HD HnswLds hnsw_lds_layout(int E, bool QLDS, uint32_t hop_cap, uint32_t acorn, uint32_t explore_cap, uint32_t lds_query_bytes, uint32_t ef,
                                      uint32_t vis_lds, bool has_pq8, uint32_t pq8_stride) {
    HnswLds l;
    l.hop_ids = 0;
    l.hop_scores = 4 * (size_t)hop_cap;
    l.explore = hnsw_hop_lds(hop_cap);
    l.query = l.explore + hnsw_acorn_lds(acorn, explore_cap);
    l.beam = l.query + (QLDS ? ((size_t)lds_query_bytes + 15) / 16 * 16 : 0);
    l.ref_cands = l.beam + (E <= 0 ? hnsw_beam_lds(ef) : 0);
    l.visited = l.ref_cands + (E == HNSW_E_REF ? (size_t)HNSW_REF_CAND_LDS * 8 : 0);
    l.pq8 = l.visited + vis_lds;
    l.total = l.pq8 + (has_pq8 ? pq8_stride : 0);
    return l;
}

}  // namespace qmx
