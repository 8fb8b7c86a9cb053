// hnsw_walk_plan.hpp — what the host decides before it launches a walk (api_hnsw.hip hnsw_enqueue): whether the walk is served at all, what each search
// stages in LDS, which visited set and which PQ image it gets, the capacities of its lists, and how many searches run at once.  Integer logic on plain
// values that a host compiler reads without HIP (tools/hnsw_walk_plan_check.cpp sweeps it against the decisions written out longhand, under the
// sanitizers); each rule is stated once, as what holds of the launch.
#pragma once
#include "hnsw_layout.hpp"

namespace qmx {

// the storages the decisions tell apart (dense, SQ, BQ and TurboQuant under its integer metrics are decided alike)
enum class WalkStorage { Other, PQ, TqL1 };

struct WalkShape {
    // which walk: ACORN; search_with_vectors (the popped candidates are listed); MaxSim over multi-vector points; a custom query as the scorer; the pop trace
    bool acorn = false, expanded = false, multi = false, custom = false, traced = false;
    bool filters = false;                  // the batch carries per-request filters
    WalkStorage storage = WalkStorage::Other;
    uint32_t dim = 0;
    uint32_t pq_m = 0, n_centroids = 0;    // PQ
    bool pq_direct_ok = false;             // ... the codebook is on the device and the LUT-free walk takes it (pq_direct_walk_ok)
    uint32_t tq_l1_entry_bytes = 0;        // TurboQuant over Manhattan: tq_l1_query_bytes(dim) ...
    uint32_t tq_l1_lds_bytes = 0;          // ... and tq_l1_lds_bytes(dim, rot_dim): the entry and the hop scratch behind it
    uint32_t q_stride = 0, top = 0, ef = 0;
    bool batch_entries = true;             // the walk's entries are the batch's own (ScanArgs::queries == qmx_query::d_queries)
    uint32_t n_points = 0, m0 = 0, max_row0 = 0;      // the graph
    uint32_t max_tokens = 0;               // multi: vectors of the longest multi-query
    uint32_t max_examples = 0;             // custom: examples of the largest query
    uint32_t custom_lds_bytes = 0;         // ... whose examples are multi-vectors: bytes of the largest staged block (CustomWalk::lds_bytes), else 0
    // options (common.hpp OPT_HNSW_*)
    bool opt_pq_direct_walk = false, opt_reference_heap_order = false, opt_no_lds_visited = false, opt_no_pq_prefilter = false;
    int64_t opt_log_cap = 0;
};

// why a walk is not served, in the order the checks are made (hnsw_enqueue has the error code and text of each)
enum class WalkRefusal {
    None,
    TqL1Multi,         // multi-vector points over TurboQuant / Manhattan
    Filters,           // per-request filters on a walk whose searches are not the batch's entries
    Trace,             // the pop trace on a walk that is not the plain one
    TqL1Lds,           // TurboQuant / Manhattan: entry + hop scratch pass HNSW_LDS_QUERY_MAX      (bytes: what they take)
    CustomTqL1Lds,     // ... under a custom query                                                 (bytes)
    CustomTokensLds,   // a custom query's example tokens pass HNSW_LDS_QUERY_MAX                   (bytes)
    BeamLds,           // entry + LDS beam pass the LDS
    AcornM0,           // ACORN: m0 outside 1..128
    AcornRow,          // ACORN: a level-0 list of more than 8192 links
};

enum class PqImage { None, BatchLuts, ExactOrderLuts };

struct WalkPlan {
    WalkRefusal refusal = WalkRefusal::None;
    uint64_t refused_bytes = 0;       // the LDS bytes a *Lds refusal reports
    bool pq_direct = false;           // the LUT-free PQ walk: a search's entry is its preprocessed vector (dim floats), not its LUTs
    uint32_t entry_stride = 0;        // bytes between the entries as the walk reads them (ScanArgs::q_stride)
    bool ref_heaps = false;
    uint32_t lds_query_bytes = 0;     // bytes of entry a search stages in LDS; 0: it reads the entry from global memory
    uint32_t vis_lds = 0;             // bytes of the LDS visited table, or 0
    PqImage pq_image = PqImage::None; // the 8-bit LUT image of the hop prefilter: made from the batch's LUTs, or from LUTs in the exact summation order
    bool pq_luts_in_l2 = false;       // a PQ walk whose searches read their LUTs through L2 (option hnsw_pq_per_cu caps its occupancy)
    uint32_t hop_cap = 0, explore_cap = 0, log_cap = 0, ev_cap = 0;
    uint64_t vis_words = 0;           // words of one slot's visited bitmap(s)
};

static inline WalkPlan hnsw_walk_plan(const WalkShape &w) {
    WalkPlan p;
    const bool pq = w.storage == WalkStorage::PQ, tq_l1 = w.storage == WalkStorage::TqL1;
    const bool own_entries = !w.multi && !w.custom;      // search i scores against entry i of the batch
    const uint32_t beam_ef = w.top > w.ef ? w.top : w.ef;
    auto refuse = [&p](WalkRefusal r, uint64_t bytes = 0) {
        p.refusal = r;
        p.refused_bytes = bytes;
        return p;
    };
    if (tq_l1 && w.multi) return refuse(WalkRefusal::TqL1Multi);
    if (w.filters && !(own_entries && !w.expanded)) return refuse(WalkRefusal::Filters);
    if (w.traced && !(own_entries && !w.expanded && !w.acorn)) return refuse(WalkRefusal::Trace);

    // The entry as the walk reads it: the query as given for TurboQuant / Manhattan, the preprocessed vector for the LUT-free PQ walk, else the batch's entry.
    p.pq_direct = pq && own_entries && w.opt_pq_direct_walk && w.pq_direct_ok;
    p.entry_stride = tq_l1 ? w.tq_l1_entry_bytes : p.pq_direct ? w.dim * 4 : w.q_stride;
    // The reference's two binary heaps replace the beam of the plain walk alone.
    p.ref_heaps = w.opt_reference_heap_order && own_entries && !w.acorn && !w.expanded && !tq_l1;
    // A list longer than the register beam lives in LDS behind the entry.
    const bool lds_beam = beam_ef > HNSW_MAX_EF_REG && own_entries && !tq_l1;

    // What a search would stage, by the kind of its entry:
    const uint64_t n_examples = w.max_examples > 1 ? w.max_examples : 1, n_tokens = w.max_tokens > 1 ? w.max_tokens : 1;
    const uint64_t multi_bytes = 16 + n_tokens * w.q_stride;                      // [16-byte header][the multi-query's vectors]
    const uint64_t custom_bytes = 32 + n_examples * w.q_stride;                   // [32-byte header][the examples' entries]
    // ... TurboQuant / Manhattan: [header][the examples][one hop scratch][64 scores per example]
    const uint64_t custom_tq_l1_bytes = 32 + n_examples * p.entry_stride + (w.tq_l1_lds_bytes - w.tq_l1_entry_bytes) + n_examples * 256;
    if (tq_l1 && w.tq_l1_lds_bytes > HNSW_LDS_QUERY_MAX) return refuse(WalkRefusal::TqL1Lds, w.tq_l1_lds_bytes);
    if (tq_l1 && w.custom && custom_tq_l1_bytes > HNSW_LDS_QUERY_MAX) return refuse(WalkRefusal::CustomTqL1Lds, custom_tq_l1_bytes);
    if (w.custom && w.custom_lds_bytes > HNSW_LDS_QUERY_MAX) return refuse(WalkRefusal::CustomTokensLds, w.custom_lds_bytes);
    if (lds_beam && (size_t)p.entry_stride + hnsw_beam_lds(beam_ef) + 2048 > 160 * 1024) return refuse(WalkRefusal::BeamLds);
    if (w.acorn && !(w.m0 >= 1 && w.m0 <= 128)) return refuse(WalkRefusal::AcornM0);
    if (w.acorn && w.max_row0 > 8192) return refuse(WalkRefusal::AcornRow);

    // The entry is staged when ...
    // A PQ LUT of more than half the LDS would leave one search per CU; the walk is a chain of dependent memory round trips, so many searches per CU
    // with the LUT read through L2 win (measured: tools/bench_hnsw.py)
    const bool big_pq_lut = pq && w.q_stride > 16 * 1024;
    const uint32_t batch_entry = (w.q_stride <= HNSW_LDS_QUERY_MAX && !big_pq_lut) ? w.q_stride : 0;      // the batch's entry, where a search stages it
    if (lds_beam) p.lds_query_bytes = p.entry_stride;                  // ... the LDS beam lies behind it: always (a PQ LUT too)
    else if (w.custom && w.custom_lds_bytes) p.lds_query_bytes = w.custom_lds_bytes;      // ... the MaxSim policy reads the examples' tokens from LDS: always
    else if (w.custom && tq_l1) p.lds_query_bytes = (uint32_t)custom_tq_l1_bytes;         // ... the hop scratch lies behind the examples: always
    else if (w.custom)          // ... the examples fit a modest share of the LDS, and one of them would be staged by itself (a multi-query's always is); else the header alone
        p.lds_query_bytes = (custom_bytes <= 48 * 1024 && (w.multi || batch_entry != 0)) ? (uint32_t)custom_bytes : 32;
    else if (w.multi) p.lds_query_bytes = multi_bytes <= 64 * 1024 ? (uint32_t)multi_bytes : 16;      // ... the longest multi-query fits; else the header alone
    else if (tq_l1) p.lds_query_bytes = w.tq_l1_lds_bytes;             // ... the hop scratch lies behind it: always
    else if (p.pq_direct) p.lds_query_bytes = p.entry_stride;          // ... it is a vector, not LUTs: always
    else p.lds_query_bytes = batch_entry;
    p.pq_luts_in_l2 = pq && p.lds_query_bytes == 0;

    // The hop prefilter's image is made for a PQ walk in beam order (not ACORN, not the reference heaps) of a codebook it holds (m <= 128, <= 256
    // centroids), unless switched off: the LUT-free walk wants it in the order of the entries it recomputes, and not when it lists its pops; the walk
    // through per-search LUTs wants it when those are the batch's own and stay in global memory.
    const bool image_ok = pq && !w.opt_no_pq_prefilter && !w.acorn && !p.ref_heaps && w.pq_m <= 128 && w.n_centroids <= 256;
    if (image_ok && p.pq_direct && !w.expanded) p.pq_image = PqImage::ExactOrderLuts;
    else if (image_ok && !p.pq_direct && own_entries && w.batch_entries && big_pq_lut && p.lds_query_bytes == 0) p.pq_image = PqImage::BatchLuts;

    // The LDS visited table is on when the walk is not ACORN, not in reference-heap order, not switched off, the graph's ids fit its tags, the staged
    // entry leaves it room, and no PQ image takes that room (the bitmap in global memory stays for what its buckets cannot hold).
    const bool vis_lds = !w.acorn && !p.ref_heaps && !w.opt_no_lds_visited && w.n_points <= HNSW_VIS_LDS_MAX_POINTS && p.lds_query_bytes <= 32 * 1024 &&
                         p.pq_image == PqImage::None;
    p.vis_lds = vis_lds ? HNSW_VIS_LDS_BYTES : 0;

    // Capacities.  ACORN keeps two visited lists; every explored node may add m0 points to one scoring batch (m0 > 64: the kernel scores what it holds
    // before the buffer could overflow), and every unvisited link of the popped candidate that fails the filter is explored: a list as long as the
    // candidate's, which m0 does not bound.
    const uint64_t bitmap_words = ((uint64_t)w.n_points + 31) / 32 > 0 ? ((uint64_t)w.n_points + 31) / 32 : 1;
    p.vis_words = w.acorn ? 2 * bitmap_words : bitmap_words;
    const uint32_t acorn_hops = (w.m0 * (w.m0 + 1) + 63) / 64 * 64;
    p.hop_cap = !w.acorn ? 64 : acorn_hops < 4160 ? acorn_hops : 4160;
    p.explore_cap = !w.acorn ? 0 : w.m0 > w.max_row0 ? w.m0 : w.max_row0;
    p.log_cap = (w.opt_log_cap >= 1 && w.opt_log_cap <= (int64_t)HNSW_LOG_CAP) ? (uint32_t)w.opt_log_cap : HNSW_LOG_CAP;      // (tests force the whole-bitmap clear)
    p.ev_cap = w.expanded ? HNSW_EV_SPILL_CAP : 0;      // search_with_vectors: a slot's stack of evicted candidates that tie with the bound
    return p;
}

// how many searches run at once
struct WalkSlots {
    int per_cu;          // searches per CU the launch is sized for
    uint64_t slots;      // blocks of the launch
    uint64_t want;       // slots a (re)allocation of the handle's scratch is sized for: the most this handle can use
};
struct WalkSlotOptions {
    int64_t pq_per_cu = 0, per_cu = 0;      // OPT_HNSW_PQ_PER_CU, OPT_HNSW_PER_CU (0 or less: no cap)
};

// per_cu: what the occupancy query allows; n_searches: searches of this walk; nq: entries of the batch
static inline WalkSlots hnsw_walk_slots(const WalkPlan &p, int per_cu, uint32_t n_searches, uint32_t nq, int num_cus, const WalkSlotOptions &o) {
    auto min64 = [](uint64_t a, uint64_t b) { return a < b ? a : b; };
    if (p.pq_luts_in_l2 && o.pq_per_cu > 0 && o.pq_per_cu < per_cu) per_cu = (int)o.pq_per_cu;
    // whole waves per SIMD: with 9 searches per CU one SIMD carries three waves and the others two, and the slowest SIMD sets the pace
    // (measured on the SQ walk at 10 M points: 5.76 ms with 8 per CU, 6.09 with 9, 6.23 with 7: profiles/r5_sq_walk_visited.md)
    if (per_cu >= 8) per_cu -= per_cu % 4;
    if (o.per_cu > 0 && o.per_cu < per_cu) per_cu = (int)o.per_cu;
    const uint64_t resident = min64((uint64_t)num_cus * per_cu, HNSW_SLOT_CAP);
    const uint64_t by_budget = HNSW_VIS_BUDGET / (p.vis_words * 4) > 0 ? HNSW_VIS_BUDGET / (p.vis_words * 4) : 1;
    WalkSlots s;
    s.per_cu = per_cu;
    s.slots = min64(min64(n_searches, resident), by_budget);
    if (p.ref_heaps) s.slots = min64(s.slots, HNSW_REF_SLOT_CAP);      // (their `candidates` heaps: HNSW_REF_CAND_CAP entries per slot)
    if (s.slots == 0) s.slots = 1;
    const uint32_t most = nq > n_searches ? nq : n_searches;
    s.want = min64(min64(most > 0 ? most : 1, resident), by_budget);
    if (s.want == 0) s.want = 1;
    return s;
}

}  // namespace qmx
