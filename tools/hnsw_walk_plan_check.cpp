// hnsw_walk_plan_check.cpp — a stand-alone host run of the walk's launch decisions (qdrant_amd/csrc/hnsw_walk_plan.hpp) over the walks the entry points
// can ask for.  `longhand` below is the sequence of assignments hnsw_enqueue made before the decisions became a header (api_hnsw.hip at commit 4cc3618,
// lines 282-462), on plain integers and in its order, overwrites and all; hnsw_walk_plan and hnsw_walk_slots must give its values: every field of the plan,
// which refusal fires, and per_cu / slots / want.  A few cases are spelled out as literals behind the sweep.  Meant for the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iqdrant_amd/csrc tools/hnsw_walk_plan_check.cpp -o /tmp/hnsw_walk_plan_check
//   /tmp/hnsw_walk_plan_check
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "hnsw_walk_plan.hpp"

using namespace qmx;

namespace {

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

enum Dtype { DENSE, SQ, BQ, TQ, TQ_L1, PQ };

// what hnsw_enqueue read: the walk's optional parts as "present or not", the segment, the batch, the graph, the options
struct In {
    bool acorn, xo, mw, cw, pt;
    bool has_filters;
    Dtype dtype;
    uint32_t dim;
    uint32_t pq_m, pq_ncent;
    bool pq_centroids_and_direct_ok;      // s->d_centroids && pq_direct_walk_ok(...)
    uint32_t tq_query_bytes, tq_lds_bytes;      // tq_l1_query_bytes(dim), tq_l1_lds_bytes(dim, rot_dim)
    uint32_t q_stride, top, ef;
    bool queries_are_batch;      // fill_args: a.queries == q->d_queries
    uint32_t n_points, m0, max_row0;
    uint32_t mw_max_tokens, cw_max_examples, cw_lds_bytes;
    int64_t o_pq_direct, o_ref_heaps, o_no_lds_visited, o_no_pq_prefilter, o_log_cap, o_pq_per_cu, o_per_cu;
    int per_cu;      // what the occupancy query returned
    uint32_t n_searches, nq;
    int num_cus;
};

struct Long {
    bool pq_direct;
    uint32_t a_q_stride;
    uint32_t ref_heaps, lds_query_bytes, vis_lds;
    int image;      // 0 none, 1 from q->d_queries (the first block), 2 the LUT-free walk's (the second block)
    uint32_t log_cap, hop_cap, explore_cap, ev_cap;
    uint64_t vis_words;
    int per_cu;
    uint64_t slots, want;
    bool pq_and_no_lds;      // what the OPT_HNSW_PQ_PER_CU cap tested
};

// returns 0, or the number of the QMX_REQUIRE that fired (1..9, in the order they stood)
int longhand(const In &i, Long &h) {
    const bool tq_l1 = i.dtype == TQ_L1;
    if (!(!tq_l1 || !i.mw)) return 1;
    if (!(!i.has_filters || (!i.mw && !i.cw && !i.xo))) return 2;
    uint32_t a_q_stride = i.q_stride;
    bool a_queries_batch = i.queries_are_batch;
    if (tq_l1) {
        a_queries_batch = false;
        a_q_stride = i.tq_query_bytes;
    }
    const bool pq_direct = i.dtype == PQ && !i.cw && !i.mw && i.o_pq_direct > 0 && i.pq_centroids_and_direct_ok;
    if (pq_direct) {
        a_queries_batch = false;
        a_q_stride = i.dim * 4;
    }
    if (i.pt) {
        if (!(!i.xo && !i.acorn && !i.mw && !i.cw)) return 3;
    }
    h.ref_heaps = (i.o_ref_heaps > 0 && !i.acorn && !i.xo && !i.mw && !i.cw && !tq_l1) ? 1 : 0;
    h.lds_query_bytes = i.q_stride <= HNSW_LDS_QUERY_MAX ? i.q_stride : 0;
    if (tq_l1) {
        h.lds_query_bytes = i.tq_lds_bytes;
        if (!(h.lds_query_bytes <= HNSW_LDS_QUERY_MAX)) return 4;
    }
    if (i.mw) {
        const uint64_t need = 16 + (uint64_t)std::max<uint32_t>(i.mw_max_tokens, 1) * i.q_stride;
        h.lds_query_bytes = need <= 64 * 1024 ? (uint32_t)need : 16;
    }
    if (i.dtype == PQ && i.q_stride > 16 * 1024 && !i.mw) h.lds_query_bytes = 0;
    if (pq_direct) h.lds_query_bytes = a_q_stride;
    if (i.cw) {
        const uint64_t need = 32 + (uint64_t)std::max<uint32_t>(i.cw_max_examples, 1) * i.q_stride;
        h.lds_query_bytes = (need <= 48 * 1024 && h.lds_query_bytes != 0) ? (uint32_t)need : 32;
        if (tq_l1) {
            const uint64_t ne = std::max<uint32_t>(i.cw_max_examples, 1);
            const uint64_t need_l1 = 32 + ne * a_q_stride + (i.tq_lds_bytes - i.tq_query_bytes) + ne * 256;
            if (!(need_l1 <= HNSW_LDS_QUERY_MAX)) return 5;
            h.lds_query_bytes = (uint32_t)need_l1;
        }
        if (i.cw_lds_bytes) {
            if (!(i.cw_lds_bytes <= HNSW_LDS_QUERY_MAX)) return 6;
            h.lds_query_bytes = i.cw_lds_bytes;
        }
    }
    if (std::max(i.top, i.ef) > HNSW_MAX_EF_REG && !i.mw && !i.cw && !tq_l1) {
        const size_t beam = hnsw_beam_lds(std::max(i.top, i.ef));
        if (!((size_t)a_q_stride + beam + 2048 <= 160 * 1024)) return 7;
        h.lds_query_bytes = a_q_stride;
    }
    h.vis_lds = (!i.acorn && !h.ref_heaps && !i.o_no_lds_visited && i.n_points <= HNSW_VIS_LDS_MAX_POINTS && h.lds_query_bytes <= 32 * 1024) ? HNSW_VIS_LDS_BYTES : 0;
    h.image = 0;
    if (i.dtype == PQ && !pq_direct && !i.acorn && !i.mw && !i.cw && !h.ref_heaps && !i.o_no_pq_prefilter && a_queries_batch && i.pq_m <= 128 && i.pq_ncent <= 256 &&
        i.q_stride > 16 * 1024 && h.lds_query_bytes == 0) {
        h.image = 1;
        h.vis_lds = 0;
    }
    if (pq_direct && !i.acorn && !i.xo && !h.ref_heaps && !i.o_no_pq_prefilter && i.pq_m <= 128 && i.pq_ncent <= 256) {
        h.image = 2;
        h.vis_lds = 0;
    }
    h.log_cap = HNSW_LOG_CAP;
    {
        const int64_t v = i.o_log_cap;
        if (v >= 1 && v <= (int64_t)HNSW_LOG_CAP) h.log_cap = (uint32_t)v;
    }
    h.vis_words = ((uint64_t)i.n_points + 31) / 32;
    if (h.vis_words == 0) h.vis_words = 1;
    h.hop_cap = 64;
    h.explore_cap = 0;
    if (i.acorn) {
        if (!(i.m0 >= 1 && i.m0 <= 128)) return 8;
        h.vis_words *= 2;
        if (!(i.max_row0 <= 8192)) return 9;
        h.explore_cap = std::max<uint32_t>(i.m0, i.max_row0);
        h.hop_cap = std::min<uint32_t>((i.m0 * (i.m0 + 1) + 63) / 64 * 64, 4160);
    }
    int per_cu = i.per_cu;
    h.pq_and_no_lds = i.dtype == PQ && h.lds_query_bytes == 0;
    if (i.dtype == PQ && h.lds_query_bytes == 0 && i.o_pq_per_cu > 0) per_cu = (int)std::min<int64_t>(per_cu, i.o_pq_per_cu);
    if (per_cu >= 8) per_cu -= per_cu % 4;
    if (i.o_per_cu > 0) per_cu = (int)std::min<int64_t>(per_cu, i.o_per_cu);
    uint64_t slots = std::min<uint64_t>({(uint64_t)i.n_searches, (uint64_t)i.num_cus * per_cu, (uint64_t)HNSW_SLOT_CAP});
    const uint64_t by_budget = std::max<uint64_t>(1, HNSW_VIS_BUDGET / (h.vis_words * 4));
    slots = std::max<uint64_t>(1, std::min(slots, by_budget));
    h.ev_cap = 0;
    if (i.xo) h.ev_cap = HNSW_EV_SPILL_CAP;
    if (h.ref_heaps) slots = std::min<uint64_t>(slots, HNSW_REF_SLOT_CAP);
    h.want = std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)std::max<uint32_t>(std::max(i.nq, i.n_searches), 1), (uint64_t)i.num_cus * per_cu,
                                                        (uint64_t)HNSW_SLOT_CAP, by_budget}));
    h.pq_direct = pq_direct;
    h.a_q_stride = a_q_stride;
    h.per_cu = per_cu;
    h.slots = slots;
    return 0;
}

// the walk as hnsw_enqueue describes it to the plan (api_hnsw.hip walk_shape)
WalkShape shape_of(const In &i) {
    WalkShape w;
    w.acorn = i.acorn; w.expanded = i.xo; w.multi = i.mw; w.custom = i.cw; w.traced = i.pt;
    w.filters = i.has_filters;
    w.storage = i.dtype == PQ ? WalkStorage::PQ : i.dtype == TQ_L1 ? WalkStorage::TqL1 : WalkStorage::Other;
    w.dim = i.dim;
    if (i.dtype == PQ) { w.pq_m = i.pq_m; w.n_centroids = i.pq_ncent; w.pq_direct_ok = i.pq_centroids_and_direct_ok; }
    if (i.dtype == TQ_L1) { w.tq_l1_entry_bytes = i.tq_query_bytes; w.tq_l1_lds_bytes = i.tq_lds_bytes; }
    w.q_stride = i.q_stride; w.top = i.top; w.ef = i.ef;
    w.batch_entries = i.queries_are_batch;
    w.n_points = i.n_points; w.m0 = i.m0; w.max_row0 = i.max_row0;
    if (i.mw) w.max_tokens = i.mw_max_tokens;
    if (i.cw) { w.max_examples = i.cw_max_examples; w.custom_lds_bytes = i.cw_lds_bytes; }
    w.opt_pq_direct_walk = i.o_pq_direct > 0;
    w.opt_reference_heap_order = i.o_ref_heaps > 0;
    w.opt_no_lds_visited = i.o_no_lds_visited != 0;
    w.opt_no_pq_prefilter = i.o_no_pq_prefilter != 0;
    w.opt_log_cap = i.o_log_cap;
    return w;
}

WalkSlots slots_of(const In &i, const WalkPlan &p) {
    WalkSlotOptions o;
    o.pq_per_cu = i.o_pq_per_cu;
    o.per_cu = i.o_per_cu;
    return hnsw_walk_slots(p, i.per_cu, i.n_searches, i.nq, i.num_cus, o);
}

// the plan against the longhand, for every occupancy and slot option
uint64_t check_one(In i) {
    Long h{};
    const int refused = longhand(i, h);
    const WalkPlan p = hnsw_walk_plan(shape_of(i));
    CHECK((int)p.refusal == refused);      // WalkRefusal lists the refusals in the longhand's order
    if (refused) return 1;
    CHECK(p.pq_direct == h.pq_direct && p.entry_stride == h.a_q_stride);
    CHECK((uint32_t)p.ref_heaps == h.ref_heaps && p.lds_query_bytes == h.lds_query_bytes && p.vis_lds == h.vis_lds);
    CHECK((p.pq_image == PqImage::None ? 0 : p.pq_image == PqImage::BatchLuts ? 1 : 2) == h.image);
    CHECK(p.pq_luts_in_l2 == h.pq_and_no_lds);
    CHECK(p.hop_cap == h.hop_cap && p.explore_cap == h.explore_cap && p.vis_words == h.vis_words && p.log_cap == h.log_cap && p.ev_cap == h.ev_cap);
    uint64_t n = 1;
    for (int per_cu = 1; per_cu <= 16; ++per_cu)
        for (int64_t o_pq_per_cu : {(int64_t)0, (int64_t)2})
            for (int64_t o_per_cu : {(int64_t)-1, (int64_t)3})
                for (uint32_t n_searches : {1u, 48u, 100000u}) {      // (a custom or multi-vector walk has fewer searches than its batch has entries)
                    i.per_cu = per_cu; i.o_pq_per_cu = o_pq_per_cu; i.o_per_cu = o_per_cu; i.n_searches = n_searches; i.nq = n_searches == 48 ? 300000 : n_searches;
                    CHECK(longhand(i, h) == 0);
                    const WalkSlots s = slots_of(i, p);
                    CHECK(s.per_cu == h.per_cu && s.slots == h.slots && s.want == h.want);
                    ++n;
                }
    return n;
}

struct Kind {
    const char *name;
    bool acorn, xo, pt, mw, cw;
};
struct Storage {
    const char *name;
    Dtype dtype;
    uint32_t pq_m, pq_ncent;
    bool direct_ok;
    uint32_t tq_query_bytes, tq_lds_bytes;
};

In base_case() {
    In i{};
    i.dtype = DENSE; i.dim = 768;
    i.q_stride = 3072 + 64; i.top = 10; i.ef = 64;
    i.queries_are_batch = true;
    i.n_points = 2000; i.m0 = 32; i.max_row0 = 32;
    i.o_log_cap = -1;
    i.per_cu = 16; i.n_searches = 48; i.nq = 48; i.num_cus = 256;
    return i;
}

uint64_t sweep() {
    // the walks an entry point can produce: qmx_hnsw_search / _acorn / _with_vectors / _traced, qmx_multi_hnsw_search, qmx_custom_hnsw_search, qmx_multi_custom_hnsw_search
    const std::vector<Kind> kinds = {{"plain", false, false, false, false, false}, {"acorn", true, false, false, false, false},
                                     {"with_vectors", false, true, false, false, false}, {"traced", false, false, true, false, false},
                                     {"multi", false, false, false, true, false}, {"custom", false, false, false, false, true},
                                     {"multi_custom", false, false, false, true, true}};
    const std::vector<Storage> storages = {
        {"dense", DENSE, 0, 0, false, 0, 0}, {"sq", SQ, 0, 0, false, 0, 0}, {"bq", BQ, 0, 0, false, 0, 0}, {"tq", TQ, 0, 0, false, 0, 0},
        {"tq_l1", TQ_L1, 0, 0, false, 3072, 3072 + 768 * 8 + 12320},          // a walk that fits
        {"tq_l1 wide", TQ_L1, 0, 0, false, 40000, 60000},                     // ... whose custom walk fits with 3 examples and not with 4
        {"tq_l1 too wide", TQ_L1, 0, 0, false, 100000, 160000},               // ... that does not fit
        {"pq 16x256", PQ, 16, 256, false, 0, 0},                              // LUTs of 16 KiB (with the strides <= 16 KiB below)
        {"pq 96x256", PQ, 96, 256, false, 0, 0},                              // ... of 96 KiB (with the strides above 16 KiB)
        {"pq 96x256 direct", PQ, 96, 256, true, 0, 0},                        // ... that the LUT-free walk takes
        {"pq 129x256 direct", PQ, 129, 256, true, 0, 0},                      // ... whose image the LDS does not hold
        {"pq 96x257", PQ, 96, 257, false, 0, 0},
    };
    const std::vector<uint32_t> strides = {512,        16384 - 16, 16384,     16384 + 16, 32768,  32768 + 16, 49152 - 32, 49152 - 16, 65536 - 16,
                                           65536,      98304 + 64, 153600,    153616,     156384, 156400};      // (156384 + hnsw_beam_lds(513..600) + 2048: around 160 KiB)
    const std::vector<uint32_t> efs = {1, 128, 129, 512, 513, 4096};
    const std::vector<uint32_t> m0s = {1, 16, 32, 64, 96, 128, 129};
    const std::vector<uint32_t> rows = {63, 65, 8192, 8193};
    const std::vector<uint32_t> points = {0, 1, 2000, HNSW_VIS_LDS_MAX_POINTS, HNSW_VIS_LDS_MAX_POINTS + 1, 3000000000u};      // (the last: 22 slots fit the visited budget)
    const std::vector<int64_t> log_caps = {-1, 0, 1, 7, HNSW_LOG_CAP, (int64_t)HNSW_LOG_CAP + 1};
    uint64_t n = 0, turn = 0;
    for (const Kind &k : kinds)
        for (const Storage &st : storages)
            for (uint32_t q_stride : strides)
                for (uint32_t ef : efs)
                    for (uint32_t m0 : m0s)
                        for (uint32_t row0 : rows)
                            for (uint32_t n_points : points)
                                for (int opts = 0; opts < 16; ++opts) {
                                    In i = base_case();
                                    i.acorn = k.acorn; i.xo = k.xo; i.pt = k.pt; i.mw = k.mw; i.cw = k.cw;
                                    i.dtype = st.dtype; i.pq_m = st.pq_m; i.pq_ncent = st.pq_ncent; i.pq_centroids_and_direct_ok = st.direct_ok;
                                    i.tq_query_bytes = st.tq_query_bytes; i.tq_lds_bytes = st.tq_lds_bytes;
                                    i.q_stride = q_stride;
                                    i.ef = ef; i.top = turn % 3 == 0 ? ef : 1;            // max(top, ef) = ef either way
                                    i.m0 = m0; i.max_row0 = row0; i.n_points = n_points;
                                    i.o_pq_direct = opts & 1 ? 1 : 0; i.o_ref_heaps = opts & 2 ? 1 : 0;
                                    i.o_no_lds_visited = opts & 4 ? 1 : 0; i.o_no_pq_prefilter = opts & 8 ? 1 : 0;
                                    i.o_log_cap = log_caps[turn % log_caps.size()];
                                    i.has_filters = turn % 5 == 4;                         // (the plain and ACORN walks serve them, the others refuse)
                                    // a multi-query of 1 or 4 vectors, a custom query of 1 or 4 examples; multi-vector examples bring their staged bytes
                                    i.mw_max_tokens = k.mw ? (turn % 2 ? 4 : 1) : 0;
                                    i.cw_max_examples = k.cw ? (turn % 4 < 2 ? 4 : 1) : 0;
                                    i.cw_lds_bytes = (k.cw && k.mw) ? (turn % 7 == 0 ? HNSW_LDS_QUERY_MAX + 16 : 32 + 16 + 4 * (16 + q_stride % 30000)) : 0;
                                    ++turn;
                                    // the occupancy and the slot options are swept where the slots can depend on the case: not on m0 and the longest list
                                    if (m0 == m0s[0] && row0 == rows[0]) n += check_one(i);
                                    else {
                                        Long h{};
                                        const int refused = longhand(i, h);
                                        const WalkPlan p = hnsw_walk_plan(shape_of(i));
                                        CHECK((int)p.refusal == refused);
                                        if (!refused) {
                                            CHECK(p.hop_cap == h.hop_cap && p.explore_cap == h.explore_cap && p.vis_words == h.vis_words);
                                            CHECK(p.lds_query_bytes == h.lds_query_bytes && p.vis_lds == h.vis_lds && (uint32_t)p.ref_heaps == h.ref_heaps);
                                            const WalkSlots s = slots_of(i, p);
                                            CHECK(s.per_cu == h.per_cu && s.slots == h.slots && s.want == h.want);
                                        }
                                        ++n;
                                    }
                                }
    return n;
}

void literal_cases() {
    // ACORN hop capacity: m0 (m0 + 1) rounded up to whole 64, capped where the kernel flushes early
    const uint32_t m0[4] = {16, 32, 64, 96}, hops[4] = {320, 1088, 4160, 4160};
    for (int k = 0; k < 4; ++k) {
        In i = base_case();
        i.acorn = true; i.m0 = m0[k]; i.max_row0 = 100;
        const WalkPlan p = hnsw_walk_plan(shape_of(i));
        CHECK(p.refusal == WalkRefusal::None && p.hop_cap == hops[k] && p.explore_cap == std::max(m0[k], 100u) && p.vis_lds == 0 && p.vis_words == 2 * 63);
    }
    {   // the plain walk over a small graph: entry staged, LDS visited table, 64 hop slots
        const WalkPlan p = hnsw_walk_plan(shape_of(base_case()));
        CHECK(p.refusal == WalkRefusal::None && p.lds_query_bytes == 3072 + 64 && p.vis_lds == HNSW_VIS_LDS_BYTES && p.hop_cap == 64 && p.explore_cap == 0);
        CHECK(p.vis_words == 63 && p.log_cap == HNSW_LOG_CAP && p.ev_cap == 0 && p.pq_image == PqImage::None && !p.ref_heaps);
    }
    {   // search_with_vectors carries a spill per slot
        In i = base_case();
        i.xo = true;
        CHECK(hnsw_walk_plan(shape_of(i)).ev_cap == HNSW_EV_SPILL_CAP);
    }
    {   // PQ, 96 x 256 centroids: 96 KiB of LUT stay in global memory, the image comes from the batch's LUTs and takes the visited table's room
        In i = base_case();
        i.dtype = PQ; i.pq_m = 96; i.pq_ncent = 256; i.q_stride = 96 * 256 * 4 + 64;
        WalkPlan p = hnsw_walk_plan(shape_of(i));
        CHECK(p.refusal == WalkRefusal::None && p.lds_query_bytes == 0 && p.pq_image == PqImage::BatchLuts && p.vis_lds == 0 && p.pq_luts_in_l2 && !p.pq_direct);
        // ... the LUT-free walk of the same storage stages the vector and wants the exact-order image
        i.pq_centroids_and_direct_ok = true; i.o_pq_direct = 1;
        p = hnsw_walk_plan(shape_of(i));
        CHECK(p.pq_direct && p.entry_stride == 768 * 4 && p.lds_query_bytes == 768 * 4 && p.pq_image == PqImage::ExactOrderLuts && p.vis_lds == 0 && !p.pq_luts_in_l2);
        // ... and 16 x 256 centroids (16 KiB) are staged, without an image
        i.o_pq_direct = 0; i.pq_m = 16; i.q_stride = 16384;
        p = hnsw_walk_plan(shape_of(i));
        CHECK(p.lds_query_bytes == 16384 && p.pq_image == PqImage::None && p.vis_lds == HNSW_VIS_LDS_BYTES);
    }
    {   // max(top, ef) = 600: the list lives in LDS behind the entry, which is staged whatever its size - and refused when both and 2048 bytes pass 160 KiB
        In i = base_case();
        i.ef = 600;
        CHECK(hnsw_beam_lds(600) == 5408);
        i.q_stride = 160 * 1024 - 2048 - 5408;
        WalkPlan p = hnsw_walk_plan(shape_of(i));
        CHECK(p.refusal == WalkRefusal::None && p.lds_query_bytes == i.q_stride && p.vis_lds == 0);
        i.q_stride += 16;
        p = hnsw_walk_plan(shape_of(i));
        CHECK(p.refusal == WalkRefusal::BeamLds);
    }
    {   // whole waves per SIMD, and the caps
        In i = base_case();
        i.n_searches = i.nq = 100000;
        const WalkPlan p = hnsw_walk_plan(shape_of(i));
        i.per_cu = 9;
        WalkSlots s = slots_of(i, p);
        CHECK(s.per_cu == 8 && s.slots == 2048 && s.want == 2048);
        i.per_cu = 7;
        s = slots_of(i, p);
        CHECK(s.per_cu == 7 && s.slots == 7 * 256);
        i.per_cu = 16; i.o_per_cu = 3;
        s = slots_of(i, p);
        CHECK(s.per_cu == 3 && s.slots == 768);
        i.o_per_cu = 0; i.n_searches = 48;
        s = slots_of(i, p);
        CHECK(s.per_cu == 16 && s.slots == 48 && s.want == HNSW_SLOT_CAP);
        // the visited budget: 3 G points are 375 MB of bitmap per slot
        i.n_points = 3000000000u; i.n_searches = 100000;
        s = slots_of(i, hnsw_walk_plan(shape_of(i)));
        CHECK(s.slots == 22 && s.want == 22);
        // reference-heap order: HNSW_REF_SLOT_CAP searches in flight at most, no LDS visited table
        i = base_case();
        i.o_ref_heaps = 1; i.n_searches = i.nq = 100000;
        const WalkPlan r = hnsw_walk_plan(shape_of(i));
        CHECK(r.ref_heaps && r.vis_lds == 0);
        CHECK(slots_of(i, r).slots == HNSW_REF_SLOT_CAP);
    }
    {   // the refusals, in their order: a walk that meets two reports the earlier one
        In i = base_case();
        i.dtype = TQ_L1; i.tq_query_bytes = 100000; i.tq_lds_bytes = 160000; i.mw = true; i.has_filters = true;
        CHECK(hnsw_walk_plan(shape_of(i)).refusal == WalkRefusal::TqL1Multi);
        i.mw = false; i.cw = true;
        CHECK(hnsw_walk_plan(shape_of(i)).refusal == WalkRefusal::Filters);
        i.has_filters = false;
        const WalkPlan p = hnsw_walk_plan(shape_of(i));
        CHECK(p.refusal == WalkRefusal::TqL1Lds && p.refused_bytes == 160000);
        i = base_case();
        i.acorn = true; i.m0 = 129; i.max_row0 = 9000;
        CHECK(hnsw_walk_plan(shape_of(i)).refusal == WalkRefusal::AcornM0);
        i.m0 = 128;
        CHECK(hnsw_walk_plan(shape_of(i)).refusal == WalkRefusal::AcornRow);
    }
}

}  // namespace

int main() {
    literal_cases();
    const uint64_t n = sweep();
    printf("hnsw_walk_plan_check: %llu combinations ok\n", (unsigned long long)n);
    return 0;
}
