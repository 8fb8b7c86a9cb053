// api_search.hip — the C-ABI of include/qdrant_amd.h, brute-force top-k: the exact scans, the prefilters, the merge, the oversampled quantized search.
// (One of the api_*.hip translation units; what they share: api_internal.hpp.)
// search_enqueue: search_plan decides the route once, then one function per route runs - tq_l1_search, pq_prefilter_search, wide_exact_search (SQ / TQ), and per
// tile of the f32 / exact driver split_tile (f16_split_scan | i8_copy_scan) or exact_tile.  The prefilter routes share one skeleton, each step written once:
// prefilter_begin (plan block, verification pool, sample), bound_enqueue, the route's approximate pass, verify_and_sort, overflow_passes, close_counters.
#include "api_internal.hpp"

extern "C" {

// what one search_enqueue carries to its route: the caller's arguments, and the launches counted so far (qmx_counters::kernel_launches)
struct SearchCall {
    qmx_query *q;
    uint32_t top;
    const uint32_t *d_ids;
    uint64_t n_cand;      // rows of the id list, or of the block
    qmx_scored_point *d_out;
    uint32_t *d_counts;
    const volatile uint8_t *is_stopped;
    qmx_counters *counters;
    bool timed;
    uint32_t launches;
};

// the arguments of a scan of the whole candidate set for queries tile0 .. tile0 + nq_tile
static ScanArgs tile_args(const qmx_query *q, uint32_t top, uint64_t n_cand, uint32_t tile0, uint32_t nq_tile) {
    ScanArgs a;
    fill_args(q, tile0, nq_tile, a);
    a.n_cand = n_cand;
    a.top = top;
    return a;
}
static ScanArgs tile_args(const SearchCall &c, uint32_t tile0, uint32_t nq_tile) { return tile_args(c.q, c.top, c.n_cand, tile0, nq_tile); }

// a scoring launch between the events of timing mode; the kernel it noted is what qmx_query_last_kernel reports
#define QMX_TIMED_SCAN(c, launch)                                  \
    do {                                                           \
        size_t slot__ = 0;                                         \
        if ((c).timed) QMX_TRY(timing_begin((c).q, &slot__));      \
        QMX_TRY(launch);                                           \
        (c).q->last_kernel = last_noted_kernel();                  \
        if ((c).timed) QMX_TRY(timing_end((c).q, slot__));         \
    } while (0)

// ---- the route of a search, decided once ----
constexpr uint32_t PQF_TILE = 256;          // PQ prefilter: queries per pass (64 four-query groups; the regroup kernel's histogram)
constexpr uint32_t PQF_WCAP = 512;          // ... candidates one wave may list per pass (expected: tens)
constexpr uint32_t TQW_FQT = 32;            // SQ / TQ wide: queries per conditional exact pass

enum SearchRoute {
    ROUTE_TQ_L1,          // Manhattan TurboQuant: the score matrix, one block per query selects
    ROUTE_PQ_PREFILTER,   // pq_prefilter.hip
    ROUTE_TQ_WIDE,        // scan_tq4w.hip
    ROUTE_SQ_WIDE,        // scan_sqw.hip
    ROUTE_SPLIT_ROWS,     // scan_split.hip over the f32 rows themselves (more than 64 queries)
    ROUTE_SPLIT_F16,      // ... over an f16 copy (QMX_SEG_HALF_COPY / QMX_SEG_SPLIT_COPY)
    ROUTE_I8_COPY,        // ... over the int8 copy (QMX_SEG_I8_COPY)
    ROUTE_EXACT,          // tiles of the exact scans
};
struct SearchPlan {
    SearchRoute route;
    uint32_t tile_q;           // queries per tile of the route's loop
    uint32_t split_qt;         // the split shape: SPLIT_QT, or SPLIT_QT_MAX over a half copy
    uint32_t split_fqt;        // queries per conditional exact pass behind the f32 prefilters
    uint32_t n_pass;           // exact tiles: passes of MAX_TOP_FAST entries
    uint32_t split_min_tile;   // a tile of at least this many queries takes the split route, a smaller (remainder) tile the exact one
    bool split() const { return route == ROUTE_SPLIT_ROWS || route == ROUTE_SPLIT_F16 || route == ROUTE_I8_COPY; }
    bool tile_splits(uint32_t nq_tile) const { return split() && nq_tile >= split_min_tile; }
};

// (host arithmetic over the handles and the options: no HIP call, no allocation)
static SearchPlan search_plan(const qmx_query *q, uint32_t top, const uint32_t *d_ids, uint64_t n_cand) {
    const qmx_segment *s = q->seg;
    SearchPlan p{ROUTE_EXACT, 0, SPLIT_QT, SPLIT_FQT, (top + MAX_TOP_FAST - 1) / MAX_TOP_FAST, 0};
    auto whole = [&p](SearchRoute route, uint32_t tile_q) {      // a route that serves the whole batch in tiles of its own
        p.route = route;
        p.tile_q = tile_q;
        return p;
    };
    // (tiles of queries: at most 256 MiB of scores at a time)
    if (tq_l1(s)) return whole(ROUTE_TQ_L1, (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(q->nq, (1ull << 26) / std::max<uint64_t>(n_cand, 1))));
    if (s->dtype == QMX_DTYPE_PQ && s->d_pq_rot && !d_ids && top <= MAX_TOP_FAST && n_cand >= (1u << 18) && !option(OPT_NO_PQ_PREFILTER) &&
        q->nq >= (uint32_t)std::max<int64_t>(1, option(OPT_PQ_PREFILTER_MIN_QUERIES)))
        return whole(ROUTE_PQ_PREFILTER, PQF_TILE);
    if (s->dtype == QMX_DTYPE_TQ && s->tq_wide && !d_ids && top <= MAX_TOP_FAST && n_cand >= (1u << 18) && mfma_scan_ok(s) && option(OPT_TQ_WIDE_MIN_QUERIES) > 0 &&
        q->nq >= (uint32_t)option(OPT_TQ_WIDE_MIN_QUERIES) && (size_t)MAX_QT_MFMA * q->q_stride <= 150 * 1024 && tq4w_shape_ok(tile_args(q, top, n_cand, 0, std::min<uint32_t>(q->nq, SPLIT_QT))))
        return whole(ROUTE_TQ_WIDE, SPLIT_QT);
    if (s->dtype == QMX_DTYPE_SQ_U8 && s->sq_wide && !d_ids && top <= MAX_TOP_FAST && n_cand >= (1u << 18) && mfma_scan_ok(s) && option(OPT_SQ_WIDE_MIN_QUERIES) > 0 &&
        q->nq >= (uint32_t)option(OPT_SQ_WIDE_MIN_QUERIES) && sqw_shape_ok(tile_args(q, top, n_cand, 0, std::min<uint32_t>(q->nq, SPLIT_QT))))
        return whole(ROUTE_SQ_WIDE, SPLIT_QT);
    // f32 dot / cosine rows of 256, 512 or 768 floats, whole block: 64 queries per pass (scan_mfma16.hip); everything else 32 / 16
    const bool q64 = s->dtype == QMX_DTYPE_F32 && mfma_scan_ok(s) && q->nq > MAX_QT_MFMA && mfma16_dim_ok(64, s->dim) && !option(OPT_NO_MFMA16);
    // ... and rows of 1024 .. 1536 floats 32 per pass: that kernel keeps the queries in registers, not in an LDS tile (tile_qt's limit)
    const bool q32 = s->dtype == QMX_DTYPE_F32 && mfma_scan_ok(s) && q->nq > MAX_QT && s->dim > 768 && mfma16_dim_ok(32, s->dim) && !option(OPT_NO_MFMA16);
    // more than 64 queries over a large f32 dot / cosine block: 128 per pass through the f16-split matrix-core prefilter, the survivors
    // re-scored exactly (scan_split.hip); the result is the exact scan's, bit for bit
    // ... and with a derived copy of the block (QMX_SEG_HALF_COPY / QMX_SEG_SPLIT_COPY) that path serves EVERY batch size: it streams 2 (4) bytes
    // per element instead of 4 and is HBM-bound whatever the number of queries (10 M x 768: 3.0 ms per pass against 4.4 ms for the f32 stream)
    // (rows of up to 768 floats: conditional exact passes of 64 queries; up to 2 048 floats - 1 024, 1 536: the 32-query shape - only over a derived copy)
    const uint32_t split_fqt = split_fallback_qt(s->dim);
    const bool split_dims = s->dtype == QMX_DTYPE_F32 && mfma_scan_ok(s) && (mfma16_dim_ok(64, s->dim) || (s->d_rows_split && split_fqt != 0)) && !option(OPT_NO_MFMA16);
    const bool split = split_dims && (q64 || (s->d_rows_split && q->nq >= (uint32_t)std::max<int64_t>(1, option(OPT_SPLIT_MIN_QUERIES)))) && s->split_stats &&
                       !d_ids && top <= MAX_TOP_FAST && n_cand >= (1u << 18) && s->dim % 128 == 0 && s->row_stride % 16 == 0 && !option(OPT_NO_SPLIT_SCAN);
    // the 256-query shape halves the bytes streamed per query; a batch that does not fill it is served by the 128-query shape (less matrix work)
    if (split && s->d_rows_split && s->split_half && q->nq > SPLIT_QT && !option(OPT_NO_SPLIT256)) p.split_qt = SPLIT_QT_MAX;
    if (split_fqt) p.split_fqt = split_fqt;
    if (split) p.route = s->split_i8 ? ROUTE_I8_COPY : s->d_rows_split ? ROUTE_SPLIT_F16 : ROUTE_SPLIT_ROWS;
    // (without a copy the prefilter pays from 65 queries on: a remainder tile of at most 64 takes the exact scan)
    p.split_min_tile = s->d_rows_split ? 1 : MAX_QT_TOPK + 1;
    p.tile_q = split ? p.split_qt : q64 ? MAX_QT_TOPK : q32 ? MAX_QT_MFMA : tile_qt(s, q);
    return p;
}

// ---- the steps the routes share ----
// triage aid (qmx_set_option("debug", 2)): synchronise after every stage of the split path and name it on stderr
static int32_t split_stage(qmx_query *q, const char *what) {
    if (option(OPT_DEBUG) < 2) return QMX_OK;
    hipError_t e = hipStreamSynchronize(q->stream);
    fprintf(stderr, "[qmx] split stage %-28s %s\n", what, e == hipSuccess ? "ok" : hipGetErrorString(e));
    fflush(stderr);
    QMX_HIP(e);
    return QMX_OK;
}

// the verification pool of a search (kernels.hpp VerifyPool): SPLIT_VCAP entries per query of the batch, shared - behind qmx_query::sp_ver as
// [ids: cap][qsel: cap][off: nq][cnt: nq], exact scores in sp_vscores, the fill level in the plan block (zeroed with it at the start of a search)
static int32_t verify_pool(qmx_query *q, unsigned char *plan, VerifyPool *vp) {
    const uint32_t cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((uint64_t)q->nq * SPLIT_VCAP, 262144), 1u << 26);
    QMX_TRY(q->sp_ver.reserve(((size_t)cap * 2 + (size_t)q->nq * 2) * 4));
    QMX_TRY(q->sp_vscores.reserve((size_t)cap * 4));
    uint32_t *b = (uint32_t *)q->sp_ver.p;
    const int64_t mx = option(OPT_VERIFY_MAX_PER_QUERY);
    *vp = VerifyPool{b, b + cap, b + (size_t)2 * cap, b + (size_t)2 * cap + q->nq, (uint32_t *)(plan + SplitPlanLayout::pool_used), cap,
                     mx > 0 ? (uint32_t)std::min<int64_t>(mx, cap) : cap};
    return QMX_OK;
}

// ids of a strided sample of the candidates (rows 0, step, 2 step, ...): a sample that sees the whole block, whatever its order
__global__ void sample_ids_kernel(uint32_t *ids, uint32_t n, uint64_t step) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = (uint32_t)((uint64_t)i * step);
}

// ids of a sample made of T whole 16-row tiles (the int8 copy's operand tiles, option i8_sample_scan): tile i of the sample is row tile i * step of the
// block, step = (n / 16) / T - complete row tiles only, spread evenly.  Entry 16 i + r is row 16 i step + r (include/qdrant_amd.h states the rule)
__global__ void sample_tile_ids_kernel(uint32_t *ids, uint32_t n, uint64_t step) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = (uint32_t)((uint64_t)(i >> 4) * step * 16u + (i & 15u));
}

// what a prefilter search starts with: the plan block and the verification pool behind it, then the sample - every 2^(prescan_shift + shift)-th row,
// at least 8 192 rows, its id list kept across searches of the same block size - and the zeros of the plan block.  Returns the sample's size.
// (tiles: the int8 route's sample of whole 16-row tiles - the same size rounded down to a multiple of 16, or what option i8_sample_rows says)
static int32_t prefilter_begin(qmx_query *q, const SplitPlanLayout &pl, uint64_t n_cand, int shift, VerifyPool *vp, uint64_t *S_out, bool tiles = false) {
    QMX_TRY(q->sp_plan.reserve(pl.bytes));
    QMX_TRY(verify_pool(q, (unsigned char *)q->sp_plan.p, vp));
    const int sshift = (int)std::min<int64_t>(std::max<int64_t>(option(OPT_PRESCAN_SHIFT) + shift, 1), 20);
    uint64_t S = std::min<uint64_t>(n_cand, std::max<uint64_t>(n_cand >> sshift, 8192));
    if (tiles) {
        const int64_t rows_opt = option(OPT_I8_SAMPLE_ROWS);
        if (rows_opt > 0) S = std::min<uint64_t>(n_cand, std::max<int64_t>(rows_opt, 16));
        S &= ~(uint64_t)15;
        QMX_REQUIRE(S >= 16, QMX_ERR_OTHER, "a sample of row tiles needs a block of 16 rows");
    }
    if (q->sp_sample_n != S || q->sp_sample_of != n_cand || q->sp_sample_tiles != tiles) {
        QMX_TRY(q->sp_sample.reserve((size_t)S * 4));
        ::qmx::clear_stale_error();
        if (tiles)
            hipLaunchKernelGGL(sample_tile_ids_kernel, dim3((uint32_t)((S + 255) / 256)), dim3(256), 0, q->stream, (uint32_t *)q->sp_sample.p, (uint32_t)S,
                               (n_cand / 16) / (S / 16));
        else
            hipLaunchKernelGGL(sample_ids_kernel, dim3((uint32_t)((S + 255) / 256)), dim3(256), 0, q->stream, (uint32_t *)q->sp_sample.p, (uint32_t)S, n_cand / S);
        QMX_HIP(hipGetLastError());
        q->sp_sample_n = S;
        q->sp_sample_of = n_cand;
        q->sp_sample_tiles = tiles;
    }
    QMX_HIP(hipMemsetAsync(q->sp_plan.p, 0, pl.zero_bytes, q->stream));
    *S_out = S;
    return QMX_OK;
}

// exact scores of `n` candidates (the score-mode kernels, <= tile_qt queries per launch) -> one block per query selects its k best live ones; the k-th
// becomes the tile's bound in gthr, a lower bound of the final k-th best: of a prefilter's sample, of the prefix an exact tile scans first.
// (sample: a prefilter's - its two kernels are the head of every batch's chain and, with four batches in flight, are dispatched while another batch's
//  int8 scan holds every CU: they take the shapes that fit beside a scan block, option prescan_beside_scan.  An exact tile's prefix keeps the wide ones)
static int32_t bound_enqueue(const SearchCall &c, uint32_t tile0, uint32_t nq_tile, const uint32_t *d_ids, uint64_t n, uint32_t ktop, const DeletedView &del,
                             uint32_t *launches, bool sample) {
    qmx_query *q = c.q;
    QMX_TRY(q->scores.reserve((size_t)nq_tile * n * sizeof(float)));
    QMX_TRY(score_matrix_enqueue(q, tile0, nq_tile, d_ids, n, (float *)q->scores.p, n, launches, sample));
    // (the bound at the tile's own offset: the bounds of earlier split tiles are read again by the plan of their exact passes)
    return launch_custom_topk(q->stream, (const float *)q->scores.p, n, d_ids, del, nq_tile, ktop, c.d_out + (size_t)tile0 * c.top, c.d_counts + tile0,
                              (uint64_t *)q->gthr.p + tile0, sample);
}

// exact scores of the pool's rows (the pair kernels: the reference's bits), sorted by (score, lower id first) into the lists of queries 0 .. nq
static int32_t verify_and_sort(const SearchCall &c, const VerifyPool &vp, uint32_t nq) {
    qmx_query *q = c.q;
    const void *scan_kernel = q->last_kernel;      // (the pair kernel is not what the search reports)
    PairSel sel{vp.qsel, 0, nullptr, vp.used};
    QMX_TRY(score_pairs_device(q, sel, vp.ids, vp.cap, (float *)q->sp_vscores.p, false));
    q->last_kernel = scan_kernel;
    QMX_TRY(split_stage(q, "verify gather"));
    QMX_TRY(launch_sort_scored(q->stream, (const float *)q->sp_vscores.p, vp.ids, vp.cnt, 0, nq, c.top, c.d_out, c.d_counts, vp.off));
    return split_stage(q, "verify sort");
}

// the exact top-k scan of `fqt` packed queries: what overflow_passes launches
typedef int32_t (*OverflowScan)(hipStream_t st, int fqt, const ScanArgs &a, int num_cus, uint32_t *grid);
static int32_t overflow_scan_f32(hipStream_t st, int fqt, const ScanArgs &a, int num_cus, uint32_t *grid) {
    QMX_REQUIRE(mfma16_scan_ok(fqt, SCAN_TOPK, a), QMX_ERR_OTHER, "split fallback shape");
    return launch_scan_f32_mfma16(st, fqt, a, num_cus, grid);
}
static int32_t overflow_scan_sq(hipStream_t st, int fqt, const ScanArgs &a, int num_cus, uint32_t *grid) { return launch_scan_sq_mfma(st, fqt, SCAN_TOPK, a, num_cus, grid); }
static int32_t overflow_scan_tq(hipStream_t st, int fqt, const ScanArgs &a, int num_cus, uint32_t *grid) { return launch_scan_tq_mfma(st, fqt, SCAN_TOPK, a, num_cus, grid); }

// the exact scan of the queries (of 0 .. nq) whose lists overflowed - masses of near-equal scores, a sample that is all deleted -, and of those only:
// packed, one 16-query pass when 1..16 of them, passes of FQT otherwise.  The kernels start, read their flag and return when it is clear.
static int32_t overflow_passes(const SearchCall &c, const SplitPlanLayout &pl, uint32_t nq, uint32_t FQT, OverflowScan scan, uint32_t *launches) {
    qmx_query *q = c.q;
    unsigned char *plan = (unsigned char *)q->sp_plan.p;
    uint32_t *ovf_list = (uint32_t *)(plan + pl.list);
    uint64_t *gthr_packed = (uint64_t *)(plan + pl.gthr_packed);
    const uint32_t n_run = (nq + FQT - 1) / FQT;
    // (per-request filters: the packed queries' bitmap indices, packed with them)
    if (q->has_filters) QMX_TRY(q->filter_of_packed.reserve((size_t)n_run * FQT * 4));
    const uint32_t *fof_packed = q->has_filters ? (const uint32_t *)q->filter_of_packed.p : nullptr;
    QMX_TRY(launch_split_plan(q->stream, (const uint32_t *)(plan + pl.ovf_q), nq, (const uint64_t *)q->gthr.p, ovf_list, gthr_packed, n_run * FQT,
                              (uint32_t *)(plan + pl.count), (int *)(plan + pl.run16), (int *)(plan + pl.run64), n_run, (SplitStats *)plan, q->d_queries,
                              q->q_stride, q->sp_fq.p, q->has_filters ? (const uint32_t *)q->filter_of.p : nullptr, (uint32_t *)q->filter_of_packed.p));
    for (uint32_t pass = 0; pass <= n_run; ++pass) {      // pass 0: the 16-query shape; pass p >= 1: packed queries FQT (p - 1) ..
        if (pass && nq <= 16) break;
        const uint32_t p0 = pass ? (pass - 1) * FQT : 0;
        const uint32_t nq_sub = pass ? std::min<uint32_t>(FQT, nq - p0) : std::min<uint32_t>(16, nq);
        const int *run_if = pass ? (const int *)(plan + pl.run64) + (pass - 1) : (const int *)(plan + pl.run16);
        ScanArgs a = tile_args(c, 0, nq_sub);
        a.queries = (const char *)q->sp_fq.p + (size_t)p0 * q->q_stride;
        if (fof_packed) a.del.filter_of = fof_packed + p0;
        a.partial = (uint64_t *)q->partial.p;
        a.gthr = gthr_packed + p0;
        a.run_if = run_if;
        const int fqt = (int)std::max<uint32_t>(16, pow2_ceil(nq_sub));
        a.partial_qt = (uint32_t)fqt;
        uint32_t grid = (uint32_t)q->seg->num_cus * 8;
        QMX_TRY(scan(q->stream, fqt, a, q->seg->num_cus, &grid));
        QMX_TRY(launch_merge_keys(q->stream, (const uint64_t *)q->partial.p, grid, (uint32_t)fqt, nq_sub, c.top, c.d_out, c.d_counts, c.top, 0, nullptr, run_if,
                                  ovf_list + p0));
        if (launches) *launches += 2;
    }
    return split_stage(q, "fallback (conditional)");
}

// The int8 route's form of the same that starts beside a running int8 scan (option fallback_beside_scan): the plan, ONE launch of the 16-query shape whose
// block row g serves packed queries 16 g .. 16 g + 15 (launch_scan_f32_mfma16_groups), one merge over all packed slots.  With four batches in flight
// another batch's scan holds every CU while these are dispatched; blocks of the passes above cannot start there, and on a search without overflow
// they start only to find that out.
// Does a block of that launch fit on a CU beside a block of this segment's int8 scan?  The numbers the launches use: the scan's LDS at this row length
// plus the pass's against the CU's 160 KiB, the scan's two waves per SIMD plus the pass's one against 512 registers (the kernels' attributes).
static int32_t fallback_groups_fit(const qmx_query *q, uint32_t top, bool *fit) {
    const qmx_segment *s = q->seg;
    *fit = false;
    if (option(OPT_FALLBACK_BESIDE_SCAN) <= 0 || !mfma16_dim_ok(16, s->dim) || top > 64 || s->row_stride % 16 != 0) return QMX_OK;
    const uint32_t ks = s->dim / 128, perq = q->has_filters ? 1 : 0, res = option(OPT_I8_RESIDENT) > 0 ? 1 : 0;
    static std::atomic<int> known[2][2][17];      // 0: not asked yet, 1: fits, 2: does not ([resident scan][per-request filters][K-steps]: what picks the kernels)
    int k = known[res][perq][ks].load(std::memory_order_relaxed);
    if (k == 0) {
        size_t scan_lds = 0, pass_lds = 0;
        int scan_regs = 0, pass_regs = 0;
        QMX_TRY(split_i8_scan_footprint(s->dim, &scan_lds, &scan_regs));
        QMX_TRY(mfma16_groups_footprint(s->dim, perq != 0, &pass_lds, &pass_regs));
        k = scan_lds + pass_lds <= (size_t)160 * 1024 && scan_regs + pass_regs <= 512 ? 1 : 2;
        known[res][perq][ks].store(k, std::memory_order_relaxed);
    }
    *fit = k == 1;
    return QMX_OK;
}
// (partial lists: grid.x <= 2 blocks per CU, by ceil(nq / 16) groups, of 16 x top keys - search_enqueue reserves them)
static size_t overflow_groups_partial_bytes(const qmx_query *q, uint32_t top) {
    return (size_t)q->seg->num_cus * 2 * ((q->nq + 15) / 16) * 16 * top * sizeof(uint64_t);
}
static int32_t overflow_groups_pass(const SearchCall &c, const SplitPlanLayout &pl, uint32_t nq) {
    qmx_query *q = c.q;
    unsigned char *plan = (unsigned char *)q->sp_plan.p;
    uint32_t *ovf_list = (uint32_t *)(plan + pl.list);
    uint64_t *gthr_packed = (uint64_t *)(plan + pl.gthr_packed);
    if (q->has_filters) QMX_TRY(q->filter_of_packed.reserve((size_t)pl.list_cap * 4));
    QMX_TRY(launch_split_plan(q->stream, (const uint32_t *)(plan + pl.ovf_q), nq, (const uint64_t *)q->gthr.p, ovf_list, gthr_packed, pl.list_cap,
                              (uint32_t *)(plan + pl.count), (int *)(plan + pl.run16), (int *)(plan + pl.run64), pl.n_run64, (SplitStats *)plan, q->d_queries,
                              q->q_stride, q->sp_fq.p, q->has_filters ? (const uint32_t *)q->filter_of.p : nullptr, (uint32_t *)q->filter_of_packed.p));
    ScanArgs a = tile_args(c, 0, nq);      // (nq: the packed slots; the kernel's block rows take 16 of them each and read how many are filled)
    a.queries = q->sp_fq.p;
    if (q->has_filters) a.del.filter_of = (const uint32_t *)q->filter_of_packed.p;
    a.partial = (uint64_t *)q->partial.p;
    a.partial_qt = 16;
    a.gthr = gthr_packed;
    a.run_if = (const int *)(plan + pl.count);
    QMX_REQUIRE(mfma16_scan_ok(16, SCAN_TOPK, a), QMX_ERR_OTHER, "split fallback shape");
    uint32_t grid = (uint32_t)q->seg->num_cus * 2;      // (the cap the reservation was made for)
    QMX_REQUIRE(nq <= q->nq && overflow_groups_partial_bytes(q, c.top) <= q->partial.cap, QMX_ERR_OTHER, "split fallback: partial lists");
    QMX_TRY(launch_scan_f32_mfma16_groups(q->stream, a, q->seg->num_cus, &grid));
    QMX_TRY(launch_merge_keys(q->stream, (const uint64_t *)q->partial.p, grid, 16, nq, c.top, c.d_out, c.d_counts, c.top, 0, nullptr, a.run_if, ovf_list, 0, true));
    return split_stage(q, "fallback (conditional, one launch)");
}

// the PQ form of the same: the exact PQ kernel takes the overflowed queries through q_map, one launch over slabs of the block
static int32_t pq_overflow_pass(const SearchCall &c, const SplitPlanLayout &pl) {
    qmx_query *q = c.q;
    const qmx_segment *s = q->seg;
    unsigned char *plan = (unsigned char *)q->sp_plan.p;
    uint32_t *ovf_list = (uint32_t *)(plan + pl.list);
    QMX_TRY(launch_split_plan(q->stream, (const uint32_t *)(plan + pl.ovf_q), q->nq, (const uint64_t *)q->gthr.p, ovf_list, (uint64_t *)(plan + pl.gthr_packed),
                              pl.list_cap, (uint32_t *)(plan + pl.count), (int *)(plan + pl.run16), (int *)(plan + pl.run64), pl.n_run64, (SplitStats *)plan, nullptr, 0,
                              nullptr));
    ScanArgs a = tile_args(c, 0, q->nq);
    a.q_map = ovf_list;
    a.run_if = (const int *)(plan + pl.count);
    const uint64_t want = (c.n_cand + 1023) / 1024, cap = std::max<uint64_t>(1, ((uint64_t)s->num_cus * 2 + q->nq - 1) / q->nq);
    uint32_t slabs = (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
    QMX_TRY(q->partial.reserve((size_t)slabs * q->nq * c.top * sizeof(uint64_t)));
    a.partial = (uint64_t *)q->partial.p;
    a.partial_qt = q->nq;
    QMX_TRY(launch_scan_pq(q->stream, SCAN_TOPK, a, s->num_cus, &slabs));
    return launch_merge_keys(q->stream, (const uint64_t *)q->partial.p, slabs, q->nq, q->nq, c.top, c.d_out, c.d_counts, c.top, 0, nullptr, a.run_if, ovf_list,
                             slabs * q->nq);
}

// what the host knows of a search at enqueue -> qmx_query::last_counters and the caller's; the prefilter's own share (candidates, verified rows, exact
// passes of overflowed queries) is on the device until the stream is synchronised: fold_split_counters
static void close_counters(const SearchCall &c, uint64_t vectors_scored, uint64_t bytes_read, uint64_t launches, uint32_t prefilter_queries) {
    qmx_query *q = c.q;
    qmx_counters &lc = q->last_counters;
    lc.vectors_scored = vectors_scored;
    lc.bytes_read = bytes_read;
    lc.kernel_launches = launches;
    lc.prefilter_queries = prefilter_queries;
    q->last_row_bytes = q->seg->row_bytes;
    q->last_n_cand = c.n_cand;
    if (c.counters) *c.counters = lc;
}

// ---- Manhattan TurboQuant: the score matrix of a tile of queries, then one block per query selects its k best live candidates ----
static int32_t tq_l1_search(const SearchCall &c, const SearchPlan &plan) {
    qmx_query *q = c.q;
    const qmx_segment *s = q->seg;
    const uint32_t qtile = plan.tile_q;
    ScanArgs a;
    fill_args(q, 0, q->nq, a);
    QMX_TRY(q->scores.reserve((size_t)qtile * std::max<uint64_t>(c.n_cand, 1) * sizeof(float)));
    for (uint32_t q0 = 0; q0 < q->nq; q0 += qtile) {
        QMX_CHECK_CANCELLED(c.is_stopped);
        const uint32_t nq_tile = std::min<uint32_t>(qtile, q->nq - q0);
        QMX_TRY(tq_l1_scores_device(q, q0, nq_tile, c.d_ids, c.n_cand, (float *)q->scores.p, c.n_cand, nullptr));
        DeletedView del = a.del;      // (block b of the selection is query q0 + b)
        if (del.filter_of) del.filter_of += q0;
        QMX_TRY(launch_custom_topk(q->stream, (const float *)q->scores.p, c.n_cand, c.d_ids, del, nq_tile, c.top, c.d_out + (size_t)q0 * c.top, c.d_counts + q0));
        if (c.counters) c.counters->kernel_launches += 1 + 3 * (uint32_t)((c.n_cand + 65535) / 65536);
    }
    if (c.counters) {      // (this route adds to the caller's counters and leaves last_counters at zero)
        c.counters->vectors_scored += (uint64_t)q->nq * c.n_cand;
        c.counters->bytes_read += (uint64_t)((q->nq + qtile - 1) / qtile) * c.n_cand * s->row_bytes;
    }
    return QMX_OK;
}

// ---- PQ top-k of 4 and more queries over a large block: the 6-bit prefilter + exact verification (pq_prefilter.hip).  Same contract as the f32
// prefilter below: the lists are the exact scan's, a query whose lists overflow takes the exact scan alone. ----
static int32_t pq_prefilter_search(SearchCall &c) {
    qmx_query *q = c.q;
    const qmx_segment *s = q->seg;
    const SplitPlanLayout pl(q->nq);
    const uint32_t m = s->pq_m, m_pad = (m + 31) / 32 * 32;
    const uint32_t tile_max = std::min<uint32_t>(PQF_TILE, q->nq);
    const uint32_t grid_max = pq_prefilter_grid(s->num_cus, tile_max, nullptr);
    QMX_TRY(q->gthr.reserve((size_t)std::max<uint32_t>(q->nq_padded, PQF_TILE) * sizeof(uint64_t)));
    QMX_TRY(q->pq_table.reserve(pq_prefilter_table_bytes(m, tile_max) + (size_t)(PQF_TILE + 4) * 4));
    QMX_TRY(q->sp_f32.reserve(SplitF32::floats_wide * sizeof(float)));
    QMX_TRY(q->sp_cand.reserve((size_t)tile_max * SPLIT_CAND_CAP * sizeof(uint64_t)));
    QMX_TRY(q->sp_cnt.reserve((size_t)SPLIT_QT_MAX * 4));
    {   // (the grid of a smaller last tile may be larger than the first tile's: size for the worst over tile sizes 1..tile_max)
        uint32_t g = grid_max;
        for (uint32_t t = 4; t <= tile_max; t += 4) g = std::max(g, pq_prefilter_grid(s->num_cus, t, nullptr));
        QMX_TRY(q->sp_wl.reserve(pq_prefilter_wlists_bytes(g, PQF_WCAP)));
    }
    // the sample (as for the f32 prefilter): its k-th best exact score per query is a lower bound of the final k-th best
    VerifyPool vp;
    uint64_t S = 0;
    QMX_TRY(prefilter_begin(q, pl, c.n_cand, -2, &vp, &S));
    unsigned char *plan = (unsigned char *)q->sp_plan.p;
    float *band = SplitF32(q->sp_f32.p).pq_band;       // [PQF_TILE] in units of the integer score
    uint32_t n_tiles = 0;
    for (uint32_t tile0 = 0; tile0 < q->nq; tile0 += PQF_TILE, ++n_tiles) {
        const uint32_t nq_tile = std::min<uint32_t>(PQF_TILE, q->nq - tile0);
        QMX_CHECK_CANCELLED(c.is_stopped);
        const uint64_t *gthr = (const uint64_t *)q->gthr.p + tile0;
        const ScanArgs a = tile_args(c, tile0, nq_tile);
        // 1. exact scores of the sample (the exact kernel's score mode over an id list) -> k-th best per query
        QMX_TRY(bound_enqueue(c, tile0, nq_tile, (const uint32_t *)q->sp_sample.p, S, c.top, a.del, &c.launches, true));
        // 2. the 6-bit tables of the tile's query groups, thresholds and bands in units of the integer score
        int32_t *thr = (int32_t *)((unsigned char *)q->pq_table.p + pq_prefilter_table_bytes(m, tile_max));
        QMX_TRY(launch_pq_lut8(q->stream, a.queries, q->q_stride, nq_tile, m, s->pq.n_centroids, gthr, q->pq_table.p, thr, band));
        QMX_HIP(hipMemsetAsync(q->sp_cnt.p, 0, (size_t)SPLIT_QT_MAX * 4, q->stream));
        // 3. the approximate scan of the whole block over the rotated copy
        uint32_t grid = 0;
        QMX_TIMED_SCAN(c, launch_pq_prefilter(q->stream, a, s->d_pq_rot, q->pq_table.p, thr, nq_tile, s->num_cus, q->sp_wl.p, PQF_WCAP, &grid));
        // 4. per-wave lists -> per-query lists (deleted rows dropped), then the rows worth an exact score
        int *tile_ovf = (int *)(plan + pl.tile_ovf) + n_tiles;
        QMX_TRY(launch_regroup_lists(q->stream, a.del, (const unsigned char *)q->sp_wl.p + pq_prefilter_wlists_counts_bytes(grid), (const uint32_t *)q->sp_wl.p, PQF_WCAP,
                                     grid * 16, (uint64_t *)q->sp_cand.p, (uint32_t *)q->sp_cnt.p, SPLIT_CAND_CAP, tile_ovf));
        QMX_TRY(launch_split_select(q->stream, (const uint64_t *)q->sp_cand.p, (const uint32_t *)q->sp_cnt.p, SPLIT_CAND_CAP, band, nq_tile, c.top, vp, tile0,
                                    tile_ovf, (uint32_t *)(plan + pl.ovf_q) + tile0, (SplitStats *)plan));
        c.launches += 6;
    }
    // 5. exact scores of the survivors (pq_pair_kernel: score_point_sse's order), sorted; 6. the exact scan of the queries whose lists overflowed
    QMX_TRY(verify_and_sort(c, vp, q->nq));
    QMX_TRY(pq_overflow_pass(c, pl));
    c.launches += 5;
    q->last_split = true;
    q->last_pq = true;
    // the rotated copy once per four-query group (all but the first find it in L2) + the sample's rows per query
    close_counters(c, (uint64_t)q->nq * c.n_cand, (uint64_t)((q->nq + 3) / 4) * c.n_cand * m_pad + (uint64_t)q->nq * S * s->row_bytes, c.launches, q->nq);
    return QMX_OK;
}

// ---- 4-bit TurboQuant / scalar-int8 top-k of 33 and more queries over a large block: 128 queries per pass of the codes (scan_tq4w.hip, scan_sqw.hip).  The pass's scores are exact;
// what it shares with the prefilters is the plumbing: a sample's k-th best score admits the candidates, per-wave lists are regrouped per query, the k best
// keys of a query (band 0: every tie of the k-th score with them) are re-scored by the pair kernel and sorted; a query whose lists overflowed (masses of
// equal scores, a sample that is all deleted) takes the 32-query scan - conditional launches that read their flag and return. ----
static int32_t wide_exact_search(SearchCall &c) {
    qmx_query *q = c.q;
    const qmx_segment *s = q->seg;
    const bool sq = s->dtype == QMX_DTYPE_SQ_U8;
    // TurboQuant, option tq_wide_high_digit: the pass multiplies the queries' HIGH digits only; its scores are within band[q] of the exact ones, the selection
    // keeps what an exact score >= T could hide behind (approximate >= max(T - band, A_k - 2 band)) and the pair kernel re-scores that
    const bool tq_high = !sq && option(OPT_TQ_WIDE_HIGH_DIGIT) != 0;
    const SplitPlanLayout pl(q->nq, TQW_FQT);
    QMX_TRY(q->gthr.reserve((size_t)std::max<uint32_t>(q->nq_padded, SPLIT_QT) * sizeof(uint64_t)));
    QMX_TRY(q->sp_bq.reserve(sq ? sqw_query_bytes(s->scan_dim) : tq4w_query_bytes(s->scan_dim)));
    QMX_TRY(q->sp_f32.reserve(SplitF32::floats_wide * sizeof(float)));
    QMX_TRY(q->sp_cand.reserve((size_t)SPLIT_QT * SPLIT_CAND_CAP * sizeof(uint64_t)));
    QMX_TRY(q->sp_cnt.reserve((size_t)SPLIT_QT_MAX * 4));
    QMX_TRY(q->sp_wl.reserve(sq ? sqw_wlists_bytes(s->num_cus) : tq4w_wlists_bytes(s->num_cus)));
    QMX_TRY(q->sp_fq.reserve((size_t)pl.list_cap * q->q_stride));
    QMX_TRY(q->partial.reserve((size_t)s->num_cus * 8 * TQW_FQT * std::min<uint32_t>(c.top, MAX_TOP_FAST) * sizeof(uint64_t)));
    // the sample: every 128-th row (prescan_shift - 3; at least 8 192 rows): its k-th best score leaves ~128 k candidates per query to the pass - the pass's
    // epilogue pays per candidate (10 M x 768, 128 queries: 2.07 / 2.00 / 2.01 ms with every 256-th / 128-th / 64-th row, whose own scores cost more).
    // SQ: every 256-th (its epilogue is one integer add and compare per pair; the sample's scores and their selection are 0.19 ms of the search at 1 / 128)
    VerifyPool vp;
    uint64_t S = 0;
    QMX_TRY(prefilter_begin(q, pl, c.n_cand, sq ? -2 : -3, &vp, &S));
    unsigned char *plan = (unsigned char *)q->sp_plan.p;
    const SplitF32 f(q->sp_f32.p);      // band: zero - the pass's scores are the exact ones - or infinite: a query without a usable bound
    uint32_t n_tiles = 0;
    c.launches = 2;     // (this route counts its verification's two launches up front, and not the plan of the conditional passes)
    for (uint32_t tile0 = 0; tile0 < q->nq; tile0 += SPLIT_QT, ++n_tiles) {
        const uint32_t nq_tile = std::min<uint32_t>(SPLIT_QT, q->nq - tile0);
        QMX_CHECK_CANCELLED(c.is_stopped);
        const uint64_t *gthr = (const uint64_t *)q->gthr.p + tile0;
        const ScanArgs a = tile_args(c, tile0, nq_tile);
        // 1. exact scores of the sample -> the k-th best of each query = a lower bound of its final k-th best
        QMX_TRY(bound_enqueue(c, tile0, nq_tile, (const uint32_t *)q->sp_sample.p, S, c.top, a.del, &c.launches, true));
        // 2. the queries' codes / digits as operand images, the integer reject bounds
        if (sq) QMX_TRY(launch_sqw_pack(q->stream, a, gthr, s->sq_off_absmax, q->sp_bq.p, f.wide_thr, f.wide_qinfo, f.band, (uint32_t *)q->sp_cnt.p, SPLIT_QT_MAX));
        else QMX_TRY(launch_tq4w_pack(q->stream, a, gthr, s->tq_sf_min, s->tq_sf_max, s->tq_l2_min, s->tq_l2_max, s->tq_c1, tq_high ? 1 : 0, q->sp_bq.p, f.wide_thr,
                                      f.wide_qinfo, f.band, (uint32_t *)q->sp_cnt.p, SPLIT_QT_MAX));
        // 3. the pass
        uint32_t grid = 0;
        if (sq) QMX_TIMED_SCAN(c, launch_scan_sqw(q->stream, a, q->sp_bq.p, f.wide_thr, s->d_sq_bi, f.wide_qinfo, s->num_cus, q->sp_wl.p, &grid));
        else QMX_TIMED_SCAN(c, launch_scan_tq4w(q->stream, a, q->sp_bq.p, f.wide_thr, f.wide_qinfo, tq_high ? f.band : nullptr, s->num_cus, q->sp_wl.p, &grid));
        // 4. per-wave lists -> per-query lists (deleted rows dropped), then the k best keys of each query
        int *tile_ovf = (int *)(plan + pl.tile_ovf) + n_tiles;
        QMX_TRY(launch_regroup_lists(q->stream, a.del, (const unsigned char *)q->sp_wl.p + (sq ? sqw_wlists_counts_bytes(s->num_cus) : tq4w_wlists_counts_bytes(s->num_cus)),
                                     (const uint32_t *)q->sp_wl.p, sq ? sqw_wcap() : tq4w_wcap(), grid * 8, (uint64_t *)q->sp_cand.p, (uint32_t *)q->sp_cnt.p,
                                     SPLIT_CAND_CAP, tile_ovf));
        QMX_TRY(launch_split_select(q->stream, (const uint64_t *)q->sp_cand.p, (const uint32_t *)q->sp_cnt.p, SPLIT_CAND_CAP, f.band, nq_tile, c.top, vp, tile0, tile_ovf,
                                    (uint32_t *)(plan + pl.ovf_q) + tile0, (SplitStats *)plan, tq_high ? f.wide_high : nullptr, tq_high));
        c.launches += 6;
    }
    // 5. the selected rows through the pair kernel (the same bits), sorted; 6. the 32-query scan of the queries whose lists overflowed
    QMX_TRY(verify_and_sort(c, vp, q->nq));
    QMX_TRY(overflow_passes(c, pl, q->nq, TQW_FQT, sq ? overflow_scan_sq : overflow_scan_tq, &c.launches));
    q->last_split = true;
    q->last_pq = false;
    q->last_fqt = TQW_FQT;
    close_counters(c, (uint64_t)q->nq * c.n_cand,
                   (uint64_t)n_tiles * c.n_cand * s->row_bytes + (uint64_t)((q->nq + MAX_QT_MFMA - 1) / MAX_QT_MFMA) * S * s->row_bytes, c.launches, q->nq);
    return QMX_OK;
}

// ---- the f32 prefilters (scan_split.hip, scan_i8copy.hip, split_select.hip): tiles of 128 / 256 queries; their verification and, if ever needed, the exact passes run once for all of them
// after the tile loop ----
struct SplitTiles {
    SplitPlanLayout pl;
    VerifyPool vp{};
    uint64_t S = 0;                                         // rows of the sample
    bool i8_sample = false;                                 // the int8 route with option i8_sample_scan: the sample is tiles of the copy, scored there
    bool ovf_groups = false;                                // the int8 route with option fallback_beside_scan, where it fits: overflow_groups_pass
    std::vector<std::pair<uint32_t, uint32_t>> tiles;       // (tile0, nq_tile) of the tiles that took the prefilter
    SplitTiles(uint32_t nq, uint32_t fqt) : pl(nq, fqt) {}
};

// |approximate - exact| <= band * |q| * max |row|, worst case, every term at its bound:
//   one product of f16-rounded operands (HALF copy): each operand within 2^-11 of its value -> (2^-10 + 2^-22) sum |q_i r_i| <= ... |q| |r|
//   three products of f16 pairs: x - (h + l) within 2^-22 |x|, the dropped l.l term 2^-22                    -> 3 * 2^-22
//   f32 accumulation of the matrix cores over dim terms: dim * 2^-23 * sum |terms| (a round-off of 2^-23 per addition covers
//   truncating adders as well), f16 subnormal flush of tiny elements: < 2^-27 sqrt(dim)
// both rounded up generously; the exact side carries no error (the survivors are re-scored by the reference-order kernel).
// Those terms are RELATIVE to the operands, and hold while an operand's f16 parts are normal numbers.  The scales are one power of two per block and one
// per batch (of its largest |q|; both exponents clamped at +-100), so what they leave a member far below the largest is an ABSOLUTE resolution: f16
// subnormals are 2^-24 apart, an element x s of any size is h + l to within 2^-25 - in accumulator units of its side, whatever the element's own size.
// Summed against the other side (Cauchy-Schwarz) and brought back to score units:
//     sqrt(dim) * 2^-24 * (max |row| / query scale + |q| / row scale)          (split_abs_band; twice the worst case)
// For the batch's largest query over an unclamped block that is below 2^-36 sqrt(dim) of |q| max |row| - nothing beside the relative terms; for a query
// 2^-20 of the batch's largest it is the band; for one 2^-40 of it, or a zero query, it exceeds |q| max |row|, the range of the scores themselves.  Such
// a band selects nothing, and only costs lists that overflow (a wave's list is shared by its 64 queries: the whole tile would follow), so
// sp_thresholds_kernel makes it infinite: the query collects no candidates and takes the exact scan alone, as a query without a sample bound does.  The
// alternative - every query below a fixed fraction of the batch's largest to the exact scan - needs no term, but says nothing about a block whose own
// scale is clamped (2^-110: the rows reach f16 at 2^-8 and below) and gives up queries this band still serves.
// The matrix cores of gfx950 read f16 subnormal operands as they are (measured: 32 products of 2^-24 and 2^10 accumulate to 2^-9); were they flushed, the
// resolution would be 2^-14, and this term too small by 2^10 (tests/test_split_band_model.py runs both and pins where they part).
static inline float split_rel_band(bool half, uint32_t dim) {
    const float acc = (float)dim * 1.1920929e-7f;                      // dim * 2^-23
    return (half ? 9.765625e-4f + 9.5367432e-7f : 1.9073486e-6f) + acc;  // 2^-10 + 2^-20 | 2^-19
}
static inline float split_abs_band(uint32_t dim) { return 5.9604645e-8f * sqrtf((float)dim); }      // 2^-24 sqrt(dim), accumulator units of one side

static int32_t split_begin(const SearchCall &c, const SearchPlan &plan, SplitTiles &sp) {
    qmx_query *q = c.q;
    const qmx_segment *s = q->seg;
    QMX_TRY(q->sp_bq.reserve(split_query_bytes(s->dim)));
    QMX_TRY(q->sp_f32.reserve(SplitF32::floats * sizeof(float)));
    QMX_TRY(q->sp_cand.reserve((size_t)plan.split_qt * SPLIT_CAND_CAP * sizeof(uint64_t)));
    QMX_TRY(q->sp_cnt.reserve((size_t)SPLIT_QT_MAX * 4));
    if (s->d_rows_split) QMX_TRY(q->sp_wl.reserve(split_wlists_bytes(s->num_cus)));
    QMX_TRY(q->sp_fq.reserve((size_t)sp.pl.list_cap * q->q_stride));
    if (s->split_i8) {
        QMX_TRY(q->sp_probe.reserve((size_t)q->nq * (split_i8_probe() + 1) * 4));
        QMX_TRY(q->sp_pscores.reserve((size_t)q->nq * split_i8_probe() * 4));
        // (no memset of the probe counts: the gather of a tile reads the counts of the tiles up to it - its own, written by the probe kernel in front
        // of it, and the earlier ones', emptied by their bound kernels)
    }
    // the sample: every (n_cand / S)-th row, S = n_cand / 256 (at least 8192): its k-th best leaves ~256 k candidates per query to the
    // main pass, at 1 / 256 of the pass's row traffic for the sample's exact scores (measured on C2: 1/128 .. 1/512 are equally good)
    // ("prescan_shift" - 2: the option of the exact scans' prefix pre-scan, 10 by default, moves this sample with it)
    // (with the derived copy: one more halving - 8 192 rows of a 10 M block are one tile per row stream of the sample scan, and the
    // refine step after the first sixteenth of the block owns the threshold anyway: 26 us of the step, measured)
    // (a 2 048-row sample lets the four query tiles of a 128-query batch run side by side - 22 us instead of 63 for the pre-scan - but its weaker threshold
    // triples the candidates of the first launch: regroup, refine and select together give the 40 us back, measured; 8 192 stays)
    // (the int8 copy, option i8_sample_scan: the same number of rows as whole 16-row tiles of the copy, scored by the int8 matrix instruction - i8_copy_scan)
    sp.i8_sample = s->split_i8 && option(OPT_I8_SAMPLE_SCAN) > 0;
    return prefilter_begin(q, sp.pl, c.n_cand, s->d_rows_split ? 1 : -2, &sp.vp, &sp.S, sp.i8_sample);
}

// steps 2 - 4 of a tile over the f32 rows or an f16 copy
static int32_t f16_split_scan(SearchCall &c, SplitTiles &sp, const ScanArgs &a, uint32_t tile0, uint32_t nq_tile, int *tile_ovf) {
    qmx_query *q = c.q;
    const qmx_segment *s = q->seg;
    unsigned char *plan = (unsigned char *)q->sp_plan.p;
    const SplitF32 f(q->sp_f32.p);
    // 2. the batch's queries split into f16 pairs; thresholds and bands in accumulator / score units
    const float row_scale = split_row_scale(s->row_maxabs);
    const int half = s->split_half ? 1 : 0;
    const uint32_t tqt = nq_tile > SPLIT_QT ? SPLIT_QT_MAX : SPLIT_QT;      // the shape of THIS tile (a remainder of <= 128 queries takes the 128 shape)
    QMX_TRY(launch_split_pack_queries(q->stream, (const float *)q->enc.p + (size_t)tile0 * s->dim, nq_tile, s->dim, f.qmax, f.qnorm, q->sp_bq.p, half, tqt));
    QMX_TRY(launch_split_thresholds(q->stream, (const uint64_t *)q->gthr.p + tile0, f.qnorm, f.qmax, nq_tile, split_rel_band(half, s->dim), split_abs_band(s->dim),
                                    s->row_norm_max, row_scale, f.scales, f.thr, f.band, tqt, (uint32_t *)q->sp_cnt.p, SPLIT_QT_MAX));
    QMX_TRY(split_stage(q, "pack + thresholds"));
    // 3. the approximate scan of the whole block
    // over a derived copy in two launches: the strided sixteenth of the tiles first, whose k-th best approximate score tightens the
    // threshold of the other fifteen (sp_refine_kernel): ~16 k candidates per query instead of ~10 k x 16 from the sample's threshold alone
    for (uint32_t phase = s->d_rows_split ? 1 : 0; phase <= (s->d_rows_split ? 2u : 0u); ++phase) {
        QMX_TIMED_SCAN(c, launch_scan_f32_split(q->stream, a, q->sp_bq.p, row_scale, f.scales, f.thr, (uint64_t *)q->sp_cand.p, (uint32_t *)q->sp_cnt.p, SPLIT_CAND_CAP,
                                                s->num_cus, s->d_rows_split, half, q->sp_wl.p, phase, tqt));
        if (s->d_rows_split)
            QMX_TRY(launch_split_regroup(q->stream, a, q->sp_wl.p, s->num_cus, (uint64_t *)q->sp_cand.p, (uint32_t *)q->sp_cnt.p, SPLIT_CAND_CAP, tile_ovf, phase, tqt));
        if (phase == 1)
            QMX_TRY(launch_split_refine(q->stream, (const uint64_t *)q->sp_cand.p, (const uint32_t *)q->sp_cnt.p, SPLIT_CAND_CAP, f.band, nq_tile, c.top, f.scales, f.thr));
    }
    QMX_TRY(split_stage(q, "split kernel"));
    // 4. the rows worth an exact score
    QMX_TRY(launch_split_select(q->stream, (const uint64_t *)q->sp_cand.p, (const uint32_t *)q->sp_cnt.p, SPLIT_CAND_CAP, f.band, nq_tile, c.top, sp.vp, tile0, tile_ovf,
                                (uint32_t *)(plan + sp.pl.ovf_q) + tile0, (SplitStats *)plan));
    c.launches += 8;
    return QMX_OK;
}

// steps 2' - 4' of a tile over the int8 copy (option i8_sample_scan: step 1 as well)
static int32_t i8_copy_scan(SearchCall &c, SplitTiles &sp, const ScanArgs &a, uint32_t tile0, uint32_t nq_tile, int *tile_ovf) {
    qmx_query *q = c.q;
    const qmx_segment *s = q->seg;
    unsigned char *plan = (unsigned char *)q->sp_plan.p;
    const SplitF32 f(q->sp_f32.p);
    // 2'. the int8 copy: codes, scales, worst-case bands, thresholds from the sample's exact k-th best - or, with the sample scored on the copy, no
    // threshold yet (+inf: nothing is admitted; the band of a finite query is finite)
    QMX_TRY(launch_split_i8_pack(q->stream, (const float *)q->enc.p + (size_t)tile0 * s->dim, nq_tile, s->dim, s->d_i8_scale,
                                 sp.i8_sample ? nullptr : (const uint64_t *)q->gthr.p + tile0, s->d_i8_stats, s->row_norm_max, q->sp_bq.p, f.i8_qscale, f.band, f.thr,
                                 f.i8_texact, (uint32_t *)q->sp_cnt.p, SPLIT_QT_MAX));
    QMX_TRY(split_stage(q, "int8 pack"));
    const uint32_t np = split_i8_probe();
    uint32_t *probe_ids = (uint32_t *)q->sp_probe.p, *probe_cnt = probe_ids + (size_t)q->nq * np;
    if (sp.i8_sample) {
        // 1'. "launch 0": the approximate scores of the sample's tiles, the k best live ones of each query (the top-k sees the deleted rows and the
        // requests' filters), their exact scores by the pair kernel - any k distinct live rows bound the final k-th best from below -> thr, T_exact, gthr.
        // What follows a scan launch below, with the top-k in the place of regroup and probe.
        QMX_TRY(q->scores.reserve((size_t)nq_tile * sp.S * sizeof(float)));
        QMX_TRY(launch_scan_i8copy_sample(q->stream, s->d_rows_split, q->sp_bq.p, s->dim, (const uint32_t *)q->sp_sample.p, (uint32_t)(sp.S / 16), nq_tile, f.i8_qscale,
                                          (float *)q->scores.p));
        QMX_TRY(launch_custom_topk(q->stream, (const float *)q->scores.p, sp.S, (const uint32_t *)q->sp_sample.p, a.del, nq_tile, c.top, c.d_out + (size_t)tile0 * c.top,
                                   c.d_counts + tile0, nullptr, true));
        QMX_TRY(launch_split_i8_picks(q->stream, c.d_out + (size_t)tile0 * c.top, c.d_counts + tile0, nq_tile, c.top, f.band, probe_ids + (size_t)tile0 * np,
                                      probe_cnt + tile0));
        const void *scan_kernel = q->last_kernel;
        PairSel psel{nullptr, np, probe_cnt};
        QMX_TRY(score_pairs_device(q, psel, probe_ids, (uint64_t)(tile0 + nq_tile) * np, (float *)q->sp_pscores.p, false));
        q->last_kernel = scan_kernel;
        QMX_TRY(launch_split_i8_sample_bound(q->stream, (const float *)q->sp_pscores.p + (size_t)tile0 * np, probe_ids + (size_t)tile0 * np, probe_cnt + tile0, nq_tile,
                                             c.top, f.band, f.i8_qscale, f.thr, f.i8_texact, (uint64_t *)q->gthr.p + tile0));
        QMX_TRY(split_stage(q, "int8 sample scan"));
        c.launches += 3;      // (five launches in the place of the pre-scan's two)
    }
    // 3'. the strided sixteenth, then the rest; after each launch the exact scores of the k best candidates so far renew the bound
    // (which tiles the first launch takes: every 16th, option i8_sample_stride.  Its candidates are admitted on the SAMPLE's bound - a hundred times
    // those of the main launch per tile.  With the one epilogue for both launches that, not the stream, was what bounded the first launch, and strides
    // of 8 .. 64 measured the same step time (profiles/r5_i8_sample_stride.md); with an epilogue made for dense candidates (option i8_dense_epilogue)
    // 8 / 16 / 32 were measured again: profiles/r14_i8_dense_epilogue.md)
    const int64_t sstride_opt = option(OPT_I8_SAMPLE_STRIDE);
    const uint32_t sstride = sstride_opt >= 2 && sstride_opt <= 255 ? (uint32_t)sstride_opt : 16;
    for (uint32_t ph = 1; ph <= 2; ++ph) {
        const uint32_t phase = ph | (sstride << 8);
        QMX_TIMED_SCAN(c, launch_scan_i8copy(q->stream, a, q->sp_bq.p, f.i8_qscale, f.thr, s->num_cus, s->d_rows_split, q->sp_wl.p, phase));
        QMX_TRY(launch_split_regroup(q->stream, a, q->sp_wl.p, s->num_cus, (uint64_t *)q->sp_cand.p, (uint32_t *)q->sp_cnt.p, SPLIT_CAND_CAP, tile_ovf, phase, SPLIT_QT));
        QMX_TRY(launch_split_i8_probe(q->stream, (const uint64_t *)q->sp_cand.p, (const uint32_t *)q->sp_cnt.p, SPLIT_CAND_CAP, f.band, nq_tile, c.top, tile_ovf,
                                      probe_ids + (size_t)tile0 * np, probe_cnt + tile0));
        const void *scan_kernel = q->last_kernel;
        PairSel psel{nullptr, np, probe_cnt};
        QMX_TRY(score_pairs_device(q, psel, probe_ids, (uint64_t)(tile0 + nq_tile) * np, (float *)q->sp_pscores.p, false));
        q->last_kernel = scan_kernel;
        QMX_TRY(launch_split_i8_bound(q->stream, (const float *)q->sp_pscores.p + (size_t)tile0 * np, probe_cnt + tile0, nq_tile, c.top, f.band, f.i8_qscale, f.thr,
                                      f.i8_texact));
    }
    QMX_TRY(split_stage(q, "int8 scan"));
    // 4'. the rows worth an exact score: approximate score >= T_exact - band
    QMX_TRY(launch_split_select(q->stream, (const uint64_t *)q->sp_cand.p, (const uint32_t *)q->sp_cnt.p, SPLIT_CAND_CAP, f.band, nq_tile, c.top, sp.vp, tile0, tile_ovf,
                                (uint32_t *)(plan + sp.pl.ovf_q) + tile0, (SplitStats *)plan, f.i8_texact));
    c.launches += 13;
    return QMX_OK;
}

static int32_t split_tile(SearchCall &c, const SearchPlan &plan, SplitTiles &sp, uint32_t tile0, uint32_t nq_tile) {
    qmx_query *q = c.q;
    QMX_CHECK_CANCELLED(c.is_stopped);
    const ScanArgs a = tile_args(c, tile0, nq_tile);
    // 1. exact scores of the sample -> the k-th best of each query = a lower bound of its final k-th best (launches: counted in the tile's 8 / 13)
    // (the int8 copy with option i8_sample_scan takes that bound from the copy itself, behind its pack: i8_copy_scan)
    if (!sp.i8_sample) QMX_TRY(bound_enqueue(c, tile0, nq_tile, (const uint32_t *)q->sp_sample.p, sp.S, c.top, a.del, nullptr, true));
    QMX_TRY(split_stage(q, "prescan"));
    int *tile_ovf = (int *)((unsigned char *)q->sp_plan.p + sp.pl.tile_ovf) + sp.tiles.size();
    if (plan.route == ROUTE_I8_COPY) QMX_TRY(i8_copy_scan(c, sp, a, tile0, nq_tile, tile_ovf));
    else QMX_TRY(f16_split_scan(c, sp, a, tile0, nq_tile, tile_ovf));
    QMX_TRY(split_stage(q, "select"));
    sp.tiles.push_back({tile0, nq_tile});
    return QMX_OK;
}

// 5. and 6. for the tiles that took the prefilter
static int32_t split_finish(const SearchCall &c, const SearchPlan &plan, const SplitTiles &sp) {
    qmx_query *q = c.q;
    const uint32_t first = sp.tiles.front().first, last = sp.tiles.back().first + sp.tiles.back().second;
    // (split tiles are a prefix of the batch - the remainder tile, if any, comes last -: the sort walks queries 0 .. last)
    QMX_REQUIRE(first == 0, QMX_ERR_OTHER, "split tiles must start at query 0");
    QMX_TRY(verify_and_sort(c, sp.vp, last));
    // (not counted: the tile's 8 / 13 are this route's launches)
    if (sp.ovf_groups) QMX_TRY(overflow_groups_pass(c, sp.pl, last));
    else QMX_TRY(overflow_passes(c, sp.pl, last, plan.split_fqt, overflow_scan_f32, nullptr));
    q->last_split = true;
    q->last_pq = false;
    q->last_fqt = sp.ovf_groups ? 16 : plan.split_fqt;      // (fold_split_counters: f overflowed queries stream the block ceil(f / 16) times in the one-launch form)
    return QMX_OK;
}

// ---- a tile of the exact scans: its pre-scan, then one pass per MAX_TOP_FAST entries of the lists ----
static int32_t exact_tile(SearchCall &c, const SearchPlan &plan, uint32_t tile0, uint32_t nq_tile) {
    qmx_query *q = c.q;
    const qmx_segment *s = q->seg;
    const int qt = (int)pow2_ceil(nq_tile);
    for (uint32_t pass = 0; pass < plan.n_pass; ++pass) {
        QMX_CHECK_CANCELLED(c.is_stopped);
        const uint32_t off = pass * MAX_TOP_FAST;
        const uint32_t ptop = std::min<uint32_t>(MAX_TOP_FAST, c.top - off);
        ScanArgs a = tile_args(c, tile0, nq_tile);
        a.ids = c.d_ids;
        a.top = ptop;
        a.partial = (uint64_t *)q->partial.p;
        a.partial_qt = (uint32_t)qt;
        a.key_bound = pass ? (const uint64_t *)q->bounds.p : nullptr;
        // The chain-major scan (scan_mfma16.hip) keeps one top list per wave and query: 512 lists per query on the chip, each of
        // which would learn its reject threshold from its own 1 / 512 of the rows (~k ln(n / 512 k) insertions per list, each
        // a wave-serial event the other waves of the block wait for at the next barrier).  A pre-scan of the first 1 / 1024 of the
        // block gives every list the k-th best score of that prefix as a starting threshold: a lower bound of the final k-th
        // best score, so nothing that belongs to the result is rejected (ties pass), and only ~1024 k rows per query beat it.
        // (Running the pre-scan as a top-k pass of the chain-major kernel itself was insertion-bound: 0.2 ms instead of 0.06.)
        const bool m16 = s->dtype == QMX_DTYPE_F32 && mfma_scan_ok(s) && mfma16_scan_ok(qt, SCAN_TOPK, a);
        const bool sqm = (s->dtype == QMX_DTYPE_SQ_U8 || s->dtype == QMX_DTYPE_TQ ? qt >= 4 : s->dtype == QMX_DTYPE_F16 && qt >= 8) && mfma_scan_ok(s);   // scan_sq_mfma.hip starts from the bound too
        const bool m4 = s->dtype == QMX_DTYPE_F32 && qt >= 8 && mfma_scan_ok(s);                                        // scan_mfma.hip (4x4x1) as well
        const bool bqk = s->dtype == QMX_DTYPE_BQ && qt >= 4;   // bq_rows_kernel: integer scores, selection-bound without a starting threshold
        if (pass == 0 && c.n_cand >= (1u << 18) && (m16 || sqm || m4 || bqk) && !option(OPT_NO_PRESCAN)) {
            const int pre_shift = (int)std::min<int64_t>(std::max<int64_t>(option(OPT_PRESCAN_SHIFT), 1), 20);  // tuning: measured 5..10 on C2, the main pass does not care, the pre-scan itself gets cheaper
            const uint64_t pre_n = std::max<uint64_t>(c.n_cand >> pre_shift, 1u << 13) & ~(uint64_t)15;
            QMX_TRY(bound_enqueue(c, tile0, nq_tile, c.d_ids, pre_n, ptop, a.del, nullptr, false));
            a.gthr = (const uint64_t *)q->gthr.p + tile0;
            c.launches += 2;
        }
        uint32_t grid = (uint32_t)s->num_cus * 8;      // partial lists: one per block; bound the grid by what the buffer holds
        QMX_TIMED_SCAN(c, launch_scan(q, qt, SCAN_TOPK, a, &grid));
        QMX_TRY(launch_merge_keys(q->stream, (const uint64_t *)q->partial.p, grid, (uint32_t)qt, nq_tile, ptop, c.d_out + (size_t)tile0 * c.top, c.d_counts + tile0, c.top,
                                  off, plan.n_pass > 1 ? (uint64_t *)q->bounds.p : nullptr));
        c.launches += 2;
    }
    return QMX_OK;
}

int32_t search_enqueue(qmx_query *q, uint32_t top, const uint32_t *d_ids, uint64_t n_ids,
                              qmx_scored_point *d_out, uint32_t *d_counts, const volatile uint8_t *is_stopped,
                              qmx_counters *counters, bool timed) {
    const qmx_segment *s = q->seg;
    if (is_sparse(s)) QMX_REFUSE_FILTERS(q);
    if (is_sparse(s)) return sparse_search_enqueue(q, top, d_ids, n_ids, d_out, d_counts, is_stopped, counters, timed);
    SearchCall c{q, top, d_ids, d_ids ? n_ids : s->scan_rows(), d_out, d_counts, is_stopped, counters, timed, 0};
    const SearchPlan plan = search_plan(q, top, d_ids, c.n_cand);
    q->last_counters = qmx_counters{};
    q->last_split = false;
    if (plan.route == ROUTE_TQ_L1) return tq_l1_search(c, plan);
    if (plan.route == ROUTE_PQ_PREFILTER) return pq_prefilter_search(c);
    if (plan.route == ROUTE_TQ_WIDE || plan.route == ROUTE_SQ_WIDE) return wide_exact_search(c);
    // tiles of plan.tile_q queries: the split tiles first, then - a remainder without a copy, or the whole batch - the exact ones
    const uint32_t TQ = plan.tile_q;
    QMX_TRY(q->partial.reserve((size_t)s->num_cus * 8 * std::min<uint32_t>(TQ, MAX_QT_TOPK) * std::min<uint32_t>(top, MAX_TOP_FAST) * sizeof(uint64_t)));
    if (plan.n_pass > 1) QMX_TRY(q->bounds.reserve((size_t)TQ * sizeof(uint64_t)));
    QMX_TRY(q->gthr.reserve((size_t)std::max<uint32_t>(q->nq_padded, SPLIT_QT_MAX) * sizeof(uint64_t)));
    SplitTiles sp(q->nq, plan.split_fqt);
    if (plan.route == ROUTE_I8_COPY) {
        QMX_TRY(fallback_groups_fit(q, top, &sp.ovf_groups));
        if (sp.ovf_groups) QMX_TRY(q->partial.reserve(overflow_groups_partial_bytes(q, top)));      // (before the first launch that uses the buffer)
    }
    if (plan.split()) QMX_TRY(split_begin(c, plan, sp));
    for (uint32_t tile0 = 0; tile0 < q->nq; tile0 += TQ) {
        const uint32_t nq_tile = std::min<uint32_t>(TQ, q->nq - tile0);
        if (plan.tile_splits(nq_tile)) QMX_TRY(split_tile(c, plan, sp, tile0, nq_tile));
        else QMX_TRY(exact_tile(c, plan, tile0, nq_tile));
    }
    if (!sp.tiles.empty()) QMX_TRY(split_finish(c, plan, sp));
    uint32_t split_q = 0;
    uint64_t bytes = 0;
    for (auto &t : sp.tiles) {
        split_q += t.second;
        // one pass over the derived copy (2 or 4 bytes per element; the f32 rows themselves when there is none) + the sample's exact scores
        bytes += c.n_cand * (uint64_t)s->dim * (s->split_i8 ? 1 : s->d_rows_split && s->split_half ? 2 : 4);
        // (the int8 route's sample of tiles: one byte per element, once per query group of the sample kernel; its exact rows are k per query)
        if (sp.i8_sample) {
            const uint32_t group = split_i8_sample_queries(s->dim, t.second);
            bytes += (uint64_t)((t.second + group - 1) / group) * q->sp_sample_n * s->dim + (uint64_t)t.second * std::min<uint32_t>(top, MAX_TOP_FAST) * s->row_bytes;
        } else
            bytes += (uint64_t)((t.second + tile_qt(s, q) - 1) / tile_qt(s, q)) * q->sp_sample_n * s->row_bytes;
    }
    bytes += (uint64_t)((q->nq - split_q + TQ - 1) / TQ) * c.n_cand * s->row_bytes * plan.n_pass;
    // (kernel_launches: this driver adds its launches to what the caller's counters held, and an enqueue without counters - the async call - records 0)
    close_counters(c, (uint64_t)q->nq * c.n_cand * plan.n_pass, bytes, counters ? counters->kernel_launches + c.launches : 0, split_q);
    return QMX_OK;
}

// after the stream is synchronised: the device's share of the last search's counters (prefilter candidates, exactly re-scored rows, the queries
// that took the exact scan) -> c, bytes_read completed with the rows those steps read
int32_t fold_split_counters(qmx_query *q, qmx_counters *c) {
    if (!q->last_split || !q->sp_plan.p) return QMX_OK;
    SplitStats st;
    QMX_HIP(hipMemcpy(&st, q->sp_plan.p, sizeof(st), hipMemcpyDeviceToHost));
    c->prefilter_candidates = st.candidates;
    c->verified_rows = st.verified;
    c->fallback_queries = st.fallback_queries;
    c->bytes_read += st.verified * q->last_row_bytes;
    if (st.fallback_queries) {
        const uint32_t f = st.fallback_queries;
        const uint64_t passes = q->last_pq ? f : f <= 16 ? 1 : (f + q->last_fqt - 1) / q->last_fqt;     // (the exact PQ kernel streams the codes once per query)
        c->bytes_read += passes * q->last_n_cand * q->last_row_bytes;
    }
    return QMX_OK;
}

// an empty result: zero the counts, wherever they live
static int32_t zero_counts(qmx_query *q, uint32_t *out_counts) {
    if (is_device_ptr(out_counts)) {
        QMX_HIP(hipMemsetAsync(out_counts, 0, (size_t)q->nq * 4, q->stream));
        QMX_HIP(hipStreamSynchronize(q->stream));
    } else {
        for (uint32_t i = 0; i < q->nq; ++i) out_counts[i] = 0;
    }
    return QMX_OK;
}

// the lists and counts of a call whose `out` / `out_counts` may be host memory: written on the device - in place, or in the batch's own out / counts
// buffers -, end() enqueues the copies back to what is on the host
struct StagedLists {
    qmx_query *q;
    qmx_scored_point *out, *d_out;
    uint32_t *out_counts, *d_counts;
    size_t out_bytes;
    int32_t begin(qmx_query *q_, uint32_t top, qmx_scored_point *out_, uint32_t *out_counts_) {
        *this = StagedLists{q_, out_, out_, out_counts_, out_counts_, (size_t)q_->nq * top * sizeof(qmx_scored_point)};
        if (!is_device_ptr(out)) {
            QMX_TRY(q->out.reserve(out_bytes));
            d_out = (qmx_scored_point *)q->out.p;
        }
        if (!is_device_ptr(out_counts)) {
            QMX_TRY(q->counts.reserve((size_t)q->nq * sizeof(uint32_t)));
            d_counts = (uint32_t *)q->counts.p;
        }
        return QMX_OK;
    }
    int32_t end() {
        if (d_out != out) QMX_TRY(copy_out(q->stream, out, d_out, out_bytes));
        if (d_counts != out_counts) QMX_TRY(copy_out(q->stream, out_counts, d_counts, (size_t)q->nq * sizeof(uint32_t)));
        return QMX_OK;
    }
};

int32_t qmx_search_topk(qmx_query *q, uint32_t top, const uint32_t *ids, uint64_t n_ids, qmx_scored_point *out,
                        uint32_t *out_counts, const volatile uint8_t *is_stopped, qmx_counters *counters) {
    QMX_REQUIRE(q && out && out_counts, QMX_ERR_BAD_ARG, "NULL argument");
    if (top == 0 && is_sparse(q)) {     // the sparse search returns an empty list for top 0 (TopK, lib/common/common/src/top_k.rs)
        if (counters) memset(counters, 0, sizeof(*counters));
        QMX_HIP(hipSetDevice(q->device));
        return zero_counts(q, out_counts);
    }
    QMX_REQUIRE(top >= 1, QMX_ERR_BAD_ARG, "top must be > 0 (FixedLengthPriorityQueue::new panics on 0)");
    QMX_REQUIRE(top <= MAX_TOP, QMX_ERR_NOT_SUPPORTED, "top %u > %u not supported yet", top, MAX_TOP);
    QMX_HIP(hipSetDevice(q->seg->device));
    if (counters) memset(counters, 0, sizeof(*counters));
    if (q->nq == 0) return QMX_OK;
    const void *d_ids = nullptr;
    if (ids) {
        if (n_ids == 0) return zero_counts(q, out_counts);  // empty candidate list: every queue stays empty
        QMX_TRY(stage_in(q, q->ids, ids, (size_t)n_ids * 4, &d_ids));
    }
    StagedLists st;
    QMX_TRY(st.begin(q, top, out, out_counts));
    const bool timed = q->timing || (q->seg->flags & QMX_SEG_TIME_KERNELS) != 0;
    QMX_TRY(search_enqueue(q, top, (const uint32_t *)d_ids, n_ids, st.d_out, st.d_counts, is_stopped, counters, timed));
    QMX_TRY(st.end());
    QMX_TRY(check_err_flag(q));  // synchronises the stream
    if (counters) QMX_TRY(fold_split_counters(q, counters));
    if (timed) {
        const float before = q->timing_ms;
        QMX_TRY(timing_fold(q));
        if (counters) counters->kernel_ms = q->timing_ms - before;
    }
    return QMX_OK;
}

int32_t qmx_query_last_counters(qmx_query *q, qmx_counters *out) {
    QMX_REQUIRE(q && out, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_HIP(hipSetDevice(q->device));
    QMX_HIP(hipStreamSynchronize(q->stream));
    *out = q->last_counters;
    return fold_split_counters(q, out);
}

int32_t qmx_search_topk_async(qmx_query *q, uint32_t top, const uint32_t *ids, uint64_t n_ids,
                              qmx_scored_point *out_dev, uint32_t *out_counts_dev) {
    QMX_REQUIRE(q && out_dev && out_counts_dev, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(top >= 1 && top <= MAX_TOP, QMX_ERR_NOT_SUPPORTED, "top %u not in 1..%u", top, MAX_TOP);
    QMX_REQUIRE(!ids || is_device_ptr(ids), QMX_ERR_BAD_ARG, "async search needs device ids");
    QMX_HIP(hipSetDevice(q->seg->device));
    if (q->nq == 0) return QMX_OK;
    const bool timed = q->timing || (q->seg->flags & QMX_SEG_TIME_KERNELS) != 0;
    return search_enqueue(q, top, ids, n_ids, out_dev, out_counts_dev, nullptr, nullptr, timed);
}

int32_t qmx_merge_topk(int32_t device_id, const qmx_scored_point *lists, const uint32_t *list_counts, uint32_t n_lists,
                       uint32_t nq, uint32_t k, qmx_scored_point *out, uint32_t *out_counts) {
    QMX_REQUIRE(lists && out && out_counts, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(k >= 1 && k <= MAX_TOP, QMX_ERR_NOT_SUPPORTED, "k %u not in 1..%u", k, MAX_TOP);
    QMX_TRY(check_device(device_id, nullptr));
    if (nq == 0) return QMX_OK;
    const size_t lbytes = (size_t)n_lists * nq * k * sizeof(qmx_scored_point);
    const size_t cbytes = (size_t)n_lists * nq * sizeof(uint32_t);
    const size_t obytes = (size_t)nq * k * sizeof(qmx_scored_point);
    Staging st;
    const qmx_scored_point *d_lists = nullptr;
    const uint32_t *d_lc = nullptr;
    qmx_scored_point *d_out = nullptr;
    uint32_t *d_oc = nullptr;
    QMX_TRY(st.in(lists, lbytes, &d_lists));
    QMX_TRY(st.in(list_counts, cbytes, &d_lc));
    QMX_TRY(st.out(out, obytes, &d_out));
    QMX_TRY(st.out(out_counts, (size_t)nq * 4, &d_oc));
    QMX_TRY(launch_merge_points(nullptr, d_lists, d_lc, nullptr, n_lists, nq, k, d_out, d_oc));
    QMX_TRY(st.back());
    QMX_HIP(hipDeviceSynchronize());
    return QMX_OK;
}

int32_t qmx_merge_topk_async(int32_t device_id, void *hip_stream, const qmx_scored_point *lists_dev,
                             const uint32_t *list_counts_dev, const uint32_t *list_idx_base_dev, uint32_t n_lists,
                             uint32_t nq, uint32_t k, qmx_scored_point *out_dev, uint32_t *out_counts_dev) {
    QMX_REQUIRE(lists_dev && out_dev && out_counts_dev, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(k >= 1 && k <= MAX_TOP, QMX_ERR_NOT_SUPPORTED, "k %u not in 1..%u", k, MAX_TOP);
    QMX_HIP(hipSetDevice(device_id));
    if (nq == 0) return QMX_OK;
    return launch_merge_points((hipStream_t)hip_stream, lists_dev, list_counts_dev, list_idx_base_dev, n_lists, nq, k,
                               out_dev, out_counts_dev);
}


uint64_t qmx_topk_record_bytes(uint32_t nq, uint32_t k) {
    return ((uint64_t)nq * k * sizeof(qmx_scored_point) + (uint64_t)nq * sizeof(uint32_t) + 7) & ~7ull;
}

int32_t qmx_merge_topk_packed_async(int32_t device_id, void *hip_stream, const void *records_dev, const uint32_t *list_idx_base_dev, uint32_t n_lists,
                                    uint32_t nq, uint32_t k, qmx_scored_point *out_dev, uint32_t *out_counts_dev) {
    QMX_REQUIRE(records_dev && out_dev && out_counts_dev, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(k >= 1 && k <= MAX_TOP, QMX_ERR_NOT_SUPPORTED, "k %u not in 1..%u", k, MAX_TOP);
    QMX_REQUIRE(((uintptr_t)records_dev & 7) == 0, QMX_ERR_BAD_ARG, "records must be 8-byte aligned");
    QMX_HIP(hipSetDevice(device_id));
    if (nq == 0) return QMX_OK;
    const uint64_t rec = qmx_topk_record_bytes(nq, k);
    const qmx_scored_point *lists = (const qmx_scored_point *)records_dev;
    const uint32_t *counts = (const uint32_t *)((const char *)records_dev + (uint64_t)nq * k * sizeof(qmx_scored_point));
    return launch_merge_points((hipStream_t)hip_stream, lists, counts, list_idx_base_dev, n_lists, nq, k, out_dev, out_counts_dev,
                               rec / sizeof(qmx_scored_point), rec / sizeof(uint32_t));
}

int32_t qmx_search_quantized(const qmx_hnsw *g, qmx_query *quantized, qmx_query *raw, const qmx_search_params *p, const uint32_t *ids,
                             uint64_t n_ids, qmx_scored_point *out, uint32_t *out_counts, const volatile uint8_t *is_stopped,
                             qmx_counters *counters) {
    QMX_REFUSE_SPARSE(quantized);
    QMX_REFUSE_SPARSE(raw);
    QMX_REQUIRE(quantized && p && out && out_counts, QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(p->top >= 1, QMX_ERR_BAD_ARG, "top must be > 0");
    const bool rescore = p->rescore != 0;
    QMX_REQUIRE(!rescore || raw, QMX_ERR_BAD_ARG, "rescoring needs the original-vector query batch");
    QMX_REQUIRE(!raw || (raw->nq == quantized->nq && raw->device == quantized->device), QMX_ERR_BAD_ARG, "the two query batches must match");
    // get_oversampled_top (vector_index_search_common.rs:27-46): (oversampling * top as f64) as usize when > 1.0
    // (never clamped: the reference never searches fewer candidates than oversampling asks for; what does not fit fails loudly)
    const uint32_t top_limit = g ? HNSW_MAX_EF : MAX_TOP;
    QMX_REQUIRE(p->top <= top_limit, QMX_ERR_NOT_SUPPORTED, "top %u > %u not supported", p->top, top_limit);
    uint32_t otop = p->top;
    if (p->oversampling > 1.0f) {
        const double o = (double)p->oversampling * (double)p->top;
        QMX_REQUIRE(o <= (double)top_limit, QMX_ERR_NOT_SUPPORTED, "oversampled top %.0f > %u not supported", o, top_limit);
        otop = (uint32_t)o;
    }
    QMX_HIP(hipSetDevice(quantized->device));
    if (counters) memset(counters, 0, sizeof(*counters));
    const uint32_t nq = quantized->nq;
    if (nq == 0) return QMX_OK;
    QMX_TRY(quantized->cand.reserve((size_t)nq * otop * sizeof(qmx_scored_point)));
    QMX_TRY(quantized->cand_cnt.reserve((size_t)nq * 4));
    QMX_TRY(quantized->cand_ids.reserve((size_t)nq * otop * 4));
    qmx_scored_point *d_cand = (qmx_scored_point *)quantized->cand.p;
    uint32_t *d_cnt = (uint32_t *)quantized->cand_cnt.p, *d_ids = (uint32_t *)quantized->cand_ids.p;
    // stage 1: the quantized (or raw, when the caller passes the raw batch as `quantized`) search with the oversampled top
    if (g) {
        const uint32_t ef = std::max(p->hnsw_ef, otop);     // graph_layers.rs:549
        QMX_TRY(hnsw_search_sync(g, quantized, otop, ef, d_cand, d_cnt, is_stopped, counters, p->acorn != 0));   // SearchAlgorithm of the request
    } else {
        QMX_TRY(qmx_search_topk(quantized, otop, ids, n_ids, d_cand, d_cnt, is_stopped, counters));
    }
    if (!rescore) {   // search_result.truncate(top)
        StagedLists st;
        QMX_TRY(st.begin(quantized, p->top, out, out_counts));
        QMX_TRY(launch_split_candidates(quantized->stream, d_cand, d_cnt, otop, nq, nullptr, p->top, st.d_out, st.d_counts));
        QMX_TRY(st.end());
        QMX_HIP(hipStreamSynchronize(quantized->stream));
        return QMX_OK;
    }
    // stage 2: postprocess_search_result (:48-91): re-score the candidates with the original vectors, sort, truncate
    QMX_TRY(launch_split_candidates(quantized->stream, d_cand, d_cnt, otop, nq, d_ids, 0, nullptr, nullptr));
    QMX_HIP(hipStreamSynchronize(quantized->stream));
    QMX_TRY(qmx_rescore(raw, d_ids, d_cnt, otop, std::min(p->top, otop), out, out_counts));
    if (counters) {
        counters->bytes_read += (uint64_t)nq * otop * raw->seg->row_bytes;
        counters->kernel_launches += 2;
    }
    return QMX_OK;
}

}  // extern "C"
