// kernels.hpp — host-callable launchers of the HIP kernels (internal to libqdrant_amd.so).
#pragma once
#include "common.hpp"
#include "hnsw_layout.hpp"      // the walk's integer constants (HNSW_*): a header the host compiler reads too

namespace qmx {

constexpr int MAX_QT = 16;         // queries scored per pass of the stored block
constexpr int SCAN_BLOCK = 512;    // 8 wavefronts share one LDS copy of the query tile
constexpr int MAX_TOP_FAST = 64;   // register-resident per-wave list: one entry per lane

// What a scan / gather launch needs.  Plain data, passed by value to the kernels.
struct TqEc {                  // TQ+ symmetric scoring (score_symmetric_ec): i16 weights D'^2 per coordinate, their scale, <M, M>, the rows' xm column
    const int16_t *weights;
    const float *xm;
    float weight_scale, mm_const;
};
struct ScanArgs {
    const void *rows;          // stored block (reference row layout for the dtype)
    uint64_t n_rows;
    uint64_t row_stride;       // bytes
    uint32_t dim;              // elements per row consumed by the metric (actual_dim for SQ)
    uint32_t nseg;             // full 128-byte segments of the SIMD body
    uint32_t rem_pieces;       // 16-byte pieces of the SIMD body in the last, partial segment (0 = none)
    uint32_t tail_start;       // first element of the reference's scalar tail (== dim when none)
    uint32_t aux_off;          // byte offset of the per-query aux block inside a query tile entry
    uint32_t nq;               // live queries in this tile (<= QT)
    const void *queries;       // device, [QT][q_stride] bytes, preprocessed + cast (+ aux)
    uint32_t q_stride;         // bytes between queries
    uint32_t top;
    const uint32_t *ids;       // candidate list or nullptr (= rows 0..n_cand)
    uint64_t n_cand;           // candidates to visit
    DeletedView del;
    uint64_t *partial;         // [grid][partial_qt][top] keys (top-k mode)
    uint32_t partial_qt;       // query stride of `partial` (the small-row kernel; the tiled one uses its QT)
    const uint64_t *gthr;      // [QT] keys or nullptr (scan_mfma16.hip only): a key whose score is a lower bound of the query's final k-th best
                               // score (0 = none): the k-th best of a pre-scan of a prefix of the block (api_search.hip search_enqueue)
    const uint64_t *key_bound; // [QT] exclusive upper bound on accepted keys (top > 64 runs in passes of 64), or nullptr
    float *scores;             // [nq][n_cand] (score mode)
    uint64_t scores_stride;    // elements between queries in `scores`
    int *err_flag;             // set to 1 on an out-of-range id
    const int *run_if;         // nullptr, or: the kernel returns at once unless *run_if != 0 (the exact scan behind the split prefilter, scan_split.hip)
    const uint32_t *q_map;     // pq_scan_kernel only: list q of the launch scores query q_map[q] of the batch (0xFFFFFFFF: a padding slot), or nullptr
    // SQ
    float sq_multiplier;
    const float *row_offsets;  // SQ: per-row f32 offset (SoA copy) or nullptr when inline in rows
    float sq_shift;            // SQ: MetadataInt8::get_shift (encoded_vectors_u8.rs:116-134), used when a stored row is the query
    float sq_qoff;             // SQ, stored row as the query (HNSW build): its query offset = vector_offset - shift (:105-114, 715-728)
    uint32_t flags;            // QMX_SEG_U8_SCALAR_ORDER ...
    // u8 cosine with a STORED ROW as the query (HNSW build): the row's own norm stands in for the aux block of a query entry
    const float *row_norms_f;  // [n] sum of squares of every stored u8 row, in the AVX2 leaf's order (or nullptr)
    const int32_t *row_norms_i; // [n] the same as one exact i32 (scalar-order leaf)
    float u8_qnorm_f;          // set per query row by hnsw_build.hpp query_args
    int32_t u8_qnorm_i;
    // PQ
    uint32_t pq_m, pq_ncent;
    const float *pq_centroids; // [ncent][pq_dim] the codebook (the LUT-free walk, pq.hip HopPQDirect), or nullptr
    uint32_t pq_dim, pq_chunk, pq_kind;      // ... its geometry: floats per vector, per chunk; 0 dot / cosine, 1 Manhattan, 2 Euclid (PqGeom::kind)
    const float *pq_pair;      // [m][ncent][ncent] chunk distances between centroids = the terms of EncodedVectorsPQ::score_internal, or nullptr
    uint32_t pq_invert;
    // BQ: calculate_metric (encoded_vectors_binary.rs:766-810)
    uint32_t bq_dim;           // original dimension
    uint32_t bq_flip;          // 0: zeros - xor (every distance with its own invert), 1: xor - zeros
    uint32_t bq_qbits;         // bit planes per query value: 1 (QueryEncoding::SameAsStorage, internal queries), 4 or 8 (Scalar4bits / Scalar8bits)
    // TurboQuant (scan_tq.hip): per-row extras columns, bits per value (4 | 2 | 1), VectorParameters.invert
    const float *tq_sf;        // [n] scaling_factor
    const float *tq_l2;        // [n] l2_length (DistanceType::L2) or nullptr
    uint32_t tq_bits, tq_invert;
    uint32_t tq_planes;        // 1-bit storage: bit planes of the query (8; 16 under TQ+)
    uint32_t tq_qbytes_off;    // 1-bit storage: byte offset, inside a query entry, of the i8 form of the query (the matrix-core scan's operand)
    uint32_t tq_i32;           // the integer dot of a (row, query) pair fits 32 bits (scan_sq_mfma.hip finish): 4 / 2 bits below 2000 coordinates, 1 bit below 16384
    uint32_t tq_code_bytes;    // HNSW build (HopTQInternal): code bytes of a row, before the zero padding of the device block
    TqEc tq_ec;                // ... and score_symmetric_ec's inputs (weights == nullptr without TQ+)
    // multi-vectors (MaxSim walk, hnsw.hpp HopMaxSim): point p = inner rows [mv_offsets[p], mv_offsets[p + 1]); multi-query j = query entries
    // [mv_qfirst[j], mv_qfirst[j + 1])
    const uint64_t *mv_offsets;
    uint32_t mv_q_tokens;      // HopMaxSimQ (the build over multi-vector points with PQ / TurboQuant inner rows): query entries of the point being inserted
    const uint32_t *mv_qfirst;
    // custom queries as the walk's scorer (hnsw.hpp HopCustom): search qi = custom query cq_desc[qi] over the example entries of `queries`
    const qmx_custom_query *cq_desc;
    const float *cq_coefs;
    // TurboQuant over Manhattan, the walk (tq_l1_policy.hpp): the segment's TqL1Dev (tq_rotate.hpp) on the device
    const void *tq_l1;
};

enum ScanMode { SCAN_TOPK = 0, SCAN_SCORES = 1 };

// per-query aux block (64 bytes after the padded elements of each query in the tile)
// Byte form of a 1-bit-storage query (scan_sq_mfma.hip Tq1Ops<1> / BqOps): row piece p = 4 s + kg of step s sits at slot 4 s + (0, 2, 1, 3)[kg]
__host__ __device__ inline uint32_t byte_form_slot(uint32_t piece) { return (piece & ~3u) | ((piece & 1u) << 1) | ((piece >> 1) & 1u); }

struct QueryAux {
    float f0;           // u8 cosine: norm1 (reference order) ; SQ: query offset
    int32_t i0;         // u8 cosine scalar order: norm1 as i32
    uint32_t pad[14];
};
constexpr uint32_t QUERY_AUX_BYTES = 64;

// Device-resident HNSW search (hnsw.hpp): the graph + per-launch parameters.
struct HnswArgs {
    const uint32_t *reindex;        // [n_points]   point -> slot inside levels > 0
    const uint64_t *level_offsets;  // [n_levels + 1] first offsets-slot of each level
    const uint64_t *offsets;        // [n_slots + 1]  start of each links list inside `neighbors`
    const uint32_t *neighbors;
    uint64_t n_offsets, n_neighbors; // entries of `offsets` / `neighbors`: the walk never reads past them, whatever a links file claims
    const uint32_t *l0;             // optional packed level 0: l0[p * l0_stride] = count, then the links (one round trip per hop)
    uint32_t l0_stride;
    uint32_t l0_aux_off;            // 0, or m0: l0 is then the wider table of an SQ graph - a row = [m0 link slots, 0xFFFFFFFF behind the last][m0 f32: the linked rows' vector_offset]
    uint32_t n_points, n_levels, m, m0;
    const uint32_t *ep_ids, *ep_levels;   // EntryPoints::entry_points
    uint32_t n_ep;
    const uint32_t *xp_ids, *xp_levels;   // EntryPoints::extra_entry_points (iter_unsorted order)
    uint32_t n_xp;
    uint32_t ef, top, nq;
    uint32_t *visited;              // [slots][vis_words], all zero between searches
    uint64_t vis_words;
    uint32_t *vis_log;              // [slots][log_cap] word indices touched by the running search
    uint32_t log_cap;
    qmx_scored_point *out;          // [nq][top]
    uint32_t *out_counts;           // [nq]
    uint32_t *out_scored;           // [nq] points scored by each search (HardwareCounter cpu_io), may be null
    unsigned long long *pq_stats;   // PQ walk with the hop prefilter: [0] += hop candidates that met the 8-bit bound, [1] += those scored exactly (the survivors); may be null
    uint32_t lds_query_bytes;       // bytes of the query entry staged in LDS (16-byte multiple)
    uint32_t acorn;                 // SearchAlgorithm::Acorn on level 0 (graph_layers.rs:154-243): `visited` holds two bitmaps of vis_words / 2 words
    uint32_t hop_cap;               // entries of the hop id / score buffers in LDS (64; m0 (m0 + 1) rounded up for ACORN)
    // search_on_level_with_vectors (graph_layers.rs:336-389): the candidates the level-0 loop POPS (the one that ends it included) are what
    // the base scorer sees; they are listed here for the base scoring that follows the walk (api_hnsw.hip qmx_hnsw_search_with_vectors)
    uint32_t *expanded;             // [nq][xcap] or nullptr
    uint32_t *expanded_cnt;         // [nq] popped candidates (may exceed xcap: the list is then incomplete)
    uint32_t xcap;
    uint64_t *ev_spill;             // search_with_vectors: [slots][ev_cap] keys - the evicted-unexpanded candidates of the latest score beyond the four in registers
    uint32_t ev_cap;
    // the plain walk's pop sequence (qmx_hnsw_search_traced): every candidate the level-0 loop pops AND expands, in order, with its score
    qmx_scored_point *pops;         // [nq][pop_cap] or nullptr
    uint32_t *pop_cnt;              // [nq] (may exceed pop_cap: the list is then incomplete)
    uint32_t pop_cap;
    // option hnsw_reference_heap_order (a verification mode): `nearest` and `candidates` are the reference's two binary heaps, worked by one lane
    // in std's exact sift order; `nearest` lives in LDS, `candidates` (unbounded in the reference) in this per-slot scratch
    // PQ walk (HopPQ): per search an 8-bit image of its LUT (pq.hip pq_walk_lut8_kernel: [32-byte header: L, Es, step as f64, usable][m x 256 bytes]) staged in
    // LDS; a hop's candidates are scored against it first and only those whose upper bound reaches the beam's worst score are scored exactly
    const unsigned char *pq8;       // [nq][pq8_stride] or nullptr
    uint32_t pq8_stride;            // bytes per search (16-byte multiple) = what is staged in LDS
    uint32_t *next_query;           // device counter the slots draw their next search from (starts at the grid size); nullptr: the static stride
    uint32_t vis_lds;               // bytes of the search's visited table in LDS (hnsw.hpp LdsVisited: 0 or HNSW_VIS_LDS_BYTES); the HBM bitmap then holds what its buckets cannot
    uint32_t ref_heaps;
    uint32_t ref_cap;               // entries of a slot's candidates heap; a search that needs more raises err_flag = 2
    uint2 *ref_cands;               // [slots][ref_cap]  (x = idx, y = score bits)
    uint32_t explore_cap;           // ACORN: entries of the list of nodes to explore = the graph's longest level-0 list, m0 at least (merged / loaded graphs have longer ones)
};

// The PQ walk without LUTs (pq.hip HopPQDirect): the query entry is the preprocessed f32 vector, a LUT entry is recomputed from the codebook where it is needed
bool pq_direct_walk_ok(uint32_t dim, uint32_t m, uint32_t chunk, uint32_t ncent);
int32_t launch_hnsw_pq_direct(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
// grid == 0: only report the occupancy (blocks of one wave per CU) of the instantiation in *per_cu
int32_t launch_hnsw_dense(hipStream_t st, int dtype, int distance, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
// TurboQuant (scan_tq.hip)
struct TqRotationHost {        // HadamardRotation on the device: forward maps, chunk decomposition, per-chunk 1 / sqrt(size)
    const uint32_t *d_maps, *d_chunk_off, *d_chunk_size;
    const double *d_chunk_norm;
    uint32_t n_chunks, rot_dim, padded_dim, dim;
};
int32_t launch_scan_tq(hipStream_t st, int qt, ScanMode mode, const ScanArgs &a, int num_cus, uint32_t *grid_out);
int32_t launch_scan_bq_mfma(hipStream_t st, int qt, ScanMode mode, const ScanArgs &a, int num_cus, uint32_t *grid_out);
int32_t launch_scan_tq_mfma(hipStream_t st, int qt, ScanMode mode, const ScanArgs &a, int num_cus, uint32_t *grid_out);   // scan_sq_mfma.hip, 4 / 2 bits
int32_t launch_hnsw_tq(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_tq_l1(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu, uint32_t rot_dim);   // hnsw_tq_l1.hip
int32_t launch_tq_split(hipStream_t st, const void *rows, uint64_t src_stride, uint64_t n, uint32_t code_bytes, uint32_t dst_stride, int has_l2,
                        void *codes, float *sf, float *l2, float *xm);
int32_t launch_tq_rotate(hipStream_t st, const float *d_in, uint32_t n, const TqRotationHost &h, double *d_out);
int32_t launch_tq_rotate_f64(hipStream_t st, double *d_buf, uint32_t n, const TqRotationHost &h);   // in place, h = the inverse rotation's tables
// TurboQuant over Manhattan (tq_l1.hip): DistanceType::L1 scores = dequantise + inverse rotation per row, then sum |q - v|
struct PairSel;
int32_t launch_tq_l1_dequant(hipStream_t st, const void *codes, uint64_t row_stride, const float *sf, const uint32_t *d_ids, uint64_t id0, uint64_t n,
                             uint64_t n_rows, uint32_t padded_dim, uint32_t value_bits, const float *d_shift, const float *d_scale, double *d_out, int *err_flag,
                             const PairSel *sel);   // rows d_ids[r], or id0 + r; sel: item id0 + r of a pair list (dead slots give zeros)
int32_t launch_tq_l1_diff(hipStream_t st, double *d_a, const double *d_b, uint64_t n_elems);      // a <- a - b
// scores[q * stride + col0 + i] for rows i of d_deq ([n][padded_dim]) and queries [q0, q0 + nq): the sum over k < dim of (f32)|q[k] - v[k]| in order,
// negated when `invert`; d_queries = f32 [.][q_dim] (nullptr: the zero query); sel != nullptr: one (query, row) pair per row of d_deq, scores[col0 + i]
int32_t launch_tq_l1_scores(hipStream_t st, const double *d_deq, uint64_t n, uint32_t padded_dim, uint32_t dim, const float *d_queries, uint32_t q_dim,
                            uint32_t q0, uint32_t nq, float *d_scores, uint64_t stride, uint64_t col0, int invert, const PairSel *sel, uint64_t item0);
int32_t launch_tq_plus_fit(hipStream_t st, double *d_rot, uint32_t n, uint32_t padded_dim, uint32_t distance, double min_q, double max_q, float c_outer,
                           float *d_shift, float *d_scale);
int32_t launch_tq_quantize(hipStream_t st, double *d_rot, uint32_t n, uint32_t padded_dim, uint32_t value_bits, uint32_t distance, void *d_out,
                           uint32_t out_stride, const float *d_shift, const float *d_scale);
int32_t launch_tq_query_encode(hipStream_t st, double *d_rot, uint32_t nq, uint32_t padded_dim, uint32_t bits, int need_l2, void *tile, uint32_t q_stride,
                               uint32_t aux_off, const float *d_shift, const float *d_scale, uint32_t qbytes_off);
int32_t launch_tq_internal(hipStream_t st, const void *codes, uint32_t stride, const float *sf, const float *l2, uint32_t code_bytes, uint32_t bits,
                           int invert, uint64_t n_rows, const uint32_t *a_ids, const uint32_t *b_ids, uint32_t n, float *out, int *err_flag, const TqEc *ec);
// the MaxSim walk over multi-vector points (HopMaxSim): dense, SQ and BQ inner rows
// ... with a custom query (Recommend / Discover / Context / Feedback) as the scorer (hnsw.hpp HopCustom over the storage's own hop policy)
int32_t launch_hnsw_custom_dense(hipStream_t st, int dtype, int distance, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_custom_sq(hipStream_t st, int distance, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_custom_bq(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_custom_pq(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_custom_tq(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_custom_tq_l1(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu, uint32_t rot_dim);   // (hnsw_tq_l1.hip)
// ... whose examples are multi-vectors over multi-vector points (MultiCustomQueryScorer: HopCustom over HopMaxSim); dense and SQ inner rows
int32_t launch_hnsw_custom_maxsim_dense(hipStream_t st, int dtype, int distance, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_custom_maxsim_sq(hipStream_t st, int distance, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_maxsim_dense(hipStream_t st, int dtype, int distance, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_maxsim_sq(hipStream_t st, int distance, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_maxsim_bq(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_maxsim_pq(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);      // (pq.hip; the query's tokens = their LUTs)
int32_t launch_hnsw_maxsim_tq(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);      // (hnsw_maxsim_tq.hip)
int32_t launch_hnsw_sq(hipStream_t st, int distance, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_pq(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
// the 8-bit images of a batch's LUTs for the walk's hop prefilter (HnswArgs::pq8); bytes per search: pq_walk_lut8_stride(m)
static inline uint32_t pq_walk_lut8_stride(uint32_t m) { return 32u + m * 256u; }
int32_t launch_pq_walk_lut8(hipStream_t st, const void *d_luts, uint32_t q_stride, uint32_t nq, uint32_t m, uint32_t ncent, void *d_out);
int32_t launch_hnsw_bq(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu);
int32_t launch_hnsw_pack_level0(hipStream_t st, const uint64_t *offsets, const uint32_t *neighbors, uint32_t n_points, uint32_t stride, uint32_t *l0);
// the table again, each row followed by one f32 per link slot: aux[linked row] (SQ: the offsets column travels with the links)
int32_t launch_hnsw_pack_level0_aux(hipStream_t st, const uint32_t *l0, uint32_t n_points, uint32_t stride, const float *aux, uint64_t n_aux, uint32_t *l0x);
constexpr uint32_t HNSW_BUILD_MAX_M0 = 128;     // links per level-0 list of a device build (m <= m0 <= 128)
// HNSW build (hnsw_build.hpp)
constexpr uint32_t HNSW_BUILD_MAX_LEVELS = 16;   // levels 0..15 (P(level >= 16) ~ m^-15.5)
struct BuildLinks {
    uint32_t *links0, *cnt0, *linksU, *cntU;
    const uint32_t *up_off;
    uint32_t m, m0;
#if defined(__HIPCC__)
    __device__ __forceinline__ uint32_t *list(uint32_t p, uint32_t level) const {
        return level == 0 ? links0 + (uint64_t)p * m0 : linksU + ((uint64_t)up_off[p] + level - 1) * m;
    }
    __device__ __forceinline__ uint32_t *count(uint32_t p, uint32_t level) const {
        return level == 0 ? cnt0 + p : cntU + ((uint64_t)up_off[p] + level - 1);
    }
    __device__ __forceinline__ uint32_t level_m(uint32_t level) const { return level == 0 ? m0 : m; }
#endif
};
struct HnswBuildArgs {
    BuildLinks g;
    const uint8_t *level;        // [n] level of every point
    uint32_t n_points;
    uint32_t first, count;       // the batch: points first .. first + count
    uint32_t ep_id, ep_level;    // entry point of the graph before the batch
    uint32_t ef_construct;
    uint32_t *visited;           // [slots][vis_words]
    uint64_t vis_words;
    uint32_t *vis_log;           // [slots][log_cap]
    uint32_t log_cap;
    // phase 1 -> phase 2: sel[(bi * HNSW_BUILD_MAX_LEVELS + l) * m0 + k]
    uint32_t *sel_ids;
    float *sel_scores;
    uint32_t *sel_cnt;           // [count][HNSW_BUILD_MAX_LEVELS]
    uint32_t *lock;              // [n]
    uint32_t lds_query_bytes;    // row bytes rounded up to whole 128-byte steps, staged per new point
    uint32_t row_bytes;
    // quantized storages that cannot turn a stored row into a query (PQ): the query entries of the batch, made from the ORIGINAL vectors
    // (point_scorer.rs:197-212) before phase 1; entry bi = batch_queries + bi * batch_q_stride (global memory; nullptr = stage the row)
    const unsigned char *batch_queries;
    uint64_t batch_q_stride;
    uint32_t *next;              // [2] device counters the slots of phase 1 / phase 2 draw their next insertion from (each starts at its launch's grid size); nullptr: static stride
};
// phase 1 = insertion searches + heuristic selection, phase 2 = linking; grid == 0: report occupancy only
int32_t launch_hnsw_build_bq(hipStream_t st, const ScanArgs &a, const HnswBuildArgs &h, int phase, uint32_t grid, int *per_cu);
int32_t launch_hnsw_build_sq(hipStream_t st, int distance, const ScanArgs &a, const HnswBuildArgs &h, int phase, uint32_t grid, int *per_cu);
int32_t launch_hnsw_build_dense(hipStream_t st, int dtype, int distance, const ScanArgs &a, const HnswBuildArgs &h, int phase,
                                uint32_t grid, int *per_cu);
int32_t launch_hnsw_build_maxsim_dense(hipStream_t st, int dtype, int distance, const ScanArgs &a, const HnswBuildArgs &h, int phase, uint32_t grid,
                                       int *per_cu);
int32_t launch_hnsw_build_maxsim_sq(hipStream_t st, int distance, const ScanArgs &a, const HnswBuildArgs &h, int phase, uint32_t grid, int *per_cu);
int32_t launch_hnsw_build_maxsim_bq(hipStream_t st, const ScanArgs &a, const HnswBuildArgs &h, int phase, uint32_t grid, int *per_cu);
int32_t launch_hnsw_build_tq(hipStream_t st, const ScanArgs &a, const HnswBuildArgs &h, int phase, uint32_t grid, int *per_cu);
int32_t launch_hnsw_build_tq_l1(hipStream_t st, const ScanArgs &a, const HnswBuildArgs &h, int phase, uint32_t grid, int *per_cu, uint32_t rot_dim,
                                uint32_t padded_dim);      // ... over Manhattan (hnsw_build_tq_l1.hip)
int32_t launch_hnsw_build_pq(hipStream_t st, const ScanArgs &a, const HnswBuildArgs &h, int phase, uint32_t grid, int *per_cu);
int32_t launch_hnsw_build_maxsim_pq(hipStream_t st, const ScanArgs &a, const HnswBuildArgs &h, int phase, uint32_t grid, int *per_cu);   // multi-vector points over PQ inner rows
int32_t launch_hnsw_build_maxsim_tq(hipStream_t st, const ScanArgs &a, const HnswBuildArgs &h, int phase, uint32_t grid, int *per_cu);   // ... over TurboQuant inner rows (hnsw_build_multi_tq.hip)
// pair[c][i][j] = DistanceType::distance(centroid i chunk c, centroid j chunk c): the per-chunk terms of score_internal (encoded_vectors_pq.rs:574-618)
int32_t launch_pq_pair_table(hipStream_t st, uint32_t distance, uint32_t dim, const qmx_pq_params &pq, const float *d_centroids, float *d_pair);
// norms[r] = sum of squares of u8 row r as the cosine leaf computes it for a stored row (metric_uint/avx2/cosine.rs, simple_cosine.rs)
int32_t launch_u8_row_norms(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, uint32_t flags, float *norms_f, int32_t *norms_i);

// dense f32 / f16 / u8 (scan_dense.hip)
int32_t launch_scan_dense(hipStream_t st, int dtype, int distance, int qt, ScanMode mode,
                          const ScanArgs &a, int num_cus, uint32_t *grid_out);
// f32 dot / cosine, 8..32 queries per pass on v_mfma_f32_4x4x1 with the reference's bits (scan_mfma.hip)
int32_t launch_scan_f32_mfma(hipStream_t st, int qt, ScanMode mode, const ScanArgs &a, int num_cus, uint32_t *grid_out);
// ... the scores of a short candidate list, 16 queries per tile on 4 waves: a block that fits beside one of the resident int8 scan (option prescan_beside_scan)
int32_t launch_scan_f32_mfma_beside(hipStream_t st, const ScanArgs &a, int num_cus, uint32_t *grid_out);
// SQ int8 dot / cosine / euclid, 8..32 queries per pass on v_mfma_i32_16x16x64_i8 (scan_sq_mfma.hip)
bool sq_mfma_ok(uint32_t distance, uint32_t actual_dim);
int32_t launch_scan_sq_mfma(hipStream_t st, int qt, ScanMode mode, const ScanArgs &a, int num_cus, uint32_t *grid_out);
int32_t launch_scan_f16_mfma(hipStream_t st, int qt, ScanMode mode, const ScanArgs &a, int num_cus, uint32_t *grid_out);
// which query an item belongs to: explicit list, or fixed-size slots (item / per_query, with the
// live prefix of each slot given by counts), or item == query (score_internal)
struct PairSel {
    const uint32_t *qsel;      // explicit query index per item, or nullptr
    uint32_t per_query;        // > 0: query = item / per_query
    const uint32_t *counts;    // with per_query: only the first counts[query] items of a slot are live
    const uint32_t *limit;     // or nullptr: a device-side item count - items at and behind *limit are dead (a pool filled on the device: the host knows its capacity only)
    __device__ __forceinline__ uint32_t query_of(uint64_t item) const {
        if (qsel) return qsel[item];
        if (per_query) return (uint32_t)(item / per_query);
        return (uint32_t)item;
    }
    __device__ __forceinline__ bool live(uint64_t item, uint32_t qi) const {
        if (limit && item >= (uint64_t)*limit) return false;
        if (per_query && counts) return (uint32_t)(item % per_query) < counts[qi];
        return true;
    }
};

int32_t launch_pairs_dense(hipStream_t st, int dtype, int distance, const ScanArgs &a, const PairSel &sel,
                           uint64_t n_items, int num_cus);
int32_t launch_pairs_sq(hipStream_t st, int distance, const ScanArgs &a, const PairSel &sel, uint64_t n_items, int num_cus);
// SQ int8 rows: codes SoA + offsets (scan_quant.hip)
int32_t launch_scan_sq(hipStream_t st, int distance, int qt, ScanMode mode, const ScanArgs &a, int num_cus,
                       uint32_t *grid_out);
int32_t launch_sq_encode(hipStream_t st, int distance, const qmx_sq_params &sp, uint32_t dim, const float *in, uint64_t n,
                         uint8_t *codes_out, uint64_t codes_stride, float *offsets_out, uint8_t *rows_out, int is_query,
                         uint32_t aux_off);
int32_t launch_sq_split(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t actual_dim, void *codes,
                        float *offsets);
int32_t launch_sq_gather_rows(hipStream_t st, const void *codes, const float *offsets, uint32_t actual_dim, const uint32_t *ids,
                              uint32_t n, uint64_t n_rows, void *rows_out, int *err_flag);
int32_t launch_sq_internal_query(hipStream_t st, const void *codes, const float *offsets, uint32_t actual_dim, const uint32_t *ids,
                                 uint32_t nq, uint64_t n_rows, float shift, void *tile, uint32_t q_stride, uint32_t aux_off,
                                 int *err_flag);
// f32 dot / cosine, 32- and 64-query tiles on v_mfma_f32_16x16x4_f32, chain-major (scan_mfma16.hip)
bool mfma16_dim_ok(int qt, uint32_t dim);
bool mfma16_scan_ok(int qt, ScanMode mode, const ScanArgs &a);   // qt = 16, 32 or 64
int32_t launch_scan_f32_mfma16(hipStream_t st, int qt, const ScanArgs &a, int num_cus, uint32_t *grid_out);
// ... the conditional exact pass behind the int8 prefilter in one launch of 16-query block rows, in a block that fits beside a resident int8 scan block
// (option fallback_beside_scan), and what such a block needs of a CU
int32_t launch_scan_f32_mfma16_groups(hipStream_t st, const ScanArgs &a, int num_cus, uint32_t *grid_out);
int32_t mfma16_groups_footprint(uint32_t dim, bool perq, size_t *lds_bytes, int *regs_per_simd);
// f32 dot / cosine, 65..128 queries per pass: f16-split matrix-core prefilter + exact verification (scan_split.hip; regroup, refine, select and plan: split_select.hip)
bool split_scan_ok(const ScanArgs &a);
size_t split_query_bytes(uint32_t dim);
float split_row_scale(float row_maxabs);
int32_t launch_split_row_stats(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, float scale, uint32_t *d_stats);
int32_t launch_split_pack_queries(hipStream_t st, const float *d_q, uint32_t nq, uint32_t dim, float *d_qmax, float *d_qnorm, void *d_bq, int half, uint32_t qt);
int32_t launch_split_thresholds(hipStream_t st, const uint64_t *d_gthr, const float *d_qnorm, const float *d_qmax, uint32_t nq, float rel_band, float abs_band,
                                float row_norm_max, float row_scale, float *d_scales, float *d_thr, float *d_band, uint32_t qt, uint32_t *d_cand_cnt, uint32_t n_cnt);
int32_t launch_scan_f32_split(hipStream_t st, const ScanArgs &a, const void *d_bq, float row_scale, const float *d_scales, const float *d_thr,
                              uint64_t *d_cand, uint32_t *d_cand_cnt, uint32_t cap, int num_cus, const void *d_rows_split, int half, void *d_wlists, uint32_t phase, uint32_t qt);
int32_t launch_regroup_lists(hipStream_t st, const DeletedView &del, const void *d_wlist, const uint32_t *d_wcnt, uint32_t wcap, uint32_t n_lists, uint64_t *d_cand,
                             uint32_t *d_cand_cnt, uint32_t cap, int *d_overflow);
// PQ prefilter (pq_prefilter.hip): rotated copy of the code block, 6-bit tables + thresholds per query, the approximate scan
size_t pq_rot_bytes(uint64_t n, uint32_t m);
bool pq_prefilter_shape_ok(uint32_t m, uint32_t ncent);
int32_t launch_pq_rotate(hipStream_t st, const void *codes, uint64_t row_stride, uint64_t n, uint32_t m, void *d_out);
size_t pq_prefilter_table_bytes(uint32_t m, uint32_t nq);
uint32_t pq_prefilter_grid(int num_cus, uint32_t nq, uint32_t *n_slabs_out);
size_t pq_prefilter_wlists_counts_bytes(uint32_t grid);
size_t pq_prefilter_wlists_bytes(uint32_t grid, uint32_t wcap);
int32_t launch_pq_lut8(hipStream_t st, const void *d_luts, uint32_t q_stride, uint32_t nq, uint32_t m, uint32_t ncent, const uint64_t *d_gthr, void *d_table8,
                       int32_t *d_thr, float *d_band);
int32_t launch_pq_prefilter(hipStream_t st, const ScanArgs &a, const void *d_rot, const void *d_table8, const int32_t *d_thr, uint32_t nq, int num_cus,
                            void *d_wlists, uint32_t wcap, uint32_t *grid_out);
int32_t launch_split_refine(hipStream_t st, const uint64_t *d_cand, const uint32_t *d_cand_cnt, uint32_t cap, const float *d_band, uint32_t nq, uint32_t top,
                            const float *d_scales, float *d_thr);
size_t split_wlists_bytes(int num_cus);
int32_t launch_split_regroup(hipStream_t st, const ScanArgs &a, const void *d_wlists, int num_cus, uint64_t *d_cand, uint32_t *d_cand_cnt, uint32_t cap,
                             int *d_overflow, uint32_t phase, uint32_t qt);
size_t split_copy_bytes(uint64_t n, uint32_t dim, int half);
int32_t launch_split_copy(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, float row_scale, void *d_out, int half);
// what one search through the prefilter did (device side; api_search.hip folds it into qmx_counters)
struct SplitStats {
    unsigned long long candidates;   // (row, query) pairs the approximate scan let through, deleted rows dropped
    unsigned long long verified;     // of those, re-scored exactly from the f32 rows
    uint32_t fallback_queries;       // queries whose lists overflowed: they took the exact scan of the block
    uint32_t pad;
};
// the verification pool of one search: the rows worth an exact score, of all its queries, as one ragged list filled on the device - query q's rows sit at
// ids[off[q] .. off[q] + cnt[q]) with qsel[] = q beside them (the gather kernel's explicit query index), *used = entries taken so far (zeroed per search).
// A query takes what it needs (a few hundred rows on friendly data, tens of thousands where a worst-case band is wide): only a pool that is full sends a
// query to the exact scan.
struct VerifyPool {
    uint32_t *ids, *qsel, *off, *cnt, *used;
    uint32_t cap;
    uint32_t max_per_query;     // a query with more rows than this inside its band takes the exact scan whatever room the pool has (option verify_max_per_query; default: cap)
};
int32_t launch_split_select(hipStream_t st, const uint64_t *d_cand, const uint32_t *d_cand_cnt, uint32_t cap, const float *d_band, uint32_t nq, uint32_t top,
                            const VerifyPool &pool, uint32_t q_base, const int *d_tile_overflow, uint32_t *d_ovf_q, SplitStats *d_stats,
                            const float *d_t_exact = nullptr, bool tighten = false);
// the int8 copy of an f32 block (QMX_SEG_I8_COPY) and its passes (scan_i8copy.hip; the probe: split_select.hip)
bool split_i8_dim_ok(uint32_t dim);
size_t split_i8_copy_bytes(uint64_t n, uint32_t dim);
size_t split_i8_query_bytes(uint32_t dim);
uint32_t split_i8_probe();
int32_t launch_split_i8_colstats(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, uint32_t *d_colmax, float *d_colsq);
float split_i8_choose_scales(const float *colmax, const float *colsq, uint64_t n, uint32_t dim, float *scale);   // host; returns the balance G (0 = floor scales)
int32_t launch_split_i8_rowstats(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, const float *d_scale, uint32_t *d_stats);
int32_t launch_split_i8_copy(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, const float *d_scale, void *d_out);
int32_t launch_split_i8_pack(hipStream_t st, const float *d_q, uint32_t nq, uint32_t dim, const float *d_scale, const uint64_t *d_gthr, const uint32_t *d_row_stats,
                             float row_norm_max, void *d_bq, float *d_qscale, float *d_band, float *d_thr, float *d_t_exact, uint32_t *d_cand_cnt, uint32_t n_cnt);
int32_t launch_scan_i8copy(hipStream_t st, const ScanArgs &a, const void *d_bq, const float *d_qscale, const float *d_thr, int num_cus, const void *d_rows_i8,
                           void *d_wlists, uint32_t phase);
int32_t split_i8_scan_footprint(uint32_t dim, size_t *lds_bytes, int *regs_per_simd);      // what a block of that scan holds of its CU (registers: its two waves per SIMD)
int32_t launch_split_i8_probe(hipStream_t st, const uint64_t *d_cand, const uint32_t *d_cand_cnt, uint32_t cap, const float *d_band, uint32_t nq, uint32_t top,
                              const int *d_tile_overflow, uint32_t *d_probe_ids, uint32_t *d_probe_cnt);
int32_t launch_split_i8_bound(hipStream_t st, const float *d_scores, uint32_t *d_probe_cnt, uint32_t nq, uint32_t top, const float *d_band, const float *d_qscale,
                              float *d_thr, float *d_t_exact);
// option i8_sample_scan: the sample's bound from tiles of the int8 copy (launch_split_i8_pack with d_gthr = nullptr runs first) - approximate scores of
// the sample's 16-row tiles, launch_custom_topk over them, its picks into the probe slots, the pair kernel, the bound
uint32_t split_i8_sample_queries(uint32_t dim, uint32_t nq);      // queries per block of the sample kernel
int32_t launch_scan_i8copy_sample(hipStream_t st, const void *d_rows_i8, const void *d_bq, uint32_t dim, const uint32_t *d_sample, uint32_t n_tiles, uint32_t nq,
                                  const float *d_qscale, float *d_scores);
int32_t launch_split_i8_picks(hipStream_t st, const qmx_scored_point *d_lists, const uint32_t *d_counts, uint32_t nq, uint32_t top, const float *d_band,
                              uint32_t *d_probe_ids, uint32_t *d_probe_cnt);
int32_t launch_split_i8_sample_bound(hipStream_t st, const float *d_scores, const uint32_t *d_probe_ids, uint32_t *d_probe_cnt, uint32_t nq, uint32_t top,
                                     float *d_band, const float *d_qscale, float *d_thr, float *d_t_exact, uint64_t *d_gthr);
// TurboQuant 4 bits, 128 queries per pass: codes decoded once per tile into the matrix cores' operand images, exact scores, candidate lists (scan_tq4w.hip)
bool tq4w_shape_ok(const ScanArgs &a);
size_t tq4w_query_bytes(uint32_t code_bytes);
size_t tq4w_wlists_counts_bytes(int num_cus);
size_t tq4w_wlists_bytes(int num_cus);
uint32_t tq4w_wcap();
int32_t launch_tq4w_stats(hipStream_t st, const float *d_sf, const float *d_l2, const void *d_rows, uint64_t row_stride, uint32_t code_bytes, uint64_t n, uint32_t *d_stats);
int32_t launch_tq4w_pack(hipStream_t st, const ScanArgs &a, const uint64_t *d_gthr, float sf_min, float sf_max, float l2_min, float l2_max, uint32_t c1, int high_only,
                         void *d_bq, int32_t *d_thr_i,
                         float *d_qinfo, float *d_band, uint32_t *d_cand_cnt, uint32_t n_cnt);
int32_t launch_scan_tq4w(hipStream_t st, const ScanArgs &a, const void *d_bq, const int32_t *d_thr_i, const float *d_qinfo, const float *d_band_high_only, int num_cus,
                         void *d_wlists, uint32_t *grid_out);
// scalar int8, 128 queries per pass: a wave's lanes fetch their own operand pieces, exact integer dots, candidate lists (scan_sqw.hip)
bool sqw_shape_ok(const ScanArgs &a);
size_t sqw_query_bytes(uint32_t dim);
size_t sqw_wlists_counts_bytes(int num_cus);
size_t sqw_wlists_bytes(int num_cus);
uint32_t sqw_wcap();
uint64_t sqw_bi_entries(uint64_t n);      // entries of the column launch_sqw_stats fills: n rounded up to whole 256-row tiles
int32_t launch_sqw_stats(hipStream_t st, const float *d_off, uint64_t n, float multiplier, int32_t *d_bi, uint32_t *d_stats);
int32_t launch_sqw_pack(hipStream_t st, const ScanArgs &a, const uint64_t *d_gthr, float off_absmax, void *d_bq, int32_t *d_thr_i, float *d_qinfo, float *d_band,
                        uint32_t *d_cand_cnt, uint32_t n_cnt);
int32_t launch_scan_sqw(hipStream_t st, const ScanArgs &a, const void *d_bq, const int32_t *d_thr_i, const int32_t *d_bi, const float *d_qinfo, int num_cus,
                        void *d_wlists, uint32_t *grid_out);
// the overflowed queries packed for the conditional exact passes: list, their pre-scan bounds, the passes' run flags
int32_t launch_split_plan(hipStream_t st, const uint32_t *d_ovf_q, uint32_t nq, const uint64_t *d_gthr, uint32_t *d_list, uint64_t *d_gthr_packed, uint32_t list_cap,
                          uint32_t *d_count, int *d_run16, int *d_run64, uint32_t n_run64, SplitStats *d_stats, const void *d_queries, uint32_t q_stride,
                          void *d_packed_queries, const uint32_t *d_filter_of = nullptr, uint32_t *d_filter_of_packed = nullptr);
// order statistics of a float array (quantile.hip): the SQ quantile interval
int32_t launch_order_statistics_f32(hipStream_t st, const float *d_in, float *d_tmp, uint64_t n, uint64_t lo_pos, uint64_t hi_pos, float *h_out);
// BQ 1-bit (scan_bq.hip)
int32_t launch_scan_bq(hipStream_t st, int qt, ScanMode mode, const ScanArgs &a, int num_cus, uint32_t *grid_out);
int32_t launch_pairs_bq(hipStream_t st, const ScanArgs &a, const PairSel &sel, uint64_t n_items, int num_cus);
int32_t launch_pairs_tq(hipStream_t st, const ScanArgs &a, const PairSel &sel, uint64_t n_items, int num_cus);
uint64_t bq_row_bytes(uint32_t dim, uint32_t encoding);
int32_t launch_bq_encode_scalar_query(hipStream_t st, const float *d_in, uint32_t nq, uint32_t dim, uint32_t encoding, uint32_t bits, uint8_t *d_out,
                                      uint32_t out_stride, uint32_t qbytes_off, uint32_t aux_off, uint32_t body);
int32_t launch_vector_stats(hipStream_t st, const float *d_rows, uint64_t row_stride_bytes, uint64_t n, uint32_t dim, float *d_min, float *d_max, float *d_mean,
                            float *d_stddev);
int32_t launch_bq_encode(hipStream_t st, const float *d_in, uint64_t n, uint32_t dim, uint32_t encoding, const float *d_mean, const float *d_stddev,
                         uint8_t *d_out, uint64_t out_stride);
// PQ (pq.hip)
int32_t launch_scan_pq(hipStream_t st, ScanMode mode, const ScanArgs &a, int num_cus, uint32_t *grid_out);
int32_t launch_pairs_pq(hipStream_t st, const ScanArgs &a, const PairSel &sel, uint64_t n_items, int num_cus);
int32_t launch_pq_lut(hipStream_t st, uint32_t distance, uint32_t dim, const qmx_pq_params &pq, const float *d_centroids,
                      const float *d_queries, uint32_t nq, float *d_lut);
int32_t launch_pq_internal(hipStream_t st, uint32_t distance, uint32_t dim, const qmx_pq_params &pq, const float *d_centroids,
                           const float *d_pair, const void *rows, uint64_t row_stride, uint64_t n_rows, const uint32_t *a_ids, const uint32_t *b_ids,
                           uint32_t n, float *out, int *err_flag);
int32_t launch_pq_train(hipStream_t st, uint32_t dim, uint32_t chunk_size, uint32_t n_centroids, const float *d_data, uint64_t n,
                        uint32_t max_iters, float accuracy, uint32_t threads, float *d_centroids, uint32_t *iters_host);
int32_t launch_pq_encode(hipStream_t st, uint32_t dim, const qmx_pq_params &pq, const float *d_centroids, const float *d_in,
                         uint64_t n, uint8_t *d_codes);
// query tile packing: preprocessed f32 queries -> element type, padded, + aux (preprocess.hip)
int32_t launch_pack_queries(hipStream_t st, int dtype, int distance, const void *src, int src_is_encoded,
                            uint32_t src_stride, uint32_t nq, uint32_t dim, void *tile, uint32_t q_stride, uint32_t aux_off);
// top-k merge of `n_lists` key lists per query into ScoredPointOffset rows (topk_merge.hip)
// pass p of a top > 64 search: writes out[q * out_stride + out_offset ..+top), counts accumulate when out_offset > 0,
// next_bound[q] = key of the last entry written (0 = this query is exhausted)
int32_t launch_merge_keys(hipStream_t st, const uint64_t *partial, uint32_t n_lists,
                          uint32_t qt_stride, uint32_t nq, uint32_t top, qmx_scored_point *out,
                          uint32_t *out_counts, uint32_t out_stride = 0, uint32_t out_offset = 0,
                          uint64_t *next_bound = nullptr, const int *run_if = nullptr, const uint32_t *out_map = nullptr, uint32_t shared_grid = 0,
                          bool grouped = false);   // grouped: the lists of launch_scan_f32_mfma16_groups - list q of *run_if is column q % 16 of group q / 16's n_lists lists
int32_t launch_merge_points(hipStream_t st, const qmx_scored_point *lists, const uint32_t *list_counts,
                            const uint32_t *list_idx_base, uint32_t n_lists, uint32_t nq, uint32_t k, qmx_scored_point *out,
                            uint32_t *out_counts, uint64_t list_stride = 0, uint64_t count_stride = 0);   // strides in entries / words between lists (0 = contiguous arrays)
int32_t launch_split_candidates(hipStream_t st, const qmx_scored_point *cand, const uint32_t *cand_cnt, uint32_t n_per, uint32_t nq,
                                uint32_t *ids, uint32_t top, qmx_scored_point *out, uint32_t *out_counts);
int32_t launch_sort_scored(hipStream_t st, const float *scores, const uint32_t *ids, const uint32_t *counts, uint32_t n_per_query, uint32_t nq, uint32_t top,
                           qmx_scored_point *out, uint32_t *out_counts, const uint32_t *offsets = nullptr);   // offsets: query q's entries start at offsets[q] (ragged), not at q * n_per_query

// custom queries (custom_query.hip): combine the per-example similarity matrix, top-k of a score row
int32_t launch_custom_combine(hipStream_t st, const qmx_custom_query *d_queries, uint32_t n_queries, const float *d_sims, uint64_t n,
                              const float *d_coefs, float *d_out);
int32_t launch_maxsim(hipStream_t st, const float *d_sims, uint64_t n_rows, const uint32_t *d_qfirst, uint32_t n_queries, const uint64_t *d_offsets,
                      uint32_t n_points, const uint32_t *d_ids, uint64_t n, float *d_out, int *err_flag);
int32_t launch_custom_topk(hipStream_t st, const float *d_scores, uint64_t n, const uint32_t *d_ids, const DeletedView &del, uint32_t n_queries,
                           uint32_t top, qmx_scored_point *d_out, uint32_t *d_counts, uint64_t *d_bound = nullptr,    // d_bound[q] = the k-th best key of a full list, else 0
                           bool beside_scan = false);   // a prefilter's sample bound: the 256-thread kernel where it applies (option prescan_beside_scan)

// Metric::preprocess + element casts (preprocess.hip)
int32_t launch_cosine_preprocess_f32(hipStream_t st, const float *in, float *out, uint64_t n, uint32_t dim);
int32_t launch_cast_f32(hipStream_t st, int dst_dtype, const float *in, void *out, uint64_t count);
int32_t launch_minmax_f32(hipStream_t st, const float *in, uint64_t count, float *min_out, float *max_out);
int32_t launch_gather_rows(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t row_bytes,
                           const uint32_t *ids, uint32_t n, uint64_t n_rows, void *out, int *err_flag);

// sparse vectors (sparse.hip): CSR rows sorted by index, CSR query lists, and per query the posting ranges of its dimensions (ascending)
struct SparseRows {
    const uint64_t *off;
    const uint32_t *idx;
    const float *val;
    uint64_t n;
};
struct SparseQueries {
    const uint64_t *off;
    const uint32_t *idx;
    const float *val;
};
struct SparsePlan {
    const uint32_t *off;      // [nq + 1]: query q's dimensions are entries off[q] .. off[q + 1]
    const uint64_t *start;    // posting range of the dimension in the segment's posting layout
    const uint64_t *end;
    const float *w;           // the query's weight of the dimension
};
// the posting layout of a segment whose index weights are f16 / u8 (SparseIndexConfig.datatype): structure of arrays, ids[nnz] and weights[nnz]
// (u16 = f16 bits, or u8 codes of QuantizedU8), grouped by dimension, ids ascending inside a group
struct SparsePostQ {
    const uint32_t *id;
    const void *w;
    uint32_t wtype;           // QMX_SPARSE_WEIGHT_F16 / QMX_SPARSE_WEIGHT_U8
};
// ... and the plan of a batch over it: beside each query weight the QuantizedU8Params (min, diff256) of the dimension's posting list (u8 only)
struct SparsePlanQ {
    const uint32_t *off;
    const uint64_t *start;
    const uint64_t *end;
    const float *w;
    const float *mn;
    const float *d256;
};
uint32_t sparse_tile_ids();
uint32_t sparse_ids_lists(uint64_t n_ids);
// quantized index weights: (min, diff256) of every posting list of the packed layout `post` (dir_start: [n_dims + 1] device), then the encode into
// the structure of arrays
int32_t launch_sparse_post_params(hipStream_t st, const uint64_t *post, const uint64_t *dir_start, uint32_t n_dims, float *mn, float *d256);
int32_t launch_sparse_post_encode(hipStream_t st, const uint64_t *post, const uint64_t *dir_start, uint32_t n_dims, const float *mn, const float *d256,
                                  uint32_t wtype, uint32_t *post_id, void *post_w);
int32_t launch_sparse_topk_postings_q(hipStream_t st, const SparsePostQ &post, const SparsePlanQ &plan, uint32_t q0, uint32_t nq_tile, uint64_t n_scan,
                                      const DeletedView &del, uint32_t top, const uint64_t *key_bound, uint64_t *partial, uint32_t *n_lists);
int32_t launch_sparse_topk_ids_q(hipStream_t st, const SparsePostQ &post, const SparsePlanQ &plan, uint32_t q0, uint32_t nq_tile, const uint32_t *ids,
                                 uint64_t n_ids, uint64_t n_rows, const DeletedView &del, uint32_t top, const uint64_t *key_bound, uint64_t *partial,
                                 uint32_t *n_lists);
// IDF corpus statistics: df[d] += the entries of posting range [start[d], end[d]) whose point `del` lets through (post: the packed u64 layout, or
// post_id when that is null); *n_docs += the points below n_scan that `del` lets through.  df / n_docs are zeroed by the caller.
int32_t launch_sparse_idf_corpus(hipStream_t st, const uint64_t *post, const uint32_t *post_id, const uint64_t *start, const uint64_t *end, uint32_t n_dims,
                                 uint64_t longest, const DeletedView &del, uint64_t n_scan, unsigned long long *df, unsigned long long *n_docs);
int32_t launch_sparse_check_rows(hipStream_t st, const uint64_t *offsets, const uint32_t *idx, uint64_t n, uint32_t *flags);
int32_t launch_sparse_sort_rows(hipStream_t st, const uint64_t *offsets, uint32_t *idx, float *val, uint64_t n);
int32_t launch_sparse_remap(hipStream_t st, uint32_t *idx, uint64_t nnz, const uint32_t *keys, const uint32_t *vals, uint64_t m, uint32_t *missing);
int32_t sparse_build_postings(hipStream_t st, const uint64_t *offsets, const uint32_t *idx, const float *val, uint64_t n, uint64_t nnz, uint64_t *post,
                              uint32_t *dims, uint32_t *counts, uint32_t *n_dims_dev);
int32_t launch_sparse_score_matrix(hipStream_t st, const SparseRows &r, const SparseQueries &qs, uint32_t q0, uint32_t nq, const uint32_t *ids, uint64_t n,
                                   float *scores, uint64_t stride, int *err);
int32_t launch_sparse_score_pairs(hipStream_t st, const SparseRows &r, const SparseQueries &qs, const PairSel &sel, const uint32_t *ids, uint64_t n_items,
                                  float *scores, int *err);
int32_t launch_sparse_score_internal(hipStream_t st, const SparseRows &r, const uint32_t *a, const uint32_t *b, uint64_t n, float *out, int *err);
int32_t launch_sparse_topk_postings(hipStream_t st, const uint64_t *post, const SparsePlan &plan, uint32_t q0, uint32_t nq_tile, uint64_t n_scan,
                                    const DeletedView &del, uint32_t top, const uint64_t *key_bound, uint64_t *partial, uint32_t *n_lists);
int32_t launch_sparse_topk_ids(hipStream_t st, const SparseRows &r, const SparseQueries &qs, uint32_t q0, uint32_t nq_tile, const uint32_t *ids, uint64_t n_ids,
                               const DeletedView &del, uint32_t top, const uint64_t *key_bound, uint64_t *partial, uint32_t *n_lists);
// custom queries over sparse vectors: `ex` / `plan` are the example batch's lists and posting plan in ascending ORIGINAL index order, `desc` and
// `coefs` device arrays (descriptors of the whole request, the feedback coefficients)
uint32_t sparse_custom_tile_ids();
int32_t launch_sparse_custom_score(hipStream_t st, const SparseRows &r, const SparseQueries &ex, const qmx_custom_query *desc, const float *coefs, uint32_t nq,
                                   const uint32_t *ids, uint64_t n, float *scores, int *err);
int32_t launch_sparse_custom_topk_postings(hipStream_t st, const uint64_t *post, const SparsePlan &plan, const qmx_custom_query *desc, const float *coefs,
                                           uint32_t q0, uint32_t nq_tile, uint64_t n_scan, const DeletedView &del, uint32_t top, const uint64_t *key_bound,
                                           uint64_t *partial, uint32_t *n_lists);
int32_t launch_sparse_custom_topk_ids(hipStream_t st, const SparseRows &r, const SparseQueries &ex, const qmx_custom_query *desc, const float *coefs, uint32_t q0,
                                      uint32_t nq_tile, const uint32_t *ids, uint64_t n_ids, const DeletedView &del, uint32_t top, const uint64_t *key_bound,
                                      uint64_t *partial, uint32_t *n_lists);

// hybrid queries (fusion.hip): RRF / DBSF fusion of n_sources top lists per query, one work-group per query
constexpr uint32_t FUSE_MAX_SOURCES = 64;      // the weights travel as a kernel argument
constexpr uint32_t FUSE_MAX_ENTRIES = 8192;    // n_sources * stride per query: two u64 key arrays of that many entries in LDS (128 KiB)
struct FuseArgs {
    const qmx_scored_point *lists;   // [n_sources][nq][stride]
    const uint32_t *counts;          // [n_sources][nq]
    uint32_t n_sources, nq, stride;
    uint32_t kind, rrf_k, n_weights, top;
    float weights[FUSE_MAX_SOURCES];
    qmx_scored_point *out;           // [nq][top]
    uint32_t *out_counts;            // [nq]
};
int32_t launch_fuse_topk(hipStream_t st, const FuseArgs &a);

// MMR re-ranking (mmr.hip): one work-group per request, `limit` selection steps inside one launch
constexpr uint32_t MMR_MAX_CANDIDATES = 4096;  // candidates per request (20 bytes of LDS each, beside the selected row as f32)
struct MmrArgs {
    const void *rows;                // dense f32 / f16 / u8 block
    uint64_t n_rows, row_stride;
    uint32_t dim;
    const qmx_scored_point *cand;    // [nq][stride]
    const uint32_t *counts;          // [nq]
    uint32_t stride;
    const float *rel;                // [nq][stride]: relevance of the candidate at every input position
    float lambda;
    uint32_t limit;
    qmx_scored_point *out;           // [nq][limit]
    uint32_t *out_counts;            // [nq]
    int *err_flag;                   // set to 1 on an out-of-range candidate id
};
int32_t launch_mmr_select(hipStream_t st, int dtype, int distance, const MmrArgs &a, uint32_t nq);

// MMR re-ranking over sparse vectors (sparse_mmr.hip): the same selection, pair scores in ascending ORIGINAL index order
constexpr uint32_t SPARSE_MMR_STAGE_CAP = 6144;   // entries of the staged list (query or picked row) kept in LDS: 12 bytes each beside the 80 KiB of candidates
struct SparseMmrArgs {
    SparseRows rows;                 // the segment's f32 CSR rows (sorted by remapped id)
    SparseQueries qs;                // the batch's lists in ascending original index order (remapped ids)
    const uint32_t *inv_vals;        // non-monotone dimension map: its remapped ids ascending and ...
    const uint32_t *inv_keys;        // ... the original index of each; both null where stored order IS original order
    uint32_t n_inv;
    uint32_t stage_cap;              // min(SPARSE_MMR_STAGE_CAP, the longest row or query)
    uint32_t *spill;                 // [nq][3][spill_stride]: a picked row longer than stage_cap, ranked (mapped segments only), or null
    uint64_t spill_stride;           // the segment's longest row
    const qmx_scored_point *cand;    // [nq][stride]
    const uint32_t *counts;          // [nq]
    uint32_t stride;
    float lambda;
    uint32_t limit;
    qmx_scored_point *out;           // [nq][limit]
    uint32_t *out_counts;            // [nq]
    int *err_flag;                   // set to 1 on an out-of-range candidate id
};
int32_t launch_sparse_mmr_select(hipStream_t st, const SparseMmrArgs &a, uint32_t nq);

// formula rescoring (formula.hip): the tree of a qmx_formula compiled by the host (api_formula.hip) to a linear program for a stack machine over
// f64; jumps carry the reference's short circuits (Mult at a zero factor, Div at a zero numerator)
constexpr uint32_t FORMULA_MAX_DEPTH = 16;     // values on the stack at once: the top in a register, the rest [depth - 1][lane] in LDS
constexpr uint32_t FORMULA_MAX_INSTRS = 4096;
enum FormulaInstrOp : uint32_t {
    FI_CONST = 0,      // push c[0]
    FI_SCORE,          // push $score[a], c[0] where the point has none
    FI_PAYLOAD,        // push number column a; b = has default c[0]
    FI_CONDITION,      // push 1.0 / 0.0 by the bit of condition column a
    FI_GEO,            // push haversine(origin lat c[0] lon c[1], geo column a); b = has default lat c[2] lon c[3]
    FI_DATETIME,       // push seconds of datetime column a; b = has default, c[0] = its seconds
    FI_ADD,            // [x y] -> [x + y]
    FI_MUL_SC,         // [p v] -> v == 0.0 ? [0.0], jump to a : [p * v]
    FI_DIV_SC,         // [l] -> l == 0.0 ? [0.0], jump to a : [l]
    FI_DIV,            // [l r] -> r == 0.0 and b ? [c[0]] : [l / r], which must be finite
    FI_NEG, FI_SQRT, FI_POW, FI_EXP, FI_LOG10, FI_LN, FI_ABS,
    FI_DECAY,          // [x target] -> decay of kind a (qmx_decay_kind) with lambda c[0]
};
struct FormulaInstr {
    uint32_t op, a, b, pad_;
    double c[4];
};
struct FormulaColumnDev {
    uint32_t kind, pad_;              // qmx_payload_kind
    const void *data, *data2;         // NUMBER f64 | GEO lat f64, lon f64 | DATETIME i64 micros | CONDITION u64 bitmap words
    const uint64_t *present, *invalid;
};
struct FormulaProgram {
    const FormulaInstr *instrs;       // device
    uint32_t n_instrs, depth;
    const FormulaColumnDev *cols;     // device
    uint32_t n_cols;
    uint64_t n_points;
};
struct FormulaRescoreArgs {
    FormulaProgram prog;
    const qmx_scored_point *lists;   // [n_sources][nq][stride]
    const uint32_t *counts;          // [n_sources][nq]
    uint32_t n_sources, nq, stride, limit;
    uint32_t has_threshold;
    float threshold;
    qmx_scored_point *out;           // [nq][limit]
    uint32_t *out_counts, *out_status, *out_error_point;   // [nq] each
};
int32_t launch_formula_rescore(hipStream_t st, const FormulaRescoreArgs &a);
struct FormulaEvalArgs {
    FormulaProgram prog;
    const uint32_t *ids;             // [n]
    uint64_t n;
    const float *scores;             // [n_score_vars][n] or null
    const uint8_t *score_missing;    // [n_score_vars][n] or null
    uint32_t n_score_vars;
    double *out_precise;             // [n] or null
    float *out_scores;               // [n] or null
    uint32_t *out_status;            // [n]
};
int32_t launch_formula_eval(hipStream_t st, const FormulaEvalArgs &a);

// grouped search (groups.hip): the aggregator of qmx_group_search and the selection of its fallback pages; the logic both share with the host: group_logic.hpp
struct GroupKeysDev {
    const uint32_t *keys;            // one key per point (offsets == nullptr; padded to a multiple of 4 entries with QMX_GROUP_NONE), or the CSR values
    const uint64_t *offsets;         // [n_points + 1] or nullptr
    uint64_t n_points;
};
struct GroupStats {
    unsigned long long pages;        // pages the aggregator consumed, summed over queries
    uint32_t unfinished;             // queries the last aggregate launch left unfinished
    uint32_t pad_;
};
struct GroupState {                  // per query of the batch
    uint32_t *slot_key;              // [nq][limit]
    uint32_t *slot_cnt;              // [nq][limit]
    uint64_t *slot_hits;             // [nq][limit][group_size] keys (make_key), best first
    uint32_t *n_slots, *n_full;      // [nq]
    uint64_t *bound;                 // [nq] ~0: nothing consumed yet; the last key consumed; 0: the query is done
    GroupStats *stats;
    uint32_t limit, group_size;
};
constexpr uint32_t GROUP_PAGE = MAX_TOP_FAST;     // hits per page
constexpr uint32_t GROUP_MAX_LIMIT = 1024;        // slots per query: what the aggregator and the selection keep in LDS
constexpr uint32_t GROUP_MAX_HITS = 65536;        // limit * group_size
// *bad |= 1 for a key >= n_distinct other than QMX_GROUP_NONE, |= 2 for offsets that decrease
int32_t launch_group_keys_check(hipStream_t st, const uint32_t *keys, uint64_t n_keys, uint32_t n_distinct, const uint64_t *offsets, uint64_t n_points, uint32_t *bad);
// pages : [nq][GROUP_PAGE] ranked hits, counts : [nq]; block b serves query list[b] (b without a list)
int32_t launch_group_aggregate(hipStream_t st, const GroupKeysDev &gk, const GroupState &gs, const qmx_scored_point *pages, const uint32_t *counts,
                               const uint32_t *list, uint32_t n_queries, const float *threshold);
// partial : [blocks][n_queries][GROUP_PAGE] keys of the packed queries list[0 .. n_queries), whose score rows are scores[u * stride + i] for candidate i
int32_t launch_group_select(hipStream_t st, const GroupKeysDev &gk, const GroupState &gs, const float *scores, uint64_t stride, uint64_t n_cand,
                            const uint32_t *ids, const DeletedView &del, const uint32_t *list, uint32_t n_queries, uint32_t blocks, uint64_t *partial);
int32_t launch_group_final(hipStream_t st, const GroupState &gs, uint32_t nq, uint32_t *out_keys, uint32_t *out_sizes, qmx_scored_point *out_hits,
                           uint32_t *out_n_groups);

// the distance matrix API (matrix.hip): the sampler of qmx_sample_points and the gather / finish of qmx_search_matrix; the logic both share with the host: matrix_plan.hpp
struct SampleState;
// one level of the radix select over the keys of the candidates of `del` (its `allowed` is the caller's bitmap): histogram + decision; hist [4096], zero before level 0
int32_t launch_sample_level(hipStream_t st, const DeletedView &del, uint64_t n_words, uint64_t seed, uint32_t level, SampleState *state, uint32_t *hist);
// the candidates at or below state->threshold, ascending, into out[0 .. cap); block_counts : [sample_count_blocks(n_words)] scratch
uint32_t sample_count_blocks(uint64_t n_words);
int32_t launch_sample_write(hipStream_t st, const DeletedView &del, uint64_t n_words, uint64_t seed, const SampleState *state, uint32_t *block_counts,
                            uint32_t *out, uint32_t cap);
// block row i = stored row ids[i] (ids below the rows: the caller validated them) at `pitch` bytes, a multiple of 16, zero behind row_bytes; bit i of `deleted`
// (zeros on entry) set where ids[i] is not live under `del`; positions[i] = i
int32_t launch_matrix_gather(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t row_bytes, const uint32_t *ids, uint32_t n, const DeletedView &del,
                             void *block, uint64_t pitch, uint64_t *deleted, uint32_t *positions);
// f16 rows of 32 and more elements: the same block in the layout of RowF16Avx (matrix_f16.hip) - the SIMD body as whole 128-byte segments of two AVX
// iterations each (matrix_plan.hpp matrix_f16_avx_dim: `block_dim` elements per row), the scalar tail behind them.  Rows and stride: multiples of 2 bytes.
int32_t launch_matrix_gather_f16_avx(hipStream_t st, const void *rows, uint64_t row_stride, uint32_t dim, const uint32_t *ids, uint32_t n, const DeletedView &del,
                                     void *block, uint64_t pitch, uint32_t block_dim, uint64_t *deleted, uint32_t *positions);
// ... and its exact top-k scan: `qt` (1 .. 16, a power of two) queries of such rows per pass, no id list; the sums in the order of the reference's f16 AVX leaf
int32_t launch_scan_f16_avx(hipStream_t st, int distance, int qt, ScanMode mode, const ScanArgs &a, int num_cus, uint32_t *grid_out);
// lists : [n_chunk][top] of the queries at positions c0 .. c0 + n_chunk, idx = position in the sample -> rows c0 .. of out / out_cols [.][limit] and out_counts
int32_t launch_matrix_finish(hipStream_t st, const qmx_scored_point *lists, const uint32_t *counts, uint32_t top, uint32_t c0, uint32_t n_chunk,
                             const uint32_t *sample_ids, uint32_t n_sample, uint32_t limit, qmx_scored_point *out, uint32_t *out_cols, uint32_t *out_counts);

}  // namespace qmx
