// split_common.hpp — what the prefilter scans over an f32 block and its derived copies share (scan_split.hip: the f32 rows and the f16 copies,
// scan_i8copy.hip: the int8 copy, split_select.hip: what reads their candidates; scan_sqw.hip and scan_tq4w.hip take the wave list and the
// uniform pointer): the operand layout, the kernels' arguments, the LDS-DMA copies and the stage barrier, the tile walk (split_tiles.hpp),
// the per-wave candidate list, and the staged scan over a copy (sp_staged_scan).
#pragma once
#include <type_traits>

#include "scan_common.hpp"
#include "split_tiles.hpp"

namespace qmx {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4s __attribute__((ext_vector_type(4)));
typedef int i32x4s __attribute__((ext_vector_type(4)));

constexpr int SP_BM = 256;            // rows per tile
constexpr int SP_QT = 128;            // queries per pass
constexpr int SP_QT_MAX = 256;        // ... of the 256-query shape over the half copy (scan_f16half256_kernel)
constexpr int SP_A_UNITS = SP_BM * 2 * 4;     // 16-byte units of one A chunk buffer (256 rows x {h, l} x 4 k-groups) = 32 KB
constexpr int SP_B_UNITS = SP_QT * 2 * 4;     // ... of one B chunk buffer = 16 KB
// the scans over a derived copy
constexpr int SP3_THREADS = 512;                             // 8 waves (4 row quarters x 2 query halves)
constexpr uint32_t SP_WCAP = 8192;                           // candidates one wave may list per pass (expected: ~270 in the headline's first launch, heavy-tailed rows under the int8 band: thousands; more -> overflow -> the exact scan)
constexpr int SP3_BM = SP_BM;                                // 256 rows per tile: a stage is 32 KiB of rows + 16 KiB of queries
constexpr int SP3_A_UNITS = SP_A_UNITS;
constexpr int SP3_ARING = 3;                                 // row stages in LDS: one being multiplied, two on their way
constexpr int SP4_BM = 128;                                  // the 256-query shape (scan_f16half256_kernel): 128 rows per tile ...
constexpr int SP4_QT = 256;                                  // ... against 256 queries
constexpr uint32_t SP_I8_PROBE = 64;                         // slots per query for the candidates whose exact scores renew the bound after a launch (k <= 64 of them)

// unit index of (16-row or 16-query tile t, half hl, k-group kq, row-in-tile m) inside a chunk buffer
__device__ __forceinline__ uint32_t sp_unit(uint32_t t, uint32_t hl, uint32_t kq, uint32_t m) { return ((t * 2 + hl) * 4 + kq) * 16 + (m ^ (2 * kq)); }

typedef __attribute__((address_space(3))) unsigned char sp_lds_byte;
// 1 KiB of global memory (wave-uniform base, lane i fetches bytes 16 i .. 16 i + 15) straight into LDS at the wave-uniform byte address
// lds_dst (lane i lands at lds_dst + 16 i): no staging registers.  The compiler does not count these loads: the kernel waits for them
// itself (s_waitcnt vmcnt(0) in front of the chunk barrier).
__device__ __forceinline__ void sp_glds16(const unsigned char *src, uint32_t lane_off, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(src), "s"(lds_dst) : "memory");
}

// the same for bytes that one CU reads once (the rows of a copy): non-temporal
__device__ __forceinline__ void sp_glds16_nt(const unsigned char *src, uint32_t lane_off, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(src), "s"(lds_dst) : "memory");
}

// the same without saving m0 (the kernel that uses it declares m0 clobbered: no other user of m0 in it)
__device__ __forceinline__ void sp_glds16_m0(const unsigned char *src, uint32_t lane_off, uint32_t lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(lane_off), "s"(src), "s"(lds_dst) : "memory");   // (m0 is a reserved register: the compiler neither allocates nor tracks it)
}

__device__ __forceinline__ void sp_glds16_m0_nt(const unsigned char *src, uint32_t lane_off, uint32_t lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 nt" : : "v"(lane_off), "s"(src), "s"(lds_dst) : "memory");
}

struct SplitArgs {
    const uint4 *bq;        // split queries, [dim / 32][SP_B_UNITS]
    uint32_t nchunks;       // dim / 32
    uint32_t nq;            // live queries (<= 128)
    float row_scale;        // power of two applied to the rows before the split
    const float *scales;    // device: [1] = accumulator units per score unit, [2] = inverse
    const float *thr;       // [128] candidate threshold, accumulator units
    const uint4 *rows_split; // the pre-split copy of the block (scan_f16pair_kernel), or nullptr
    uint32_t phase;         // scan_f16pair_kernel: 0 = every tile, 1 = tiles 0, 16, 32, ... (the strided sixteenth), 2 = all the others
    uint4 *wlist;           // scan_f16pair_kernel: [waves][wcap] (key lo, key hi, query, 0): candidates in the order each wave met them
    uint32_t *wcnt;         // [waves] entries each wave wanted to append (may run past wcap: overflow)
    uint32_t wcap;
    uint64_t *cand;         // [128][cap] keys (approximate score, row)
    uint32_t *cand_cnt;     // [128] appended (may run past cap: overflow)
    uint32_t cap;
};

// The stage barrier.  NOT __syncthreads(): its workgroup fence makes the compiler wait for every outstanding global load (vmcnt(0)) in front of
// the barrier, which would drain the producers' row stream at every stage (measured: a stage then lasts one loaded HBM round trip, 2.3 us).
// LDS traffic is all that crosses this barrier: wait for this wave's LDS operations, then s_barrier.
__device__ __forceinline__ void sp_stage_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// a wave-uniform address through SGPRs (readfirstlane returns a signed int: the halves are widened as unsigned)
__device__ __forceinline__ const unsigned char *sp_uniform_ptr(uint64_t v) {
    return reinterpret_cast<const unsigned char *>(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
                                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v));
}

// ---- the per-wave candidate list: wlist[list * wcap + i] = (key lo, key hi, query, 0), in the order the wave met its candidates; wcnt[list] = the
// entries the wave wanted to append (it runs past wcap: that is how the reader sees an overflow).  Position = a wave-uniform counter + the lane's
// rank in the ballot: plain stores, nothing that returns.  This type is the format's only writer, sp_regroup_kernel (split_select.hip) its only
// reader: it skips the entries of query 0xFFFFFFFF (withdrawn). ----
struct SpWaveList {
    uint4 *wl;
    uint32_t wcap, count;
    __device__ __forceinline__ SpWaveList(uint4 *wlist, uint32_t wcap_, uint32_t list) : wl(wlist + (uint64_t)list * wcap_), wcap(wcap_), count(0) {}
    static __device__ __forceinline__ uint4 entry(float score, uint32_t row, uint32_t q) {
        const uint64_t key = make_key(score, row);
        return make_uint4((uint32_t)key, (uint32_t)(key >> 32), q, 0u);
    }
    static __device__ __forceinline__ uint4 withdrawn() { return make_uint4(0u, 0u, 0xFFFFFFFFu, 0u); }
    // the lanes of `hits` (a ballot) take the next slots in lane order: a lane's slot (to be used below wcap), then the counter past all of them
    __device__ __forceinline__ uint32_t slot(uint64_t hits) const {
        return count + __builtin_amdgcn_mbcnt_hi((uint32_t)(hits >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hits, 0u));
    }
    __device__ __forceinline__ void advance(uint64_t hits) { count += (uint32_t)__builtin_popcountll(hits); }
    __device__ __forceinline__ void append(bool c, float score, uint32_t row, uint32_t q) {
        const uint64_t hits = __ballot(c);
        if (hits) {
            const uint32_t at = slot(hits);
            if (c && at < wcap) wl[at] = entry(score, row, q);
            advance(hits);
        }
    }
    // an entry whose key a kernel of the scan's own makes afterwards (sqw_finish_kernel, tq4w_finish_kernel): (x, row, query, 0) until then
    __device__ __forceinline__ void append_raw(bool c, uint32_t x, uint32_t row, uint32_t q) {
        const uint64_t hits = __ballot(c);
        if (hits) {
            if (c) {      // (the rank under the lane's own condition: the wide scans' epilogues keep the branch structure they were measured with)
                const uint32_t at = slot(hits);
                if (at < wcap) wl[at] = make_uint4(x, row, q, 0u);
            }
            advance(hits);
        }
    }
    __device__ __forceinline__ void finish(uint32_t *wcnt, uint32_t list, int lane) const {
        if (lane == 0) wcnt[list] = count;
    }
    // a wave with nothing to scan: an empty list
    static __device__ __forceinline__ void none(uint32_t *wcnt, uint32_t list, int lane) {
        if (lane == 0) wcnt[list] = 0;
    }
};
// d_wlists of the scans over a derived copy: [waves] counts, then the lists (256-byte aligned)
inline size_t split_wlists_counts_bytes(int num_cus) { return ((size_t)num_cus * (SP3_THREADS / 64) * 4 + 255) / 256 * 256; }
struct SplitWlists {
    uint32_t *counts;
    uint4 *lists;
    SplitWlists(const void *d_wlists, int num_cus)
        : counts((uint32_t *)d_wlists), lists((uint4 *)((unsigned char *)d_wlists + split_wlists_counts_bytes(num_cus))) {}
};

// ---- the epilogue of a tile of f32 accumulators (the f16 copies' scans; BM = rows per tile): accumulator register j of (mt, nt) = row
// BM tile + 64 wm + 16 mt + 4 kq_r + j, query 64 wn + 16 nt + m_r ----
template <int BM>
__device__ __forceinline__ void sp_f32_epilogue(const f32x4s (&acc)[4][4], const float (&thr)[4], float inv_scale, uint64_t tile, uint32_t wm, uint32_t wn,
                                                uint32_t kq_r, uint32_t m_r, const ScanArgs &a, const SplitArgs &s, SpWaveList &list) {
    const uint32_t row0 = (uint32_t)(tile * BM) + wm * 64 + 4 * kq_r;
    const uint32_t n_rows32 = (uint32_t)a.n_cand;
    // most (wave, tile) pairs hold no candidate once the thresholds bite: one maximum per query tile decides that in 60 instructions
    bool maybe = false;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        float mx = -__builtin_inff();
        bool nan = false;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                mx = __builtin_fmaxf(mx, acc[mt][nt][j]);
                nan = nan || acc[mt][nt][j] != acc[mt][nt][j];
            }
        maybe = maybe || !(mx < thr[nt]) || nan;
    }
    if (!__ballot(maybe)) return;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const uint32_t q = wn * 64 + (uint32_t)nt * 16 + m_r;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = acc[mt][nt][j];
                const uint32_t row = row0 + (uint32_t)mt * 16 + (uint32_t)j;
                list.append(!(v < thr[nt]) && row < n_rows32 && q < s.nq, v * inv_scale, row, q);       // NaN (greatest in OrderedFloat) is a candidate
            }
        }
}

// ---- The staged scan over a derived copy whose tiles are LDS images ([256-row tile][stage][2048 16-byte units]: the f16 pair / half copies, the int8
// copy).  block = 512 threads = 8 waves (4 row quarters x 2 query halves), every wave multiplies and copies; a ring of three stages of rows and of
// Ops::BRING stages of queries.  Ops supplies
//   operand, accum      the matrix instruction's operand (16 bytes of a plane) and accumulator types, and mfma(a, b, c)
//   CROSS               three products per stage - (plane 1, plane 0), (0, 1), (0, 0): a value and its residual - or two: (1, 1), (0, 0): two planes of one value
//   BRING               query stages in LDS: the queries run BRING - 1 stages ahead of the multiplication, the rows two
//   Bounds              the wave's thresholds and scales, load(s, wn, m_r)
//   epilogue(...)       a finished tile's accumulators -> the wave's list
// The kernels stay thin wrappers under their own names. ----
template <int N>
__device__ __forceinline__ uint32_t sp_ring_next(uint32_t slot) {
    if constexpr ((N & (N - 1)) == 0) return (slot + 1) & (N - 1);
    else return slot + 1 == N ? 0 : slot + 1;
}
template <class Ops>
__device__ __forceinline__ void sp_staged_scan(const ScanArgs a, const SplitArgs s) {
    using operand = typename Ops::operand;
    using accum = typename Ops::accum;
    constexpr int BRING = Ops::BRING, WAVES = SP3_THREADS / 64;
    static_assert(BRING == 3 || BRING == 4, "the prologue leaves six copies in flight");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t n_tiles = split_phase_tiles((a.n_cand + SP3_BM - 1) / SP3_BM, s.phase);
    const uint32_t nch = s.nchunks;
    const uint64_t my_tiles = split_block_tiles(n_tiles, blockIdx.x, gridDim.x);
    const SplitTileWalk walk(s.phase);
    if (my_tiles == 0) {
        SpWaveList::none(s.wcnt, blockIdx.x * WAVES + (uint32_t)w, lane);
        return;
    }
    const uint32_t wm = (uint32_t)w & 3u, wn = (uint32_t)w >> 2;
    const uint32_t kq_r = (uint32_t)lane >> 4, m_r = (uint32_t)lane & 15u;
    const uint32_t a_rd = sp_unit(wm * 4, 0, kq_r, m_r), b_rd = sp_unit(wn * 4, 0, kq_r, m_r);
    typename Ops::Bounds bounds;
    bounds.load(s, wn, m_r);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // from here on the kernel counts its vector-memory traffic itself
    const uint32_t lds0 = (uint32_t)(uintptr_t)(sp_lds_byte *)smem_raw;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    uint4 *b_lds = lds + SP3_ARING * SP3_A_UNITS;
    // The copy streams (LDS-DMA, 1 KiB per wave instruction): stage = (tile iteration, K-chunk) in order; per stage a wave copies 4 KiB of the
    // rows (from HBM) and 2 KiB of the queries (from L2).  The vector-memory counter retires in order, so the order of the requests fixes what a
    // wait can mean: at stage g a wave requests [queries of stage g + BRING - 1, rows of stage g + 2] and waits until only those 6 copies are out -
    // then the rows of stage g + 1 (requested a stage ago) and the queries of stage g + BRING - 2 (a stage ago, BEFORE those rows) have landed: every
    // copy has two stages to arrive.  A copy requested and awaited inside one stage makes the stage last a memory round trip (1.1 - 2 us
    // measured, whatever its size).  Requests past the last stage repeat the last one into a slot nobody reads: the count in flight is constant.
    uint64_t ra_it = 0;
    uint32_t ra_kc = 0, ra_slot = 0, rb_kc = 0, rb_slot = 0;
    // one 1 KiB copy each, so that the requests of a stage can sit BETWEEN its matrix instructions (a wave issues in order: six copies in a
    // row in front of the MFMAs keep the matrix pipe idle for ~600 cycles per stage while both waves of the SIMD are busy requesting)
    const unsigned char *ra_src = nullptr, *rb_src = nullptr;
    uint32_t ra_dst = 0, rb_dst = 0;
    auto rows_begin = [&]() {
        const uint64_t tile = walk.tile(blockIdx.x + ra_it * gridDim.x);
        ra_src = sp_uniform_ptr((uint64_t)(uintptr_t)(s.rows_split + (tile * nch + ra_kc) * SP3_A_UNITS) + (uint32_t)w * 4096u);
        ra_dst = lds0 + (ra_slot * SP3_A_UNITS) * 16u + (uint32_t)w * 4096u;
        ra_slot = sp_ring_next<SP3_ARING>(ra_slot);
        if (ra_kc + 1 < nch) ++ra_kc;
        else if (ra_it + 1 < my_tiles) { ra_kc = 0; ++ra_it; }
    };
    // (the rows non-temporal - the copy's lines are read once, whole, by this CU: the int8 scan 0.645 - 0.652 ms per launch against 0.661 - 0.670 with the
    // default policy; the queries' slices, which every block re-reads from L2, keep it)
    auto rows_piece = [&](int i) { sp_glds16_nt(ra_src + i * 1024, lane_off, ra_dst + i * 1024); };
    auto queries_begin = [&]() {
        rb_src = sp_uniform_ptr((uint64_t)(uintptr_t)(s.bq + (uint64_t)rb_kc * SP_B_UNITS) + (uint32_t)w * 2048u);
        rb_dst = lds0 + (SP3_ARING * SP3_A_UNITS + rb_slot * SP_B_UNITS) * 16u + (uint32_t)w * 2048u;
        rb_slot = sp_ring_next<BRING>(rb_slot);
        rb_kc = rb_kc + 1 == nch ? 0 : rb_kc + 1;
    };
    auto queries_piece = [&](int i) { sp_glds16(rb_src + i * 1024, lane_off, rb_dst + i * 1024); };
    auto request_rows = [&]() {
        rows_begin();
#pragma unroll
        for (int i = 0; i < 4; ++i) rows_piece(i);
    };
    auto request_queries = [&]() {
        queries_begin();
        queries_piece(0);
        queries_piece(1);
    };
    // the prologue: queries of stages 0 .. BRING - 2, rows of stages 0 and 1, each stage's queries in front of its rows
    if constexpr (BRING == 4) request_queries();          // queries of stage 0
    request_queries();                                    // ... of the next stage
    request_rows();                                       // rows of stage 0
    request_queries();
    request_rows();                                       // rows of stage 1
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");      // all but the last six: the rows of stage 0 and the queries in front of them have landed
    sp_stage_barrier();
    uint32_t slot = 0, bslot = 0;
    accum acc[4][4];
    // Candidates go to a list of this wave's own (SpWaveList): plain stores, nothing
    // that RETURNS - a returning operation (an atomic slot, a deleted-flag lookup) can only be awaited together with every copy requested
    // before it (the counter retires in order), i.e. it drains the two-stage prefetch: ~2 us per tile with a hit, 0.4 ms per pass at 128
    // queries.  The tile's epilogue therefore also runs at the TOP of the next stage, in front of that stage's requests: the wait at the end
    // of a stage leaves exactly the stage's own six copies out, stores included or not.  sp_regroup_kernel sorts the lists by query afterwards
    // (and drops deleted rows).
    SpWaveList list(s.wlist, s.wcap, blockIdx.x * WAVES + (uint32_t)w);
    auto epilogue = [&](uint64_t tile) __attribute__((always_inline)) { Ops::epilogue(acc, bounds, tile, wm, wn, kq_r, m_r, a, s, list); };
    for (uint64_t it = 0; it < my_tiles; ++it) {
        if (it) epilogue(walk.tile(blockIdx.x + (it - 1) * gridDim.x));
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = (accum){0, 0, 0, 0};
        for (uint32_t kc = 0; kc < nch; ++kc) {
            queries_begin();                              // stage g + BRING - 1 -> the slot stage g - 1 was read from (everybody is past that barrier)
            rows_begin();                                 // stage g + 2 -> likewise
            const uint4 *ab = lds + slot * SP3_A_UNITS + a_rd;
            const uint4 *bb = b_lds + bslot * SP_B_UNITS + b_rd;
            operand b0[4], b1[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                b0[nt] = *reinterpret_cast<const operand *>(bb + nt * 128);
                b1[nt] = *reinterpret_cast<const operand *>(bb + nt * 128 + 64);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const operand a0 = *reinterpret_cast<const operand *>(ab + mt * 128);
                const operand a1 = *reinterpret_cast<const operand *>(ab + mt * 128 + 64);
                // CROSS (planes = high and low parts): x y = h h' + h l' + l h' (small terms first); else the two planes are the two halves of the stage's coordinates
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = Ops::mfma(a1, Ops::CROSS ? b0[nt] : b1[nt], acc[mt][nt]);
                // the stage's six copy requests, in the order the wait below relies on (queries first), spread over the matrix work
                if (mt == 0) queries_piece(0);
                if (mt == 1) queries_piece(1);
                if (mt == 2) { rows_piece(0); rows_piece(1); }
                if (mt == 3) { rows_piece(2); rows_piece(3); }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (Ops::CROSS) {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = Ops::mfma(a0, b1[nt], acc[mt][nt]);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = Ops::mfma(a0, b0[nt], acc[mt][nt]);
            }
            slot = sp_ring_next<SP3_ARING>(slot);
            bslot = sp_ring_next<BRING>(bslot);
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");     // all but this stage's six requests have landed: rows and queries of stage g + 1 among them
            sp_stage_barrier();
        }
    }
    epilogue(walk.tile(blockIdx.x + (my_tiles - 1) * gridDim.x));
    list.finish(s.wcnt, blockIdx.x * WAVES + (uint32_t)w, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // nothing may land in LDS after the block is gone
}

}  // namespace qmx
