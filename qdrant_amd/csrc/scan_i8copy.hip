// scan_i8copy.hip — the int8 copy of an f32 dot / cosine block and the prefilter passes over it.  In the file's order: column and row statistics and
// the copy (once per segment; split_i8_choose_scales further down picks the columns' scales), sp_i8_pack_kernel (once per 128-query tile), the staged
// scan (scan_i8copy_kernel: sp_staged_scan of split_common.hpp with the int8 instruction), the scans with the queries resident in LDS
// (scan_i8copy_kernel_res / _res_dense), the bound after a launch, the sample scan with its picks and bound ("launch 0"), and the launchers.
// The lists these scans write are regrouped, probed and selected by split_select.hip.
#include "split_common.hpp"

namespace qmx {

// =====================================================================================================================================
// The INT8 copy (QMX_SEG_I8_COPY): one byte per element, the same LDS images, the same staging - half the bytes of the half copy per query.
//   rows     x_i = s_i (c_i + e_i),  s_i = max_r |x_ri| / 127 (one scale per COLUMN: an outlier coordinate costs the others nothing, and the
//            scale folds into the query), c_i = rint(x_i / s_i) in [-127, 127], |e_i| <= 1/2
//   queries  q_i s_i = t (d_i + f_i),  t = max_i |q_i s_i| / 127 (one scale per QUERY), d_i = rint(q_i s_i / t), |f_i| <= 1/2
//   score    sum x_i q_i = t [ sum c_i d_i  +  sum c_i f_i + sum e_i d_i + sum e_i f_i ]
// The first sum is the integer the matrix cores deliver (v_mfma_i32_16x16x64_i8, exact); the other three are bounded, worst case, by
//   band_q = t [ min(C1 / 2, C2 |f|_2) + (sum |d_i|) / 2 + dim / 4 ],   C1 = max_r sum_i |c_ri|,  C2 = max_r |c_r|_2   (taken once per segment)
// (+ the round-off of the f32 evaluation the exact scores carry).  On unit Gaussian rows that is ~0.7 standard deviations of the score - two
// orders above the error that really occurs, the price of a bound nobody can break - so the pass works with EXACT lower bounds T_q of the
// k-th best score instead of approximate ones: a row of the result has an approximate score >= T_q - band_q (one band, not two).  T_q comes from
// the sample first (the exact scores of its k best rows by int8 score - "launch 0", scan_i8copy_sample_kernel; option i8_sample_scan = 0: the exact scores
// of a strided row sample), then - after each of the two launches - from the exact scores of the k best candidates so far
// (sp_i8_probe_kernel, the gather kernel of qmx_rescore, sp_i8_bound_kernel): ~a few hundred rows per query are re-scored at the end.
// Everything else (per-wave candidate lists, regroup, verification, per-query exact fallback) is the f16 path's.
// =====================================================================================================================================
constexpr uint32_t SP_I8_MAX_DIM = 4096;                     // (sp_i8_colmax_kernel keeps a column maximum per thread and 256 columns)

// column maxima and sums of squares: colmax[c] = max_r |x_rc| (uint bits of a non-negative float order like the float), colsq[c] = sum_r x_rc^2 (f32, a
// statistic that only steers the choice of the scales); thread t owns columns t, t + 256, ...
__global__ __launch_bounds__(256) void sp_i8_colmax_kernel(const unsigned char *rows, uint64_t row_stride, uint64_t n, uint32_t dim, uint32_t *colmax, float *colsq) {
    float mx[SP_I8_MAX_DIM / 256], sq[SP_I8_MAX_DIM / 256];
#pragma unroll
    for (int j = 0; j < (int)(SP_I8_MAX_DIM / 256); ++j) { mx[j] = 0.0f; sq[j] = 0.0f; }
    for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const float *v = reinterpret_cast<const float *>(rows + r * row_stride);
#pragma unroll
        for (int j = 0; j < (int)(SP_I8_MAX_DIM / 256); ++j) {
            const uint32_t c = threadIdx.x + 256u * (uint32_t)j;
            if (c < dim) {
                const float x = v[c];
                mx[j] = __builtin_fmaxf(mx[j], __builtin_fabsf(x));
                sq[j] = __builtin_fmaf(x, x, sq[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < (int)(SP_I8_MAX_DIM / 256); ++j) {
        const uint32_t c = threadIdx.x + 256u * (uint32_t)j;
        if (c < dim) {
            atomicMax(&colmax[c], __float_as_uint(mx[j]));
            atomicAdd(&colsq[c], sq[j]);
        }
    }
}
__device__ __forceinline__ int sp_i8_code(float x, float s) {
    int c = (int)__builtin_rintf(x / s);
    return c > 127 ? 127 : (c < -127 ? -127 : c);
}
// stats[0] = C1 = max_r sum |c_ri|, stats[1] = C2^2 = max_r sum c_ri^2, stats[2] != 0: an element that is not finite (no int8 copy for this block)
__global__ __launch_bounds__(256) void sp_i8_row_stats_kernel(const unsigned char *rows, uint64_t row_stride, uint64_t n, uint32_t dim, const float *scale,
                                                              uint32_t *stats) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    uint32_t m1 = 0, m2 = 0;
    bool bad = false;
    for (uint64_t r = wave; r < n; r += nwaves) {
        const float *v = reinterpret_cast<const float *>(rows + r * row_stride);
        uint32_t c1 = 0, c2 = 0;
        for (uint32_t i = lane; i < dim; i += 64) {
            const float x = v[i];
            bad = bad || !(__builtin_fabsf(x) < __builtin_inff());
            const int c = sp_i8_code(x, scale[i]);
            c1 += (uint32_t)(c < 0 ? -c : c);
            c2 += (uint32_t)(c * c);
        }
        for (int o = 32; o >= 1; o >>= 1) {
            c1 += __shfl_xor(c1, o, 64);
            c2 += __shfl_xor(c2, o, 64);
        }
        m1 = c1 > m1 ? c1 : m1;
        m2 = c2 > m2 ? c2 : m2;
    }
    if (lane == 0) {
        atomicMax(&stats[0], m1);
        atomicMax(&stats[1], m2);
    }
    if (bad) atomicOr(&stats[2], 1u);
}
// the copy: one thread per 16-coordinate unit of the OUTPUT, out[(tile * nch + k128) * 2048 + unit(row, plane = which 64 of the 128, kq)], in the output's
// order - a wave writes 1 KiB of consecutive units (whole lines: the row-major order of round 3 wrote 13.3 GB for a 7.68 GB copy, profiles/
// r3_pmc_traffic_i8.md) and reads sixteen rows' 256-byte runs; rows past n are zero
__global__ __launch_bounds__(256) void sp_i8_copy_kernel(const unsigned char *rows, uint64_t row_stride, uint64_t n, uint32_t dim, const float *scale, uint4 *out) {
    const uint32_t nch = dim / 128;
    const uint64_t n_tiles = (n + SP3_BM - 1) / SP3_BM;
    const uint64_t total = n_tiles * nch * SP3_A_UNITS;
    for (uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (uint64_t)gridDim.x * 256) {
        const uint32_t u = (uint32_t)(gid % SP3_A_UNITS);
        const uint64_t blk = gid / SP3_A_UNITS, tile = blk / nch;
        const uint32_t k128 = (uint32_t)(blk % nch);
        // sp_unit(t, hl, kq, m) = ((t * 2 + hl) * 4 + kq) * 16 + (m ^ 2 kq), inverted
        const uint32_t kq = (u >> 4) & 3u, hl = (u >> 6) & 1u, t = u >> 7, m = (u & 15u) ^ (2u * kq);
        const uint64_t r = tile * SP3_BM + t * 16u + m;
        const uint32_t g = k128 * 8u + hl * 4u + kq;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (r < n) {
            const float *v = reinterpret_cast<const float *>(rows + r * row_stride) + g * 16;
            const float *sc = scale + g * 16;
#pragma unroll
            for (int e = 0; e < 16; ++e) w[e / 4] |= ((uint32_t)sp_i8_code(v[e], sc[e]) & 0xFFu) << (8 * (e % 4));
        }
        out[gid] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ---- once per 128-query tile: one block per query slot.  The query in the columns' scales, its own scale, its codes in the B-operand images
// (bq[k128][unit(query, plane, kq)], zeros past nq), its band, its first threshold (from the sample's exact k-th best score) ----
__device__ __forceinline__ float sp_block_max(float v, float *sh) {
    for (int o = 32; o >= 1; o >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return __builtin_fmaxf(__builtin_fmaxf(sh[0], sh[1]), __builtin_fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ float sp_block_sum(float v, float *sh) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__global__ __launch_bounds__(256) void sp_i8_pack_kernel(const float *q, uint32_t nq, uint32_t dim, const float *scale, const uint64_t *gthr,
                                                         const uint32_t *row_stats, float row_norm_max, uint4 *bq, float *qscale, float *band, float *thr,
                                                         float *t_exact, uint32_t *cand_cnt, uint32_t n_cnt) {
    extern __shared__ __attribute__((aligned(16))) float sh_q[];      // the query in the columns' scales
    __shared__ float sh_red[4];
    const uint32_t qi = blockIdx.x;
    const bool live = qi < nq;
    if (qi == 0)
        for (uint32_t i = threadIdx.x; i < n_cnt; i += 256) cand_cnt[i] = 0;
    float mx = 0.0f, ss = 0.0f, bad = 0.0f;
    for (uint32_t i = threadIdx.x; i < dim; i += 256) {
        const float raw = live ? q[(uint64_t)qi * dim + i] : 0.0f;
        const float v = raw * scale[i];
        sh_q[i] = v;
        mx = __builtin_fmaxf(mx, __builtin_fabsf(v));
        ss = __builtin_fmaf(raw, raw, ss);
        if (!(__builtin_fabsf(v) < __builtin_inff())) bad = 1.0f;
    }
    mx = sp_block_max(mx, sh_red);
    ss = sp_block_sum(ss, sh_red);
    bad = sp_block_max(bad, sh_red);                                  // (the barriers inside also publish sh_q)
    const float t = mx > 1.0e-30f ? mx / 127.0f : 1.0f;
    float sabs = 0.0f, sf2 = 0.0f;                                    // sum |d_i| (an integer below 2^24: exact in f32), sum f_i^2
    for (uint32_t u = threadIdx.x; u < dim / 16; u += 256) {
        const uint32_t k128 = u / 8, hl = (u / 4) & 1u, kq = u % 4;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float x = sh_q[u * 16 + e] / t;
            float c = __builtin_rintf(x);
            c = c > 127.0f ? 127.0f : (c < -127.0f ? -127.0f : c);
            if (!(c == c)) c = 0.0f;
            const float f = x - c;
            sabs += __builtin_fabsf(c);
            sf2 = __builtin_fmaf(f, f, sf2);
            w[e / 4] |= ((uint32_t)(int)c & 0xFFu) << (8 * (e % 4));
        }
        bq[(uint64_t)k128 * SP_B_UNITS + sp_unit(qi >> 4, hl, kq, qi & 15u)] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    sabs = sp_block_sum(sabs, sh_red);
    sf2 = sp_block_sum(sf2, sh_red);
    if (threadIdx.x != 0) return;
    if (!live) {
        qscale[qi] = 0.0f;
        band[qi] = 0.0f;
        thr[qi] = __builtin_inff();
        t_exact[qi] = -__builtin_inff();
        return;
    }
    const float c1 = (float)row_stats[0], c2 = __builtin_sqrtf((float)row_stats[1]);
    const float cf = __builtin_fminf(0.5f * c1, c2 * __builtin_sqrtf(sf2));
    // (1.001: the roundings of x / s, q s, q s / t and of this sum; the last term: the f32 evaluation of the exact score, dim 2^-23 |q| |row|, twice)
    const float b = t * (cf + 0.5f * sabs + 0.25f * (float)dim) * 1.001f + 2.0f * (float)dim * 1.1920929e-7f * row_norm_max * __builtin_sqrtf(ss);
    // gthr == nullptr (option i8_sample_scan): the pack runs FIRST and the sample's bound comes after it, from the int8 copy itself
    // (scan_i8copy_sample_kernel ... sp_i8_sample_bound_kernel): the band of a finite query is finite, nothing is admitted yet
    const uint64_t k = gthr ? gthr[qi] : 0;
    const bool finite = bad == 0.0f && b < 3.0e38f;
    const bool ok = finite && k != 0;
    // no bound (the sample holds fewer than k live rows) or a query that is not finite: no candidates, and the infinite band sends the query - alone -
    // to the exact scan
    qscale[qi] = t;
    band[qi] = (gthr ? ok : finite) ? b : __builtin_inff();
    t_exact[qi] = ok ? key_score(k) : -__builtin_inff();
    thr[qi] = ok ? (key_score(k) - b) / t : __builtin_inff();
}

// The staged scan: sp_staged_scan (split_common.hpp) with the int8 instruction and two products, as scan_f16pair_kernel<true> has them.  A stage is 256 rows x 128 coordinates (two planes of 64) = 32 KiB of rows + 16 KiB of
// queries, 32 matrix instructions per wave as there; nch = dim / 128 stages per tile.  s.scales = the queries' scales (score units per accumulator
// unit), s.thr in accumulator units.
// SP8_BRING = 3 query stages in LDS: the queries of stage g + 2 are requested during stage g (the 96 KiB of query images stay in L2: 2.9 us ahead is plenty),
// 96 + 48 = 144 KiB - which leaves 16 KiB of every CU's LDS to the OTHER batches' small kernels (regroup, probe, exact gather, bound, select, sort, pack ...):
// they run beside this scan instead of queueing behind it.  Rounds 3 - 5 kept four stages (160 KiB, the CU's whole LDS: nothing that needs LDS could start
// on a CU while a block of the scan lived there); measured in round 6 (C2, 128 queries per step; profiles/r6_i8_lanes_experiment.txt): 2 / 3 / 4 batches in
// flight 87.5 / 88.1 / 88.6 k QPS with 160 KiB, 88.3 / 90.0 / 91.4 k with 144 KiB.
constexpr int SP8_BRING = 3;
constexpr int SP8_LDS = (SP3_ARING * SP3_A_UNITS + SP8_BRING * SP_B_UNITS) * 16;
struct I8CopyOps {
    using operand = i32x4s;
    using accum = i32x4s;
    static constexpr bool CROSS = false;
    static constexpr int BRING = SP8_BRING;
    static __device__ __forceinline__ accum mfma(operand x, operand y, accum c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(x, y, c, 0, 0, 0); }
    struct Bounds {
        float thr[4], qs[4];      // per query: the threshold (accumulator units), the scale (score units per accumulator unit)
        __device__ __forceinline__ void load(const SplitArgs &s, uint32_t wn, uint32_t m_r) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                thr[nt] = s.thr[wn * 64 + nt * 16 + m_r];
                qs[nt] = s.scales[wn * 64 + nt * 16 + m_r];
            }
        }
    };
    // The epilogue of a tile.  With a band of 0.7 standard deviations a wave meets ~2 candidates per tile (the f16 passes: 0.4), so nearly every tile
    // has one somewhere: the search for them narrows by wave-uniform steps - the query tile (16 queries x the wave's 64 rows), then the 16-row tile, then
    // the four rows of a lane - instead of testing all 256 accumulators of a lane one ballot at a time (14 % of the kernel at 128 queries, measured
    // against the same launch with one live query).
    static __device__ __forceinline__ void epilogue(const accum (&acc)[4][4], const Bounds &b, uint64_t tile, uint32_t wm, uint32_t wn, uint32_t kq_r, uint32_t m_r,
                                                    const ScanArgs &a, const SplitArgs &s, SpWaveList &list) {
        const uint32_t row0 = (uint32_t)(tile * SP3_BM) + wm * 64 + 4 * kq_r;
        const uint32_t n_rows32 = (uint32_t)a.n_cand;
        bool hit[4];
        bool maybe = false;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            int mx = acc[0][nt][0];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int j = 0; j < 4; ++j) mx = acc[mt][nt][j] > mx ? acc[mt][nt][j] : mx;
            hit[nt] = !((float)mx < b.thr[nt]);
            maybe = maybe || hit[nt];
        }
        if (!__ballot(maybe)) return;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            if (!__ballot(hit[nt])) continue;
            const uint32_t q = wn * 64 + (uint32_t)nt * 16 + m_r;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                int m4 = acc[mt][nt][0];
#pragma unroll
                for (int j = 1; j < 4; ++j) m4 = acc[mt][nt][j] > m4 ? acc[mt][nt][j] : m4;
                if (!__ballot(!((float)m4 < b.thr[nt]))) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = (float)acc[mt][nt][j];
                    const uint32_t row = row0 + (uint32_t)mt * 16 + (uint32_t)j;
                    list.append(!(v < b.thr[nt]) && row < n_rows32 && q < s.nq, v * b.qs[nt], row, q);
                }
            }
        }
    }
};
__global__ __launch_bounds__(SP3_THREADS, 1) void scan_i8copy_kernel(const ScanArgs a, const SplitArgs s) {
    sp_staged_scan<I8CopyOps>(a, s);
}

// Other structures of this scan were built in round 4 and measured slower - half stages with 80 KiB of rows in flight per CU (14 % slower: twice the
// barriers), wave-owned rows behind private rings with no stage hand-over (5 % slower), rows straight into the operand registers - and are gone from the
// code since round 6; the measurements stay (profiles/r4_i8_deep_ring.md).

// ---- The same scan with the queries' WHOLE operand image resident in LDS (round 6, last session; the structure scan_sqw.hip found for the scalar-int8 block,
// on this copy's tiled layout).  Rows up to 1 024 coordinates: nch x 16 KiB of query images (96 KiB at 768) + 1 KiB of thresholds and scales, copied once per
// block; after that copy the waves share nothing: no stage barrier, no LDS ring of rows.  A wave OWNS row tiles 2 w and 2 w + 1 of a 256-row tile: their operand
// images are the 4 KiB [4 w KiB, + 4 KiB) of every 32 KiB stage of the copy (sp_unit: ((t * 2 + hl) * 4 + kq) * 16 + swizzle(m) - a lane's 16 bytes sit at one
// lane-constant offset inside each 1 KiB image), so a stage is four `global_load_dwordx4` of 1 KiB each, contiguous, INTO the matrix instruction's operand
// registers, issued AHEAD stages in front of the matrix work and waited for by the kernel's own vmcnt (in-order); per stage and wave 32 matrix instructions
// against all 128 queries and 16 operand reads.  Same integers, same thresholds, same candidates as scan_i8copy_kernel (which stays for longer rows and as option
// i8_resident = 0); LDS per CU 97 KiB instead of 144, 2 waves and 320 registers per SIMD: a block of another batch in flight starts beside a scan block when it
// needs at most 64 512 B of LDS and 192 registers per SIMD.  The sample's exact scores did NOT, whatever this comment said until round 15: their 32-query tile
// is 105 KiB at 768 coordinates (8 waves at 176 registers), and the 1024-thread top-k behind them holds 64 KiB of keys; both waited for a CU without a scan
// block.  With option prescan_beside_scan (default 1) they run as a 16-query tile of 52.5 KiB on 4 waves at 192 registers (scan_mfma.hip launch_scan_f32_mfma_beside) and a
// 256-thread top-k with 16 KiB (custom_query.hip custom_topk_beside_kernel), which do; profiles/r15_step_footprint.md lists every kernel of the step. ----
constexpr uint32_t SP8R_MAX_NCH = 8;
__host__ __device__ constexpr size_t sp8r_lds_bytes(uint32_t nch) { return (size_t)nch * SP_B_UNITS * 16 + 2 * SP_QT * 4; }
// (non-temporal: every line of the copy is read once per pass, by one CU, whole - a load instruction covers 1 KiB of consecutive bytes; with plain loads the same
// kernel ran at 0.68 ms per launch instead of 0.61 - 0.63, the step at 90.3 - 90.9 k QPS instead of 96.5 - 97.2 k: profiles/r6_i8_resident.md)
template <int OFF>
__device__ __forceinline__ void sp_gload16(i32x4s &dst, const unsigned char *sbase, uint32_t voff) {
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3 nt" : "=v"(dst) : "v"(voff), "s"(sbase), "n"(OFF) : "memory");
}
template <int I, int N, class F>
__device__ __forceinline__ void sp_static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        sp_static_for<I + 1, N>(f);
    }
}
// Measured and gone from the code (profiles/r6_i8_resident.md): two / three stages of loads ahead (equal or slower: 170 / 200 registers), four row tiles per wave -
// waves 0 - 3 on the block's even tiles, 4 - 7 on its odd ones: half the operand reads per matrix instruction, 250 registers - (equal), a block's tiles consecutive
// instead of every gridDim-th (equal).  Ablation (wrong results, the same launches): without the matrix instructions and operand reads 0.628 ms per launch
// instead of 0.68 - 0.69, with half of them 0.655: the stream alone - this kernel's loads and waits - is 0.76 of HBM, the matrix work costs 9 %.
//
// DENSE: the epilogue of the FIRST launch (the strided sixteenth of the tiles, admitted on the sample's bound: ~1 % of a wave's 4 096 (row, query) pairs per
// tile pass, ~28 candidates per wave and tile on the headline against 0.2 in the second launch).  The narrowing epilogue below visits a query tile's eight (row
// tile, row) slots one ballot and one branch at a time - right where nearly every ballot is empty, as long as the tile's stream where a third of them are not
// (~1 500 instructions per wave and tile; the dense one ~620, first launch 0.121 -> 0.098 ms: profiles/r14_i8_dense_epilogue.md).  The dense one
// takes, per query tile, an 8-bit hit mask per lane (the same test on integers, sp_i8_int_threshold), and hands out the wave's slots one LEVEL at a time - every
// lane's first hit, then every lane's second, ... - by one ballot per level: a level costs what one slot with a hit costs below, and there are as many levels as
// the fullest lane has hits (one, rarely two; eight at most).  The same set of entries per launch, in another order inside a wave's list (regroup, probe and select
// do not look at the order); the list's count goes on past `wcap` as below, which is how sp_regroup_kernel sees an overflow.  One copy of the epilogue in the kernel
// instead of three: the loop runs over stages and meets the tile's end in one place.
// A pair is a candidate unless (float)acc < th.  |acc| <= 1 024 x 128 x 128 = 2^24 is exact in f32, so for a finite th that is acc >= ceil(th); !(x < NaN) holds
// for every x; a query slot past nq admits nothing.  The integer stays within +-2^30, so that acc - threshold cannot wrap: its sign bit is the test.
__device__ __forceinline__ int sp_i8_int_threshold(float th, bool live_query) {
    constexpr int NOTHING = 1 << 30, EVERYTHING = -(1 << 30);
    if (!live_query) return NOTHING;
    if (!(th > -1.0e9f)) return EVERYTHING;               // NaN, -inf, anything below every accumulator
    if (th > 1.0e9f) return NOTHING;
    return (int)ceilf(th);
}
template <int AHEAD, bool DENSE>
__device__ __forceinline__ void sp_i8copy_res_scan(const ScanArgs a, const SplitArgs s) {
    constexpr int SLOTS = AHEAD + 1, WAVES = SP3_THREADS / 64, THREADS = SP3_THREADS, MT = 2, NL = 2 * MT;
    static_assert(SP3_BM == WAVES * MT * 16, "a wave owns two row tiles of a 256-row tile");
    static_assert(NL * AHEAD <= 62, "vmcnt is six bits");
    static_assert(SP8R_MAX_NCH * 128u * 128u * 128u <= (1u << 24), "the dense epilogue compares integers: every accumulator is exact in f32");
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
    const uint32_t ws = (uint32_t)w;
    auto my_tile = [&](uint64_t i) -> uint64_t { return walk.tile(blockIdx.x + i * gridDim.x); };
    float *thr_lds = reinterpret_cast<float *>(smem_raw + (size_t)nch * SP_B_UNITS * 16), *qs_lds = thr_lds + SP_QT;
#pragma unroll 4
    for (uint32_t u = (uint32_t)tid; u < nch * SP_B_UNITS; u += THREADS) lds[u] = s.bq[u];
    for (int u = tid; u < SP_QT; u += THREADS) {
        if constexpr (DENSE) thr_lds[u] = __int_as_float(sp_i8_int_threshold(s.thr[u], (uint32_t)u < s.nq));
        else thr_lds[u] = s.thr[u];
        qs_lds[u] = s.scales[u];
    }
    __syncthreads();
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // from here on the kernel counts its vector-memory traffic itself
    const uint32_t kq_r = (uint32_t)lane >> 4, m_r = (uint32_t)lane & 15u;
    const uint32_t lane_unit = kq_r * 16u + (m_r ^ (2u * kq_r));      // sp_unit(0, 0, kq_r, m_r)
    const uint4 *const b_rd = lds + lane_unit;
    const uint32_t lane_off = lane_unit * 16u;
    // one stage's 2 MT loads: the images (row tile MT w + mt, plane hl) of stage kc of a tile -> rc[mt * 2 + hl]
    auto load_stage = [&](uint64_t tile, uint32_t kc, i32x4s (&rc)[NL]) __attribute__((always_inline)) {
        const unsigned char *src = sp_uniform_ptr((uint64_t)(uintptr_t)(s.rows_split + (tile * nch + kc) * SP3_A_UNITS) + ws * (NL * 1024u));
        sp_gload16<0>(rc[0], src, lane_off);
        sp_gload16<1024>(rc[1], src, lane_off);
        sp_gload16<2048>(rc[2], src, lane_off);
        sp_gload16<3072>(rc[3], src, lane_off);
    };
    i32x4s acc[MT][8];
    SpWaveList list(s.wlist, s.wcap, blockIdx.x * WAVES + (uint32_t)w);
    const uint32_t n_rows32 = (uint32_t)a.n_cand;
    // the epilogue of a tile: scan_i8copy_kernel's test (a pair is a candidate unless its accumulator is below the query's threshold), narrowing by
    // wave-uniform steps: the query tile, then the lane's 4 MT rows
    auto epilogue = [&](uint64_t tile) __attribute__((always_inline)) {
        const uint32_t row0 = (uint32_t)(tile * SP3_BM) + ws * (MT * 16u) + 4 * kq_r;
        uint32_t hits8 = 0;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            int mx = acc[0][nt][0];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int j = 0; j < 4; ++j) mx = acc[mt][nt][j] > mx ? acc[mt][nt][j] : mx;
            if (!((float)mx < thr_lds[nt * 16 + (int)m_r])) hits8 |= 1u << nt;
        }
        if (!__ballot(hits8 != 0)) return;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            if (!__ballot((hits8 >> nt) & 1u)) continue;
            const uint32_t q = (uint32_t)nt * 16 + m_r;
            const float th = thr_lds[q], qs = qs_lds[q];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = (float)acc[mt][nt][j];
                    const uint32_t row = row0 + (uint32_t)mt * 16 + (uint32_t)j;
                    list.append(!(v < th) && row < n_rows32 && q < s.nq, v * qs, row, q);
                }
            }
        }
    };
    // the dense epilogue (DENSE; thr_lds holds sp_i8_int_threshold's integers).  Bit 4 mt + j of a lane's mask is row row0 + 16 mt + j.
    auto epilogue_dense = [&](uint64_t tile) __attribute__((always_inline)) {
        static_assert(MT == 2, "a lane's hit mask is eight bits: two row tiles of four rows");
        const uint32_t row0 = (uint32_t)(tile * SP3_BM) + ws * (MT * 16u) + 4 * kq_r;
        uint32_t rows_there = 0xFFu;
        if ((tile + 1) * SP3_BM > a.n_cand) {                        // (the block's last tile, when it is ragged)
            rows_there = 0;
#pragma unroll
            for (int b = 0; b < 8; ++b) rows_there |= row0 + (uint32_t)(b >> 2) * 16 + (uint32_t)(b & 3) < n_rows32 ? 1u << b : 0u;
        }
        const int *const ith_lds = reinterpret_cast<const int *>(thr_lds);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const uint32_t q = (uint32_t)nt * 16 + m_r;
            const int ith = ith_lds[q];
            // the misses' bits: the sign of acc - threshold, shifted in from the right, row 7 first (two instructions per accumulator, no condition code)
            uint32_t miss = 0;
#pragma unroll
            for (int b = 7; b >= 0; --b) miss = __builtin_amdgcn_alignbit(miss, (uint32_t)(acc[b >> 2][nt][b & 3] - ith), 31);
            uint32_t m = ~miss & rows_there;
            uint64_t level = __ballot(m != 0);
            if (!level) continue;                                    // nobody in the wave has a hit for these 16 queries
            const float qs = qs_lds[q];
            do {                                                     // every lane's lowest remaining hit
                const uint32_t at = list.slot(level);
                if (m != 0 && at < list.wcap) {
                    // accumulator h of the lane's eight: a tree of seven bitwise selects under the three bits of h (as `?:` the compiler sees an
                    // indexed vector element and spends fourteen conditional moves and seven compares on it)
                    const uint32_t h = (uint32_t)__builtin_ctz(m);
                    const int h0 = -(int)(h & 1u), h1 = -(int)((h >> 1) & 1u), h2 = -(int)(h >> 2);
                    auto pick = [](int mask, int if_clear, int if_set) { return (if_set & mask) | (if_clear & ~mask); };
                    const int x = pick(h1, pick(h0, acc[0][nt][0], acc[0][nt][1]), pick(h0, acc[0][nt][2], acc[0][nt][3]));
                    const int y = pick(h1, pick(h0, acc[1][nt][0], acc[1][nt][1]), pick(h0, acc[1][nt][2], acc[1][nt][3]));
                    const float v = (float)pick(h2, x, y);
                    list.wl[at] = SpWaveList::entry(v * qs, row0 + (h >> 2) * 16 + (h & 3u), q);
                }
                m &= m - 1;
                list.advance(level);
                level = __ballot(m != 0);
            } while (level);
        }
    };
    const uint64_t n_stages = my_tiles * nch;
    // the stage the loads are at, as (tile, kc), by running counters (the walk's tile() divides: once per tile, not per stage); past the block's last stage they
    // repeat it (the waits count loads, not bytes)
    uint64_t itr = 0, tile_r = my_tile(0);
    uint32_t kr = 0;
    auto advance_r = [&]() {
        if (kr + 1 < nch) ++kr;
        else if (itr + 1 < my_tiles) { kr = 0; ++itr; tile_r = my_tile(itr); }
    };
    i32x4s rc[SLOTS][NL];
    sp_static_for<0, AHEAD>([&](auto DC) __attribute__((always_inline)) {
        load_stage(tile_r, kr, rc[decltype(DC)::value]);
        advance_r();
    });
    uint64_t it = 0, tile_c = my_tile(0), tile_done = 0;
    uint32_t kc = 0;
    // one stage; I = g mod SLOTS selects the register sets at compile time
    auto clear_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) acc[mt][nt] = (i32x4s){0, 0, 0, 0};
    };
    auto one_stage = [&](auto IC) __attribute__((always_inline)) {
        constexpr int I = decltype(IC)::value, IL = (I + AHEAD) % SLOTS;
        if constexpr (!DENSE) {
            if (kc == 0) {
                if (it) epilogue(tile_done);
                clear_acc();
            }
        }
        load_stage(tile_r, kr, rc[IL]);                           // stage g + AHEAD -> the register set stage g - 1 ran on
        advance_r();
        asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NL * AHEAD) : "memory");      // all but the last 2 MT AHEAD loads have landed: this stage's among them
        asm volatile("" : "+v"(rc[I][0]), "+v"(rc[I][1]), "+v"(rc[I][2]), "+v"(rc[I][3]) : : "memory");
#pragma unroll
        for (int hl = 0; hl < 2; ++hl) {
            const uint4 *bb = b_rd + kc * SP_B_UNITS + hl * 64;
            constexpr int RA = 3;
            i32x4s bv[RA + 1];
#pragma unroll
            for (int k = 0; k < RA; ++k) bv[k] = *reinterpret_cast<const i32x4s *>(bb + k * 128);
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) {
                if (nt + RA < 8) bv[(nt + RA) % (RA + 1)] = *reinterpret_cast<const i32x4s *>(bb + (nt + RA) * 128);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(rc[I][mt * 2 + hl], bv[nt % (RA + 1)], acc[mt][nt], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if constexpr (!DENSE) {
            if (++kc == nch) {
                kc = 0;
                tile_done = tile_c;
                if (++it < my_tiles) tile_c = my_tile(it);
            }
        }
    };
    if constexpr (DENSE) {
        // one stage per trip, on the register set g mod SLOTS; the tile's end - the one copy of the epilogue - where the stage that ran was the tile's last
        // (the loads of the next AHEAD stages are on their way meanwhile, as they are when the other form meets its epilogue)
        uint32_t set = 0;
        clear_acc();
        for (uint64_t g = 0; g < n_stages; ++g) {
            sp_static_for<0, SLOTS>([&](auto IC) __attribute__((always_inline)) {
                if (set == (uint32_t)decltype(IC)::value) one_stage(IC);
            });
            set = set + 1 == (uint32_t)SLOTS ? 0 : set + 1;
            if (++kc == nch) {
                kc = 0;
                epilogue_dense(tile_c);
                clear_acc();
                if (++it < my_tiles) tile_c = my_tile(it);
            }
        }
        // the loads past the last stage are still on their way into registers the compiler takes for free from here on (the count's store below among
        // them: a list length of row bytes, an overflow out of nothing - seen at 10 M rows with few queries, where the last epilogue is short)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        for (uint64_t g = 0; g < n_stages; g += SLOTS) {
            sp_static_for<0, SLOTS>([&](auto IC) __attribute__((always_inline)) {
                if (g + decltype(IC)::value < n_stages) one_stage(IC);
            });
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        epilogue(tile_done);
    }
    list.finish(s.wcnt, blockIdx.x * WAVES + (uint32_t)w, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
template <int AHEAD>
__global__ __launch_bounds__(SP3_THREADS, 1) void scan_i8copy_kernel_res(const ScanArgs a, const SplitArgs s) {
    sp_i8copy_res_scan<AHEAD, false>(a, s);
}
// the first launch's instantiation (option i8_dense_epilogue): a kernel of its own name, so that what a search reports names the epilogue that ran
template <int AHEAD>
__global__ __launch_bounds__(SP3_THREADS, 1) void scan_i8copy_kernel_res_dense(const ScanArgs a, const SplitArgs s) {
    sp_i8copy_res_scan<AHEAD, true>(a, s);
}

// ---- after a launch: the k best candidates of every query get an exact look (sp_i8_probe_kernel, split_select.hip, then the gather kernel of
// qmx_rescore), and this is what their exact scores say: T = the k-th best of them is a lower bound of the final k-th best score; the threshold of the next launch
// and the cut of the selection follow it (never lowered).  One wave per query; the probe list is emptied for the next round.
__global__ __launch_bounds__(64) void sp_i8_bound_kernel(const float *scores, uint32_t *probe_cnt, uint32_t top, const float *band, const float *qscale,
                                                         float *thr, float *t_exact) {
    const uint32_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t n = probe_cnt[q];
    const float sc = (uint32_t)lane < n ? scores[(uint64_t)q * SP_I8_PROBE + lane] : -__builtin_inff();
    uint32_t rank = 0;
    for (int j = 0; j < 64; ++j) {
        const float o = __shfl(sc, j, 64);
        rank += (o > sc || (o == sc && j < lane)) ? 1u : 0u;
    }
    if (lane == 0) probe_cnt[q] = 0;
    if (n < top || !(band[q] < 3.0e38f)) return;
    if ((uint32_t)lane < n && rank == top - 1 && sc == sc) {
        if (sc > t_exact[q]) t_exact[q] = sc;
        const float t = (sc - band[q]) / qscale[q];
        if (t > thr[q]) thr[q] = t;
    }
}

// ---- "Launch 0" (option i8_sample_scan): the sample's bound from the int8 copy itself.  The sample is T = S / 16 whole 16-row tiles of the copy
// (api_search.hip sample_tile_ids_kernel states which), a 16-row tile is 2 KiB contiguous per 128-coordinate stage - two 1 KiB plane images at
// (row tile mod 16) * 2048 inside the stage's 32 KiB - and loads by the resident scan's pattern (sp_gload16 into the operand registers, the next stage's
// loads on their way behind the matrix work, the kernel's own vmcnt).
// A block is 4 waves, a wave owns two sample tiles (two independent addresses), the block keeps the operand images of NQ queries of the tile in LDS
// (nch x NQ / 16 x 2 KiB: 48 KiB for 64 queries at 768 coordinates) - at most 64 accumulator and 32 row registers per lane, so that the block starts beside
// a block of the resident scan (tools/step_footprint.py).  It writes scores[q][16 i + r] = (float)acc * qscale[q] for row r of sample tile i: the matrix
// launch_custom_topk reads, whose k best live columns the pair kernel then scores exactly (sp_i8_picks_kernel, sp_i8_sample_bound_kernel).
// Grid: (ceil(T / 8), ceil(nq / NQ)).
template <int NQ>
__global__ __launch_bounds__(256) void scan_i8copy_sample_kernel(const uint4 *rows_i8, const uint4 *bq, uint32_t nch, const uint32_t *sample_ids, uint32_t n_tiles,
                                                                 uint32_t nq, const float *qscale, float *scores) {
    constexpr int NT = NQ / 16, MT = 2, NL = 2 * MT;
    static_assert(NQ == 16 || NQ == 32 || NQ == 64, "whole query tiles, a divisor of the 128-query tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t q0 = blockIdx.y * NQ;
    // the images of queries q0 .. q0 + NQ: NT x 128 units of each stage's SP_B_UNITS
    for (uint32_t u = (uint32_t)tid; u < nch * (NT * 128u); u += 256) {
        const uint32_t kc = u / (NT * 128u), r = u % (NT * 128u);
        lds[u] = bq[(uint64_t)kc * SP_B_UNITS + (q0 / 16u) * 128u + r];
    }
    __syncthreads();
    const uint32_t t0 = (blockIdx.x * 4u + w) * MT;              // the wave's first sample tile
    if (t0 >= n_tiles) return;
    const bool two = t0 + 1 < n_tiles;                           // (a last, odd tile: the wave loads it twice and stores it once)
    const unsigned char *base[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const uint32_t rt = (uint32_t)__builtin_amdgcn_readfirstlane((int)(sample_ids[(uint64_t)(two ? t0 + (uint32_t)mt : t0) * 16u] >> 4));   // row tile of the block
        base[mt] = reinterpret_cast<const unsigned char *>(rows_i8) + ((uint64_t)(rt >> 4) * nch) * (SP3_A_UNITS * 16u) + (rt & 15u) * 2048u;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // from here on the kernel counts its vector-memory traffic itself
    const uint32_t kq_r = (uint32_t)lane >> 4, m_r = (uint32_t)lane & 15u;
    const uint32_t lane_unit = kq_r * 16u + (m_r ^ (2u * kq_r));      // sp_unit(0, 0, kq_r, m_r)
    const uint4 *const b_rd = lds + lane_unit;
    const uint32_t lane_off = lane_unit * 16u;
    // one stage's four loads: (sample tile mt, plane hl) of stage kc -> rc[mt * 2 + hl]; past the last stage the loads repeat it (the waits count loads)
    auto load_stage = [&](uint32_t kc, i32x4s (&rc)[NL]) __attribute__((always_inline)) {
        const uint64_t off = (uint64_t)(kc < nch ? kc : nch - 1) * (SP3_A_UNITS * 16u);
        sp_gload16<0>(rc[0], base[0] + off, lane_off);
        sp_gload16<1024>(rc[1], base[0] + off, lane_off);
        sp_gload16<0>(rc[2], base[1] + off, lane_off);
        sp_gload16<1024>(rc[3], base[1] + off, lane_off);
    };
    i32x4s acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (i32x4s){0, 0, 0, 0};
    auto landed = [](i32x4s (&rc)[NL]) __attribute__((always_inline)) { asm volatile("" : "+v"(rc[0]), "+v"(rc[1]), "+v"(rc[2]), "+v"(rc[3]) : : "memory"); };
    auto one_stage = [&](uint32_t kc, const i32x4s (&cur)[NL]) __attribute__((always_inline)) {
#pragma unroll
        for (int hl = 0; hl < 2; ++hl) {
            const uint4 *bb = b_rd + (size_t)kc * (NT * 128u) + hl * 64;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const i32x4s bv = *reinterpret_cast<const i32x4s *>(bb + nt * 128);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(cur[mt * 2 + hl], bv, acc[mt][nt], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // Two stages per trip: the loads of both are issued together, stage kc + 1's are on their way while stage kc runs (`vmcnt(4)`: all but the last four
    // have landed).  Every load is issued AND waited for inside the trip: no register with a load on its way lives across a branch or the loop's edge,
    // where the compiler may copy it or hand it to somebody else (round 14's fault: a load that landed in a register with a new owner) - a row of an odd
    // number of stages loads its last stage twice and multiplies it once.
    i32x4s ra[NL], rb[NL];
    for (uint32_t kc = 0; kc < nch; kc += 2) {
        load_stage(kc, ra);
        load_stage(kc + 1, rb);
        asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NL) : "memory");
        landed(ra);
        one_stage(kc, ra);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        landed(rb);
        if (kc + 1 < nch) one_stage(kc + 1, rb);
    }
    const uint64_t S = (uint64_t)n_tiles * 16u;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const uint32_t q = q0 + (uint32_t)nt * 16u + m_r;
        if (q >= nq) continue;
        const float qs = qscale[q];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (mt == 1 && !two) continue;
            float4 v;
            v.x = (float)acc[mt][nt][0] * qs;
            v.y = (float)acc[mt][nt][1] * qs;
            v.z = (float)acc[mt][nt][2] * qs;
            v.w = (float)acc[mt][nt][3] * qs;
            *reinterpret_cast<float4 *>(scores + (uint64_t)q * S + (uint64_t)(t0 + (uint32_t)mt) * 16u + 4u * kq_r) = v;      // rows 4 kq_r .. + 3 of the tile
        }
    }
}
// the k best live sample rows of every query, as the top-k behind the sample kernel left them in the tile's output lists -> the probe slots the pair
// kernel reads.  One wave per query; a query that is not finite (infinite band since the pack) has nothing to learn here.
__global__ __launch_bounds__(64) void sp_i8_picks_kernel(const qmx_scored_point *lists, const uint32_t *counts, uint32_t top, const float *band, uint32_t *probe_ids,
                                                         uint32_t *probe_cnt) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    uint32_t n = counts[q] < top ? counts[q] : top;
    n = n < SP_I8_PROBE ? n : SP_I8_PROBE;
    if (!(band[q] < 3.0e38f)) n = 0;
    if (lane < n) probe_ids[(uint64_t)q * SP_I8_PROBE + lane] = lists[(uint64_t)q * top + lane].idx;
    if (lane == 0) probe_cnt[q] = n;
}
// ... and what their exact scores say, sp_i8_bound_kernel's form for the sample: any k distinct live rows bound the final k-th best from below, so the
// smallest key (score, lower id first) of the k picks sets the first threshold, T_exact and gthr - the bound the conditional exact passes start from
// (sp_plan_kernel).  Fewer than k live sample rows: no bound - the band becomes infinite, which sends the query alone to the exact scan.
__global__ __launch_bounds__(64) void sp_i8_sample_bound_kernel(const float *scores, const uint32_t *probe_ids, uint32_t *probe_cnt, uint32_t top, float *band,
                                                                const float *qscale, float *thr, float *t_exact, uint64_t *gthr) {
    const uint32_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t n = probe_cnt[q];
    const float sc = (uint32_t)lane < n ? scores[(uint64_t)q * SP_I8_PROBE + lane] : 0.0f;
    const uint64_t key = (uint32_t)lane < n && sc == sc ? make_key(sc, probe_ids[(uint64_t)q * SP_I8_PROBE + lane]) : 0ull;
    uint32_t rank = 0;
    for (int j = 0; j < 64; ++j) rank += (uint64_t)__shfl((unsigned long long)key, j, 64) > key ? 1u : 0u;      // (live keys are distinct: they carry the row)
    if (lane == 0) probe_cnt[q] = 0;
    const bool finite = band[q] < 3.0e38f;
    const bool mine = finite && n >= top && key != 0 && rank == top - 1;
    if (!__ballot(mine)) {
        if (lane == 0) {
            band[q] = __builtin_inff();
            gthr[q] = 0;
        }
        return;
    }
    if (mine) {
        t_exact[q] = sc;
        thr[q] = (sc - band[q]) / qscale[q];
        gthr[q] = key;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// ---- the int8 copy ----
bool split_i8_dim_ok(uint32_t dim) { return dim % 128 == 0 && dim >= 128 && dim <= SP_I8_MAX_DIM; }
size_t split_i8_copy_bytes(uint64_t n, uint32_t dim) { return (size_t)((n + SP3_BM - 1) / SP3_BM) * (dim / 128) * SP3_A_UNITS * 16; }
size_t split_i8_query_bytes(uint32_t dim) { return (size_t)(dim / 128) * SP_B_UNITS * 16; }
uint32_t split_i8_probe() { return SP_I8_PROBE; }
// pass 1 of the copy: d_colmax [dim] <- max_r |x_rc| (uint bits), d_colsq [dim] <- sum_r x_rc^2 (both zeroed here)
int32_t launch_split_i8_colstats(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, uint32_t *d_colmax, float *d_colsq) {
    QMX_REQUIRE(split_i8_dim_ok(dim), QMX_ERR_BAD_ARG, "int8 copy of dim %u", dim);
    ::qmx::clear_stale_error();
    QMX_HIP(hipMemsetAsync(d_colmax, 0, (size_t)dim * 4, st));
    QMX_HIP(hipMemsetAsync(d_colsq, 0, (size_t)dim * 4, st));
    if (n) hipLaunchKernelGGL(sp_i8_colmax_kernel, dim3(2048), dim3(256), 0, st, (const unsigned char *)rows, row_stride, n, dim, d_colmax, d_colsq);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
// The columns' scales (host, dim numbers).  Any s_i >= max_r |x_ri| / 127 keeps the codes inside [-127, 127] and |e_i| <= 1/2, so the band formula holds for
// every such choice; WHICH choice decides how wide the band is.  With s_i at its floor a block whose columns differ in size (a few dominant coordinates: what
// transformer embeddings with outlier dimensions look like) gives its queries - one scale t per query, set by the largest q_i s_i - codes of 0 / +-1 in
// the small columns: the queries' rounding then costs C2 |f|_2 t on columns whose row codes use the full range.  Raising the small columns' scales to
// 1 / G of the largest typical |q_i s_i| moves range from their row codes (more row error: sum |d_i| / 2 grows) to their query codes (less query error:
// C2 shrinks): the G that minimises the predicted band for queries distributed like the rows is taken.  Predicted band (score units), |q_i| ~ sigma_i:
//   v_i = sigma_i s_i,  t = 3 max v / 127,  rows' rounding 0.4 sum v_i,  queries' rounding t sqrt(sum (sigma_i / s_i)^2) sqrt(sum min(1/12, (v_i / t)^2))
// (restated in tests/test_i8_prefilter_model.py: on eight coordinates twelve times the others the band drops from 1.06 to 0.43 standard deviations of the
// score, the rows inside it from 5 200 to 360 per query; columns of one size - Gaussian, Laplace, Student rows - keep their floor scales: G changes nothing there)
float split_i8_choose_scales(const float *colmax, const float *colsq, uint64_t n, uint32_t dim, float *scale) {
    std::vector<double> s0(dim), sig(dim);
    double wmax = 0.0;
    for (uint32_t i = 0; i < dim; ++i) {
        s0[i] = colmax[i] > 1.0e-30f ? (double)colmax[i] / 127.0 : 1.0;    // (an all-zero or vanishing column: codes 0, |e| = |x| <= 1/2 all the same)
        sig[i] = n ? sqrt((double)colsq[i] / (double)n) : 0.0;
        if (!(sig[i] < 1.0e30)) sig[i] = 0.0;
        wmax = std::max(wmax, sig[i] * s0[i]);
    }
    auto scales_of = [&](double G, std::vector<double> &s) {
        for (uint32_t i = 0; i < dim; ++i) {
            const double w = sig[i] * s0[i];
            s[i] = (w > 0.0 && wmax / G > w && colmax[i] > 1.0e-30f) ? s0[i] * (wmax / G / w) : s0[i];
        }
    };
    auto predicted = [&](const std::vector<double> &s) {
        double vmax = 0.0, vsum = 0.0, c2 = 0.0;
        for (uint32_t i = 0; i < dim; ++i) {
            const double v = sig[i] * s[i];
            vmax = std::max(vmax, v);
            vsum += v;
            c2 += (sig[i] / s[i]) * (sig[i] / s[i]);
        }
        const double t = 3.0 * vmax / 127.0;
        if (!(t > 0.0)) return 0.0;
        double f2 = 0.0;
        for (uint32_t i = 0; i < dim; ++i) f2 += std::min(1.0 / 12.0, (sig[i] * s[i] / t) * (sig[i] * s[i] / t));
        return 0.4 * vsum + t * sqrt(c2) * sqrt(f2);
    };
    static const double grid[] = {1.0e30, 64.0, 45.0, 32.0, 23.0, 16.0, 11.0, 8.0, 5.6, 4.0, 2.8, 2.0};
    std::vector<double> s(dim), best(dim);
    double best_b = 0.0, best_g = grid[0];
    for (size_t k = 0; k < sizeof(grid) / sizeof(grid[0]); ++k) {
        scales_of(grid[k], s);
        const double b = predicted(s);
        if (k == 0 || b < best_b * 0.98) {       // (a candidate has to pay: equal predictions keep the floor scales)
            best_b = b;
            best_g = grid[k];
            best = s;
        }
    }
    for (uint32_t i = 0; i < dim; ++i) {
        float f = (float)best[i];
        const float floor_s = colmax[i] > 1.0e-30f ? colmax[i] / 127.0f : 1.0f;
        scale[i] = f >= floor_s ? f : floor_s;     // (never below the floor, whatever the roundings above did)
    }
    return best_g >= 1.0e29 ? 0.0f : (float)best_g;
}
// pass 2: d_stats [4] <- {C1, C2^2, not finite, -} under the scales d_scale (zeroed here); then the copy itself (split_i8_copy_bytes)
int32_t launch_split_i8_rowstats(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, const float *d_scale, uint32_t *d_stats) {
    QMX_REQUIRE(split_i8_dim_ok(dim), QMX_ERR_BAD_ARG, "int8 copy of dim %u", dim);
    ::qmx::clear_stale_error();
    QMX_HIP(hipMemsetAsync(d_stats, 0, 16, st));
    if (n) hipLaunchKernelGGL(sp_i8_row_stats_kernel, dim3(2048), dim3(256), 0, st, (const unsigned char *)rows, row_stride, n, dim, d_scale, d_stats);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_split_i8_copy(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, const float *d_scale, void *d_out) {
    if (n == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_i8_copy_kernel, dim3(8192), dim3(256), 0, st, (const unsigned char *)rows, row_stride, n, dim, d_scale, (uint4 *)d_out);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
// one 128-query tile: codes, scales, bands, first thresholds (d_gthr: the sample's exact k-th best keys; nullptr: no threshold yet, +inf - the sample
// is scored behind this launch, launch_scan_i8copy_sample); zeroes the tile's candidate counters
int32_t launch_split_i8_pack(hipStream_t st, const float *d_q, uint32_t nq, uint32_t dim, const float *d_scale, const uint64_t *d_gthr, const uint32_t *d_row_stats,
                             float row_norm_max, void *d_bq, float *d_qscale, float *d_band, float *d_thr, float *d_t_exact, uint32_t *d_cand_cnt, uint32_t n_cnt) {
    QMX_REQUIRE(nq <= (uint32_t)SP_QT, QMX_ERR_BAD_ARG, "int8 tile of %u queries", nq);
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_i8_pack_kernel, dim3(SP_QT), dim3(256), (size_t)dim * 4, st, d_q, nq, dim, d_scale, d_gthr, d_row_stats, row_norm_max, (uint4 *)d_bq,
                       d_qscale, d_band, d_thr, d_t_exact, d_cand_cnt, n_cnt);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_scan_i8copy(hipStream_t st, const ScanArgs &a, const void *d_bq, const float *d_qscale, const float *d_thr, int num_cus, const void *d_rows_i8,
                           void *d_wlists, uint32_t phase) {
    // rows of up to 1 024 coordinates: the queries' whole image resident in LDS (scan_i8copy_kernel_res; option i8_resident = 0: the staged kernel)
    const uint32_t nch_r = a.dim / 128;
    const bool resident = option(OPT_I8_RESIDENT) > 0 && nch_r <= SP8R_MAX_NCH;
    // ... and its first launch, dense in candidates, with the epilogue made for that (option i8_dense_epilogue = 0: the one kernel for both launches)
    const bool dense = resident && (phase & 0xFFu) == 1 && option(OPT_I8_DENSE_EPILOGUE) > 0;
    void (*kfn)(const ScanArgs, const SplitArgs) = dense ? scan_i8copy_kernel_res_dense<1> : resident ? scan_i8copy_kernel_res<1> : scan_i8copy_kernel;
    const size_t lds_bytes = resident ? sp8r_lds_bytes(nch_r) : (size_t)SP8_LDS;
    static thread_local DeviceOnce attr_once;
    if (attr_once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_i8copy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SP8_LDS));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_i8copy_kernel_res<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp8r_lds_bytes(SP8R_MAX_NCH)));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_i8copy_kernel_res_dense<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp8r_lds_bytes(SP8R_MAX_NCH)));
        attr_once.mark();
    }
    QMX_REQUIRE(d_rows_i8 && d_wlists && split_i8_dim_ok(a.dim), QMX_ERR_BAD_ARG, "the int8 scan reads the int8 copy and writes per-wave candidate lists");
    SplitArgs s;
    s.rows_split = (const uint4 *)d_rows_i8;
    s.bq = (const uint4 *)d_bq;
    s.nchunks = a.dim / 128;
    s.nq = a.nq;
    s.row_scale = 1.0f;
    s.scales = d_qscale;
    s.thr = d_thr;
    s.cand = nullptr;
    s.cand_cnt = nullptr;
    s.cap = 0;
    s.wcap = SP_WCAP;
    const SplitWlists wl(d_wlists, num_cus);
    s.wcnt = wl.counts;
    s.wlist = wl.lists;
    s.phase = phase;
    const SplitGrid g = split_scan_grid(a.n_cand, SP3_BM, phase, num_cus);
    if (g.n_tiles == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    QMX_NOTE_KERNEL(kfn);
    hipLaunchKernelGGL(kfn, dim3(g.grid), dim3(SP3_THREADS), lds_bytes, st, a, s);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_split_i8_bound(hipStream_t st, const float *d_scores, uint32_t *d_probe_cnt, uint32_t nq, uint32_t top, const float *d_band, const float *d_qscale,
                              float *d_thr, float *d_t_exact) {
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_i8_bound_kernel, dim3(nq), dim3(64), 0, st, d_scores, d_probe_cnt, top, d_band, d_qscale, d_thr, d_t_exact);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
// queries per block of the sample kernel: the largest of 64 / 32 / 16 whose operand image fits in the LDS a resident scan block leaves on its CU at this row
// length - and no more than the tile holds.  Longer rows take the staged scan, beside which nothing fits: 16.
uint32_t split_i8_sample_queries(uint32_t dim, uint32_t nq) {
    const uint32_t nch = dim / 128;
    if (nch > SP8R_MAX_NCH) return 16;
    const size_t free_lds = (size_t)160 * 1024 - sp8r_lds_bytes(nch);
    uint32_t pick = 16;
    for (uint32_t c = 32; c <= 64; c *= 2)
        if ((size_t)nch * (c / 16) * 2048 <= free_lds && c / 2 < nq) pick = c;
    return pick;
}
// what a block of the int8 scan launch_scan_i8copy picks for this row length holds of its CU: LDS (static + dynamic) and registers per SIMD (512 threads: two
// waves per SIMD, registers allocated in units of 8).  What another launch must fit into to start beside it: 160 KiB and 512 registers less these.
int32_t split_i8_scan_footprint(uint32_t dim, size_t *lds_bytes, int *regs_per_simd) {
    const uint32_t nch = dim / 128;
    const bool resident = option(OPT_I8_RESIDENT) > 0 && nch <= SP8R_MAX_NCH;
    void (*kfn)(const ScanArgs, const SplitArgs) = resident ? scan_i8copy_kernel_res<1> : scan_i8copy_kernel;
    hipFuncAttributes fa;
    QMX_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(kfn)));
    *lds_bytes = (resident ? sp8r_lds_bytes(nch) : (size_t)SP8_LDS) + fa.sharedSizeBytes;
    *regs_per_simd = SP3_THREADS / 256 * ((fa.numRegs + 7) / 8 * 8);
    return QMX_OK;
}
// the approximate scores of the sample's tiles (d_sample: their 16 n_tiles row ids, tile after tile) for the nq queries packed in d_bq -> d_scores [nq][16 n_tiles]
int32_t launch_scan_i8copy_sample(hipStream_t st, const void *d_rows_i8, const void *d_bq, uint32_t dim, const uint32_t *d_sample, uint32_t n_tiles, uint32_t nq,
                                  const float *d_qscale, float *d_scores) {
    QMX_REQUIRE(d_rows_i8 && split_i8_dim_ok(dim) && nq >= 1 && nq <= (uint32_t)SP_QT && n_tiles >= 1, QMX_ERR_BAD_ARG, "int8 sample scan of %u queries", nq);
    const uint32_t nch = dim / 128, NQ = split_i8_sample_queries(dim, nq);
    const size_t lds_bytes = (size_t)nch * (NQ / 16) * 2048;
    QMX_REQUIRE(lds_bytes <= 65536, QMX_ERR_OTHER, "int8 sample scan: %zu B of query images", lds_bytes);
    const dim3 grid((n_tiles + 7) / 8, (nq + NQ - 1) / NQ);
    ::qmx::clear_stale_error();
    if (NQ == 64)
        hipLaunchKernelGGL(scan_i8copy_sample_kernel<64>, grid, dim3(256), lds_bytes, st, (const uint4 *)d_rows_i8, (const uint4 *)d_bq, nch, d_sample, n_tiles, nq, d_qscale, d_scores);
    else if (NQ == 32)
        hipLaunchKernelGGL(scan_i8copy_sample_kernel<32>, grid, dim3(256), lds_bytes, st, (const uint4 *)d_rows_i8, (const uint4 *)d_bq, nch, d_sample, n_tiles, nq, d_qscale, d_scores);
    else
        hipLaunchKernelGGL(scan_i8copy_sample_kernel<16>, grid, dim3(256), lds_bytes, st, (const uint4 *)d_rows_i8, (const uint4 *)d_bq, nch, d_sample, n_tiles, nq, d_qscale, d_scores);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
// the tile's lists (the top-k of the approximate sample scores) -> probe slots; then, behind the pair kernel, the sample's bound
int32_t launch_split_i8_picks(hipStream_t st, const qmx_scored_point *d_lists, const uint32_t *d_counts, uint32_t nq, uint32_t top, const float *d_band,
                              uint32_t *d_probe_ids, uint32_t *d_probe_cnt) {
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_i8_picks_kernel, dim3(nq), dim3(64), 0, st, d_lists, d_counts, top, d_band, d_probe_ids, d_probe_cnt);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_split_i8_sample_bound(hipStream_t st, const float *d_scores, const uint32_t *d_probe_ids, uint32_t *d_probe_cnt, uint32_t nq, uint32_t top,
                                     float *d_band, const float *d_qscale, float *d_thr, float *d_t_exact, uint64_t *d_gthr) {
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_i8_sample_bound_kernel, dim3(nq), dim3(64), 0, st, d_scores, d_probe_ids, d_probe_cnt, top, d_band, d_qscale, d_thr, d_t_exact, d_gthr);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

}  // namespace qmx
