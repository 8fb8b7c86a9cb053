// scan_l2i8.hip — the int8 prefilter of an f32 EUCLID block (QMX_SEG_L2_I8_COPY): 128 queries per pass of a quarter-size copy on v_mfma_i32_16x16x64_i8,
// the survivors re-scored exactly (api_search.hip l2_i8_search).  In the file's order: the centred copy (once per segment: column means, column and row
// statistics of y = x - mu, the codes, the row-norm column), l2i8_pack_kernel (once per 128-query tile), scan_l2i8_kernel (the hot path), the conditional
// exact Euclid pass of the queries whose lists overflowed (scan_l2_exact_groups_kernel), and the launchers.
//
// Squared Euclid distance decomposes, |q - x|^2 = |q|^2 + |x|^2 - 2 q.x, and does not move under a common shift of q and x.  So the block is stored as
// int8 codes of y = x - mu (mu: the column means - Euclid data sits far from the origin, SIFT is non-negative; uncentred, the column scales and with them
// the band would follow |x| instead of the rows' spread) in the operand-tile layout of scan_i8copy.hip, with one f32 per row beside it, N_r = |y_r|^2.
// A query is shifted the same way, p = q - mu, coded in the columns' scales with a scale t of its own, and the score of a pair is
//     A = 2 t I - N_r - Q,      I = the integer dot of the codes, Q = |p|^2,
// within l2i8_band (l2i8_band.hpp: the derivation, term by term) of the reference's f32 score R = -|q - x|^2.  The tail is the wide routes': a strided
// sample's exact k-th best score T_q admits the candidates (A >= T_q - band), per-wave lists are regrouped per query, the selection keeps
// A >= max(T_q - band, A_k - 2 band), the pair kernel re-scores those rows with the reference's bits, and a query whose lists overflowed takes the exact
// Euclid scan alone.
#include "dense_policies.hpp"
#include "l2i8_band.hpp"
#include "split_common.hpp"

namespace qmx {

constexpr uint32_t L2_RES_NCH = 8;                           // rows of up to 1 024 coordinates: the queries' image stays resident in LDS (128 KiB at 1 024) - scan_l2i8_kernel
constexpr uint32_t L2_MAX_NCH = 16;                          // ... of up to 2 048: rows and queries staged through LDS rings - scan_l2i8_staged_kernel
constexpr uint32_t L2_MAX_DIM = L2_MAX_NCH * 128;
constexpr int L2_QT = SP_QT;                                 // queries per pass
__host__ __device__ constexpr size_t l2_lds_bytes(uint32_t nch) { return (size_t)nch * SP_B_UNITS * 16 + 4 * L2_QT * 4; }

// ---- once per segment ----
// colsum[c] += sum_r x_rc in f64; thread t owns columns t, t + 256, ...
__global__ __launch_bounds__(256) void l2_colsum_kernel(const unsigned char *rows, uint64_t row_stride, uint64_t n, uint32_t dim, double *colsum) {
    double sm[L2_MAX_DIM / 256];
#pragma unroll
    for (int j = 0; j < (int)(L2_MAX_DIM / 256); ++j) sm[j] = 0.0;
    for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const float *v = reinterpret_cast<const float *>(rows + r * row_stride);
#pragma unroll
        for (int j = 0; j < (int)(L2_MAX_DIM / 256); ++j) {
            const uint32_t c = threadIdx.x + 256u * (uint32_t)j;
            if (c < dim) sm[j] += (double)v[c];
        }
    }
#pragma unroll
    for (int j = 0; j < (int)(L2_MAX_DIM / 256); ++j) {
        const uint32_t c = threadIdx.x + 256u * (uint32_t)j;
        if (c < dim) atomicAdd(&colsum[c], sm[j]);
    }
}
// sp_i8_colmax_kernel on y = x - mu: colmax[c] = max_r |y_rc| (f32, rounded UP: the scale's floor must cover every row), colsq[c] = sum_r y_rc^2 (a
// statistic that only steers split_i8_choose_scales)
__global__ __launch_bounds__(256) void l2_colmax_kernel(const unsigned char *rows, uint64_t row_stride, uint64_t n, uint32_t dim, const float *mu, uint32_t *colmax,
                                                        float *colsq) {
    float mx[L2_MAX_DIM / 256], sq[L2_MAX_DIM / 256];
    double m[L2_MAX_DIM / 256];
#pragma unroll
    for (int j = 0; j < (int)(L2_MAX_DIM / 256); ++j) {
        const uint32_t c = threadIdx.x + 256u * (uint32_t)j;
        mx[j] = 0.0f;
        sq[j] = 0.0f;
        m[j] = c < dim ? (double)mu[c] : 0.0;
    }
    for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const float *v = reinterpret_cast<const float *>(rows + r * row_stride);
#pragma unroll
        for (int j = 0; j < (int)(L2_MAX_DIM / 256); ++j) {
            const uint32_t c = threadIdx.x + 256u * (uint32_t)j;
            if (c < dim) {
                const float y = __double2float_ru(__builtin_fabs((double)v[c] - m[j]));
                mx[j] = __builtin_fmaxf(mx[j], y);
                sq[j] = __builtin_fmaf(y, y, sq[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < (int)(L2_MAX_DIM / 256); ++j) {
        const uint32_t c = threadIdx.x + 256u * (uint32_t)j;
        if (c < dim) {
            atomicMax(&colmax[c], __float_as_uint(mx[j]));
            atomicAdd(&colsq[c], sq[j]);
        }
    }
}
// the code of one element: y in f64 (exact, or within 2^-53), the quotient in f64: |y / s - c| <= 1/2 (1 + 2^-50)
__device__ __forceinline__ int l2_code(float x, float mu, float s) {
    double c = __builtin_rint(((double)x - (double)mu) / (double)s);
    c = c > 127.0 ? 127.0 : (c < -127.0 ? -127.0 : c);
    return c == c ? (int)c : 0;
}
// one wave per row: norms[r] = N_r = |y_r|^2 (f64 sum, stored f32; zeros behind row n up to the whole tile), stats[0] = C1 = max_r sum |c_ri|, stats[1] = C2^2,
// stats[2] != 0: an element or a norm that is not finite (no copy for this block), stats[3] = max_r N_r (f32 bits, rounded up)
__global__ __launch_bounds__(256) void l2_row_stats_kernel(const unsigned char *rows, uint64_t row_stride, uint64_t n, uint64_t n_pad, uint32_t dim, const float *mu,
                                                           const float *scale, float *norms, uint32_t *stats) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    uint32_t m1 = 0, m2 = 0;
    float mn = 0.0f;
    bool bad = false;
    for (uint64_t r = wave; r < n_pad; r += nwaves) {
        if (r >= n) {
            if (lane == 0) norms[r] = 0.0f;
            continue;
        }
        const float *v = reinterpret_cast<const float *>(rows + r * row_stride);
        uint32_t c1 = 0, c2 = 0;
        double nn = 0.0;
        for (uint32_t i = lane; i < dim; i += 64) {
            const float x = v[i];
            bad = bad || !(__builtin_fabsf(x) < __builtin_inff());
            const double y = (double)x - (double)mu[i];
            nn = __builtin_fma(y, y, nn);
            const int c = l2_code(x, mu[i], scale[i]);
            c1 += (uint32_t)(c < 0 ? -c : c);
            c2 += (uint32_t)(c * c);
        }
        for (int o = 32; o >= 1; o >>= 1) {
            c1 += __shfl_xor(c1, o, 64);
            c2 += __shfl_xor(c2, o, 64);
            nn += __shfl_xor(nn, o, 64);
        }
        bad = bad || !(nn < 1.0e38);
        m1 = c1 > m1 ? c1 : m1;
        m2 = c2 > m2 ? c2 : m2;
        if (!bad) mn = __builtin_fmaxf(mn, __double2float_ru(nn));
        if (lane == 0) norms[r] = (float)nn;
    }
    if (lane == 0) {
        atomicMax(&stats[0], m1);
        atomicMax(&stats[1], m2);
        atomicMax(&stats[3], __float_as_uint(mn));
    }
    if (bad) atomicOr(&stats[2], 1u);
}
// the copy: sp_i8_copy_kernel's layout - out[(tile * nch + k128) * 2048 + sp_unit(row tile, plane, kq, row)], one thread per 16-coordinate unit of the
// OUTPUT, rows past n zero - of the codes of y
__global__ __launch_bounds__(256) void l2_copy_kernel(const unsigned char *rows, uint64_t row_stride, uint64_t n, uint32_t dim, const float *mu, const float *scale,
                                                      uint4 *out) {
    const uint32_t nch = dim / 128;
    const uint64_t n_tiles = (n + SP3_BM - 1) / SP3_BM;
    const uint64_t total = n_tiles * nch * SP3_A_UNITS;
    for (uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (uint64_t)gridDim.x * 256) {
        const uint32_t u = (uint32_t)(gid % SP3_A_UNITS);
        const uint64_t blk = gid / SP3_A_UNITS, tile = blk / nch;
        const uint32_t k128 = (uint32_t)(blk % nch);
        const uint32_t kq = (u >> 4) & 3u, hl = (u >> 6) & 1u, t = u >> 7, m = (u & 15u) ^ (2u * kq);      // sp_unit, inverted
        const uint64_t r = tile * SP3_BM + t * 16u + m;
        const uint32_t g = k128 * 8u + hl * 4u + kq;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (r < n) {
            const float *v = reinterpret_cast<const float *>(rows + r * row_stride) + g * 16;
#pragma unroll
            for (int e = 0; e < 16; ++e) w[e / 4] |= ((uint32_t)l2_code(v[e], mu[g * 16 + e], scale[g * 16 + e]) & 0xFFu) << (8 * (e % 4));
        }
        out[gid] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ---- once per 128-query tile: one block per query slot.  p = q - mu in the columns' scales, the query's scale t (an f32 number, rounded up: every code
// stays inside [-127, 127]), its codes in the B-operand images (bq[k128][sp_unit(query, plane, kq)], zeros past nq), Q = |p|^2, the band (l2i8_band) and
// the two coefficients of the epilogue's compare from the sample's exact k-th best score (l2i8_compare_coefs).  All sums in f64. ----
__device__ __forceinline__ double l2_block_max(double v, double *sh) {
    for (int o = 32; o >= 1; o >>= 1) v = __builtin_fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return __builtin_fmax(__builtin_fmax(sh[0], sh[1]), __builtin_fmax(sh[2], sh[3]));
}
__device__ __forceinline__ double l2_block_sum(double v, double *sh) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
struct L2I8Coefs {       // [L2_QT] each, device: what the pack hands to the scan and the selection
    float *t_exact;      // T_q, the sample's exact k-th best score (-inf: none)
    float *band;         // l2i8_band (+inf: a query without a usable bound - it takes the exact scan alone)
    float *ca, *cb;      // the compare: a pair is a candidate when fl32(I) - cb N_r >= ca
    float *q2t, *qn;     // 2 t and Q: A = fma(2 t, I, -N_r) - Q
};
__global__ __launch_bounds__(256) void l2i8_pack_kernel(const unsigned char *queries, uint32_t q_stride, uint32_t nq, uint32_t dim, const float *mu, const float *scale,
                                                        const uint64_t *gthr, const uint32_t *row_stats, uint4 *bq, L2I8Coefs k, uint32_t *cand_cnt, uint32_t n_cnt) {
    extern __shared__ __attribute__((aligned(16))) double sh_u[];      // p_i s_i
    __shared__ double sh_red[4];
    const uint32_t qi = blockIdx.x;
    const bool live = qi < nq;
    if (qi == 0)
        for (uint32_t i = threadIdx.x; i < n_cnt; i += 256) cand_cnt[i] = 0;
    const float *q = reinterpret_cast<const float *>(queries + (uint64_t)qi * q_stride);
    double mx = 0.0, qq = 0.0, bad = 0.0;
    for (uint32_t i = threadIdx.x; i < dim; i += 256) {
        const double p = live ? (double)q[i] - (double)mu[i] : 0.0;
        const double u = p * (double)scale[i];
        sh_u[i] = u;
        mx = __builtin_fmax(mx, __builtin_fabs(u));
        qq = __builtin_fma(p, p, qq);
        if (!(__builtin_fabs(u) < 1.0e38)) bad = 1.0;
    }
    mx = l2_block_max(mx, sh_red);
    qq = l2_block_sum(qq, sh_red);
    bad = l2_block_max(bad, sh_red);                                   // (the barriers inside also publish sh_u)
    const float t_f = mx > 1.0e-30 && bad == 0.0 ? __double2float_ru(mx / 127.0) : 1.0f;
    const double t = (double)t_f;
    double sabs = 0.0, sf2 = 0.0;
    for (uint32_t u = threadIdx.x; u < dim / 16; u += 256) {
        const uint32_t k128 = u / 8, hl = (u / 4) & 1u, kq = u % 4;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const double x = sh_u[u * 16 + e] / t;
            double c = __builtin_rint(x);
            c = c > 127.0 ? 127.0 : (c < -127.0 ? -127.0 : c);
            if (!(c == c)) c = 0.0;
            const double f = x - c;
            sabs += __builtin_fabs(c);
            sf2 = __builtin_fma(f, f, sf2);
            w[e / 4] |= ((uint32_t)(int)c & 0xFFu) << (8 * (e % 4));
        }
        bq[(uint64_t)k128 * SP_B_UNITS + sp_unit(qi >> 4, hl, kq, qi & 15u)] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    sabs = l2_block_sum(sabs, sh_red);
    sf2 = l2_block_sum(sf2, sh_red);
    if (threadIdx.x != 0) return;
    float te = -__builtin_inff(), bd = 0.0f, ca = __builtin_inff(), cb = 0.0f;      // a dead slot admits nothing
    if (live) {
        const L2I8Query lq{t, sabs, __builtin_sqrt(sf2), qq};
        const L2I8Rows lr{(double)row_stats[0], __builtin_sqrt((double)row_stats[1]), (double)__uint_as_float(row_stats[3]), dim};
        const float b = l2i8_band(lq, lr);
        const uint64_t key = gthr[qi];
        const float ts = key ? key_score(key) : 0.0f;
        // no bound (the sample holds fewer than k live rows), or a query that is not finite: no candidates, and the infinite band sends the query - alone -
        // to the exact scan (sp_select_kernel)
        bd = __builtin_inff();
        if (bad == 0.0 && b < 3.0e38f && key != 0 && ts == ts && __builtin_fabsf(ts) < 3.0e38f) {
            bd = b;
            te = ts;
            l2i8_compare_coefs((double)ts - (double)b, lq, lr, &ca, &cb);
            if (!(__builtin_fabsf(ca) < 3.0e38f) || !(cb < 3.0e38f)) { bd = __builtin_inff(); te = -__builtin_inff(); ca = __builtin_inff(); cb = 0.0f; }
        }
    }
    k.t_exact[qi] = te;
    k.band[qi] = bd;
    k.ca[qi] = ca;
    k.cb[qi] = cb;
    k.q2t[qi] = 2.0f * t_f;
    k.qn[qi] = (float)qq;
}

// ---- The scan.  Work split and data movement are scan_i8copy_kernel_res's (which took them from scan_sqw.hip): block = 8 waves, one block per CU, persistent
// over 256-row tiles; the queries' whole operand image RESIDENT in LDS (nch x 16 KiB: 96 KiB at 768 coordinates) with the four per-query coefficients behind
// it, copied once per block - after that copy the waves share nothing: no barrier in the K-loop.  A wave owns row tiles 2 w and 2 w + 1 of a tile: per
// 128-coordinate stage four contiguous 1 KiB non-temporal `global_load_dwordx4` INTO the matrix instruction's operand registers, one stage ahead of the
// matrix work, waited for by the kernel's own in-order vmcnt; 32 v_mfma_i32_16x16x64_i8 against all 128 queries per stage and wave.
// What is new is the row term: the lane that owns accumulator rows 4 kq .. 4 kq + 3 of a row tile loads their four N_r as ONE 16-byte piece per row tile and
// tile (two loads per tile and lane, issued in front of the tile's first stage: the stage waits retire them), and the epilogue compares
//     fl32(I) - cb_q N_r >= ca_q        (one fused multiply-add per pair; l2i8_compare_coefs: ca carries the slack of the f32 roundings)
// narrowing by wave-uniform steps as the other scans do, then lists (A, row, query) with A = fma(2 t, I, -N_r) - Q in the wave's list (SpWaveList: the
// format launch_regroup_lists reads). ----
struct L2I8Args {
    const uint4 *rows_i8;     // the centred int8 copy, [tile][k128][2048 units]
    const float *norms;       // [tiles * 256] N_r
    const uint4 *bq;          // [nch][SP_B_UNITS] the queries' operand images
    uint32_t nch, nq;
    const float *ca, *cb, *q2t, *qn;
    uint4 *wlist;
    uint32_t *wcnt;
    uint32_t wcap;
};
template <int OFF>
__device__ __forceinline__ void l2_gload16(i32x4s &dst, const unsigned char *sbase, uint32_t voff) {
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3 nt" : "=v"(dst) : "v"(voff), "s"(sbase), "n"(OFF) : "memory");
}
template <int I, int N, class F>
__device__ __forceinline__ void l2_static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        l2_static_for<I + 1, N>(f);
    }
}
template <int AHEAD>
__global__ __launch_bounds__(SP3_THREADS, 1) void scan_l2i8_kernel(const ScanArgs a, const L2I8Args s) {
    constexpr int SLOTS = AHEAD + 1, WAVES = SP3_THREADS / 64, THREADS = SP3_THREADS, MT = 2, NL = 2 * MT;
    static_assert(SP3_BM == WAVES * MT * 16, "a wave owns two row tiles of a 256-row tile");
    static_assert(NL * AHEAD <= 62, "vmcnt is six bits");
    static_assert(L2_RES_NCH * 128u * 127u * 127u < (1u << 24), "fl32(I) is exact");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t n_tiles = (a.n_cand + SP3_BM - 1) / SP3_BM;
    const uint32_t nch = s.nch;
    const uint64_t my_tiles = blockIdx.x < n_tiles ? (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    if (my_tiles == 0) {
        SpWaveList::none(s.wcnt, blockIdx.x * WAVES + (uint32_t)w, lane);
        return;
    }
    const uint32_t ws = (uint32_t)w;
    auto my_tile = [&](uint64_t i) -> uint64_t { return blockIdx.x + i * gridDim.x; };
    float *ca_lds = reinterpret_cast<float *>(smem_raw + (size_t)nch * SP_B_UNITS * 16), *cb_lds = ca_lds + L2_QT, *q2t_lds = cb_lds + L2_QT, *qn_lds = q2t_lds + L2_QT;
#pragma unroll 4
    for (uint32_t u = (uint32_t)tid; u < nch * SP_B_UNITS; u += THREADS) lds[u] = s.bq[u];
    for (int u = tid; u < L2_QT; u += THREADS) {
        ca_lds[u] = (uint32_t)u < s.nq ? s.ca[u] : __builtin_inff();
        cb_lds[u] = s.cb[u];
        q2t_lds[u] = s.q2t[u];
        qn_lds[u] = s.qn[u];
    }
    __syncthreads();
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // from here on the kernel counts its vector-memory traffic itself
    const uint32_t kq_r = (uint32_t)lane >> 4, m_r = (uint32_t)lane & 15u;
    const uint32_t lane_unit = kq_r * 16u + (m_r ^ (2u * kq_r));      // sp_unit(0, 0, kq_r, m_r)
    const uint4 *const b_rd = lds + lane_unit;
    const uint32_t lane_off = lane_unit * 16u;
    // one stage's 2 MT loads: the images (row tile MT w + mt, plane hl) of stage kc of a tile -> rc[mt * 2 + hl]
    auto load_stage = [&](uint64_t tile, uint32_t kc, i32x4s (&rc)[NL]) __attribute__((always_inline)) {
        const unsigned char *src = sp_uniform_ptr((uint64_t)(uintptr_t)(s.rows_i8 + (tile * nch + kc) * SP3_A_UNITS) + ws * (NL * 1024u));
        l2_gload16<0>(rc[0], src, lane_off);
        l2_gload16<1024>(rc[1], src, lane_off);
        l2_gload16<2048>(rc[2], src, lane_off);
        l2_gload16<3072>(rc[3], src, lane_off);
    };
    // N of the lane's eight rows of a tile (rows 4 kq_r .. + 3 of both row tiles of the wave): entry j of n8[mt] is row 256 tile + 32 w + 16 mt + 4 kq_r + j -
    // inside the column also in the block's last tile, which is padded to whole tiles with zeros (l2i8_norm_entries)
    i32x4s n8[MT] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    const uint32_t n_off = (ws * (MT * 16u) + 4u * kq_r) * 4u;
    auto load_norms = [&](uint64_t tile) __attribute__((always_inline)) {
        const unsigned char *src = sp_uniform_ptr((uint64_t)(uintptr_t)(s.norms + tile * SP3_BM));
        l2_gload16<0>(n8[0], src, n_off);
        l2_gload16<64>(n8[1], src, n_off);
    };
    i32x4s acc[MT][8];
    SpWaveList list(s.wlist, s.wcap, blockIdx.x * WAVES + (uint32_t)w);
    const uint32_t n_rows32 = (uint32_t)a.n_cand;
    auto epilogue = [&](uint64_t tile) __attribute__((always_inline)) {
        const uint32_t row0 = (uint32_t)(tile * SP3_BM) + ws * (MT * 16u) + 4 * kq_r;
        uint32_t hits8 = 0;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const float nb = -cb_lds[nt * 16 + (int)m_r];
            float mx = -__builtin_inff();
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int j = 0; j < 4; ++j) mx = __builtin_fmaxf(mx, __builtin_fmaf(nb, __int_as_float(n8[mt][j]), (float)acc[mt][nt][j]));
            if (mx >= ca_lds[nt * 16 + (int)m_r]) hits8 |= 1u << nt;
        }
        if (!__ballot(hits8 != 0)) return;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            if (!__ballot((hits8 >> nt) & 1u)) continue;
            const uint32_t q = (uint32_t)nt * 16 + m_r;
            const float ca = ca_lds[q], nb = -cb_lds[q], t2 = q2t_lds[q], qn = qn_lds[q];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float fi = (float)acc[mt][nt][j], nr = __int_as_float(n8[mt][j]);
                    const uint32_t row = row0 + (uint32_t)mt * 16 + (uint32_t)j;
                    const float score = __builtin_fmaf(t2, fi, -nr) - qn;
                    list.append(__builtin_fmaf(nb, nr, fi) >= ca && row < n_rows32 && q < s.nq, score, row, q);
                }
            }
        }
    };
    const uint64_t n_stages = my_tiles * nch;
    // the stage the loads are at, as (tile, kc), by running counters; past the block's last stage they repeat it (the waits count loads, not bytes)
    uint64_t itr = 0, tile_r = my_tile(0);
    uint32_t kr = 0;
    auto advance_r = [&]() {
        if (kr + 1 < nch) ++kr;
        else if (itr + 1 < my_tiles) { kr = 0; ++itr; tile_r = my_tile(itr); }
    };
    i32x4s rc[SLOTS][NL];
    l2_static_for<0, AHEAD>([&](auto DC) __attribute__((always_inline)) {
        load_stage(tile_r, kr, rc[decltype(DC)::value]);
        advance_r();
    });
    uint64_t it = 0, tile_c = my_tile(0), tile_done = 0;
    uint32_t kc = 0;
    // one stage; I = g mod SLOTS selects the register sets at compile time
    auto one_stage = [&](auto IC) __attribute__((always_inline)) {
        constexpr int I = decltype(IC)::value, IL = (I + AHEAD) % SLOTS;
        if (kc == 0) {
            if (it) {
                // the finished tile's N were requested in front of ITS first stage's loads, and every stage since has waited for all but the last NL AHEAD loads
                asm volatile("" : "+v"(n8[0]), "+v"(n8[1]) : : "memory");
                epilogue(tile_done);
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 8; ++nt) acc[mt][nt] = (i32x4s){0, 0, 0, 0};
            load_norms(tile_c);
        }
        load_stage(tile_r, kr, rc[IL]);                           // stage g + AHEAD -> the register set stage g - 1 ran on
        advance_r();
        asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NL * AHEAD) : "memory");      // all but the last NL AHEAD loads have landed: this stage's, and the tile's N
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
        if (++kc == nch) {
            kc = 0;
            tile_done = tile_c;
            if (++it < my_tiles) tile_c = my_tile(it);
        }
    };
    for (uint64_t g = 0; g < n_stages; g += SLOTS) {
        l2_static_for<0, SLOTS>([&](auto IC) __attribute__((always_inline)) {
            if (g + decltype(IC)::value < n_stages) one_stage(IC);
        });
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(n8[0]), "+v"(n8[1]) : : "memory");
    epilogue(tile_done);
    list.finish(s.wcnt, blockIdx.x * WAVES + (uint32_t)w, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- The scan of rows of 1 152 .. 2 048 coordinates: the queries' image (144 .. 256 KiB) no longer fits in LDS, so rows AND queries are staged, with the work
// split and the rings of sp_staged_scan (split_common.hpp; this kernel is a text of its own: that one carries the dot route and the f16 copies).  block = 8
// waves = 4 row quarters (wm) x 2 query halves (wn), acc[4][4] per wave; a stage = 256 rows x 128 coordinates = 32 KiB of rows (non-temporal LDS-DMA from the
// copy) + 16 KiB of query images (LDS-DMA from L2), three stages of each in LDS; per stage and wave six 1 KiB requests spread between 32 matrix
// instructions, ONE s_waitcnt vmcnt and the stage barrier.
// The row term comes the way everything else does.  A wave needs the 64 N_r of its row quarter once per tile: at the top of the tile's FIRST stage - in front of
// that stage's six requests - it requests them with one global_load_lds_dword (256 B; lane l <- N of row 256 tile + 64 wm + l) into a 256-byte slot of its own
// behind the stage rings, and the tile's epilogue reads the lane's sixteen back with four ds_read_b128.  The wave reads only what it copied itself: no barrier.
// The vector-memory count, stage by stage (it retires in order; g = the stage, requests of stage g: [N of the tile if kc == 0, queries of g + 2, rows of g + 2]):
//   kc == 0: seven requests, s_waitcnt vmcnt(7);  kc > 0: six, vmcnt(6)
// - either way exactly the stage's OWN requests stay out, so rows and queries of stage g + 1 have landed, and so have, after the tile's second stage, its N
// (a tile has at least nine stages).  The epilogue of tile it runs at the top of tile it + 1, in FRONT of that stage's requests (its stores retire under the
// same wait), or after the last stage.  The slot ring has TWO slots per wave, tile it -> slot it & 1: the request of tile it + 1, issued right after the
// epilogue of tile it, lands in the OTHER slot; the one that lands on slot it & 1 again is tile it + 2's, a whole tile after those reads.
// fl32(I) is no longer exact here (127^2 dim >= 2^24): l2i8_band.hpp term (6) pays for it in the band and in the compare. ----
constexpr uint32_t L2S_RING_BYTES = (SP3_ARING * SP3_A_UNITS + 3 * SP_B_UNITS) * 16;      // 96 + 48 KiB
constexpr uint32_t L2S_NSLOTS = 2;                                                        // N slots per wave
constexpr uint32_t L2S_LDS = L2S_RING_BYTES + (SP3_THREADS / 64) * L2S_NSLOTS * 256;      // + 4 KiB = 148 KiB
// 256 B of global memory (wave-uniform base, lane i fetches bytes 4 i .. 4 i + 3) into LDS at the wave-uniform byte address lds_dst
__device__ __forceinline__ void l2_glds4(const unsigned char *src, uint32_t lane_off, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(src), "s"(lds_dst) : "memory");
}
__global__ __launch_bounds__(SP3_THREADS, 1) void scan_l2i8_staged_kernel(const ScanArgs a, const L2I8Args s) {
    constexpr int BRING = 3, WAVES = SP3_THREADS / 64;
    static_assert(L2_MAX_NCH * 128u * 127u * 127u < (1u << 25), "fl32(I) is within 1 of I (l2i8_int_rounding)");
    static_assert(L2S_LDS <= 160 * 1024, "one block per CU");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t n_tiles = (a.n_cand + SP3_BM - 1) / SP3_BM;
    const uint32_t nch = s.nch;
    const uint64_t my_tiles = blockIdx.x < n_tiles ? (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    if (my_tiles == 0) {
        SpWaveList::none(s.wcnt, blockIdx.x * WAVES + (uint32_t)w, lane);
        return;
    }
    auto my_tile = [&](uint64_t i) -> uint64_t { return blockIdx.x + i * gridDim.x; };
    const uint32_t wm = (uint32_t)w & 3u, wn = (uint32_t)w >> 2;
    const uint32_t kq_r = (uint32_t)lane >> 4, m_r = (uint32_t)lane & 15u;
    const uint32_t a_rd = sp_unit(wm * 4, 0, kq_r, m_r), b_rd = sp_unit(wn * 4, 0, kq_r, m_r);
    // the wave's 64 queries, 4 per lane (query 64 wn + 16 nt + m_r): the compare's a and -b, 2 t, Q; a slot past nq admits nothing
    float ca[4], nb[4], t2[4], qn[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const uint32_t q = wn * 64 + (uint32_t)nt * 16 + m_r;
        ca[nt] = q < s.nq ? s.ca[q] : __builtin_inff();
        nb[nt] = -s.cb[q];
        t2[nt] = s.q2t[q];
        qn[nt] = s.qn[q];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // from here on the kernel counts its vector-memory traffic itself
    const uint32_t lds0 = (uint32_t)(uintptr_t)(sp_lds_byte *)smem_raw;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    uint4 *b_lds = lds + SP3_ARING * SP3_A_UNITS;
    // the wave's N slots: bytes, and as the lane reads them (its rows 16 mt + 4 kq_r + j of the quarter: piece 4 mt + kq_r)
    const uint32_t n_slot0 = L2S_RING_BYTES + (uint32_t)w * (L2S_NSLOTS * 256u);
    const uint4 *n_rd = reinterpret_cast<const uint4 *>(smem_raw + n_slot0) + kq_r;
    // the copy streams, as in sp_staged_scan: running (tile, stage) counters; past the block's last stage the requests repeat it into a slot nobody reads
    uint64_t ra_it = 0;
    uint32_t ra_kc = 0, ra_slot = 0, rb_kc = 0, rb_slot = 0;
    const unsigned char *ra_src = nullptr, *rb_src = nullptr;
    uint32_t ra_dst = 0, rb_dst = 0;
    auto rows_begin = [&]() {
        ra_src = sp_uniform_ptr((uint64_t)(uintptr_t)(s.rows_i8 + (my_tile(ra_it) * nch + ra_kc) * SP3_A_UNITS) + (uint32_t)w * 4096u);
        ra_dst = lds0 + (ra_slot * SP3_A_UNITS) * 16u + (uint32_t)w * 4096u;
        ra_slot = sp_ring_next<SP3_ARING>(ra_slot);
        if (ra_kc + 1 < nch) ++ra_kc;
        else if (ra_it + 1 < my_tiles) { ra_kc = 0; ++ra_it; }
    };
    auto rows_piece = [&](int i) { sp_glds16_nt(ra_src + i * 1024, lane_off, ra_dst + i * 1024); };
    auto queries_begin = [&]() {
        rb_src = sp_uniform_ptr((uint64_t)(uintptr_t)(s.bq + (uint64_t)rb_kc * SP_B_UNITS) + (uint32_t)w * 2048u);
        rb_dst = lds0 + (SP3_ARING * SP3_A_UNITS + rb_slot * SP_B_UNITS) * 16u + (uint32_t)w * 2048u;
        rb_slot = sp_ring_next<BRING>(rb_slot);
        rb_kc = rb_kc + 1 == nch ? 0 : rb_kc + 1;
    };
    auto queries_piece = [&](int i) { sp_glds16(rb_src + i * 1024, lane_off, rb_dst + i * 1024); };
    // N of the wave's row quarter of a tile -> slot it & 1 (inside the column also in the block's last tile: it is padded to whole tiles, l2i8_norm_entries)
    auto request_norms = [&](uint64_t it) {
        const unsigned char *src = sp_uniform_ptr((uint64_t)(uintptr_t)(s.norms + my_tile(it) * SP3_BM + wm * 64u));
        l2_glds4(src, (uint32_t)lane * 4u, lds0 + n_slot0 + ((uint32_t)it & 1u) * 256u);
    };
    // the prologue: queries of stages 0 and 1, rows of stages 0 and 1, each stage's queries in front of its rows
    for (int st = 0; st < 2; ++st) {
        queries_begin();
        queries_piece(0);
        queries_piece(1);
        rows_begin();
#pragma unroll
        for (int i = 0; i < 4; ++i) rows_piece(i);
    }
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");      // all but the last six: queries and rows of stage 0 have landed
    sp_stage_barrier();
    uint32_t slot = 0, bslot = 0;
    i32x4s acc[4][4];
    SpWaveList list(s.wlist, s.wcap, blockIdx.x * WAVES + (uint32_t)w);
    const uint32_t n_rows32 = (uint32_t)a.n_cand;
    // the epilogue of tile it: accumulator register j of (mt, nt) = row 256 tile + 64 wm + 16 mt + 4 kq_r + j, query 64 wn + 16 nt + m_r.  The resident
    // kernel's test and score, narrowing by wave-uniform steps as I8CopyOps::epilogue does: the query tile, the 16-row tile, the four rows of a lane.
    auto epilogue = [&](uint64_t it) __attribute__((always_inline)) {
        const uint32_t row0 = (uint32_t)(my_tile(it) * SP3_BM) + wm * 64 + 4 * kq_r;
        const uint4 *np = n_rd + ((uint32_t)it & 1u) * 16u;
        f32x4s nr[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) nr[mt] = *reinterpret_cast<const f32x4s *>(np + mt * 4);
        bool hit[4];
        bool maybe = false;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            float mx = -__builtin_inff();
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int j = 0; j < 4; ++j) mx = __builtin_fmaxf(mx, __builtin_fmaf(nb[nt], nr[mt][j], (float)acc[mt][nt][j]));
            hit[nt] = mx >= ca[nt];
            maybe = maybe || hit[nt];
        }
        if (!__ballot(maybe)) return;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            if (!__ballot(hit[nt])) continue;
            const uint32_t q = wn * 64 + (uint32_t)nt * 16 + m_r;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                float m4 = -__builtin_inff();
#pragma unroll
                for (int j = 0; j < 4; ++j) m4 = __builtin_fmaxf(m4, __builtin_fmaf(nb[nt], nr[mt][j], (float)acc[mt][nt][j]));
                if (!__ballot(m4 >= ca[nt])) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float fi = (float)acc[mt][nt][j], n = nr[mt][j];
                    const uint32_t row = row0 + (uint32_t)mt * 16 + (uint32_t)j;
                    const float score = __builtin_fmaf(t2[nt], fi, -n) - qn[nt];
                    list.append(__builtin_fmaf(nb[nt], n, fi) >= ca[nt] && row < n_rows32 && q < s.nq, score, row, q);
                }
            }
        }
    };
    for (uint64_t it = 0; it < my_tiles; ++it) {
        if (it) epilogue(it - 1);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = (i32x4s){0, 0, 0, 0};
        for (uint32_t kc = 0; kc < nch; ++kc) {
            if (kc == 0) request_norms(it);               // the stage's first request
            queries_begin();                              // stage g + 2 -> the slot stage g - 1 was read from (everybody is past that barrier)
            rows_begin();                                 // likewise
            const uint4 *ab = lds + slot * SP3_A_UNITS + a_rd;
            const uint4 *bb = b_lds + bslot * SP_B_UNITS + b_rd;
            i32x4s b0[4], b1[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                b0[nt] = *reinterpret_cast<const i32x4s *>(bb + nt * 128);
                b1[nt] = *reinterpret_cast<const i32x4s *>(bb + nt * 128 + 64);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const i32x4s a0 = *reinterpret_cast<const i32x4s *>(ab + mt * 128);
                const i32x4s a1 = *reinterpret_cast<const i32x4s *>(ab + mt * 128 + 64);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1[nt], acc[mt][nt], 0, 0, 0);
                // the stage's six copy requests, in the order the wait below relies on (queries first), spread over the matrix work
                if (mt == 0) queries_piece(0);
                if (mt == 1) queries_piece(1);
                if (mt == 2) { rows_piece(0); rows_piece(1); }
                if (mt == 3) { rows_piece(2); rows_piece(3); }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0[nt], acc[mt][nt], 0, 0, 0);
            }
            slot = sp_ring_next<SP3_ARING>(slot);
            bslot = sp_ring_next<BRING>(bslot);
            // all but this stage's own requests have landed: rows and queries of stage g + 1 among them, and by the tile's second stage its N
            if (kc == 0) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            sp_stage_barrier();
        }
    }
    epilogue(my_tiles - 1);
    list.finish(s.wcnt, blockIdx.x * WAVES + (uint32_t)w, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // nothing may land in LDS after the block is gone
}

// ---- The conditional exact pass: the queries whose lists overflowed (packed by launch_split_plan: a.queries, a.del.filter_of; *a.run_if = how many) take the
// exact Euclid top-k scan, 16 per block row - grid.y = the 16-query groups of the batch, a block row whose group holds none returns at once, which on a
// search without overflow is every block.  Per (row, query) the instructions of the 16-query tile of scan_kernel<RowF32<M_EUCLID>, 16, 2, 2> (scan_common.hpp:
// scan_step, RowF32::finish - the reference's bits), over the whole block (no id list, no key bound); a.partial: grid.x x groups lists of 16 x top keys,
// group-major, as launch_merge_keys(..., grouped) reads them. ----
template <bool PERQ>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_l2_exact_groups_kernel(const ScanArgs a) {
    typedef RowF32<M_EUCLID> P;
    constexpr int QT = 16, R = P::R16, NW = SCAN_BLOCK / WAVE;
    const uint32_t count = (uint32_t)*a.run_if, q0 = blockIdx.y * QT;
    if (q0 >= count) return;
    const uint32_t nq = count - q0 < (uint32_t)QT ? count - q0 : (uint32_t)QT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned char *>(a.queries) + (uint64_t)q0 * a.q_stride);
        uint4 *dst = reinterpret_cast<uint4 *>(smem);
        const uint32_t n16 = (uint32_t)QT * a.q_stride / 16;
        for (uint32_t i = tid; i < n16; i += SCAN_BLOCK) dst[i] = src[i];
    }
    __syncthreads();
    const int t = lane & 7, g = lane >> 3;
    const int piece_off = lane_piece(t) * 16;
    const unsigned char *rows = reinterpret_cast<const unsigned char *>(a.rows);
    uint64_t list[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) list[q] = 0;
    constexpr uint32_t TILE = 8 * R;
    const uint64_t n_tiles = (a.n_cand + TILE - 1) / TILE;
    for (uint64_t tile = blockIdx.x * NW + wave; tile < n_tiles; tile += (uint64_t)gridDim.x * NW) {
        uint32_t rid[R];
        bool valid[R];
        const unsigned char *rp[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t c = tile * TILE + (uint32_t)(r * 8 + g);
            valid[r] = c < a.n_cand;
            rid[r] = valid[r] ? (uint32_t)c : 0u;
            rp[r] = rows + (uint64_t)rid[r] * a.row_stride + piece_off;
        }
        float acc[QT][R][P::NACC], raux[R][1];
#pragma unroll
        for (int q = 0; q < QT; ++q)
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int k = 0; k < P::NACC; ++k) acc[q][r][k] = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) raux[r][0] = 0;
#pragma unroll 2
        for (uint32_t sg = 0; sg < a.nseg; ++sg) {
            uint4 v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) v[r] = load_row_piece<true>(rp[r] + (uint64_t)sg * 128);
            scan_step<P, QT, R>(acc, raux, v, smem, sg * 128 + piece_off, a.q_stride, true);
        }
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            if (q < (int)nq) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float score = P::finish(acc[q][r], raux[r], smem + (uint32_t)q * a.q_stride, rows + (uint64_t)rid[r] * a.row_stride, rid[r], a);
                    const uint64_t key = make_key(score, rid[r]);
                    bool c = valid[r] && (t == 0) && key > readlane_u64(list[q], (int)a.top - 1);
                    if (__ballot(c)) {
                        if constexpr (PERQ) c = c && a.del.live(rid[r], q0 + (uint32_t)q);
                        else c = c && a.del.live(rid[r]);
                        uint64_t m = __ballot(c);
                        while (m) {
                            const int src = __builtin_ctzll(m);
                            m &= m - 1;
                            const uint64_t nk = readlane_u64(key, src);
                            if (nk > readlane_u64(list[q], (int)a.top - 1)) wave_list_insert(list[q], nk, lane);
                        }
                    }
                }
            }
        }
    }
    // block merge: 8 wave lists -> 1 list per query, one global write per block
    __syncthreads();
    uint64_t *lds_keys = reinterpret_cast<uint64_t *>(smem);
    const uint32_t top = a.top;
#pragma unroll
    for (int q = 0; q < QT; ++q)
        if (lane < (int)top) lds_keys[((uint32_t)wave * QT + q) * top + lane] = list[q];
    __syncthreads();
    uint64_t *partial = a.partial + (uint64_t)blockIdx.y * gridDim.x * QT * top;
    for (uint32_t q = wave; q < (uint32_t)QT; q += NW) {
        uint64_t merged = 0;
        if (q < nq)
            for (int sw = 0; sw < NW; ++sw) wave_offer(merged, lane < (int)top ? lds_keys[((uint32_t)sw * QT + q) * top + lane] : 0ull, (int)top, lane);
        if (lane < (int)top) partial[((uint64_t)blockIdx.x * QT + q) * top + lane] = merged;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
bool l2i8_dim_ok(uint32_t dim) { return dim % 128 == 0 && dim >= 128 && dim <= L2_MAX_DIM; }
// the conditional exact pass keeps 16 query entries of q_stride bytes in LDS (launch_scan_l2_exact_groups): a segment whose entries would not fit gets no copy
bool l2i8_exact_pass_fits(uint32_t q_stride) { return (size_t)16 * q_stride <= 160 * 1024; }
uint64_t l2i8_norm_entries(uint64_t n) { return (n + SP3_BM - 1) / SP3_BM * SP3_BM; }
size_t l2i8_wlists_counts_bytes(int num_cus) { return split_wlists_counts_bytes(num_cus); }
size_t l2i8_wlists_bytes(int num_cus) { return split_wlists_counts_bytes(num_cus) + (size_t)num_cus * (SP3_THREADS / 64) * SP_WCAP * 16; }
uint32_t l2i8_wcap() { return SP_WCAP; }

// d_colsum [dim] f64 <- the columns' sums (zeroed here)
int32_t launch_l2i8_colsum(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, double *d_colsum) {
    QMX_REQUIRE(l2i8_dim_ok(dim), QMX_ERR_BAD_ARG, "Euclid int8 copy of dim %u", dim);
    ::qmx::clear_stale_error();
    QMX_HIP(hipMemsetAsync(d_colsum, 0, (size_t)dim * 8, st));
    if (n) hipLaunchKernelGGL(l2_colsum_kernel, dim3(2048), dim3(256), 0, st, (const unsigned char *)rows, row_stride, n, dim, d_colsum);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
// launch_split_i8_colstats on y = x - mu
int32_t launch_l2i8_colstats(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, const float *d_mu, uint32_t *d_colmax, float *d_colsq) {
    QMX_REQUIRE(l2i8_dim_ok(dim), QMX_ERR_BAD_ARG, "Euclid int8 copy of dim %u", dim);
    ::qmx::clear_stale_error();
    QMX_HIP(hipMemsetAsync(d_colmax, 0, (size_t)dim * 4, st));
    QMX_HIP(hipMemsetAsync(d_colsq, 0, (size_t)dim * 4, st));
    if (n) hipLaunchKernelGGL(l2_colmax_kernel, dim3(2048), dim3(256), 0, st, (const unsigned char *)rows, row_stride, n, dim, d_mu, d_colmax, d_colsq);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
// d_norms [l2i8_norm_entries(n)] <- N_r, d_stats [4] <- {C1, C2^2, not finite, max N_r} (zeroed here)
int32_t launch_l2i8_rowstats(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, const float *d_mu, const float *d_scale, float *d_norms,
                             uint32_t *d_stats) {
    QMX_REQUIRE(l2i8_dim_ok(dim), QMX_ERR_BAD_ARG, "Euclid int8 copy of dim %u", dim);
    ::qmx::clear_stale_error();
    QMX_HIP(hipMemsetAsync(d_stats, 0, 16, st));
    if (n) hipLaunchKernelGGL(l2_row_stats_kernel, dim3(2048), dim3(256), 0, st, (const unsigned char *)rows, row_stride, n, l2i8_norm_entries(n), dim, d_mu, d_scale,
                              d_norms, d_stats);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
// d_out: split_i8_copy_bytes(n, dim)
int32_t launch_l2i8_copy(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, const float *d_mu, const float *d_scale, void *d_out) {
    if (n == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(l2_copy_kernel, dim3(8192), dim3(256), 0, st, (const unsigned char *)rows, row_stride, n, dim, d_mu, d_scale, (uint4 *)d_out);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
// one 128-query tile (a.queries: f32 entries): d_bq split_i8_query_bytes(dim); d_coefs: six arrays of 128 floats (t_exact, band, ca, cb, 2 t, Q); zeroes the tile's
// candidate counters
int32_t launch_l2i8_pack(hipStream_t st, const ScanArgs &a, const float *d_mu, const float *d_scale, const uint64_t *d_gthr, const uint32_t *d_row_stats, void *d_bq,
                         float *d_t_exact, float *d_band, float *d_ca, float *d_cb, float *d_q2t, float *d_qn, uint32_t *d_cand_cnt, uint32_t n_cnt) {
    QMX_REQUIRE(a.nq <= (uint32_t)L2_QT && l2i8_dim_ok(a.dim) && a.q_stride >= a.dim * 4, QMX_ERR_BAD_ARG, "Euclid int8 tile of %u queries", a.nq);
    ::qmx::clear_stale_error();
    const L2I8Coefs k{d_t_exact, d_band, d_ca, d_cb, d_q2t, d_qn};
    hipLaunchKernelGGL(l2i8_pack_kernel, dim3(L2_QT), dim3(256), (size_t)a.dim * 8, st, (const unsigned char *)a.queries, a.q_stride, a.nq, a.dim, d_mu, d_scale, d_gthr,
                       d_row_stats, (uint4 *)d_bq, k, d_cand_cnt, n_cnt);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
// d_wlists: l2i8_wlists_bytes(num_cus); *grid_out = blocks launched (8 lists each)
int32_t launch_scan_l2i8(hipStream_t st, const ScanArgs &a, const void *d_rows_i8, const float *d_norms, const void *d_bq, const float *d_ca, const float *d_cb,
                         const float *d_q2t, const float *d_qn, int num_cus, void *d_wlists, uint32_t *grid_out) {
    QMX_REQUIRE(d_rows_i8 && d_norms && d_wlists && l2i8_dim_ok(a.dim) && !a.ids && a.n_cand >= 1 && a.n_cand < 0xFFFFFFFFull && a.nq <= (uint32_t)L2_QT, QMX_ERR_BAD_ARG,
                "the Euclid int8 scan reads the centred copy of the whole block");
    L2I8Args s;
    s.rows_i8 = (const uint4 *)d_rows_i8;
    s.norms = d_norms;
    s.bq = (const uint4 *)d_bq;
    s.nch = a.dim / 128;
    s.nq = a.nq;
    s.ca = d_ca;
    s.cb = d_cb;
    s.q2t = d_q2t;
    s.qn = d_qn;
    const SplitWlists wl(d_wlists, num_cus);
    s.wcnt = wl.counts;
    s.wlist = wl.lists;
    s.wcap = SP_WCAP;
    const uint64_t n_tiles = (a.n_cand + SP3_BM - 1) / SP3_BM;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)num_cus, n_tiles);
    // rows of up to 1 024 coordinates: the queries resident; longer ones: the staged rings
    const bool resident = s.nch <= L2_RES_NCH;
    void (*kfn)(const ScanArgs, const L2I8Args) = resident ? scan_l2i8_kernel<1> : scan_l2i8_staged_kernel;
    static thread_local DeviceOnce once;
    ::qmx::clear_stale_error();
    if (once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_l2i8_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l2_lds_bytes(L2_RES_NCH)));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_l2i8_staged_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L2S_LDS));
        once.mark();
    }
    QMX_NOTE_KERNEL(kfn);
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(SP3_THREADS), resident ? l2_lds_bytes(s.nch) : (size_t)L2S_LDS, st, a, s);
    QMX_HIP(hipGetLastError());
    if (grid_out) *grid_out = grid;
    return QMX_OK;
}
// a.nq packed slots in a.queries (a.del.filter_of packed with them), *a.run_if = how many of them are to be scanned; a.partial: grid.x x groups lists of 16 x top
// keys.  *grid_out: in: the cap on grid.x, out: grid.x
int32_t launch_scan_l2_exact_groups(hipStream_t st, const ScanArgs &a, int num_cus, uint32_t *grid_out) {
    constexpr int QT = 16, NW = SCAN_BLOCK / WAVE;
    QMX_REQUIRE(a.run_if && a.partial && !a.ids && !a.key_bound && a.nq >= 1 && grid_out && a.top >= 1 && a.top <= (uint32_t)MAX_TOP_FAST && a.rem_pieces == 0 &&
                    a.tail_start == a.dim && a.nseg * 32 == a.dim,
                QMX_ERR_BAD_ARG, "Euclid exact groups: a packed conditional pass over whole 128-byte segments");
    size_t lds = std::max((size_t)QT * a.q_stride, (size_t)NW * QT * a.top * sizeof(uint64_t));
    lds = (lds + 15) & ~(size_t)15;
    QMX_REQUIRE(lds <= 160 * 1024, QMX_ERR_NOT_SUPPORTED, "query tile needs %zu B of LDS (> 160 KiB)", lds);
    void (*kfn)(const ScanArgs) = a.del.filter_of ? scan_l2_exact_groups_kernel<true> : scan_l2_exact_groups_kernel<false>;
    static thread_local DeviceOnce once;
    ::qmx::clear_stale_error();
    if (once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_l2_exact_groups_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_l2_exact_groups_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        once.mark();
    }
    const uint64_t n_tiles = (a.n_cand + 8 * RowF32<M_EUCLID>::R16 - 1) / (8 * RowF32<M_EUCLID>::R16);
    uint32_t grid = (uint32_t)std::min<uint64_t>((n_tiles + NW - 1) / NW, (uint64_t)num_cus);
    if (grid < 1) grid = 1;
    if (*grid_out && grid > *grid_out) grid = *grid_out;
    *grid_out = grid;
    hipLaunchKernelGGL(kfn, dim3(grid, (a.nq + QT - 1) / QT), dim3(SCAN_BLOCK), lds, st, a);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

}  // namespace qmx
