// scan_u8w.hip - dense u8 rows (Metric<u8>, `datatype: uint8`), brute-force top-k for LARGE query batches: 128 queries per pass of the block on
// v_mfma_i32_16x16x64_i8, with NO copy of the block (QMX_SEG_U8_WIDE; api_search.hip u8_wide_search).
//
// A u8 row is one byte per element already; the matrix instruction multiplies SIGNED bytes, so both operands are biased by 128 - one xor with 0x80 per
// byte, in registers for the rows (after the wait for their loads), once per tile of queries for the queries (u8w_pack_kernel).  With x' = x - 128,
// q' = q - 128 and I = sum q' x' the exact integers of a pair follow from I, a per-row column made once per segment and a per-query term (u8w_band.hpp: the
// identities, the band |A - R| of the pass's score A against the reference's f32 score R, the integer / float compare and why it admits every pair the
// selection's cut admits).  In the file's order: the per-row columns, u8w_pack_kernel, scan_u8w_kernel (the hot path for rows of up to 1 024 bytes:
// scan_sqw.hip's work split with the bias, the columns and a per-metric epilogue), scan_u8w_staged_kernel (rows of 1 088 .. 2 048 bytes: rows and queries
// through LDS rings, the rows by LDS-DMA straight from the row-major block), u8w_finish_kernel, and the conditional exact pass of the queries whose lists
// overflowed.
//
// The tail is the wide routes': a strided sample's exact k-th best score T_q admits the candidates (A >= T_q - band), per-wave lists are regrouped per
// query, the selection keeps A >= max(T_q - band, A_k - 2 band), the pair kernel re-scores that (the reference's bits in either order of
// QMX_SEG_U8_SCALAR_ORDER) and a query whose lists overflowed - masses of ties are normal with integer scores - takes the exact scan.
#include "dense_policies.hpp"
#include "split_common.hpp"
#include "u8w_band.hpp"

namespace qmx {

typedef int i32x4u __attribute__((ext_vector_type(4)));

constexpr int UW_THREADS = 512;
constexpr int UW_BM = 256;                                   // rows per tile
constexpr int UW_QT = 128;                                   // queries per pass
constexpr int UW_B_UNITS = UW_QT * 4;                        // 16-byte units of a 64-byte stage of the queries' image: 8 KiB
constexpr uint32_t UW_RES_NCH = 16;                          // rows of up to 1 024 bytes: the queries' whole image stays in LDS (128 KiB at 1 024) - scan_u8w_kernel
constexpr uint32_t UW_MAX_NCH = 32;                          // ... of up to 2 048: rows and queries staged through LDS rings - scan_u8w_staged_kernel
constexpr uint32_t UW_MAX_DIM = UW_MAX_NCH * 64;
constexpr int UW_LDS_TAIL = UW_QT * 12;                      // behind the resident image: the integer bounds, the cosine's k and a
constexpr int UW_LDS_MAX = UW_RES_NCH * UW_B_UNITS * 16 + UW_LDS_TAIL;
// what u8w_band.hpp's derivation asks of the longest row: the AVX2 leaf's eight lane totals convert exactly, a pair's integers stay below 2^27, I fits
static_assert(65025ull * UW_MAX_DIM / 8 < (1ull << 24), "a lane total of the reference's AVX2 leaf converts to f32 exactly");
static_assert(65025ull * UW_MAX_DIM < (1ull << 27), "|Z| < 2^27: one rounding of A, the compare's slack of 4 / 8 / 16");
static_assert(128ull * 128ull * UW_MAX_DIM <= (1ull << 25), "I = sum q' x' fits the accumulator (and 2 I + C an int32)");
constexpr uint32_t UW_WCAP = 8192;                           // candidates one wave may list per pass
constexpr uint32_t UW_BIAS = 0x80808080u;

// unit index of (16-query tile t, piece kq, query-in-tile m) inside a stage of the queries' image: conflict-free for the operand reads (scan_sqw.hip sw_unit)
__device__ __forceinline__ uint32_t uw_unit(uint32_t t, uint32_t kq, uint32_t m) { return (t * 4 + kq) * 16 + (m ^ (2 * kq)); }

struct U8WideArgs {
    const uint4 *bq;          // the queries' biased bytes as operand images (u8w_pack_kernel): [nch][UW_B_UNITS], or - nch > UW_RES_NCH - [(nch + 1) / 2][SP_B_UNITS]
    uint32_t nch;             // 64-byte chunks of a row: dim / 64 (the resident scan's stages per tile; the staged scan's are pairs of them)
    uint32_t nq;              // live queries (<= 128)
    const int32_t *thr_i;     // [128] Dot / Euclid: a pair with V below this cannot reach the query's cut
    const float *kq, *aq;     // [128] Cosine: a pair with fma(-k, F[row], fl32(V)) below a cannot
    const int32_t *col;       // [u8w_col_entries(n)] C[row]
    const float *colf;        // ... F[row] (Cosine)
    uint4 *wlist;             // [waves][wcap] (I, row, query, 0); u8w_finish_kernel turns them into (key lo, key hi, query, 0)
    uint32_t *wcnt;           // [waves] entries each wave wanted to append (may run past wcap: overflow)
    uint32_t wcap;
};

// ---- once per segment: C[row] = 128 sum(x) (Dot, Cosine) or 256 sum(x) - sum(x^2) (Euclid: every term x (256 - x) >= 0); Cosine also F[row], an f32
// number below sqrt(sum(x^2)), and N2[row] = sum(x^2) itself for the finish.  Sixteen lanes per row, a 16-byte piece per lane and step.  The streamed
// columns are padded to whole 256-row tiles with zeros: the scan loads the entries of a lane's four rows as one 16-byte piece, those of rows past the
// block included, and drops such rows by their number ----
__global__ __launch_bounds__(256) void u8w_columns_kernel(const unsigned char *rows, uint64_t row_stride, uint64_t n, uint64_t n_pad, uint32_t dim, int metric,
                                                          int32_t *col, float *colf, int32_t *n2) {
    const uint32_t l16 = threadIdx.x & 15u;
    for (uint64_t r = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 4); r < n_pad; r += (uint64_t)gridDim.x * 16) {
        uint32_t s1 = 0, s2 = 0;
        if (r < n) {
            const uint4 *p = reinterpret_cast<const uint4 *>(rows + r * row_stride);
            for (uint32_t u = l16; u < dim / 16; u += 16) {
                const uint4 v = p[u];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s1 = __builtin_amdgcn_udot4(w[k], 0x01010101u, s1, false);
                    s2 = __builtin_amdgcn_udot4(w[k], w[k], s2, false);
                }
            }
        }
        for (int o = 8; o >= 1; o >>= 1) {
            s1 += __shfl_xor(s1, o, 64);
            s2 += __shfl_xor(s2, o, 64);
        }
        if (l16 != 0) continue;
        col[r] = metric == U8W_EUCLID ? (int32_t)(256u * s1 - s2) : (int32_t)(128u * s1);
        if (metric == U8W_COSINE) {
            colf[r] = u8w_row_f((int64_t)s2);
            if (r < n) n2[r] = (int32_t)s2;
        }
    }
}

// ---- once per 128-query tile: one wave per query slot.  The query's bytes, biased, in the B-operand images; its sums; from the sample's k-th best exact
// score T the band, the cut T - band and the compare's terms.  A dead slot, or a query without a usable bound (the sample holds fewer than k live rows),
// passes nothing and gets an infinite band: the selection sends such a query - alone - to the exact pass ----
struct U8WideQuery {      // [UW_QT] each, device: what the pack hands to the scan, the finish and the selection
    float *t_exact;       // T_q (-inf: none)
    float *band;
    float *cut;           // T_q - band, rounded down: the finish withdraws entries below it
    int32_t *thr_i;
    float *kq, *aq;
    int32_t *qoff, *n1;   // the query's term of the integer score; sum(q^2)
};
__global__ __launch_bounds__(64) void u8w_pack_kernel(const unsigned char *queries, uint32_t q_stride, uint32_t nq, uint32_t dim, int metric, uint32_t scalar_order,
                                                      const uint64_t *gthr, uint4 *bq, U8WideQuery k, uint32_t *cand_cnt, uint32_t n_cnt) {
    const uint32_t qi = blockIdx.x, lane = threadIdx.x;
    const bool live = qi < nq;
    if (qi == 0)
        for (uint32_t i = lane; i < n_cnt; i += 64) cand_cnt[i] = 0;
    const unsigned char *entry = queries + (uint64_t)qi * q_stride;
    U8WQuery sums{0, 0, 0};
    // dim <= 1024: one piece per lane, the resident scan's image ([dim / 64][UW_B_UNITS]).  Longer rows: two pieces per lane, the staged scan's image -
    // [stages of 128 bytes][SP_B_UNITS] in the unit order its LDS-DMA copies verbatim; a last stage of one 64-byte chunk (dim = 64 mod 128) gets its
    // missing chunk as q' = 0, whose product is zero whatever the row bytes are
    const uint32_t nch = dim / 64, n_pieces = nch > UW_RES_NCH ? (nch + 1) / 2 * 8 : nch * 4;
    for (uint32_t p = lane; p < n_pieces; p += 64) {
        const bool real = p < dim / 16;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (live && real) v = *reinterpret_cast<const uint4 *>(entry + (uint64_t)p * 16);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        if (live && real)
#pragma unroll
            for (int e = 0; e < 16; ++e) u8w_query_add(sums, (w[e / 4] >> (8 * (e % 4))) & 0xFFu);
        const uint4 image = real ? make_uint4(v.x ^ UW_BIAS, v.y ^ UW_BIAS, v.z ^ UW_BIAS, v.w ^ UW_BIAS) : make_uint4(0u, 0u, 0u, 0u);
        if (nch > UW_RES_NCH) bq[(uint64_t)(p >> 3) * SP_B_UNITS + sp_unit(qi >> 4, (p >> 2) & 1u, p & 3u, qi & 15u)] = image;
        else bq[(uint64_t)(p >> 2) * UW_B_UNITS + uw_unit(qi >> 4, p & 3u, qi & 15u)] = image;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        sums.sum_q += __shfl_xor(sums.sum_q, o, 64);
        sums.sum_q2 += __shfl_xor(sums.sum_q2, o, 64);
        sums.far2 += __shfl_xor(sums.far2, o, 64);
    }
    if (lane != 0) return;
    const int64_t qoff = live ? u8w_qoff(metric, sums, dim) : 0;
    float te = -__builtin_inff(), bd = __builtin_inff(), ct = __builtin_inff(), kq = 0.0f, aq = __builtin_inff();
    int32_t ti = 0x7FFFFFFF;
    const uint64_t key = live ? gthr[qi] : 0;
    const float t = key ? key_score(key) : 0.0f;
    if (key != 0 && t == t && __builtin_fabsf(t) < 3.0e38f) {
        te = t;
        bd = u8w_band(metric, scalar_order != 0, sums);
        const double cut = (double)t - (double)bd;
        ct = -u8w_up(-cut);
        if (metric == U8W_COSINE) u8w_cos_coefs(cut, sums, qoff, &kq, &aq);
        else ti = u8w_int_bound(cut, qoff);
    }
    k.t_exact[qi] = te;
    k.band[qi] = bd;
    k.cut[qi] = ct;
    k.thr_i[qi] = ti;
    k.kq[qi] = kq;
    k.aq[qi] = aq;
    k.qoff[qi] = (int32_t)qoff;
    k.n1[qi] = (int32_t)sums.sum_q2;
}

// (default cache policy: a load instruction touches sixteen 64-byte HALF-lines whose other halves the group's next load is meant to hit; scan_sqw.hip measured it)
__device__ __forceinline__ void uw_gload16(i32x4u &dst, const unsigned char *sbase, uint32_t voff) {
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(sbase) : "memory");
}
template <int I, int N, class F>
__device__ __forceinline__ void uw_static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        uw_static_for<I + 1, N>(f);
    }
}
// vmcnt(n) for a wave-uniform even n <= 14 (the immediate has to be one)
__device__ __forceinline__ void uw_wait_vm_dyn(uint32_t n) {
    switch (n >> 1) {
#define UW_W(k) case k: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * k) : "memory"); break;
        UW_W(1) UW_W(2) UW_W(3) UW_W(4) UW_W(5) UW_W(6) UW_W(7)
#undef UW_W
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

// ---- The scan.  Work split and data movement are scan_sqw_kernel's: block = 8 waves, one block per CU, persistent over 256-row tiles; the queries' WHOLE
// biased image RESIDENT in LDS (dim / 64 x 8 KiB: 96 KiB at 768, 128 KiB at 1 024) with the compare's per-query terms behind it, copied once per block -
// after that copy the waves share nothing: no barrier in the K-loop.  A wave OWNS 32 rows of the tile; lane (m, kg) loads, per 64-byte stage, bytes
// [16 kg, +16) of rows m and 16 + m straight from the row-major u8 block into its operand registers (`global_load_dwordx4` by inline asm, by GROUPS of G
// stages, AHEAD groups in front of the matrix work, waited for by the kernel's own in-order `s_waitcnt vmcnt`).  What is this operand's own:
//   the bias - after the wait the group's pieces are xor-ed with 0x80 per byte (four v_xor_b32 per piece), unsigned byte x becomes int8 x - 128;
//   the columns - C (and the cosine's F) of the lane's eight rows, two (four) 16-byte loads on the tile's first group, IN FRONT of that group's row
//     loads: in-order counting only makes the waits behind them more conservative, and by the tile's epilogue 2 G ngr younger loads have been issued of
//     which the last wait left at most 2 G AHEAD in flight (a tile of fewer groups than AHEAD: the explicit wait in front of the epilogue);
//   the epilogue - per metric, narrowing by wave-uniform steps (any pair of a query tile, then the pairs): Dot V = I + C >= bound, Euclid V = 2 I + C >=
//     bound (the maximum over the lane's eight rows first), Cosine one convert and one fma per pair against F[row] and the query's k. ----
template <int METRIC, int G, int AHEAD>
__global__ __launch_bounds__(UW_THREADS, 1) void scan_u8w_kernel(const ScanArgs a, const U8WideArgs s) {
    constexpr int WAVES = UW_THREADS / 64, T = UW_THREADS, BM = UW_BM;
    constexpr bool COS = METRIC == M_COSINE;
    static_assert(BM == WAVES * 32, "a wave owns 32 rows of a tile");
    constexpr int SLOTS = AHEAD + 1;
    static_assert(2 * G * AHEAD <= 62, "vmcnt is six bits");
    static_assert(2 * G * (AHEAD - 1) <= 14, "uw_wait_vm_dyn covers the short-row case up to 14");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem_raw);
    const uint32_t nch = s.nch;
    const uint32_t ngr = (nch + G - 1) / G;                          // groups per tile
    int32_t *thr_lds = reinterpret_cast<int32_t *>(smem_raw + (size_t)nch * UW_B_UNITS * 16);
    float *kq_lds = reinterpret_cast<float *>(thr_lds + UW_QT), *aq_lds = kq_lds + UW_QT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t n_tiles = (a.n_cand + BM - 1) / BM;
    const uint64_t my_tiles = blockIdx.x < n_tiles ? (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    if (my_tiles == 0) {
        SpWaveList::none(s.wcnt, blockIdx.x * (WAVES) + (uint32_t)w, lane);
        return;
    }
#pragma unroll 4
    for (uint32_t u = (uint32_t)tid; u < nch * UW_B_UNITS; u += T) lds[u] = s.bq[u];
    if (tid < UW_QT) {
        thr_lds[tid] = s.thr_i[tid];
        kq_lds[tid] = s.kq[tid];
        aq_lds[tid] = s.aq[tid];
    }
    __syncthreads();
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // from here on the kernel counts its vector-memory traffic itself
    const uint32_t kq_r = (uint32_t)lane >> 4, m_r = (uint32_t)lane & 15u;
    const uint4 *const b_rd = lds + uw_unit(0, kq_r, m_r);
    const unsigned char *rows = reinterpret_cast<const unsigned char *>(a.rows);
    const uint64_t last_row = a.n_cand - 1;
    const uint32_t row_stride32 = (uint32_t)a.row_stride;
    const uint32_t rl0 = (uint32_t)w * 32u + m_r, rl1 = rl0 + 16u;

    // One group's 2 G loads: the lane's pieces of row tiles 0 and 1 of group b of the block's it-th tile (rows past the block: the last row's bytes, their
    // scores are dropped; stages past the row: the group's last piece again - the waits count loads)
    auto load_group = [&](uint64_t it, uint32_t b, i32x4u (&rc)[G][2]) __attribute__((always_inline)) {
        const uint64_t row0 = (blockIdx.x + it * gridDim.x) * BM;
        const unsigned char *csrc = sp_uniform_ptr((uint64_t)(uintptr_t)(rows + row0 * a.row_stride + b * (G * 64u)));
        const uint32_t gsz = nch - b * G < (uint32_t)G ? nch - b * G : (uint32_t)G;
        uint32_t r0 = rl0, r1 = rl1;
        const uint64_t room = last_row - row0;                      // (row0 <= last_row: the tile exists)
        if (room < BM - 1) {                                     // the block's last, partial tile (wave-uniform)
            r0 = (uint64_t)rl0 < room ? rl0 : (uint32_t)room;
            r1 = (uint64_t)rl1 < room ? rl1 : (uint32_t)room;
        }
        const uint32_t o0 = r0 * row_stride32 + kq_r * 16u, o1 = r1 * row_stride32 + kq_r * 16u;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const uint32_t jj = (uint32_t)j < gsz ? (uint32_t)j : gsz - 1u;
            uw_gload16(rc[j][0], csrc, o0 + jj * 64u);
            uw_gload16(rc[j][1], csrc, o1 + jj * 64u);
        }
    };

    i32x4u acc[2][8];
    SpWaveList list(s.wlist, s.wcap, blockIdx.x * (WAVES) + (uint32_t)w);
    const uint32_t n_rows32 = (uint32_t)a.n_cand;
    // the columns' entries of the lane's eight rows of the running tile (rows 4 kq_r .. + 3 of both 16-row tiles of the wave): inside the columns also in
    // the block's last tile - they are padded to whole tiles (u8w_col_entries)
    i32x4u ci8[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, cf8[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    auto load_cols = [&](uint64_t it) __attribute__((always_inline)) {
        const uint64_t row0 = (blockIdx.x + it * gridDim.x) * BM;
        const unsigned char *src = sp_uniform_ptr((uint64_t)(uintptr_t)(s.col + row0));
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const uint32_t r = (uint32_t)w * 32u + (uint32_t)mt * 16u + 4 * kq_r;
            uw_gload16(ci8[mt], src, r * 4u);
            if constexpr (COS) uw_gload16(cf8[mt], sp_uniform_ptr((uint64_t)(uintptr_t)(s.colf + row0)), r * 4u);
        }
    };
    auto col_f = [&](int mt, int j) __attribute__((always_inline)) { return __int_as_float(cf8[mt][j]); };

    auto epilogue = [&](uint64_t it) __attribute__((always_inline)) {
        const uint64_t tile = blockIdx.x + it * gridDim.x;
        const uint32_t row0 = (uint32_t)(tile * BM) + (uint32_t)w * 32u + 4 * kq_r;
        uint32_t hits8 = 0;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const int q = nt * 16 + (int)m_r;
            if constexpr (COS) {
                const float k = kq_lds[q];
                float mx = -__builtin_inff();
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) mx = __builtin_fmaxf(mx, __builtin_fmaf(-k, col_f(mt, j), (float)(acc[mt][nt][j] + ci8[mt][j])));
                if (mx >= aq_lds[q]) hits8 |= 1u << nt;
            } else {
                int mx = (int)0x80000000;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int v = (METRIC == M_EUCLID ? 2 * acc[mt][nt][j] : acc[mt][nt][j]) + ci8[mt][j];
                        mx = v > mx ? v : mx;
                    }
                if (mx >= thr_lds[q]) hits8 |= 1u << nt;
            }
        }
        if (!__ballot(hits8 != 0)) return;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            if (!__ballot((hits8 >> nt) & 1u)) continue;
            const uint32_t q = (uint32_t)nt * 16 + m_r;
            const int ti = thr_lds[q];
            const float k = kq_lds[q], aq = aq_lds[q];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int v = acc[mt][nt][j];
                    const uint32_t row = row0 + (uint32_t)mt * 16 + (uint32_t)j;
                    bool hit;
                    if constexpr (COS) hit = __builtin_fmaf(-k, col_f(mt, j), (float)(v + ci8[mt][j])) >= aq;
                    else hit = (METRIC == M_EUCLID ? 2 * v : v) + ci8[mt][j] >= ti;
                    list.append_raw(hit && row < n_rows32 && q < s.nq, (uint32_t)v, row, q);
                }
            }
        }
    };

    const uint64_t n_groups = my_tiles * ngr;
    // the group the loads are at, as (tile, b), by running counters; past the block's last group they repeat it (the waits count loads, not bytes)
    uint64_t itr = 0;
    uint32_t br = 0;
    auto advance_r = [&]() {
        if (br + 1 < ngr) ++br;
        else if (itr + 1 < my_tiles) { br = 0; ++itr; }
    };
    i32x4u rc[SLOTS][G][2];
    // ---- prologue: the loads of groups 0 .. AHEAD - 1 ----
    uw_static_for<0, AHEAD>([&](auto DC) __attribute__((always_inline)) {
        load_group(itr, br, rc[decltype(DC)::value]);
        advance_r();
    });
    uint64_t it = 0;
    uint32_t b = 0;
    // one group; I = g mod SLOTS selects the register sets at compile time
    auto one_group = [&](auto IC) __attribute__((always_inline)) {
        constexpr int I = decltype(IC)::value, IL = (I + AHEAD) % SLOTS;
        if (b == 0) {
            if (it) {
                if (ngr < (uint32_t)AHEAD) uw_wait_vm_dyn(2u * G * ngr);
                asm volatile("" : "+v"(ci8[0]), "+v"(ci8[1]) : : "memory");
                if constexpr (COS) asm volatile("" : "+v"(cf8[0]), "+v"(cf8[1]) : : "memory");
                epilogue(it - 1);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 8; ++nt) acc[mt][nt] = (i32x4u){0, 0, 0, 0};
            load_cols(it);
        }
        // group g + AHEAD -> the register set group g - 1 ran on
        load_group(itr, br, rc[IL]);
        advance_r();
        const uint32_t gsz = nch - b * G < (uint32_t)G ? nch - b * G : (uint32_t)G;
        // all but the last 2 G AHEAD loads have landed: this group's bytes among them
        asm volatile("s_waitcnt vmcnt(%0)" : : "n"(2 * G * AHEAD) : "memory");
#pragma unroll
        for (int J = 0; J < G; ++J) asm volatile("" : "+v"(rc[I][J][0]), "+v"(rc[I][J][1]) : : "memory");
        // the bias: unsigned bytes -> int8 (x - 128), in the operand registers
#pragma unroll
        for (int J = 0; J < G; ++J)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) rc[I][J][mt] ^= (i32x4u){(int)UW_BIAS, (int)UW_BIAS, (int)UW_BIAS, (int)UW_BIAS};
#pragma unroll
        for (int J = 0; J < G; ++J) {
            if ((uint32_t)J < gsz) {
                const uint4 *bb = b_rd + (b * G + J) * UW_B_UNITS;
                constexpr int B_AHEAD = 3;
                i32x4u bv[B_AHEAD + 1];
#pragma unroll
                for (int k = 0; k < B_AHEAD; ++k) bv[k] = *reinterpret_cast<const i32x4u *>(bb + k * 64);
#pragma unroll
                for (int nt = 0; nt < 8; ++nt) {
                    if (nt + B_AHEAD < 8) bv[(nt + B_AHEAD) % (B_AHEAD + 1)] = *reinterpret_cast<const i32x4u *>(bb + (nt + B_AHEAD) * 64);
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(rc[I][J][mt], bv[nt % (B_AHEAD + 1)], acc[mt][nt], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (++b == ngr) { b = 0; ++it; }
    };
    for (uint64_t g = 0; g < n_groups; g += SLOTS) {
        uw_static_for<0, SLOTS>([&](auto IC) __attribute__((always_inline)) {
            if (g + decltype(IC)::value < n_groups) one_group(IC);
        });
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(ci8[0]), "+v"(ci8[1]) : : "memory");
    if constexpr (COS) asm volatile("" : "+v"(cf8[0]), "+v"(cf8[1]) : : "memory");
    epilogue(my_tiles - 1);
    list.finish(s.wcnt, blockIdx.x * (WAVES) + (uint32_t)w, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- The scan of rows of 1 088 .. 2 048 bytes: the queries' image (136 .. 256 KiB) no longer fits in LDS, so rows AND queries are staged, with the work split
// and the rings of sp_staged_scan / scan_l2i8_staged_kernel (this kernel is a text of its own: its rows are no LDS image but the row-major u8 block itself).
// block = 8 waves = 4 row quarters (wm) x 2 query halves (wn), acc[4][4] per wave; a stage = 256 rows x 128 bytes of K = 32 KiB of rows + 16 KiB of query
// images (u8w_pack_kernel wrote them in LDS order: a verbatim LDS-DMA copy from L2), three stages of each in LDS; per stage and wave six 1 KiB requests spread
// between 32 matrix instructions, ONE s_waitcnt vmcnt and the stage barrier.
// The rows.  LDS-DMA puts lane i's 16 bytes at dst + 16 i, but the GLOBAL address is the lane's own: the lane that owns unit p of a request fetches the
// (row, piece) the operand layout sp_unit wants at p.  Request i (0 .. 3) of wave w fills units 256 w + 64 i + lane = sp_unit(2 w + (i >> 1), i & 1, kq, m)
// with kq = lane >> 4, m = (lane & 15) ^ (2 kq): bytes [64 (i & 1) + 16 kq, + 16) of the stage's 128 of row 16 (2 w + (i >> 1)) + m of the tile.  An
// instruction touches sixteen 64-byte half-lines (the resident kernel's pattern); requests 2 j and 2 j + 1 ask for the two halves of the same sixteen lines
// back to back.  Lane offsets are 32-bit inside a tile (u8w_segment_ok).  Rows past the block (the last tile) clamp to its last row and are dropped by number.
// A row of 64 (mod 128) bytes ends in a stage of ONE chunk: the requests of the missing chunk repeat the real one - no byte past dim of any row is read - and
// the pack made the queries' missing chunk q' = 0.  The bias is applied to the A operand in registers, between its ds_read and the matrix instruction.
// The columns come the way N_r does in scan_l2i8_staged_kernel: at the top of a tile's FIRST stage - in front of that stage's requests - a wave requests the
// 64 C[row] of its row quarter with one global_load_lds_dword (Cosine: the 64 F[row] with a second) into a slot of its own behind the rings, tile it -> slot
// it & 1, and the tile's epilogue reads the lane's sixteen back with four ds_read_b128 (eight).  The wave reads only what it copied itself: no barrier.
// The vector-memory count, stage by stage (it retires in order; requests of stage g: [C (, F) of the tile if kc == 0, queries of g + 2, rows of g + 2]):
//   kc == 0: seven requests (Cosine: eight), s_waitcnt vmcnt(7) (vmcnt(8));  kc > 0: six, vmcnt(6)
// - either way exactly the stage's OWN requests stay out, so rows and queries of stage g + 1 have landed, and so have, after the tile's second stage, its
// columns (a tile has at least nine stages).  The epilogue of tile it runs at the top of tile it + 1, in FRONT of that stage's requests (its stores retire
// under the same wait), or after the last stage.  The request of tile it + 1, issued right after the epilogue of tile it, lands in the OTHER slot; the one
// that lands on slot it & 1 again is tile it + 2's, a whole tile after those reads.
// The epilogue is the resident kernel's per metric, from registers: the lane's four queries' bound (Dot, Euclid) or k and a (Cosine), narrowing by
// wave-uniform steps - the query tile, the 16-row tile, the lane's four rows. ----
constexpr uint32_t UWS_RING_BYTES = (SP3_ARING * SP3_A_UNITS + 3 * SP_B_UNITS) * 16;      // 96 + 48 KiB
constexpr uint32_t UWS_NSLOTS = 2;                                                        // column slots per wave
constexpr uint32_t uws_lds_bytes(bool cosine) { return UWS_RING_BYTES + (UW_THREADS / 64) * UWS_NSLOTS * (cosine ? 512u : 256u); }      // + 4 KiB (Cosine: 8)
// 256 B of global memory (wave-uniform base, lane i fetches bytes 4 i .. 4 i + 3) into LDS at the wave-uniform byte address lds_dst
__device__ __forceinline__ void uw_glds4(const unsigned char *src, uint32_t lane_off, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(src), "s"(lds_dst) : "memory");
}
template <int METRIC>
__global__ __launch_bounds__(UW_THREADS, 1) void scan_u8w_staged_kernel(const ScanArgs a, const U8WideArgs s) {
    constexpr int BRING = 3, WAVES = UW_THREADS / 64, BM = UW_BM;
    constexpr bool COS = METRIC == M_COSINE;
    constexpr uint32_t CB = COS ? 512u : 256u;                    // bytes of a column slot: C, then F
    static_assert(UW_THREADS == SP3_THREADS && UW_BM == SP3_BM && UW_QT == SP_QT, "the staged scans' work split");
    static_assert(uws_lds_bytes(true) <= 160 * 1024, "one block per CU");
    static_assert((UW_RES_NCH + 2) / 2 >= 3, "the shortest staged tile ((UW_RES_NCH + 2) / 2 stages): its columns land at least two stages before its epilogue");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t n_tiles = (a.n_cand + BM - 1) / BM;
    const uint32_t nch = s.nch, nst = (nch + 1) / 2;              // 64-byte chunks, 128-byte stages per tile
    const uint64_t my_tiles = blockIdx.x < n_tiles ? (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    if (my_tiles == 0) {
        SpWaveList::none(s.wcnt, blockIdx.x * WAVES + (uint32_t)w, lane);
        return;
    }
    auto my_tile = [&](uint64_t i) -> uint64_t { return blockIdx.x + i * gridDim.x; };
    const uint32_t wm = (uint32_t)w & 3u, wn = (uint32_t)w >> 2;
    const uint32_t kq_r = (uint32_t)lane >> 4, m_r = (uint32_t)lane & 15u;
    const uint32_t a_rd = sp_unit(wm * 4, 0, kq_r, m_r), b_rd = sp_unit(wn * 4, 0, kq_r, m_r);
    // the wave's 64 queries, 4 per lane (query 64 wn + 16 nt + m_r): the compare's terms; a dead slot or a query without a bound admits nothing (u8w_pack_kernel)
    typedef std::conditional_t<COS, float, int32_t> val_t;       // what a pair is compared in: Dot V = I + C, Euclid V = 2 I + C, Cosine fma(-k, F, fl32(I + C))
    val_t lim[4];                                                 // ... against the integer bound, or the cosine's a
    float nk[4];                                                  // the cosine's -k
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const uint32_t q = wn * 64 + (uint32_t)nt * 16 + m_r;
        if constexpr (COS) {
            lim[nt] = s.aq[q];
            nk[nt] = -s.kq[q];
        } else {
            lim[nt] = s.thr_i[q];
            nk[nt] = 0.0f;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // from here on the kernel counts its vector-memory traffic itself
    const uint32_t lds0 = (uint32_t)(uintptr_t)(sp_lds_byte *)smem_raw;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    uint4 *b_lds = lds + SP3_ARING * SP3_A_UNITS;
    // the wave's column slots: bytes, and as the lane reads them (its rows 16 mt + 4 kq_r + j of the quarter: piece 4 mt + kq_r)
    const uint32_t c_slot0 = UWS_RING_BYTES + (uint32_t)w * (UWS_NSLOTS * CB);
    const uint4 *c_rd = reinterpret_cast<const uint4 *>(smem_raw + c_slot0) + kq_r;
    const unsigned char *rows = reinterpret_cast<const unsigned char *>(a.rows);
    const uint64_t last_row = a.n_cand - 1;
    const uint32_t row_stride32 = (uint32_t)a.row_stride;
    // the rows the lane fetches for requests 0, 1 and 2, 3 of a stage, and its piece of their 64-byte chunk
    const uint32_t rl0 = (uint32_t)w * 32u + (m_r ^ (2u * kq_r)), rl1 = rl0 + 16u;
    // the copy streams, as in sp_staged_scan: running (tile, stage) counters; past the block's last stage the requests repeat it into a slot nobody reads
    uint64_t ra_it = 0;
    uint32_t ra_kc = 0, ra_slot = 0, rb_kc = 0, rb_slot = 0;
    const unsigned char *ra_src = nullptr, *rb_src = nullptr;
    uint32_t ra_dst = 0, rb_dst = 0, ra_hi = 0, ra_off0 = 0, ra_off1 = 0;
    auto rows_begin = [&]() {
        const uint64_t row0 = my_tile(ra_it) * BM;
        ra_src = sp_uniform_ptr((uint64_t)(uintptr_t)(rows + row0 * a.row_stride + ra_kc * 128u));
        ra_hi = ra_kc * 2u + 1u < nch ? 64u : 0u;                // the stage's second chunk, or - past the row's end - the first again
        uint32_t r0 = rl0, r1 = rl1;
        const uint64_t room = last_row - row0;                   // (row0 <= last_row: the tile exists)
        if (room < BM - 1) {                                     // the block's last, partial tile (wave-uniform)
            r0 = (uint64_t)rl0 < room ? rl0 : (uint32_t)room;
            r1 = (uint64_t)rl1 < room ? rl1 : (uint32_t)room;
        }
        ra_off0 = r0 * row_stride32 + kq_r * 16u;
        ra_off1 = r1 * row_stride32 + kq_r * 16u;
        ra_dst = lds0 + (ra_slot * SP3_A_UNITS) * 16u + (uint32_t)w * 4096u;
        ra_slot = sp_ring_next<SP3_ARING>(ra_slot);
        if (ra_kc + 1 < nst) ++ra_kc;
        else if (ra_it + 1 < my_tiles) { ra_kc = 0; ++ra_it; }
    };
    // (non-temporal: both halves of a line are asked for back to back and never again)
    auto rows_piece = [&](int i) { sp_glds16_nt(ra_src + (i & 1 ? ra_hi : 0u), i & 2 ? ra_off1 : ra_off0, ra_dst + i * 1024); };
    auto queries_begin = [&]() {
        rb_src = sp_uniform_ptr((uint64_t)(uintptr_t)(s.bq + (uint64_t)rb_kc * SP_B_UNITS) + (uint32_t)w * 2048u);
        rb_dst = lds0 + (SP3_ARING * SP3_A_UNITS + rb_slot * SP_B_UNITS) * 16u + (uint32_t)w * 2048u;
        rb_slot = sp_ring_next<BRING>(rb_slot);
        rb_kc = rb_kc + 1 == nst ? 0 : rb_kc + 1;
    };
    auto queries_piece = [&](int i) { sp_glds16(rb_src + i * 1024, lane_off, rb_dst + i * 1024); };
    // C (and F) of the wave's row quarter of a tile -> slot it & 1 (inside the columns also in the block's last tile: they are padded to whole tiles, u8w_col_entries)
    auto request_cols = [&](uint64_t it) {
        const uint64_t row0 = my_tile(it) * BM + wm * 64u;
        const uint32_t dst = lds0 + c_slot0 + ((uint32_t)it & 1u) * CB;
        uw_glds4(sp_uniform_ptr((uint64_t)(uintptr_t)(s.col + row0)), (uint32_t)lane * 4u, dst);
        if constexpr (COS) uw_glds4(sp_uniform_ptr((uint64_t)(uintptr_t)(s.colf + row0)), (uint32_t)lane * 4u, dst + 256u);
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
    // the epilogue of tile it: accumulator register j of (mt, nt) = row 256 tile + 64 wm + 16 mt + 4 kq_r + j, query 64 wn + 16 nt + m_r
    auto epilogue = [&](uint64_t it) __attribute__((always_inline)) {
        const uint32_t row0 = (uint32_t)(my_tile(it) * BM) + wm * 64 + 4 * kq_r;
        const uint4 *cp = c_rd + ((uint32_t)it & 1u) * (CB / 16u);
        i32x4s cr[4];
        f32x4s fr[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            cr[mt] = *reinterpret_cast<const i32x4s *>(cp + mt * 4);
            if constexpr (COS) fr[mt] = *reinterpret_cast<const f32x4s *>(cp + 16 + mt * 4);
        }
        auto val = [&](int mt, int nt, int j) __attribute__((always_inline)) -> val_t {
            const int v = (METRIC == M_EUCLID ? 2 * acc[mt][nt][j] : acc[mt][nt][j]) + cr[mt][j];
            if constexpr (COS) return __builtin_fmaf(nk[nt], fr[mt][j], (float)v);
            else return v;
        };
        auto max4 = [&](int mt, int nt) __attribute__((always_inline)) -> val_t {
            val_t mx = val(mt, nt, 0);
#pragma unroll
            for (int j = 1; j < 4; ++j) mx = val(mt, nt, j) > mx ? val(mt, nt, j) : mx;
            return mx;
        };
        bool hit[4];
        bool maybe = false;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            val_t mx = max4(0, nt);
#pragma unroll
            for (int mt = 1; mt < 4; ++mt) mx = max4(mt, nt) > mx ? max4(mt, nt) : mx;
            hit[nt] = mx >= lim[nt];
            maybe = maybe || hit[nt];
        }
        if (!__ballot(maybe)) return;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            if (!__ballot(hit[nt])) continue;
            const uint32_t q = wn * 64 + (uint32_t)nt * 16 + m_r;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                if (!__ballot(max4(mt, nt) >= lim[nt])) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t row = row0 + (uint32_t)mt * 16 + (uint32_t)j;
                    list.append_raw(val(mt, nt, j) >= lim[nt] && row < n_rows32 && q < s.nq, (uint32_t)acc[mt][nt][j], row, q);
                }
            }
        }
    };
    const i32x4s bias = {(int)UW_BIAS, (int)UW_BIAS, (int)UW_BIAS, (int)UW_BIAS};
    for (uint64_t it = 0; it < my_tiles; ++it) {
        if (it) epilogue(it - 1);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = (i32x4s){0, 0, 0, 0};
        for (uint32_t kc = 0; kc < nst; ++kc) {
            if (kc == 0) request_cols(it);                // the stage's first request(s)
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
                // the bias: unsigned bytes -> int8 (x - 128), in the operand registers
                const i32x4s a0 = *reinterpret_cast<const i32x4s *>(ab + mt * 128) ^ bias;
                const i32x4s a1 = *reinterpret_cast<const i32x4s *>(ab + mt * 128 + 64) ^ bias;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1[nt], acc[mt][nt], 0, 0, 0);
                // the stage's six copy requests, in the order the wait below relies on (queries first), spread over the matrix work; the two halves of the
                // rows' 128-byte lines back to back
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
            // all but this stage's own requests have landed: rows and queries of stage g + 1 among them, and by the tile's second stage its columns
            if (kc == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(COS ? 8 : 7) : "memory");
            else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            sp_stage_barrier();
        }
    }
    epilogue(my_tiles - 1);
    list.finish(s.wcnt, blockIdx.x * WAVES + (uint32_t)w, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // nothing may land in LDS after the block is gone
}

// ---- after the scan: an entry (I, row, query) becomes (key lo, key hi, query) with the pass's score A (u8w_score of the pair's exact integers) when A is
// not below the query's cut T - band, else an entry the regroup skips.  One wave per list. ----
__global__ __launch_bounds__(256) void u8w_finish_kernel(uint4 *wlist, const uint32_t *wcnt, uint32_t wcap, uint32_t n_lists, int metric, const int32_t *col,
                                                         const int32_t *n2, const int32_t *qoff, const int32_t *n1, const float *cut) {
    const uint32_t l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= n_lists) return;
    uint32_t cnt = wcnt[l];
    cnt = cnt < wcap ? cnt : wcap;
    uint4 *list = wlist + (uint64_t)l * wcap;
    for (uint32_t i = threadIdx.x & 63u; i < cnt; i += 64) {
        const uint4 e = list[i];
        const uint32_t row = e.y, q = e.z;
        const int64_t dot = (int64_t)(int32_t)e.x;
        const int64_t z = (metric == U8W_EUCLID ? 2 * dot : dot) + col[row] + qoff[q];
        const float score = u8w_score(metric, z, n1[q], metric == U8W_COSINE ? n2[row] : 0);
        list[i] = !(score < cut[q]) ? SpWaveList::entry(score, row, q) : SpWaveList::withdrawn();
    }
}

// ---- The conditional exact pass: the queries whose lists overflowed (packed by launch_split_plan: a.queries, a.del.filter_of; *a.run_if = how many) take the
// exact u8 top-k scan, 16 per block row - grid.y = the 16-query groups of the batch, a block row whose group holds none returns at once, which on a search
// without overflow is every block.  Per (row, query) the instructions of the 16-query tile of scan_kernel<RowU8<METRIC>, 16, ...> (scan_common.hpp:
// scan_step, RowU8::finish - the reference's bits in either order of QMX_SEG_U8_SCALAR_ORDER), over the whole block (no id list, no key bound);
// a.partial: grid.x x groups lists of 16 x top keys, group-major, as launch_merge_keys(..., grouped) reads them (scan_l2i8.hip: the same pass over f32) ----
template <int METRIC, bool PERQ>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_u8_exact_groups_kernel(const ScanArgs a) {
    typedef RowU8<METRIC> P;
    constexpr int QT = 16, R = P::R16, NW = SCAN_BLOCK / WAVE, NRA = P::NRAUX > 0 ? P::NRAUX : 1;
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
    const int piece = lane_piece(t), piece_off = piece * 16;
    const bool piece_in_rem = piece < (int)a.rem_pieces;
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
        typename P::acc_t acc[QT][R][P::NACC], raux[R][NRA];
#pragma unroll
        for (int q = 0; q < QT; ++q)
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int k = 0; k < P::NACC; ++k) acc[q][r][k] = 0;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < NRA; ++k) raux[r][k] = 0;
#pragma unroll 2
        for (uint32_t sg = 0; sg < a.nseg; ++sg) {
            uint4 v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) v[r] = load_row_piece<true>(rp[r] + (uint64_t)sg * 128);
            scan_step<P, QT, R>(acc, raux, v, smem, sg * 128 + piece_off, a.q_stride, true);
        }
        if (a.rem_pieces) {      // the last, partial 128-byte segment (rows of 64 (mod 128) bytes): pieces past it are zero on both sides, rows are never read past
            uint4 v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                v[r] = make_uint4(0, 0, 0, 0);
                if (piece_in_rem) v[r] = *reinterpret_cast<const uint4 *>(rp[r] + (uint64_t)a.nseg * 128);
            }
            scan_step<P, QT, R>(acc, raux, v, smem, a.nseg * 128 + piece_off, a.q_stride, piece_in_rem);
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
static int u8w_metric(int distance) { return distance == QMX_DISTANCE_DOT ? U8W_DOT : distance == QMX_DISTANCE_EUCLID ? U8W_EUCLID : distance == QMX_DISTANCE_COSINE ? U8W_COSINE : -1; }
bool u8w_segment_ok(int distance, uint32_t dim, uint64_t row_stride, uint64_t n) {
    return u8w_metric(distance) >= 0 && dim % 64 == 0 && dim >= 64 && dim <= UW_MAX_DIM && row_stride % 16 == 0 && n >= (1u << 18) && n < 0xFFFFFFFFull &&
           row_stride * (UW_BM - 1) + dim < (1ull << 31);
}
// the queries' image: [dim / 64] stages of 8 KiB for the resident scan, [stages of 128 bytes] of 16 KiB for the staged one (u8w_pack_kernel)
size_t u8w_query_bytes(uint32_t dim) {
    const uint32_t nch = dim / 64;
    return nch <= UW_RES_NCH ? (size_t)nch * UW_B_UNITS * 16 : (size_t)((nch + 1) / 2) * SP_B_UNITS * 16;
}
size_t u8w_wlists_counts_bytes(int num_cus) { return ((size_t)num_cus * (UW_THREADS / 64) * 4 + 255) / 256 * 256; }
size_t u8w_wlists_bytes(int num_cus) { return u8w_wlists_counts_bytes(num_cus) + (size_t)num_cus * (UW_THREADS / 64) * UW_WCAP * 16; }
uint32_t u8w_wcap() { return UW_WCAP; }
uint64_t u8w_col_entries(uint64_t n) { return (n + UW_BM - 1) / UW_BM * UW_BM; }

// d_col: u8w_col_entries(n) entries; Cosine: d_colf as many, d_n2 n
int32_t launch_u8w_columns(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, int distance, int32_t *d_col, float *d_colf, int32_t *d_n2) {
    const int metric = u8w_metric(distance);
    QMX_REQUIRE(u8w_segment_ok(distance, dim, row_stride, n) && d_col && (metric != U8W_COSINE || (d_colf && d_n2)), QMX_ERR_BAD_ARG, "u8 wide columns of dim %u", dim);
    ::qmx::clear_stale_error();
    const uint64_t n_pad = u8w_col_entries(n);
    hipLaunchKernelGGL(u8w_columns_kernel, dim3((uint32_t)std::min<uint64_t>(8192, n_pad / 16)), dim3(256), 0, st, (const unsigned char *)rows, row_stride, n, n_pad, dim,
                       metric, d_col, d_colf, d_n2);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

// one 128-query tile (a.queries: u8 entries): d_bq u8w_query_bytes(dim); k: eight arrays of 128 entries; zeroes the tile's candidate counters
int32_t launch_u8w_pack(hipStream_t st, const ScanArgs &a, int distance, const uint64_t *d_gthr, void *d_bq, float *d_t_exact, float *d_band, float *d_cut,
                        int32_t *d_thr_i, float *d_kq, float *d_aq, int32_t *d_qoff, int32_t *d_n1, uint32_t *d_cand_cnt, uint32_t n_cnt) {
    QMX_REQUIRE(a.nq <= (uint32_t)UW_QT && u8w_metric(distance) >= 0 && a.dim % 64 == 0 && a.dim >= 64 && a.dim <= UW_MAX_DIM && a.q_stride >= a.dim, QMX_ERR_BAD_ARG,
                "u8 wide tile of %u queries", a.nq);
    ::qmx::clear_stale_error();
    const U8WideQuery k{d_t_exact, d_band, d_cut, d_thr_i, d_kq, d_aq, d_qoff, d_n1};
    hipLaunchKernelGGL(u8w_pack_kernel, dim3(UW_QT), dim3(64), 0, st, (const unsigned char *)a.queries, a.q_stride, a.nq, a.dim, u8w_metric(distance),
                       a.flags & QMX_SEG_U8_SCALAR_ORDER, d_gthr, (uint4 *)d_bq, k, d_cand_cnt, n_cnt);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

// d_wlists: [counts: u8w_wlists_counts_bytes][lists]; *grid_out = blocks launched (8 lists each).  The scan, then the finish of its lists
int32_t launch_scan_u8w(hipStream_t st, const ScanArgs &a, int distance, const void *d_bq, const int32_t *d_thr_i, const float *d_kq, const float *d_aq,
                        const int32_t *d_col, const float *d_colf, const int32_t *d_n2, const int32_t *d_qoff, const int32_t *d_n1, const float *d_cut, int num_cus,
                        void *d_wlists, uint32_t *grid_out) {
    const int metric = u8w_metric(distance);
    QMX_REQUIRE(u8w_segment_ok(distance, a.dim, a.row_stride, a.n_rows) && !a.ids && a.n_cand >= 1 && a.n_cand <= a.n_rows && a.nq <= (uint32_t)UW_QT && d_col &&
                    d_wlists && (metric != U8W_COSINE || (d_colf && d_n2)),
                QMX_ERR_NOT_SUPPORTED, "u8 wide scan: shape not supported");
    U8WideArgs s;
    s.bq = (const uint4 *)d_bq;
    s.nch = a.dim / 64;
    s.nq = a.nq;
    s.thr_i = d_thr_i;
    s.kq = d_kq;
    s.aq = d_aq;
    s.col = d_col;
    s.colf = d_colf;
    s.wcnt = (uint32_t *)d_wlists;
    s.wlist = (uint4 *)((unsigned char *)d_wlists + u8w_wlists_counts_bytes(num_cus));
    s.wcap = UW_WCAP;
    const uint64_t n_tiles = (a.n_cand + UW_BM - 1) / UW_BM;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)num_cus, n_tiles);
    // rows of up to 1 024 bytes: the queries resident; longer ones: the staged rings
    const bool resident = s.nch <= UW_RES_NCH;
    const size_t lds_bytes = resident ? (size_t)s.nch * UW_B_UNITS * 16 + UW_LDS_TAIL : (size_t)uws_lds_bytes(metric == U8W_COSINE);
    void (*kfn)(const ScanArgs, const U8WideArgs) =
        resident ? (metric == U8W_DOT ? scan_u8w_kernel<M_DOT, 2, 2> : metric == U8W_EUCLID ? scan_u8w_kernel<M_EUCLID, 2, 2> : scan_u8w_kernel<M_COSINE, 2, 2>)
                 : (metric == U8W_DOT ? scan_u8w_staged_kernel<M_DOT> : metric == U8W_EUCLID ? scan_u8w_staged_kernel<M_EUCLID> : scan_u8w_staged_kernel<M_COSINE>);
    static thread_local DeviceOnce once;
    ::qmx::clear_stale_error();
    if (once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_u8w_staged_kernel<M_DOT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)uws_lds_bytes(false)));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_u8w_staged_kernel<M_EUCLID>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)uws_lds_bytes(false)));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_u8w_staged_kernel<M_COSINE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)uws_lds_bytes(true)));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_u8w_kernel<M_DOT, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, UW_LDS_MAX));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_u8w_kernel<M_EUCLID, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, UW_LDS_MAX));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_u8w_kernel<M_COSINE, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, UW_LDS_MAX));
        once.mark();
    }
    QMX_NOTE_KERNEL(kfn);
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(UW_THREADS), lds_bytes, st, a, s);
    QMX_HIP(hipGetLastError());
    const uint32_t n_lists = grid * (UW_THREADS / 64);
    hipLaunchKernelGGL(u8w_finish_kernel, dim3((n_lists + 3) / 4), dim3(256), 0, st, s.wlist, s.wcnt, s.wcap, n_lists, metric, d_col, d_n2, d_qoff, d_n1, d_cut);
    QMX_HIP(hipGetLastError());
    if (grid_out) *grid_out = grid;
    return QMX_OK;
}

// a.nq packed slots in a.queries (a.del.filter_of packed with them), *a.run_if = how many of them are to be scanned; a.partial: grid.x x groups lists of 16 x top
// keys.  *grid_out: in: the cap on grid.x, out: grid.x
template <int METRIC>
static int32_t launch_u8_exact_groups_metric(hipStream_t st, const ScanArgs &a, int num_cus, uint32_t *grid_out) {
    constexpr int QT = 16, NW = SCAN_BLOCK / WAVE;
    size_t lds = std::max((size_t)QT * a.q_stride, (size_t)NW * QT * a.top * sizeof(uint64_t));
    lds = (lds + 15) & ~(size_t)15;
    QMX_REQUIRE(lds <= 160 * 1024, QMX_ERR_NOT_SUPPORTED, "query tile needs %zu B of LDS (> 160 KiB)", lds);
    void (*kfn)(const ScanArgs) = a.del.filter_of ? scan_u8_exact_groups_kernel<METRIC, true> : scan_u8_exact_groups_kernel<METRIC, false>;
    static thread_local DeviceOnce once;
    ::qmx::clear_stale_error();
    if (once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_u8_exact_groups_kernel<METRIC, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_u8_exact_groups_kernel<METRIC, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        once.mark();
    }
    const uint64_t n_tiles = (a.n_cand + 8 * RowU8<METRIC>::R16 - 1) / (8 * RowU8<METRIC>::R16);
    uint32_t grid = (uint32_t)std::min<uint64_t>((n_tiles + NW - 1) / NW, (uint64_t)num_cus);
    if (grid < 1) grid = 1;
    if (*grid_out && grid > *grid_out) grid = *grid_out;
    *grid_out = grid;
    hipLaunchKernelGGL(kfn, dim3(grid, (a.nq + QT - 1) / QT), dim3(SCAN_BLOCK), lds, st, a);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_scan_u8_exact_groups(hipStream_t st, int distance, const ScanArgs &a, int num_cus, uint32_t *grid_out) {
    QMX_REQUIRE(a.run_if && a.partial && !a.ids && !a.key_bound && a.nq >= 1 && grid_out && a.top >= 1 && a.top <= (uint32_t)MAX_TOP_FAST && a.dim >= 32 &&
                    a.tail_start == a.dim && (a.nseg * 8 + a.rem_pieces) * 16 == a.dim,
                QMX_ERR_BAD_ARG, "u8 exact groups: a packed conditional pass over whole 16-byte pieces");
    switch (distance) {
        case QMX_DISTANCE_DOT: return launch_u8_exact_groups_metric<M_DOT>(st, a, num_cus, grid_out);
        case QMX_DISTANCE_EUCLID: return launch_u8_exact_groups_metric<M_EUCLID>(st, a, num_cus, grid_out);
        case QMX_DISTANCE_COSINE: return launch_u8_exact_groups_metric<M_COSINE>(st, a, num_cus, grid_out);
    }
    set_error("u8 exact groups: distance %d", distance);
    return QMX_ERR_NOT_SUPPORTED;
}

}  // namespace qmx
