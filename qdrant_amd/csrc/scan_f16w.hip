// scan_f16w.hip - dense f16 rows (Metric<f16>, `datatype: float16`), brute-force top-k for LARGE query batches: 128 queries per pass of the block on
// v_mfma_f32_16x16x32_f16, with NO copy of the block (QMX_SEG_F16_WIDE; api_search.hip f16_wide_search).
//
// An f16 row already is the matrix cores' operand: lane (m, kq) of a 16-row tile holds bytes [16 kq, + 16) of a 64-byte chunk of row m - eight halfs, one
// K-step of 32 - which is the byte geometry of scan_u8w.hip's int8 operand, so the work split and the data movement are that file's.  What is this
// operand's own: f32 accumulators in an order the hardware chooses, hence a band (f16w_band.hpp: |A - R| of the pass's score A against the reference's
// AVX-order score R, the sample's bound, subnormal operands), a float epilogue that lists the scored pair itself (no finish kernel), one f32 column
// N[row] = |x|^2 for Euclid and none for Dot / Cosine, and - because no f16 scan of the stored layout sums in the reference's order - a pair kernel and a
// conditional exact pass that keep the 32 running sums of metric_f16/avx/*.rs apart, so the lists carry the reference's bits.  In the file's order: the
// per-segment statistics, f16w_pack_kernel, scan_f16w_kernel (rows of up to 1 024 bytes: the queries' image resident in LDS), scan_f16w_staged_kernel
// (1 088 .. 2 048 bytes: rows and queries through LDS rings, the rows by LDS-DMA straight from the row-major block), the pair kernel, the exact pass.
//
// The tail is the wide routes': a strided sample's k-th best score T_q admits the candidates (A >= T_q - band), per-wave lists are regrouped per query,
// the selection keeps A >= max(T_q - band, A_k - 2 band), the pair kernel re-scores that and a query whose lists overflowed takes the exact pass.
#include "dense_policies.hpp"
#include "f16_avx_leaf.hpp"
#include "f16w_band.hpp"
#include "split_common.hpp"

namespace qmx {

typedef int i32x4h __attribute__((ext_vector_type(4)));
typedef float f32x4h __attribute__((ext_vector_type(4)));

constexpr int FW_THREADS = 512;
constexpr int FW_BM = 256;                                   // rows per tile
constexpr int FW_QT = 128;                                   // queries per pass
constexpr int FW_B_UNITS = FW_QT * 4;                        // 16-byte units of a 64-byte chunk of the queries' image: 8 KiB
constexpr uint32_t FW_RES_NCH = 16;                          // rows of up to 1 024 bytes (dim <= 512): the queries' whole image stays in LDS (128 KiB) - scan_f16w_kernel
constexpr uint32_t FW_MAX_NCH = 32;                          // ... of up to 2 048 (dim <= 1 024): staged through LDS rings - scan_f16w_staged_kernel
constexpr int FW_LDS_TAIL = FW_QT * 8;                       // behind the resident image: the cuts and Q
constexpr int FW_LDS_MAX = FW_RES_NCH * FW_B_UNITS * 16 + FW_LDS_TAIL;
static_assert(FW_MAX_NCH * 32 == F16W_MAX_DIM, "the band's derivation ends where the staged scan does");
static_assert(FW_LDS_MAX <= 160 * 1024, "one block per CU");
constexpr uint32_t FW_WCAP = 8192;                           // candidates one wave may list per pass

// unit index of (16-query tile t, piece kq, query-in-tile m) inside a chunk of the queries' image: conflict-free for the operand reads (scan_u8w.hip uw_unit)
__device__ __forceinline__ uint32_t fw_unit(uint32_t t, uint32_t kq, uint32_t m) { return (t * 4 + kq) * 16 + (m ^ (2 * kq)); }

struct F16WideArgs {
    const uint4 *bq;          // the queries' f16 bytes as operand images (f16w_pack_kernel): [nch][FW_B_UNITS], or - nch > FW_RES_NCH - [(nch + 1) / 2][SP_B_UNITS]
    uint32_t nch;             // 64-byte chunks (K-steps of 32 halfs) of a row: dim / 32
    uint32_t nq;              // live queries (<= 128)
    const float *cut;         // [128] a pair with A below this cannot reach the query's list (+inf: nothing passes)
    const float *qq;          // [128] Euclid: Qf
    const float *col;         // Euclid: [f16w_col_entries(n)] Nf[row]
    uint4 *wlist;             // [waves][wcap] (key lo, key hi, query, 0)
    uint32_t *wcnt;           // [waves] entries each wave wanted to append (may run past wcap: overflow)
    uint32_t wcap;
};

// ---- once per segment, one pass over the block: stats[0] = the largest |x|^2 as f32 bits, moved up (non-negative floats order as their bits),
// stats[1] != 0: an Inf / NaN element, stats[2] != 0: a subnormal element; Euclid: col[row] = fl32(|x|^2 summed in f64), padded with zeros to whole
// 256-row tiles (the scan loads the entries of a lane's four rows as one 16-byte piece, those of rows past the block included, and drops such rows by
// their number).  Sixteen lanes per row, a 16-byte piece per lane and step ----
__global__ __launch_bounds__(256) void f16w_stats_kernel(const unsigned char *rows, uint64_t row_stride, uint64_t n, uint64_t n_pad, uint32_t dim, float *col,
                                                         uint32_t *stats) {
    const uint32_t l16 = threadIdx.x & 15u;
    uint32_t bad = 0, sub = 0;
    float mx = 0.0f;
    for (uint64_t r = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 4); r < n_pad; r += (uint64_t)gridDim.x * 16) {
        double s2 = 0.0;
        if (r < n) {
            const uint4 *p = reinterpret_cast<const uint4 *>(rows + r * row_stride);
            for (uint32_t u = l16; u < dim / 8; u += 16) {
                const uint4 v = p[u];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t h = (w[e / 2] >> (16 * (e % 2))) & 0xFFFFu, ex = h & 0x7C00u;
                    bad |= ex == 0x7C00u;
                    sub |= ex == 0 && (h & 0x3FFu) != 0;
                    const double x = (double)fw_h2f(h);
                    s2 += x * x;
                }
            }
        }
        for (int o = 8; o >= 1; o >>= 1) s2 += __shfl_xor(s2, o, 64);
        if (l16 != 0) continue;
        if (col) col[r] = (float)s2;
        mx = __builtin_fmaxf(mx, f16w_up(s2));
    }
    if (mx > 0.0f && mx == mx) atomicMax(&stats[0], __float_as_uint(mx));
    if (bad) atomicOr(&stats[1], 1u);
    if (sub) atomicOr(&stats[2], 1u);
}

// ---- once per 128-query tile: one wave per query slot.  The query's f16 bytes in the B-operand images; Q, sum |q|, its subnormal count; from the sample's
// k-th best score T the band and the cut T - band, rounded down.  A dead slot, or a query without a usable bound (the sample holds fewer than k live
// rows, an Inf / NaN element), passes nothing and gets an infinite band: the selection sends such a query - alone - to the exact pass ----
__global__ __launch_bounds__(64) void f16w_pack_kernel(const unsigned char *queries, uint32_t q_stride, uint32_t nq, uint32_t dim, int metric, float rowmax,
                                                       uint32_t seg_subnormal, const uint64_t *gthr, uint4 *bq, float *t_exact, float *band, float *cut, float *qq,
                                                       uint32_t *cand_cnt, uint32_t n_cnt) {
    const uint32_t qi = blockIdx.x, lane = threadIdx.x;
    const bool live = qi < nq;
    if (qi == 0)
        for (uint32_t i = lane; i < n_cnt; i += 64) cand_cnt[i] = 0;
    const unsigned char *entry = queries + (uint64_t)qi * q_stride;
    F16WQuery s{0.0, 0.0, 0u, 0u};
    // dim <= 512: the resident scan's image ([dim / 32][FW_B_UNITS]).  Longer rows: the staged scan's - [stages of 128 bytes][SP_B_UNITS] in the unit order
    // its LDS-DMA copies verbatim; a last stage of one chunk (dim = 32 mod 64) gets its missing chunk as zeros, whose products are zero whatever the
    // (finite) row bytes are
    const uint32_t nch = dim / 32, n_pieces = nch > FW_RES_NCH ? (nch + 1) / 2 * 8 : nch * 4;
    for (uint32_t p = lane; p < n_pieces; p += 64) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (live && p < dim / 8) {
            v = *reinterpret_cast<const uint4 *>(entry + (uint64_t)p * 16);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t h = (w[e / 2] >> (16 * (e % 2))) & 0xFFFFu, ex = h & 0x7C00u;
                s.bad += ex == 0x7C00u;
                s.nsub += ex == 0 && (h & 0x3FFu) != 0;
                const double x = ex == 0x7C00u ? 0.0 : (double)fw_h2f(h);
                s.q2 += x * x;
                s.l1 += fabs(x);
            }
        }
        if (nch > FW_RES_NCH) bq[(uint64_t)(p >> 3) * SP_B_UNITS + sp_unit(qi >> 4, (p >> 2) & 1u, p & 3u, qi & 15u)] = v;
        else bq[(uint64_t)(p >> 2) * FW_B_UNITS + fw_unit(qi >> 4, p & 3u, qi & 15u)] = v;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        s.q2 += __shfl_xor(s.q2, o, 64);
        s.l1 += __shfl_xor(s.l1, o, 64);
        s.nsub += __shfl_xor(s.nsub, o, 64);
        s.bad += __shfl_xor(s.bad, o, 64);
    }
    if (lane != 0) return;
    float te = -__builtin_inff(), bd = __builtin_inff(), ct = __builtin_inff();
    const uint64_t key = live ? gthr[qi] : 0;
    const float t = key ? key_score(key) : 0.0f;
    if (key != 0 && s.bad == 0 && t == t && __builtin_fabsf(t) < 3.0e38f) {
        te = t;
        bd = f16w_band(metric, dim, s, rowmax, seg_subnormal != 0);
        ct = f16w_cut(t, bd);
    }
    t_exact[qi] = te;
    band[qi] = bd;
    cut[qi] = ct;
    qq[qi] = (float)s.q2;
}

// the pass's score of a pair (f16w_band.hpp: these operations, in this order)
template <int METRIC>
__device__ __forceinline__ float fw_score(float d, float nf, float qf) {
    if constexpr (METRIC == M_EUCLID) return __builtin_fmaf(2.0f, d, -nf) - qf;
    else return d;
}

// (non-temporal: a row's bytes are read once, by one CU; the two 64-byte halves of a line are asked for back to back)
__device__ __forceinline__ void fw_gload16(i32x4h &dst, const unsigned char *sbase, uint32_t voff) {
    asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(dst) : "v"(voff), "s"(sbase) : "memory");
}
// (the columns' entries: default policy)
__device__ __forceinline__ void fw_gload16_col(i32x4h &dst, const unsigned char *sbase, uint32_t voff) {
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(sbase) : "memory");
}
template <int I, int N, class F>
__device__ __forceinline__ void fw_static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        fw_static_for<I + 1, N>(f);
    }
}
// vmcnt(n) for a wave-uniform even n <= 14 (the immediate has to be one)
__device__ __forceinline__ void fw_wait_vm_dyn(uint32_t n) {
    switch (n >> 1) {
#define FW_W(k) case k: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * k) : "memory"); break;
        FW_W(1) FW_W(2) FW_W(3) FW_W(4) FW_W(5) FW_W(6) FW_W(7)
#undef FW_W
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

// ---- The scan of rows of up to 1 024 bytes.  Work split and data movement are scan_u8w_kernel's: block = 8 waves, one block per CU, persistent over 256-row
// tiles; the queries' WHOLE image RESIDENT in LDS (dim / 32 x 8 KiB: 128 KiB at dim 512) with the cuts and Q behind it, copied once per block - after that
// copy the waves share nothing: no barrier in the K-loop.  A wave OWNS 32 rows of the tile; lane (m, kg) loads, per 64-byte chunk, bytes [16 kg, + 16) of
// rows m and 16 + m straight from the row-major f16 block into its operand registers (`global_load_dwordx4 ... nt` by inline asm, by GROUPS of G chunks,
// AHEAD groups in front of the matrix work, waited for by the kernel's own in-order `s_waitcnt vmcnt`); a chunk is one K-step of
// v_mfma_f32_16x16x32_f16 against each of the eight query tiles.  Euclid: Nf of the lane's eight rows, two 16-byte loads on the tile's first group, IN FRONT of
// that group's row loads (in-order counting only makes the waits behind them more conservative; a tile of fewer groups than AHEAD: the explicit wait in
// front of the epilogue).  The epilogue evaluates A per pair (fw_score), narrowing by wave-uniform steps - any pair of a query tile, then the pairs -
// and lists (A, row, query) where A >= cut. ----
template <int METRIC, int G, int AHEAD>
__global__ __launch_bounds__(FW_THREADS, 1) void scan_f16w_kernel(const ScanArgs a, const F16WideArgs s) {
    constexpr int WAVES = FW_THREADS / 64, T = FW_THREADS, BM = FW_BM;
    constexpr bool EUC = METRIC == M_EUCLID;
    static_assert(BM == WAVES * 32, "a wave owns 32 rows of a tile");
    constexpr int SLOTS = AHEAD + 1;
    static_assert(2 * G * AHEAD <= 62, "vmcnt is six bits");
    static_assert(2 * G * (AHEAD - 1) <= 14, "fw_wait_vm_dyn covers the short-row case up to 14");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem_raw);
    const uint32_t nch = s.nch;
    const uint32_t ngr = (nch + G - 1) / G;                          // groups per tile
    float *cut_lds = reinterpret_cast<float *>(smem_raw + (size_t)nch * FW_B_UNITS * 16), *qq_lds = cut_lds + FW_QT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t n_tiles = (a.n_cand + BM - 1) / BM;
    const uint64_t my_tiles = blockIdx.x < n_tiles ? (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    if (my_tiles == 0) {
        SpWaveList::none(s.wcnt, blockIdx.x * (WAVES) + (uint32_t)w, lane);
        return;
    }
#pragma unroll 4
    for (uint32_t u = (uint32_t)tid; u < nch * FW_B_UNITS; u += T) lds[u] = s.bq[u];
    if (tid < FW_QT) {
        cut_lds[tid] = s.cut[tid];
        qq_lds[tid] = s.qq[tid];
    }
    __syncthreads();
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // from here on the kernel counts its vector-memory traffic itself
    const uint32_t kq_r = (uint32_t)lane >> 4, m_r = (uint32_t)lane & 15u;
    const uint4 *const b_rd = lds + fw_unit(0, kq_r, m_r);
    const unsigned char *rows = reinterpret_cast<const unsigned char *>(a.rows);
    const uint64_t last_row = a.n_cand - 1;
    const uint32_t row_stride32 = (uint32_t)a.row_stride;
    const uint32_t rl0 = (uint32_t)w * 32u + m_r, rl1 = rl0 + 16u;

    // One group's 2 G loads: the lane's pieces of row tiles 0 and 1 of group b of the block's it-th tile (rows past the block: the last row's bytes, their
    // scores are dropped; chunks past the row: the group's last piece again - the waits count loads)
    auto load_group = [&](uint64_t it, uint32_t b, i32x4h (&rc)[G][2]) __attribute__((always_inline)) {
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
            fw_gload16(rc[j][0], csrc, o0 + jj * 64u);
            fw_gload16(rc[j][1], csrc, o1 + jj * 64u);
        }
    };

    f32x4h acc[2][8];
    SpWaveList list(s.wlist, s.wcap, blockIdx.x * (WAVES) + (uint32_t)w);
    const uint32_t n_rows32 = (uint32_t)a.n_cand;
    // Nf of the lane's eight rows of the running tile (rows 4 kq_r .. + 3 of both 16-row tiles of the wave): inside the column also in the block's last
    // tile - it is padded to whole tiles (f16w_col_entries)
    i32x4h nf8[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    auto load_cols = [&](uint64_t it) __attribute__((always_inline)) {
        if constexpr (EUC) {
            const uint64_t row0 = (blockIdx.x + it * gridDim.x) * BM;
            const unsigned char *src = sp_uniform_ptr((uint64_t)(uintptr_t)(s.col + row0));
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) fw_gload16_col(nf8[mt], src, ((uint32_t)w * 32u + (uint32_t)mt * 16u + 4 * kq_r) * 4u);
        }
    };
    auto score = [&](int mt, int nt, int j, float qf) __attribute__((always_inline)) { return fw_score<METRIC>(acc[mt][nt][j], __int_as_float(nf8[mt][j]), qf); };

    auto epilogue = [&](uint64_t it) __attribute__((always_inline)) {
        const uint64_t tile = blockIdx.x + it * gridDim.x;
        const uint32_t row0 = (uint32_t)(tile * BM) + (uint32_t)w * 32u + 4 * kq_r;
        uint32_t hits8 = 0;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const int q = nt * 16 + (int)m_r;
            const float qf = qq_lds[q];
            float mx = -__builtin_inff();
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int j = 0; j < 4; ++j) mx = __builtin_fmaxf(mx, score(mt, nt, j, qf));
            if (mx >= cut_lds[q]) hits8 |= 1u << nt;
        }
        if (!__ballot(hits8 != 0)) return;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            if (!__ballot((hits8 >> nt) & 1u)) continue;
            const uint32_t q = (uint32_t)nt * 16 + m_r;
            const float ct = cut_lds[q], qf = qq_lds[q];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = score(mt, nt, j, qf);
                    const uint32_t row = row0 + (uint32_t)mt * 16 + (uint32_t)j;
                    list.append(v >= ct && row < n_rows32 && q < s.nq, v, row, q);
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
    i32x4h rc[SLOTS][G][2];
    // ---- prologue: the loads of groups 0 .. AHEAD - 1 ----
    fw_static_for<0, AHEAD>([&](auto DC) __attribute__((always_inline)) {
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
                if (ngr < (uint32_t)AHEAD) fw_wait_vm_dyn(2u * G * ngr);
                if constexpr (EUC) asm volatile("" : "+v"(nf8[0]), "+v"(nf8[1]) : : "memory");
                epilogue(it - 1);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 8; ++nt) acc[mt][nt] = (f32x4h){0.0f, 0.0f, 0.0f, 0.0f};
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
#pragma unroll
        for (int J = 0; J < G; ++J) {
            if ((uint32_t)J < gsz) {
                const uint4 *bb = b_rd + (b * G + J) * FW_B_UNITS;
                constexpr int B_AHEAD = 3;
                half8 bv[B_AHEAD + 1];
#pragma unroll
                for (int k = 0; k < B_AHEAD; ++k) bv[k] = *reinterpret_cast<const half8 *>(bb + k * 64);
#pragma unroll
                for (int nt = 0; nt < 8; ++nt) {
                    if (nt + B_AHEAD < 8) bv[(nt + B_AHEAD) % (B_AHEAD + 1)] = *reinterpret_cast<const half8 *>(bb + (nt + B_AHEAD) * 64);
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, rc[I][J][mt]), bv[nt % (B_AHEAD + 1)], acc[mt][nt], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (++b == ngr) { b = 0; ++it; }
    };
    for (uint64_t g = 0; g < n_groups; g += SLOTS) {
        fw_static_for<0, SLOTS>([&](auto IC) __attribute__((always_inline)) {
            if (g + decltype(IC)::value < n_groups) one_group(IC);
        });
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(nf8[0]), "+v"(nf8[1]) : : "memory");
    epilogue(my_tiles - 1);
    list.finish(s.wcnt, blockIdx.x * (WAVES) + (uint32_t)w, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- The scan of rows of 1 088 .. 2 048 bytes (dim 544 .. 1 024): the queries' image (136 .. 256 KiB) no longer fits in LDS, so rows AND queries are staged,
// with the work split and the rings of sp_staged_scan / scan_u8w_staged_kernel: block = 8 waves = 4 row quarters (wm) x 2 query halves (wn), acc[4][4] per
// wave; a stage = 256 rows x 128 bytes of K (two K-steps) = 32 KiB of rows + 16 KiB of query images (f16w_pack_kernel wrote them in LDS order: a verbatim
// LDS-DMA copy from L2), three stages of each in LDS; per stage and wave six 1 KiB requests spread between 32 matrix instructions, ONE s_waitcnt vmcnt and
// the stage barrier.
// The rows.  LDS-DMA puts lane i's 16 bytes at dst + 16 i, but the GLOBAL address is the lane's own: the lane that owns unit p of a request fetches the
// (row, piece) the operand layout sp_unit wants at p.  Request i (0 .. 3) of wave w fills units 256 w + 64 i + lane = sp_unit(2 w + (i >> 1), i & 1, kq, m)
// with kq = lane >> 4, m = (lane & 15) ^ (2 kq): bytes [64 (i & 1) + 16 kq, + 16) of the stage's 128 of row 16 (2 w + (i >> 1)) + m of the tile; requests
// 2 j and 2 j + 1 ask for the two halves of the same sixteen lines back to back.  Lane offsets are 32-bit inside a tile (f16w_segment_ok).  Rows past the
// block (the last tile) clamp to its last row and are dropped by number.  A row of 32 (mod 64) halfs ends in a stage of ONE chunk: the requests of the
// missing chunk repeat the real one - no byte past dim of any row is read - and the pack made the queries' missing chunk zero (finite rows: a zero product).
// Euclid's column comes as scan_u8w_staged_kernel's: at the top of a tile's FIRST stage - in front of that stage's requests - a wave requests the 64 Nf of
// its row quarter with one global_load_lds_dword into a slot of its own behind the rings, tile it -> slot it & 1, and the tile's epilogue reads the lane's
// sixteen back with four ds_read_b128.  The wave reads only what it copied itself: no barrier.
// The vector-memory count, stage by stage (it retires in order; requests of stage g: [Nf of the tile if kc == 0 (Euclid), queries of g + 2, rows of g + 2]):
//   kc == 0, Euclid: seven requests, s_waitcnt vmcnt(7);  else six, vmcnt(6)
// - either way exactly the stage's OWN requests stay out, so rows and queries of stage g + 1 have landed, and so has, after the tile's second stage, its
// column (a tile has at least nine stages).  The epilogue of tile it runs at the top of tile it + 1, in FRONT of that stage's requests, or after the last
// stage.  The request of tile it + 1, issued right after the epilogue of tile it, lands in the OTHER slot. ----
constexpr uint32_t FWS_RING_BYTES = (SP3_ARING * SP3_A_UNITS + 3 * SP_B_UNITS) * 16;      // 96 + 48 KiB
constexpr uint32_t FWS_NSLOTS = 2;                                                        // column slots per wave, 256 bytes each
constexpr uint32_t FWS_LDS_BYTES = FWS_RING_BYTES + (FW_THREADS / 64) * FWS_NSLOTS * 256u;
// 256 B of global memory (wave-uniform base, lane i fetches bytes 4 i .. 4 i + 3) into LDS at the wave-uniform byte address lds_dst
__device__ __forceinline__ void fw_glds4(const unsigned char *src, uint32_t lane_off, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(src), "s"(lds_dst) : "memory");
}
template <int METRIC>
__global__ __launch_bounds__(FW_THREADS, 1) void scan_f16w_staged_kernel(const ScanArgs a, const F16WideArgs s) {
    constexpr int BRING = 3, WAVES = FW_THREADS / 64, BM = FW_BM;
    constexpr bool EUC = METRIC == M_EUCLID;
    static_assert(FW_THREADS == SP3_THREADS && FW_BM == SP3_BM && FW_QT == SP_QT, "the staged scans' work split");
    static_assert(FWS_LDS_BYTES <= 160 * 1024, "one block per CU");
    static_assert((FW_RES_NCH + 2) / 2 >= 3, "the shortest staged tile ((FW_RES_NCH + 2) / 2 stages): its column lands at least two stages before its epilogue");
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
    // the wave's 64 queries, 4 per lane (query 64 wn + 16 nt + m_r): the cut and Q; a dead slot or a query without a bound admits nothing (f16w_pack_kernel)
    float lim[4], qf[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const uint32_t q = wn * 64 + (uint32_t)nt * 16 + m_r;
        lim[nt] = s.cut[q];
        qf[nt] = s.qq[q];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // from here on the kernel counts its vector-memory traffic itself
    const uint32_t lds0 = (uint32_t)(uintptr_t)(sp_lds_byte *)smem_raw;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    uint4 *b_lds = lds + SP3_ARING * SP3_A_UNITS;
    // the wave's column slots: bytes, and as the lane reads them (its rows 16 mt + 4 kq_r + j of the quarter: piece 4 mt + kq_r)
    const uint32_t c_slot0 = FWS_RING_BYTES + (uint32_t)w * (FWS_NSLOTS * 256u);
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
    // Nf of the wave's row quarter of a tile -> slot it & 1 (inside the column also in the block's last tile: it is padded to whole tiles, f16w_col_entries)
    auto request_col = [&](uint64_t it) {
        if constexpr (EUC) {
            const uint64_t row0 = my_tile(it) * BM + wm * 64u;
            fw_glds4(sp_uniform_ptr((uint64_t)(uintptr_t)(s.col + row0)), (uint32_t)lane * 4u, lds0 + c_slot0 + ((uint32_t)it & 1u) * 256u);
        }
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
    f32x4s acc[4][4];
    SpWaveList list(s.wlist, s.wcap, blockIdx.x * WAVES + (uint32_t)w);
    const uint32_t n_rows32 = (uint32_t)a.n_cand;
    // the epilogue of tile it: accumulator register j of (mt, nt) = row 256 tile + 64 wm + 16 mt + 4 kq_r + j, query 64 wn + 16 nt + m_r
    auto epilogue = [&](uint64_t it) __attribute__((always_inline)) {
        const uint32_t row0 = (uint32_t)(my_tile(it) * BM) + wm * 64 + 4 * kq_r;
        f32x4s nr[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            if constexpr (EUC) nr[mt] = *reinterpret_cast<const f32x4s *>(c_rd + ((uint32_t)it & 1u) * 16u + mt * 4);
            else nr[mt] = (f32x4s){0.0f, 0.0f, 0.0f, 0.0f};
        }
        auto val = [&](int mt, int nt, int j) __attribute__((always_inline)) { return fw_score<METRIC>(acc[mt][nt][j], nr[mt][j], qf[nt]); };
        auto max4 = [&](int mt, int nt) __attribute__((always_inline)) {
            float mx = val(mt, nt, 0);
#pragma unroll
            for (int j = 1; j < 4; ++j) mx = __builtin_fmaxf(mx, val(mt, nt, j));
            return mx;
        };
        bool hit[4];
        bool maybe = false;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            float mx = max4(0, nt);
#pragma unroll
            for (int mt = 1; mt < 4; ++mt) mx = __builtin_fmaxf(mx, max4(mt, nt));
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
                    const float v = val(mt, nt, j);
                    list.append(v >= lim[nt] && row < n_rows32 && q < s.nq, v, row, q);
                }
            }
        }
    };
    for (uint64_t it = 0; it < my_tiles; ++it) {
        if (it) epilogue(it - 1);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = (f32x4s){0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t kc = 0; kc < nst; ++kc) {
            if (kc == 0) request_col(it);                 // the stage's first request (Euclid)
            queries_begin();                              // stage g + 2 -> the slot stage g - 1 was read from (everybody is past that barrier)
            rows_begin();                                 // likewise
            const uint4 *ab = lds + slot * SP3_A_UNITS + a_rd;
            const uint4 *bb = b_lds + bslot * SP_B_UNITS + b_rd;
            half8 b0[4], b1[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                b0[nt] = *reinterpret_cast<const half8 *>(bb + nt * 128);
                b1[nt] = *reinterpret_cast<const half8 *>(bb + nt * 128 + 64);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const half8 a0 = *reinterpret_cast<const half8 *>(ab + mt * 128);
                const half8 a1 = *reinterpret_cast<const half8 *>(ab + mt * 128 + 64);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1[nt], acc[mt][nt], 0, 0, 0);
                // the stage's six copy requests, in the order the wait below relies on (queries first), spread over the matrix work; the two halves of the
                // rows' 128-byte lines back to back
                if (mt == 0) queries_piece(0);
                if (mt == 1) queries_piece(1);
                if (mt == 2) { rows_piece(0); rows_piece(1); }
                if (mt == 3) { rows_piece(2); rows_piece(3); }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b0[nt], acc[mt][nt], 0, 0, 0);
            }
            slot = sp_ring_next<SP3_ARING>(slot);
            bslot = sp_ring_next<BRING>(bslot);
            // all but this stage's own requests have landed: rows and queries of stage g + 1 among them, and by the tile's second stage its column
            if (EUC && kc == 0) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            sp_stage_barrier();
        }
    }
    epilogue(my_tiles - 1);
    list.finish(s.wcnt, blockIdx.x * WAVES + (uint32_t)w, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // nothing may land in LDS after the block is gone
}

// ---- the reference's bits: half_avx's 32 running f32 sums and their fold (f16_avx_leaf.hpp: fw_term, f16_avx_pair).  dim is a multiple of 32 here: no tail. ----
__device__ __forceinline__ float fw_hsum8(const float (&s)[8]) { return ((s[4] + s[0]) + (s[5] + s[1])) + ((s[6] + s[2]) + (s[7] + s[3])); }

// the pair kernel over the stored row-major layout: 32 lanes per pair, lane l owns sum l and takes elements l, l + 32, ... in order
template <int METRIC>
__global__ __launch_bounds__(256) void f16w_pairs_kernel(const ScanArgs a, const PairSel sel, uint64_t n_items) {
    const uint32_t lane = threadIdx.x & 63u, l = lane & 31u;
    const uint64_t n_live = sel.limit ? (n_items < (uint64_t)*sel.limit ? n_items : (uint64_t)*sel.limit) : n_items;
    const unsigned char *rows = reinterpret_cast<const unsigned char *>(a.rows), *queries = reinterpret_cast<const unsigned char *>(a.queries);
    for (uint64_t base = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2; base < n_live; base += (uint64_t)gridDim.x * 8) {
        const uint64_t item = base + (lane >> 5);
        bool valid = item < n_live;
        uint32_t qi = valid ? sel.query_of(item) : 0;
        valid = valid && sel.live(item, qi);
        uint32_t id = valid ? a.ids[item] : 0;
        if (valid && (id >= a.n_rows || qi >= a.nq)) {
            *a.err_flag = 1;
            valid = false;
            id = 0;
            qi = 0;
        }
        const unsigned short *x = reinterpret_cast<const unsigned short *>(rows + (uint64_t)id * a.row_stride) + l;
        const unsigned short *y = reinterpret_cast<const unsigned short *>(queries + (uint64_t)qi * a.q_stride) + l;
        const float result = f16_avx_pair<METRIC>(x, y, a.dim, lane);
        if (valid && l == 0) a.scores[item] = METRIC == M_EUCLID ? -result : result;
    }
}

// ---- The conditional exact pass: the queries whose lists overflowed (packed by launch_split_plan: a.queries, a.del.filter_of; *a.run_if = how many) take a
// top-k scan of the whole block with the reference's bits, 16 per block row - grid.y = the 16-query groups of the batch, a block row whose group holds
// none returns at once, which on a search without overflow is every block.  Not a hot path: four lanes per row, lane r holds the eight sums of AVX
// register r across the iterations (its 16-byte piece of every 64-byte chunk), four queries at a time (the row's bytes come back from the cache for the
// next four).  a.partial: grid.x x groups lists of 16 x top keys, group-major, as launch_merge_keys(..., grouped) reads them ----
template <int METRIC, bool PERQ>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_f16_avx_groups_kernel(const ScanArgs a) {
    constexpr int QT = 16, QB = 4, NW = SCAN_BLOCK / WAVE;
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
    const uint32_t r4 = (uint32_t)lane & 3u, g = (uint32_t)lane >> 2;
    const unsigned char *rows = reinterpret_cast<const unsigned char *>(a.rows);
    const uint32_t n_it = a.dim / 32;
    uint64_t list[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) list[q] = 0;
    const uint64_t n_tiles = (a.n_cand + 15) / 16;
    for (uint64_t tile = (uint64_t)blockIdx.x * NW + wave; tile < n_tiles; tile += (uint64_t)gridDim.x * NW) {
        const uint64_t c = tile * 16 + g;
        const bool valid = c < a.n_cand;
        const uint32_t rid = valid ? (uint32_t)c : 0u;
        const unsigned char *rp = rows + (uint64_t)rid * a.row_stride + r4 * 16u;
#pragma unroll
        for (int qb = 0; qb < QT / QB; ++qb) {
            if ((uint32_t)(qb * QB) >= nq) break;
            float s[QB][8];
#pragma unroll
            for (int k = 0; k < QB; ++k)
#pragma unroll
                for (int e = 0; e < 8; ++e) s[k][e] = 0.0f;
#pragma unroll 2
            for (uint32_t it = 0; it < n_it; ++it) {
                const uint4 v = *reinterpret_cast<const uint4 *>(rp + (uint64_t)it * 64);
                const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
                float x[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = fw_h2f((vw[e / 2] >> (16 * (e % 2))) & 0xFFFFu);
#pragma unroll
                for (int k = 0; k < QB; ++k) {
                    const uint4 u = *reinterpret_cast<const uint4 *>(smem + (uint32_t)(qb * QB + k) * a.q_stride + it * 64u + r4 * 16u);
                    const uint32_t uw[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) s[k][e] = fw_term<METRIC>(s[k][e], fw_h2f((uw[e / 2] >> (16 * (e % 2))) & 0xFFFFu), x[e]);
                }
            }
#pragma unroll
            for (int k = 0; k < QB; ++k) {
                const int q = qb * QB + k;
                const float reg = fw_hsum8(s[k]);
                const int l0 = lane & ~3;
                const float result = ((__shfl(reg, l0, 64) + __shfl(reg, l0 + 1, 64)) + __shfl(reg, l0 + 2, 64)) + __shfl(reg, l0 + 3, 64);
                if (q < (int)nq) {
                    const uint64_t key = make_key(METRIC == M_EUCLID ? -result : result, rid);
                    bool cnd = valid && r4 == 0 && key > readlane_u64(list[q], (int)a.top - 1);
                    if (__ballot(cnd)) {
                        if constexpr (PERQ) cnd = cnd && a.del.live(rid, q0 + (uint32_t)q);
                        else cnd = cnd && a.del.live(rid);
                        uint64_t m = __ballot(cnd);
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
static int f16w_metric(int distance) { return distance == QMX_DISTANCE_DOT || distance == QMX_DISTANCE_COSINE ? F16W_DOT : distance == QMX_DISTANCE_EUCLID ? F16W_EUCLID : -1; }
bool f16w_segment_ok(int distance, uint32_t dim, uint64_t row_stride, uint64_t n) {
    return f16w_metric(distance) >= 0 && dim % 32 == 0 && dim >= 64 && dim <= F16W_MAX_DIM && row_stride % 16 == 0 && row_stride >= (uint64_t)dim * 2 && n >= (1u << 18) &&
           n < 0xFFFFFFFFull && row_stride * (FW_BM - 1) + (uint64_t)dim * 2 < (1ull << 31);
}
// the statistics pass alone (the fused f16 MaxSim wants them of small blocks and of rows of 32 halves too: maxsim_f16.hip)
bool f16w_stats_ok(int distance, uint32_t dim, uint64_t row_stride, uint64_t n) {
    return f16w_metric(distance) >= 0 && dim % 32 == 0 && dim >= 32 && dim <= F16W_MAX_DIM && row_stride % 16 == 0 && row_stride >= (uint64_t)dim * 2 && n >= 1 &&
           n < 0xFFFFFFFFull;
}
// the queries' image: [dim / 32] chunks of 8 KiB for the resident scan, [stages of 128 bytes] of 16 KiB for the staged one (f16w_pack_kernel)
size_t f16w_query_bytes(uint32_t dim) {
    const uint32_t nch = dim / 32;
    return nch <= FW_RES_NCH ? (size_t)nch * FW_B_UNITS * 16 : (size_t)((nch + 1) / 2) * SP_B_UNITS * 16;
}
size_t f16w_wlists_counts_bytes(int num_cus) { return ((size_t)num_cus * (FW_THREADS / 64) * 4 + 255) / 256 * 256; }
size_t f16w_wlists_bytes(int num_cus) { return f16w_wlists_counts_bytes(num_cus) + (size_t)num_cus * (FW_THREADS / 64) * FW_WCAP * 16; }
uint32_t f16w_wcap() { return FW_WCAP; }
uint64_t f16w_col_entries(uint64_t n) { return (n + FW_BM - 1) / FW_BM * FW_BM; }

// d_col: f16w_col_entries(n) floats (Euclid) or nullptr; d_stats: three zeroed dwords
int32_t launch_f16w_stats(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, int distance, float *d_col, uint32_t *d_stats) {
    QMX_REQUIRE(f16w_stats_ok(distance, dim, row_stride, n) && d_stats && (f16w_metric(distance) != F16W_EUCLID || d_col), QMX_ERR_BAD_ARG, "f16 wide statistics of dim %u", dim);
    ::qmx::clear_stale_error();
    const uint64_t n_pad = f16w_col_entries(n);
    hipLaunchKernelGGL(f16w_stats_kernel, dim3((uint32_t)std::min<uint64_t>(8192, n_pad / 16)), dim3(256), 0, st, (const unsigned char *)rows, row_stride, n, n_pad, dim,
                       f16w_metric(distance) == F16W_EUCLID ? d_col : nullptr, d_stats);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

// one 128-query tile (a.queries: f16 entries): d_bq f16w_query_bytes(dim); four arrays of 128 floats; zeroes the tile's candidate counters
int32_t launch_f16w_pack(hipStream_t st, const ScanArgs &a, int distance, float rowmax, bool seg_subnormal, const uint64_t *d_gthr, void *d_bq, float *d_t_exact,
                         float *d_band, float *d_cut, float *d_qq, uint32_t *d_cand_cnt, uint32_t n_cnt) {
    QMX_REQUIRE(a.nq <= (uint32_t)FW_QT && f16w_metric(distance) >= 0 && a.dim % 32 == 0 && a.dim >= 64 && a.dim <= F16W_MAX_DIM && a.q_stride >= a.dim * 2 &&
                    a.q_stride % 16 == 0,
                QMX_ERR_BAD_ARG, "f16 wide tile of %u queries", a.nq);
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(f16w_pack_kernel, dim3(FW_QT), dim3(64), 0, st, (const unsigned char *)a.queries, a.q_stride, a.nq, a.dim, f16w_metric(distance), rowmax,
                       seg_subnormal ? 1u : 0u, d_gthr, (uint4 *)d_bq, d_t_exact, d_band, d_cut, d_qq, d_cand_cnt, n_cnt);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

// d_wlists: [counts: f16w_wlists_counts_bytes][lists]; *grid_out = blocks launched (8 lists each)
int32_t launch_scan_f16w(hipStream_t st, const ScanArgs &a, int distance, const void *d_bq, const float *d_cut, const float *d_qq, const float *d_col, int num_cus,
                         void *d_wlists, uint32_t *grid_out) {
    const int metric = f16w_metric(distance);
    QMX_REQUIRE(f16w_segment_ok(distance, a.dim, a.row_stride, a.n_rows) && !a.ids && a.n_cand >= 1 && a.n_cand <= a.n_rows && a.nq <= (uint32_t)FW_QT && d_wlists &&
                    (metric != F16W_EUCLID || d_col),
                QMX_ERR_NOT_SUPPORTED, "f16 wide scan: shape not supported");
    F16WideArgs s;
    s.bq = (const uint4 *)d_bq;
    s.nch = a.dim / 32;
    s.nq = a.nq;
    s.cut = d_cut;
    s.qq = d_qq;
    s.col = d_col;
    s.wcnt = (uint32_t *)d_wlists;
    s.wlist = (uint4 *)((unsigned char *)d_wlists + f16w_wlists_counts_bytes(num_cus));
    s.wcap = FW_WCAP;
    const uint64_t n_tiles = (a.n_cand + FW_BM - 1) / FW_BM;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)num_cus, n_tiles);
    // rows of up to 1 024 bytes: the queries resident; longer ones: the staged rings
    const bool resident = s.nch <= FW_RES_NCH, euclid = metric == F16W_EUCLID;
    const size_t lds_bytes = resident ? (size_t)s.nch * FW_B_UNITS * 16 + FW_LDS_TAIL : (size_t)FWS_LDS_BYTES;
    void (*kfn)(const ScanArgs, const F16WideArgs) = resident ? (euclid ? scan_f16w_kernel<M_EUCLID, 2, 2> : scan_f16w_kernel<M_DOT, 2, 2>)
                                                              : (euclid ? scan_f16w_staged_kernel<M_EUCLID> : scan_f16w_staged_kernel<M_DOT>);
    static thread_local DeviceOnce once;
    ::qmx::clear_stale_error();
    if (once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_f16w_staged_kernel<M_DOT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FWS_LDS_BYTES));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_f16w_staged_kernel<M_EUCLID>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FWS_LDS_BYTES));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_f16w_kernel<M_DOT, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, FW_LDS_MAX));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_f16w_kernel<M_EUCLID, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, FW_LDS_MAX));
        once.mark();
    }
    QMX_NOTE_KERNEL(kfn);
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(FW_THREADS), lds_bytes, st, a, s);
    QMX_HIP(hipGetLastError());
    if (grid_out) *grid_out = grid;
    return QMX_OK;
}

// the reference's bits of the listed pairs (a.ids, a.scores, sel.qsel; sel.limit: the device-side count)
int32_t launch_pairs_f16_avx(hipStream_t st, int distance, const ScanArgs &a, const PairSel &sel, uint64_t n_items, int num_cus) {
    QMX_REQUIRE(f16w_metric(distance) >= 0 && a.dim % 32 == 0 && a.dim >= 32 && a.ids && a.scores && (sel.qsel || !sel.per_query || !sel.counts), QMX_ERR_BAD_ARG,
                "f16 AVX-order pairs: one sequence of items over rows of whole 32-element iterations");
    if (n_items == 0) return QMX_OK;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n_items + 7) / 8, (uint64_t)num_cus * 8);
    ::qmx::clear_stale_error();
    if (f16w_metric(distance) == F16W_EUCLID) hipLaunchKernelGGL(f16w_pairs_kernel<M_EUCLID>, dim3(grid), dim3(256), 0, st, a, sel, n_items);
    else hipLaunchKernelGGL(f16w_pairs_kernel<M_DOT>, dim3(grid), dim3(256), 0, st, a, sel, n_items);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

// a.nq packed slots in a.queries (a.del.filter_of packed with them), *a.run_if = how many of them are to be scanned; a.partial: grid.x x groups lists of 16 x top
// keys.  *grid_out: in: the cap on grid.x, out: grid.x
template <int METRIC>
static int32_t launch_f16_avx_groups_metric(hipStream_t st, const ScanArgs &a, int num_cus, uint32_t *grid_out) {
    constexpr int QT = 16, NW = SCAN_BLOCK / WAVE;
    size_t lds = std::max((size_t)QT * a.q_stride, (size_t)NW * QT * a.top * sizeof(uint64_t));
    lds = (lds + 15) & ~(size_t)15;
    QMX_REQUIRE(lds <= 160 * 1024, QMX_ERR_NOT_SUPPORTED, "query tile needs %zu B of LDS (> 160 KiB)", lds);
    void (*kfn)(const ScanArgs) = a.del.filter_of ? scan_f16_avx_groups_kernel<METRIC, true> : scan_f16_avx_groups_kernel<METRIC, false>;
    static thread_local DeviceOnce once;
    ::qmx::clear_stale_error();
    if (once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_f16_avx_groups_kernel<METRIC, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_f16_avx_groups_kernel<METRIC, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        once.mark();
    }
    const uint64_t n_tiles = (a.n_cand + 15) / 16;
    uint32_t grid = (uint32_t)std::min<uint64_t>((n_tiles + NW - 1) / NW, (uint64_t)num_cus);
    if (grid < 1) grid = 1;
    if (*grid_out && grid > *grid_out) grid = *grid_out;
    *grid_out = grid;
    hipLaunchKernelGGL(kfn, dim3(grid, (a.nq + QT - 1) / QT), dim3(SCAN_BLOCK), lds, st, a);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_scan_f16_avx_groups(hipStream_t st, int distance, const ScanArgs &a, int num_cus, uint32_t *grid_out) {
    QMX_REQUIRE(a.run_if && a.partial && !a.ids && !a.key_bound && a.nq >= 1 && grid_out && a.top >= 1 && a.top <= (uint32_t)MAX_TOP_FAST && a.dim >= 32 && a.dim % 32 == 0 &&
                    a.q_stride % 16 == 0 && a.q_stride >= a.dim * 2 && a.row_stride % 16 == 0,
                QMX_ERR_BAD_ARG, "f16 exact groups: a packed conditional pass over rows of whole 32-element iterations");
    if (f16w_metric(distance) == F16W_EUCLID) return launch_f16_avx_groups_metric<M_EUCLID>(st, a, num_cus, grid_out);
    if (f16w_metric(distance) == F16W_DOT) return launch_f16_avx_groups_metric<M_DOT>(st, a, num_cus, grid_out);
    set_error("f16 exact groups: distance %d", distance);
    return QMX_ERR_NOT_SUPPORTED;
}

}  // namespace qmx
