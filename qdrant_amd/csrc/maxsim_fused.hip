// maxsim_fused.hip — Colbert MaxSim over dense f32 multi-vector points on v_mfma_f32_16x16x4_f32, without the [tokens][rows] similarity matrix
// (score_max_similarity, lib/segment/src/vector_storage/query_scorer/mod.rs:70-97; the two-step route is score_ids_device + maxsim_kernel).
//
// What it computes.  cq_scores[j * n + c] = sum over the tokens of multi-query j, in order from 0.0, of max over the rows of candidate c of
// dot(token, row) - the bits of maxsim_kernel over the scan's similarities.  Dot and Cosine alike (stored Cosine rows and the query tokens
// are normalised already), dim a multiple of 32 in 32 .. 256.
//
// Bits.  dot_similarity_avx keeps 32 independent fma chains per (row, token): chain c takes elements c, c + 32, c + 64, ... in order (the
// header of scan_mfma16.hip).  A chain is the K stream of one 16x16x4 instruction (two at dim > 128): lane (m = lane & 15, k = lane >> 4)
// supplies element c + 32 (4 s + k) of row m (A) and of token m (B) to K-step s.  A chain of 1 .. 3 or 5 .. 7 elements is padded to whole
// K-steps with zeros in BOTH operands: fma(0, 0, acc) leaves acc alone, and no chain value is -0.0 because a chain starts from +0.0.  The 32
// chain tiles fold elementwise in the reference's tree: T_j = (C_j + C_8+j) + (C_16+j + C_24+j) (four_way_hsum), lr_j = T_j+4 + T_j,
// score = (lr_0 + lr_1) + (lr_2 + lr_3) (hsum256_ps_avx).  The max over a point's rows is order-free (`if sim > max` from -inf, as the
// reference: a NaN is skipped; a +-0 disagreement cannot reach the sum, which starts at +0.0); the sum over tokens is serial.
//
// Row stream and work split.  The candidates' rows form one stream: candidate c is the run S[c] .. S[c + 1] of it (S = the prefix sums of
// the candidates' lengths, written by maxsim_prefix_kernel; without a candidate list S is point_offsets itself).  cmap[stream row] = its
// candidate (maxsim_map_kernel) spares the kernel a search per tile.  Block x of grid.x owns the candidates whose S[c] falls in its equal
// share of the stream: a point is never shared between blocks, nothing is atomic; a point longer than a share makes its block run long.
// grid.y = groups of 64 tokens, whose B operands (packed once per call by maxsim_pack_kernel as [token tile][chain][K-step][64 lanes])
// stay resident in LDS.
//
// Data movement.  The block walks its stream in tiles of TR rows.  Rows go HBM -> LDS by global_load_lds_dwordx4 (non-temporal, per-lane
// source: 64 16-byte pieces per instruction) into a ring of NBUF tiles, counted with s_waitcnt vmcnt(N).  Piece e of tile row m lands in
// slot m * (dim / 4) + (e ^ (m & 7)): the A operand of (chain, K-step) is then one ds_read_b32 per lane, 4 lanes per bank.
//   dim <= 128: TR = 64, 16 rows x 4 token tiles per wave, ring of 3;   dim 160 .. 256: TR = 32 (a tile is 32 KiB again), 16 rows x 2 token
//   tiles per wave, ring of 2.  LDS: 146 KiB at dim 128, 138 KiB at dim 256.
// Segmented max.  A wave writes its similarities to the scratch tile sim[TR][64 tokens]; thread (token, quarter of the rows) turns its
// quarter into running maxima that restart at every point start; then per (point end in the tile, token) the maxima of the quarters the
// point spans and the carry of a point that began in an earlier tile are merged, and written to tokmax[token][candidate] - or carried on
// when the point continues.  maxsim_sum_kernel does the serial sums (a point without rows: -inf per token).
#include "maxsim_common.hpp"      // (the LDS-DMA copy, the LDS-only barrier, MSF_NONE, MSF_SIM_P: shared with maxsim_f16.hip)

namespace qmx {

typedef float msf_f32x4 __attribute__((ext_vector_type(4)));

template <int D32>
struct MsfShape {
    static constexpr int DIM = 32 * D32;
    static constexpr int KS = (D32 + 3) / 4;                 // K-steps per chain
    static constexpr int TR = KS == 1 ? 64 : 32;             // rows per tile
    static constexpr int RB = TR / 16;                       // 16-row blocks of a tile
    static constexpr int NTW = 4 / (4 / RB);                 // token tiles per wave (4 waves = RB row blocks x 4 / RB token halves)
    static constexpr int PPR = DIM / 4;                      // 16-byte pieces per row
    static constexpr int TILE_B = TR * DIM * 4;
    static constexpr int IPW = TILE_B / 4096;                // LDS-DMA instructions per wave and tile
    static constexpr int NBUF = KS == 1 ? 3 : 2;
    static constexpr int CH = TR / 4;                        // rows per quarter of the segmented max
    static constexpr int BPACK_F = 4 * 32 * KS * 64;         // floats of a token group's B operands
    static constexpr int OFF_RING = BPACK_F * 4;
    static constexpr int OFF_SIM = OFF_RING + NBUF * TILE_B;
    static constexpr int OFF_META = OFF_SIM + TR * MSF_SIM_P * 4;
    static constexpr int OFF_CARRY = OFF_META + (NBUF + 1) * TR * 4;
    static constexpr int LDS = OFF_CARRY + 2 * 64 * 4;         // the carry of the tile before, the carry of this one
    static_assert(TILE_B % 4096 == 0 && LDS <= 160 * 1024, "whole 1 KiB instructions per wave; the CU's LDS");
};

struct MsfArgs {
    const unsigned char *rows;
    uint64_t row_stride;       // bytes
    const uint64_t *S;         // [n + 1]
    const uint32_t *cmap;      // [total]: candidate of stream row s0 + i
    const uint64_t *delta;     // [n] with a candidate list: (first storage row of candidate c) - S[c], wrapping; nullptr: the stream IS the storage
    const float *bpack;        // [token groups][BPACK_F]
    float *tokmax;             // [n_tokens][n]
    uint64_t n, s0, total;
    uint32_t n_tokens;
};

template <int D32>
__global__ __launch_bounds__(256) void maxsim_fused_kernel(const MsfArgs a) {
    typedef MsfShape<D32> S;
    constexpr int KS = S::KS, TR = S::TR, RB = S::RB, NTW = S::NTW, PPR = S::PPR, IPW = S::IPW, NBUF = S::NBUF, CH = S::CH;
    extern __shared__ __attribute__((aligned(16))) unsigned char msf_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *lds_b = reinterpret_cast<float *>(msf_smem);
    float *sim = reinterpret_cast<float *>(msf_smem + S::OFF_SIM);
    uint32_t *meta = reinterpret_cast<uint32_t *>(msf_smem + S::OFF_META);
    float *carry = reinterpret_cast<float *>(msf_smem + S::OFF_CARRY);
    const uint32_t ring0 = (uint32_t)(uintptr_t)(msf_lds_byte *)msf_smem + S::OFF_RING;

    // ---- the block's run of the stream: the candidates whose start falls in [lo, hi)
    const MsfRun run = msf_block_run(a.S, a.cmap, a.s0, a.total);
    const uint64_t b0 = run.b0, b1 = run.b1;
    if (b0 >= b1) return;
    const uint64_t n_tiles = (b1 - b0 + TR - 1) / TR;

    // ---- the token group's B operands
    {
        const float4 *src = reinterpret_cast<const float4 *>(a.bpack + (size_t)blockIdx.y * S::BPACK_F);
        float4 *dst = reinterpret_cast<float4 *>(lds_b);
        for (int i = tid; i < S::BPACK_F / 4; i += 256) dst[i] = src[i];
    }

    // position of this lane in tile t (every wave resolves the whole tile; at TR = 32 the upper half of the wave repeats the lower)
    const uint32_t lpos = (uint32_t)lane & (uint32_t)(TR - 1);
    auto tile_pos = [&](uint64_t t, bool *valid) -> uint64_t {  // the stream row, clamped into the block's run (phantom loads stay inside the storage)
        const uint64_t pos = b0 + t * TR + lpos;
        *valid = pos < b1;
        return *valid ? pos : b1 - 1;
    };
    // the tile's rows -> ring slot: instruction i of wave w moves pieces (w IPW + i) 64 .. + 63 of the tile's swizzled image
    auto issue_tile = [&](uint64_t row_of_lane, uint32_t slot) {
        const unsigned char *base = a.rows + row_of_lane * a.row_stride;
        const uint32_t blo = (uint32_t)(uintptr_t)base, bhi = (uint32_t)((uintptr_t)base >> 32);
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
            const uint32_t g = (uint32_t)(w * IPW + i) * 64u + (uint32_t)lane;
            const uint32_t m = g / PPR, e = (g % PPR) ^ (m & 7u);
            const uint32_t slo = (uint32_t)__shfl((int)blo, (int)m), shi = (uint32_t)__shfl((int)bhi, (int)m);
            const unsigned char *src = reinterpret_cast<const unsigned char *>(((uint64_t)shi << 32) | slo) + e * 16u;
            msf_glds16(src, ring0 + slot * (uint32_t)S::TILE_B + (uint32_t)(w * IPW + i) * 1024u);
        }
    };
    auto stage_tile = [&](uint64_t t, uint32_t cand, uint64_t d, uint32_t slot) {   // cand / d: cmap and delta of the lane's (clamped) position
        bool valid;
        const uint64_t pos = tile_pos(t, &valid);
        if (w == 0 && lane < TR) meta[(uint32_t)(t % (NBUF + 1)) * TR + lane] = valid ? cand : MSF_NONE;
        issue_tile(pos + d, slot);
    };
    auto load_cand = [&](uint64_t t) -> uint32_t {
        bool valid;
        return a.cmap[tile_pos(t, &valid) - a.s0];
    };
    for (int p = 0; p < NBUF; ++p) {
        const uint32_t c = load_cand(p);
        stage_tile(p, c, a.delta ? a.delta[c] : 0ull, (uint32_t)p);
    }
    uint32_t c_cur = load_cand(NBUF);       // cmap of the tile staged during iteration 0

    const int rb = w % RB, tq0 = (w / RB) * NTW;
    const int mrow = rb * 16 + (lane & 15), kq = lane >> 4;
    const uint32_t a_row = (uint32_t)mrow * (uint32_t)(PPR * 16), sw = (uint32_t)mrow & 7u;
    uint32_t slot = 0;
    uint32_t prev_last = MSF_NONE;          // candidate of the previous tile's last row
    const int tk = tid & 63, qtr = tid >> 6;
    const uint64_t tok = (uint64_t)blockIdx.y * 64 + (uint32_t)tk;

    for (uint64_t t = 0; t < n_tiles; ++t) {
        // B1: tile t has landed (this wave's share: at most the NBUF - 1 tiles issued after it are outstanding; the barrier: everyone's), and
        // every wave is done with the previous tile's scratch
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NBUF - 1) * IPW) : "memory");
        msf_barrier();
        // the rows of tile t + NBUF: delta of its candidates, and cmap of the tile after it - both arrive under the matrix work
        bool nvalid;
        (void)tile_pos(t + NBUF, &nvalid);
        const uint64_t d_next = a.delta ? a.delta[c_cur] : 0ull;
        const uint32_t c_next = load_cand(t + NBUF + 1);

        // ---- similarities of (16 rows) x (NTW token tiles), chain by chain, folded in the reference's tree
        const unsigned char *tile = msf_smem + S::OFF_RING + slot * S::TILE_B + a_row;
        auto lds_a = [&](int c, int s) -> float {
            const int kidx = 4 * s + kq;
            const uint32_t e = (uint32_t)(c >> 2) + 8u * (uint32_t)(kidx < D32 ? kidx : 0);
            const float v = *reinterpret_cast<const float *>(tile + ((e ^ sw) * 16u) + (uint32_t)(c & 3) * 4u);
            return (D32 % 4 == 0 || kidx < D32) ? v : 0.0f;
        };
        msf_f32x4 lr[4][NTW];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            msf_f32x4 T[2][NTW];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                msf_f32x4 C[4][NTW];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = 8 * r + jj + 4 * h;
#pragma unroll
                    for (int tt = 0; tt < NTW; ++tt) C[r][tt] = (msf_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < KS; ++s) {
                        const float av = lds_a(c, s);
#pragma unroll
                        for (int tt = 0; tt < NTW; ++tt)
                            C[r][tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, lds_b[(((tq0 + tt) * 32 + c) * KS + s) * 64 + lane], C[r][tt], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int tt = 0; tt < NTW; ++tt) T[h][tt] = (C[0][tt] + C[1][tt]) + (C[2][tt] + C[3][tt]);      // four_way_hsum, SIMD lane jj + 4 h
            }
#pragma unroll
            for (int tt = 0; tt < NTW; ++tt) lr[jj][tt] = T[1][tt] + T[0][tt];                                // extractf128(x, 1) + cast(x)
        }
#pragma unroll
        for (int tt = 0; tt < NTW; ++tt) {
            const msf_f32x4 score = (lr[0][tt] + lr[1][tt]) + (lr[2][tt] + lr[3][tt]);                        // hadd, p1 + p2
#pragma unroll
            for (int j = 0; j < 4; ++j) sim[(rb * 16 + 4 * kq + j) * MSF_SIM_P + 16 * (tq0 + tt) + (lane & 15)] = score[j];
        }
        // B2: the scratch tile is whole, and nobody reads ring slot `slot` any more: refill it
        msf_barrier();
        // (c_next is waited for here, where the tiles in flight were issued an iteration ago - not at the top of the next iteration, behind this
        // iteration's stores, where the compiler's vmcnt(0) would drain the ring)
        asm volatile("" :: "v"(c_next), "v"(d_next));
        stage_tile(t + NBUF, c_cur, d_next, slot);
        c_cur = c_next;

        // ---- segmented max, step 1: running maxima inside (point, quarter of the tile's rows)
        const uint32_t *mt = meta + (uint32_t)(t % (NBUF + 1)) * TR;
        {
            uint32_t prev = MSF_NONE;
            float mx = -__builtin_inff();
#pragma unroll
            for (int r = qtr * CH; r < qtr * CH + CH; ++r) {
                const uint32_t c = mt[r];
                const float v = sim[r * MSF_SIM_P + tk];
                if (c != prev) { mx = -__builtin_inff(); prev = c; }
                if (v > mx) mx = v;
                sim[r * MSF_SIM_P + tk] = mx;
            }
        }
        msf_barrier();         // B3
        // ---- step 2: every point end of this quarter: merge the quarters the point spans and its carry; write or carry on
        {
            const uint32_t first_c = mt[0];
            const bool cont_in = first_c == prev_last;
            const uint32_t next_first = meta[(uint32_t)((t + 1) % (NBUF + 1)) * TR];
            for (int r = qtr * CH; r < qtr * CH + CH; ++r) {
                const uint32_t c = mt[r];
                if (c == MSF_NONE) break;
                if (r != TR - 1 && mt[r + 1] == c) continue;
                float v = sim[r * MSF_SIM_P + tk];
                for (int qq = qtr - 1; qq >= 0; --qq) {
                    const int re = qq * CH + CH - 1;
                    if (mt[re] != c) break;
                    const float x = sim[re * MSF_SIM_P + tk];
                    if (x > v) v = x;
                }
                if (cont_in && c == first_c) {
                    const float x = carry[(int)(~t & 1) * 64 + tk];
                    if (x > v) v = x;
                }
                if (r == TR - 1 && next_first == c) carry[(int)(t & 1) * 64 + tk] = v;      // (another quarter may still read the previous tile's)
                else if (tok < a.n_tokens) a.tokmax[tok * a.n + c] = v;
            }
            prev_last = mt[TR - 1];
        }
        slot = slot + 1 == NBUF ? 0 : slot + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the phantom tiles land before the block's LDS is given back
}

// ---- the small kernels around it ----
// S[c] = rows of candidates 0 .. c - 1 (one block: a candidate list is a rerank's, not a collection), delta[c] = offsets[ids[c]] - S[c]; an id past
// n_points raises the error flag, as maxsim_kernel does, and counts as an empty point
__global__ __launch_bounds__(1024) void maxsim_prefix_kernel(const uint32_t *ids, uint64_t n, const uint64_t *offsets, uint32_t n_points, uint64_t *S,
                                                             uint64_t *delta, int *err_flag) {
    __shared__ uint64_t sh[1024];
    uint64_t base_sum = 0;
    for (uint64_t base = 0; base < n; base += 1024) {
        const uint64_t c = base + threadIdx.x;
        uint64_t len = 0, first = 0;
        if (c < n) {
            const uint32_t p = ids[c];
            if (p >= n_points) *err_flag = 1;
            else { first = offsets[p]; len = offsets[p + 1] - first; }
        }
        sh[threadIdx.x] = len;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const uint64_t add = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        const uint64_t excl = base_sum + sh[threadIdx.x] - len;
        if (c < n) { S[c] = excl; delta[c] = first - excl; }
        base_sum += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) S[n] = base_sum;
}

// cmap[S[c] - s0 .. S[c + 1] - s0) = c: a wave per candidate
__global__ __launch_bounds__(256) void maxsim_map_kernel(const uint64_t *S, uint64_t n, uint64_t s0, uint32_t *cmap) {
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    const int lane = threadIdx.x & 63;
    for (uint64_t c = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += n_waves) {
        const uint64_t e = S[c + 1];
        for (uint64_t i = S[c] + (uint32_t)lane; i < e; i += 64) cmap[i - s0] = (uint32_t)c;
    }
}

// the tokens as B operands: out[((tile * 32 + c) * KS + s) * 64 + lane] = element c + 32 (4 s + (lane >> 4)) of token 16 tile + (lane & 15); 0 past either end
__global__ __launch_bounds__(256) void maxsim_pack_kernel(const unsigned char *queries, uint32_t q_stride, uint32_t n_tokens, uint32_t d32, uint32_t ks,
                                                          uint64_t count, float *out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const uint32_t lane = (uint32_t)(i & 63), s = (uint32_t)((i >> 6) % ks), c = (uint32_t)((i / (64 * ks)) & 31);
    const uint64_t tile = i / (64ull * ks * 32);
    const uint64_t token = 16 * tile + (lane & 15);
    const uint32_t kidx = 4 * s + (lane >> 4);
    out[i] = (token < n_tokens && kidx < d32) ? reinterpret_cast<const float *>(queries + token * q_stride)[c + 32 * kidx] : 0.0f;
}

// the serial sums: out[j * n + c] = sum over tokens qfirst[j] .. qfirst[j + 1] of tokmax[token][c], from 0.0; a point without rows: -inf per token
__global__ __launch_bounds__(256) void maxsim_sum_kernel(const float *tokmax, const uint64_t *S, uint64_t n, const uint32_t *qfirst, uint32_t n_queries, float *out) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t j = blockIdx.y;
    if (c >= n || j >= n_queries) return;
    const bool empty = S[c + 1] == S[c];
    float sum = 0.0f;
    for (uint32_t t = qfirst[j]; t < qfirst[j + 1]; ++t) sum += empty ? -__builtin_inff() : tokmax[(uint64_t)t * n + c];
    out[(uint64_t)j * n + c] = sum;
}

bool maxsim_fused_dim_ok(uint32_t dim) { return dim % 32 == 0 && dim >= 32 && dim <= 256; }
uint64_t maxsim_fused_pack_floats(uint32_t dim, uint32_t n_tokens) { return (uint64_t)((n_tokens + 63) / 64) * 4 * 32 * ((dim / 32 + 3) / 4) * 64; }

int32_t launch_maxsim_prefix(hipStream_t st, const uint32_t *d_ids, uint64_t n, const uint64_t *d_offsets, uint32_t n_points, uint64_t *d_S, uint64_t *d_delta,
                             int *err_flag) {
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(maxsim_prefix_kernel, dim3(1), dim3(1024), 0, st, d_ids, n, d_offsets, n_points, d_S, d_delta, err_flag);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_maxsim_map(hipStream_t st, const uint64_t *d_S, uint64_t n, uint64_t s0, uint32_t *d_cmap) {
    hipLaunchKernelGGL(maxsim_map_kernel, dim3((uint32_t)std::min<uint64_t>((n + 3) / 4, 8192)), dim3(256), 0, st, d_S, n, s0, d_cmap);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_maxsim_sum(hipStream_t st, const float *d_tokmax, const uint64_t *d_S, uint64_t n, const uint32_t *d_qfirst, uint32_t n_queries, float *d_out) {
    hipLaunchKernelGGL(maxsim_sum_kernel, dim3((uint32_t)((n + 255) / 256), n_queries), dim3(256), 0, st, d_tokmax, d_S, n, d_qfirst, n_queries, d_out);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

template <int D32>
static int32_t launch_msf(hipStream_t st, const MsfArgs &a, int num_cus) {
    typedef MsfShape<D32> S;
    static thread_local DeviceOnce attr_once;
    if (attr_once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(maxsim_fused_kernel<D32>), hipFuncAttributeMaxDynamicSharedMemorySize, S::LDS));
        attr_once.mark();
    }
    const uint32_t gy = (a.n_tokens + 63) / 64;
    // two blocks per CU over all token groups (one is resident: the tail of a long point then overlaps the next block), at least a few tiles each
    const uint64_t by_tiles = (a.total + 4 * S::TR - 1) / (4 * S::TR), by_cus = ((uint64_t)2 * num_cus + gy - 1) / gy;
    const uint32_t gx = (uint32_t)std::max<uint64_t>(1, std::min(by_tiles, by_cus));
    QMX_NOTE_KERNEL(maxsim_fused_kernel<D32>);
    hipLaunchKernelGGL(maxsim_fused_kernel<D32>, dim3(gx, gy), dim3(256), (size_t)S::LDS, st, a);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

// The caller checked maxsim_fused_dim_ok(dim), 16-byte aligned rows and n < 2^32 - 1.  d_S: [n + 1] (with a candidate list: written by
// launch_maxsim_prefix, d_delta with it; without: the point offsets, d_delta = nullptr), s0 = S[0] and total = S[n] - S[0] as the host knows
// them.  Scratch: d_cmap [total] u32, d_pack [maxsim_fused_pack_floats] f32, d_tokmax [n_tokens][n] f32.
int32_t launch_maxsim_fused(hipStream_t st, const void *d_rows, uint64_t row_stride, uint32_t dim, const void *d_tokens, uint32_t q_stride, uint32_t n_tokens,
                            const uint64_t *d_S, const uint64_t *d_delta, uint64_t n, uint64_t s0, uint64_t total, uint32_t *d_cmap, float *d_pack,
                            float *d_tokmax, const uint32_t *d_qfirst, uint32_t n_queries, float *d_out, int num_cus) {
    if (n == 0 || n_queries == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    if (total && n_tokens) {
        const uint32_t d32 = dim / 32, ks = (d32 + 3) / 4;
        const uint64_t count = maxsim_fused_pack_floats(dim, n_tokens);
        hipLaunchKernelGGL(maxsim_pack_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, st, (const unsigned char *)d_tokens, q_stride, n_tokens, d32,
                           ks, count, d_pack);
        QMX_HIP(hipGetLastError());
        QMX_TRY(launch_maxsim_map(st, d_S, n, s0, d_cmap));
        MsfArgs a;
        a.rows = (const unsigned char *)d_rows; a.row_stride = row_stride; a.S = d_S; a.cmap = d_cmap; a.delta = d_delta; a.bpack = d_pack;
        a.tokmax = d_tokmax; a.n = n; a.s0 = s0; a.total = total; a.n_tokens = n_tokens;
        switch (d32) {
            case 1: QMX_TRY(launch_msf<1>(st, a, num_cus)); break;
            case 2: QMX_TRY(launch_msf<2>(st, a, num_cus)); break;
            case 3: QMX_TRY(launch_msf<3>(st, a, num_cus)); break;
            case 4: QMX_TRY(launch_msf<4>(st, a, num_cus)); break;
            case 5: QMX_TRY(launch_msf<5>(st, a, num_cus)); break;
            case 6: QMX_TRY(launch_msf<6>(st, a, num_cus)); break;
            case 7: QMX_TRY(launch_msf<7>(st, a, num_cus)); break;
            case 8: QMX_TRY(launch_msf<8>(st, a, num_cus)); break;
            default: set_error("maxsim_fused: unsupported row length %u", dim); return QMX_ERR_BAD_ARG;
        }
    } else {
        QMX_NOTE_KERNEL(maxsim_fused_kernel<4>);      // (no rows or no tokens: the sums alone)
    }
    return launch_maxsim_sum(st, d_tokmax, d_S, n, d_qfirst, n_queries, d_out);
}

}  // namespace qmx
