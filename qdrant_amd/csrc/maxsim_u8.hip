// maxsim_u8.hip — Colbert MaxSim over dense u8 multi-vector points (`datatype: uint8`) on v_mfma_i32_16x16x64_i8, without the [tokens][rows]
// similarity matrix and with the reference's bits in ONE kernel (the siblings: maxsim_fused.hip for f32 rows, maxsim_f16.hip for f16 rows, whose row
// stream, work split and prefix / map / sum kernels this file reuses).  Dot, Cosine and Euclid, dim a multiple of 32 in 32 .. 256, either order of
// QMX_SEG_U8_SCALAR_ORDER (api_custom.hip multi_prepare).
//
// What it computes.  cq_scores[j * n + c] = sum over the tokens of multi-query j, in order from 0.0, of max over the rows of candidate c of
// R(token, row), R the reference's u8 score (avx_dot_similarity_bytes / avx_cosine_similarity_bytes / avx_euclid_similarity_bytes, or the scalar
// leaves of metric_uint/simple_*.rs).
//
// Bits.  The AVX2 leaves keep 8 i32 lanes (bytes 4 j .. 4 j + 3 of every 32-byte block in lane j), convert each with cvtepi32_ps and add them with
// hsum256.  With dim <= 256 and dim % 32 == 0 there is no remainder loop; a lane total is at most 32 * 255^2 = 2 080 800 < 2^24 and the whole sum
// at most 256 * 255^2 = 16 646 400 < 2^24 (the static_asserts below).  So every conversion and every partial sum of the hsum is an integer below
// 2^24, i.e. exact, and the leaf returns (float) of the exact integer - which is also what the scalar leaves return (one i32 total, cast once).  Both
// orders therefore have the same bits here, and one kernel serves both.  The integers come from the matrix cores:
//   Dot     (float)V, V = sum q x.  The point's maximum is kept as an int32 (MSU_NONE: no row yet, written out as -inf), converted once per point.
//   Euclid  -(float)(Sq2 + Sx2 - 2 V) (= -sum (q - x)^2 <= 2^24 as well): the same integer maximum of the negated distance.
//   Cosine  n1 = (float)Sq2, n2 = (float)Sx2 (exact), den = n1 * n2, den == 0 ? 0.0f : (float)V / __builtin_sqrtf(den) - the expression of
//           RowU8::finish_with (dense_policies.hpp; correctly rounded division and square root, no contraction), the scalar leaf's
//           `n1 == 0 || n2 == 0` being the same test (a product of two nonzero integers below 2^24 is at least 1).  `if x > max` from -inf in f32.
// The max over a point's rows is order-free (equal maxima are equal bits); the sum over tokens is maxsim_sum_kernel, serial.
//
// Operands.  The matrix instruction multiplies SIGNED bytes: both sides are biased by 128, one xor with 0x80808080 per dword (scan_u8w.hip) - the
// rows in registers after the LDS read, the tokens once per call by maxsim_u8_pack_kernel.  With x' = x - 128, q' = q - 128 and I = sum q' x' (the
// accumulator): V = I + 128 (Sx' + Sq') + 16384 dim = I + 128 Sx + (128 Sq - 16384 dim).  The pack kernel writes (128 Sq - 16384 dim, Sq2) per token
// beside the B images; Sx and Sx2 of a row come from the A-operand dwords a lane already holds, before the xor (udot4 with 0x01010101 and with
// itself), summed over the K-steps and over the four lanes that share the row - a few VALU instructions per K-step under the matrix work.  A K-step
// contracts 64 bytes; at dim = 32 mod 64 the upper half of the last K-step is padding: the B image is zero there (q' = 0), so I is unaffected
// whatever the A side holds; the A side re-reads the lower half's pieces (inside the row, inside the tile) and leaves them out of the row sums.
// Token slots past the last token are zeros and are never written out.
//
// Data movement.  The row stream, the blocks' shares (msf_block_run) and the tile ring (msf_glds16, counted with s_waitcnt vmcnt) are
// maxsim_fused.hip's.  What is u8's own:
//   * a row is dim bytes = dim / 16 pieces; a tile is TR = 128 rows at every dim (4 KiB per 32 coordinates: dim / 32 whole LDS-DMA instructions per
//     wave, wave w moving rows 32 w .. 32 w + 31; waves 0 / 1 and 2 / 3 resolve cmap / delta of rows 0 .. 63 and 64 .. 127);
//   * the A operand of K-step s is the lane's sixteen consecutive bytes k = 64 s + 16 (lane >> 4) ..: ONE ds_read_b128 of piece e = 4 s + (lane >> 4)
//     of row m = lane & 15, from slot m (dim / 16) + (e ^ (msf_swz16(m) & mask)) (maxsim_common.hpp: conflict-free at every row length; a row of
//     2 (2 j + 1) pieces needs no swizzle);
//   * the tokens are B operands [token tile][K-step][64 lanes][16 bytes], a group's 64 tokens resident in LDS (4 KiB per 64 coordinates), one
//     ds_read_b128 per lane at 16 lane: conflict-free;
//   * wave w owns rows 32 w .. 32 w + 31 of the tile against all four token tiles: per K-step two A reads, four B reads, eight matrix instructions
//     into eight accumulators - 8 ceil(dim / 64) instructions per 32 rows x 64 tokens;
//   * up to dim 128 the block fits 80 KiB with a ring of 2 .. 4 tiles and two blocks share a CU (one's segmented max runs under the other's
//     matrix work); from dim 160 on one block per CU with a ring of 3 .. 4.
// Segmented max.  As in the f32 kernel - scratch tile [TR][64 tokens] (ONE plane: a value, no row index, no second best), running maxima per
// (token, quarter of the tile's rows) that restart at point starts, then per point end the merge of the quarters and of the carry of a point that
// began in an earlier tile, double-buffered by tile parity.
// LDS (KiB)   dim   32    64    96    128   160    192    224    256
//   tokens          4.5   4.5   8.5   8.5   12.5   12.5   16.5   16.5     (B images + 512 B of constants)
//   ring            4x4   4x8   2x12  2x16  4x20   4x24   3x28   3x32
//   plane + meta + carry  34 + 2.5 + 0.5 = 37 at every dim
//   total           57.5  73.5  69.5  77.5  129.5  145.5  137.5  149.5
#include "maxsim_common.hpp"
#include "dense_policies.hpp"      // M_DOT / M_EUCLID / M_COSINE

namespace qmx {

typedef int msu_i32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t MSU_BIAS = 0x80808080u;
constexpr int32_t MSU_NONE = INT32_MIN;         // Dot / Euclid: no row of the point yet
constexpr int MSU_MAX_DIM = 256;
static_assert(32ll * 255 * 255 < (1ll << 24), "an i32 lane of the AVX2 leaves converts exactly");
static_assert((long long)MSU_MAX_DIM * 255 * 255 < (1ll << 24), "sum q x, sum x^2 and sum (q - x)^2 are exact f32: hsum256 adds exactly, (float) of the total is the leaf's value");
static_assert((long long)MSU_MAX_DIM * 128 * 128 + 128ll * 255 * MSU_MAX_DIM * 2 + 16384ll * MSU_MAX_DIM < (1ll << 31), "I, 128 Sx and the token's constant stay inside an int32");

template <int D32>
struct MsuShape {
    static constexpr int DIM = 32 * D32;
    static constexpr int KS = (D32 + 1) / 2;                 // K-steps of 64 bytes (the last one half padding at odd D32)
    static constexpr int TR = 128;                           // rows per tile
    static constexpr int PPR = 2 * D32;                      // 16-byte pieces per row
    static constexpr int TILE_B = TR * DIM;
    static constexpr int IPW = TILE_B / 4096;                // LDS-DMA instructions per wave and tile
    static constexpr int CH = TR / 4;                        // rows per quarter of the segmented max
    static constexpr int BPACK_B = 4 * KS * 64 * 16;         // bytes of a token group's B operands
    static constexpr int GROUP_B = BPACK_B + 64 * 8;         // ... and its 64 x (128 Sq - 16384 dim, Sq2)
    static constexpr int PLANE_B = TR * MSF_SIM_P * 4;
    static constexpr int META_B = 5 * TR * 4;                // (ring + 1 tiles, for the deepest ring)
    static constexpr int CARRY_B = 2 * 64 * 4;               // the carry of the tile before, the carry of this one
    static constexpr int FIXED_B = GROUP_B + PLANE_B + META_B + CARRY_B;
    static constexpr int FIT2 = (80 * 1024 - FIXED_B) / TILE_B, FIT1 = (160 * 1024 - FIXED_B) / TILE_B;
    static constexpr int BPC = FIT2 >= 2 ? 2 : 1;            // blocks per CU
    static constexpr int FIT = BPC == 2 ? FIT2 : FIT1;
    static constexpr int NBUF = FIT > 4 ? 4 : FIT;
    static constexpr int OFF_RING = GROUP_B;
    static constexpr int OFF_PLANE = OFF_RING + NBUF * TILE_B;
    static constexpr int OFF_META = OFF_PLANE + PLANE_B;
    static constexpr int OFF_CARRY = OFF_META + META_B;
    static constexpr int LDS = OFF_CARRY + CARRY_B;
    static constexpr uint32_t SWZ_MASK = msf_swz16_mask(PPR);
    static_assert(DIM <= MSU_MAX_DIM && IPW * 4096 == TILE_B && IPW == D32, "whole 1 KiB instructions per wave: wave w moves rows 32 w .. 32 w + 31");
    static_assert(NBUF >= 2 && LDS * BPC <= 160 * 1024 && (NBUF - 1) * IPW < 64, "a ring of two tiles at least; the CU's LDS; the vmcnt field");
    static_assert(PPR % (SWZ_MASK + 1) == 0 && GROUP_B % 16 == 0, "the swizzle stays inside the row");
};

// how a point's maximum is kept: the exact integer (Dot, Euclid), or the f32 quotient (Cosine)
template <int METRIC>
struct MsuVal {
    typedef int32_t T;
    static __device__ __forceinline__ T none() { return MSU_NONE; }
    // (Euclid: the leaf negates its f32 sum, so a distance of 0 is -0.0 there too)
    static __device__ __forceinline__ float out(T v) { return v == MSU_NONE ? -__builtin_inff() : METRIC == M_EUCLID ? -(float)(-v) : (float)v; }
};
template <>
struct MsuVal<M_COSINE> {
    typedef float T;
    static __device__ __forceinline__ T none() { return -__builtin_inff(); }
    static __device__ __forceinline__ float out(T v) { return v; }
};

struct MsuArgs {
    const unsigned char *rows;
    uint64_t row_stride;       // bytes
    const uint64_t *S;         // [n + 1]
    const uint32_t *cmap;      // [total]: candidate of stream row s0 + i
    const uint64_t *delta;     // [n] with a candidate list: (first storage row of candidate c) - S[c], wrapping; nullptr: the stream IS the storage
    const uint4 *bpack;        // [token groups][GROUP_B / 16]
    float *tokmax;             // [n_tokens][n]
    uint64_t n, s0, total;
    uint32_t n_tokens;
};

template <int METRIC, int D32>
__global__ __launch_bounds__(256) void maxsim_u8_kernel(const MsuArgs a) {
    typedef MsuShape<D32> S;
    typedef MsuVal<METRIC> V;
    typedef typename V::T val_t;
    constexpr int KS = S::KS, TR = S::TR, PPR = S::PPR, IPW = S::IPW, NBUF = S::NBUF, CH = S::CH, P = MSF_SIM_P;
    constexpr bool NEED_SX2 = METRIC != M_DOT;
    extern __shared__ __attribute__((aligned(16))) unsigned char msu_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    val_t *plane = reinterpret_cast<val_t *>(msu_smem + S::OFF_PLANE);
    uint32_t *meta = reinterpret_cast<uint32_t *>(msu_smem + S::OFF_META);
    val_t *carry = reinterpret_cast<val_t *>(msu_smem + S::OFF_CARRY);
    const uint32_t ring0 = (uint32_t)(uintptr_t)(msf_lds_byte *)msu_smem + S::OFF_RING;

    // ---- the block's run of the stream: the candidates whose start falls in its share
    const MsfRun run = msf_block_run(a.S, a.cmap, a.s0, a.total);
    const uint64_t b0 = run.b0, b1 = run.b1;
    if (b0 >= b1) return;
    const uint64_t n_tiles = (b1 - b0 + TR - 1) / TR;

    // ---- the token group's B operands and constants
    {
        const uint4 *src = a.bpack + (size_t)blockIdx.y * (S::GROUP_B / 16);
        uint4 *dst = reinterpret_cast<uint4 *>(msu_smem);
        for (int i = tid; i < S::GROUP_B / 16; i += 256) dst[i] = src[i];
    }

    // position of this lane in tile t: waves 0 / 1 resolve rows 0 .. 63 of the tile, waves 2 / 3 rows 64 .. 127 (a wave moves 32 of its 64)
    const uint32_t half = (uint32_t)w >> 1, lrow = half * 64u + (uint32_t)lane;
    auto tile_pos = [&](uint64_t t, bool *valid) -> uint64_t {  // the stream row, clamped into the block's run (phantom loads stay inside the storage)
        const uint64_t pos = b0 + t * TR + lrow;
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
            const uint32_t m = g / PPR, e = (g % PPR) ^ (msf_swz16(m & 15u) & S::SWZ_MASK);
            const uint32_t slo = (uint32_t)__shfl((int)blo, (int)(m & 63u)), shi = (uint32_t)__shfl((int)bhi, (int)(m & 63u));
            const unsigned char *src = reinterpret_cast<const unsigned char *>(((uint64_t)shi << 32) | slo) + e * 16u;
            msf_glds16(src, ring0 + slot * (uint32_t)S::TILE_B + (uint32_t)(w * IPW + i) * 1024u);
        }
    };
    auto stage_tile = [&](uint64_t t, uint32_t cand, uint64_t d, uint32_t slot) {   // cand / d: cmap and delta of the lane's (clamped) position
        bool valid;
        const uint64_t pos = tile_pos(t, &valid);
        if ((w & 1) == 0) meta[(uint32_t)(t % (NBUF + 1)) * TR + lrow] = valid ? cand : MSF_NONE;
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

    const uint32_t kq = (uint32_t)lane >> 4, ncol = (uint32_t)lane & 15u;
    const uint32_t a_row = (uint32_t)(w * 32 + (int)ncol) * (uint32_t)(PPR * 16), sw = msf_swz16(ncol) & S::SWZ_MASK;
    const uint4 *lds_b = reinterpret_cast<const uint4 *>(msu_smem) + lane;
    uint32_t slot = 0;
    uint32_t prev_last = MSF_NONE;          // candidate of the previous tile's last row
    const int tk = tid & 63, qtr = tid >> 6;
    const uint64_t tok = (uint64_t)blockIdx.y * 64 + (uint32_t)tk;
    // the constants of the lane's four tokens 16 tt + (lane & 15): 128 Sq - 16384 dim, Sq2
    msf_barrier();
    int32_t tc[4], tq2[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
        const int2 c = reinterpret_cast<const int2 *>(msu_smem + S::BPACK_B)[16 * tt + (int)ncol];
        tc[tt] = c.x;
        tq2[tt] = c.y;
    }

    for (uint64_t t = 0; t < n_tiles; ++t) {
        // B1: tile t has landed (this wave's share: at most the NBUF - 1 tiles issued after it are outstanding; the barrier: everyone's), and
        // every wave is done with the previous tile's scratch
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NBUF - 1) * IPW) : "memory");
        msf_barrier();
        // the rows of tile t + NBUF: delta of its candidates, and cmap of the tile after it - both arrive under the matrix work
        const uint64_t d_next = a.delta ? a.delta[c_cur] : 0ull;
        const uint32_t c_next = load_cand(t + NBUF + 1);

        // ---- I = sum q' x' of the wave's 32 rows x 64 tokens, and the rows' Sx / Sx2 from the operand dwords
        const unsigned char *tile = msu_smem + S::OFF_RING + slot * S::TILE_B + a_row;
        msu_i32x4 acc[2][4];
        uint32_t sx[2] = {0u, 0u}, sx2[2] = {0u, 0u};
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) acc[rb][tt] = (msu_i32x4){0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            constexpr bool ODD = D32 % 2 != 0;
            const bool padded = ODD && s == KS - 1 && kq >= 2;         // the lane's piece lies past the row: re-read piece e - 2, count nothing
            const uint32_t e = 4u * (uint32_t)s + kq - (padded ? 2u : 0u);
            msu_i32x4 av[2];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                const uint4 x = *reinterpret_cast<const uint4 *>(tile + (uint32_t)rb * (uint32_t)(16 * PPR * 16) + ((e ^ sw) * 16u));
                const uint32_t xd[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t live = padded ? 0u : xd[k];
                    sx[rb] = __builtin_amdgcn_udot4(live, 0x01010101u, sx[rb], false);
                    if (NEED_SX2) sx2[rb] = __builtin_amdgcn_udot4(live, live, sx2[rb], false);
                }
                av[rb] = (msu_i32x4){(int)(x.x ^ MSU_BIAS), (int)(x.y ^ MSU_BIAS), (int)(x.z ^ MSU_BIAS), (int)(x.w ^ MSU_BIAS)};
            }
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const uint4 bv = lds_b[(tt * KS + s) * 64];
                const msu_i32x4 b = (msu_i32x4){(int)bv.x, (int)bv.y, (int)bv.z, (int)bv.w};
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) acc[rb][tt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[rb], b, acc[rb][tt], 0, 0, 0);
            }
        }
        // the four lanes (m, kq = 0 .. 3) of a row hold its four quarters: every lane gets the row's totals
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            sx[rb] += (uint32_t)__shfl_xor((int)sx[rb], 16, 64);
            sx[rb] += (uint32_t)__shfl_xor((int)sx[rb], 32, 64);
            if (NEED_SX2) {
                sx2[rb] += (uint32_t)__shfl_xor((int)sx2[rb], 16, 64);
                sx2[rb] += (uint32_t)__shfl_xor((int)sx2[rb], 32, 64);
            }
        }
        // D register j of lane (kq, n) is (row 4 kq + j, token n): that row's totals sit in lane 4 kq + j
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int from = 4 * (int)kq + j;
                const int32_t r1 = 128 * __shfl((int)sx[rb], from, 64);
                const int32_t r2 = NEED_SX2 ? __shfl((int)sx2[rb], from, 64) : 0;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int32_t v = acc[rb][tt][j] + r1 + tc[tt];          // V = sum q x
                    val_t out;
                    if (METRIC == M_DOT) out = (val_t)v;
                    else if (METRIC == M_EUCLID) out = (val_t)(2 * v - tq2[tt] - r2);
                    else {
                        const float den = (float)tq2[tt] * (float)r2;           // norm1 * norm2 (RowU8::finish_with)
                        out = (val_t)(den == 0.0f ? 0.0f : (float)v / __builtin_sqrtf(den));
                    }
                    plane[(w * 32 + rb * 16 + 4 * (int)kq + j) * P + 16 * tt + (int)ncol] = out;
                }
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
            val_t mx = V::none();
#pragma unroll 8
            for (int r = qtr * CH; r < qtr * CH + CH; ++r) {
                const uint32_t c = mt[r];
                const val_t v = plane[r * P + tk];
                if (c != prev) { mx = V::none(); prev = c; }
                if (v > mx) mx = v;
                plane[r * P + tk] = mx;
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
                val_t v = plane[r * P + tk];
                for (int qq = qtr - 1; qq >= 0; --qq) {
                    const int re = qq * CH + CH - 1;
                    if (mt[re] != c) break;
                    const val_t x = plane[re * P + tk];
                    if (x > v) v = x;
                }
                if (cont_in && c == first_c) {
                    const val_t x = carry[(int)(~t & 1) * 64 + tk];
                    if (x > v) v = x;
                }
                if (r == TR - 1 && next_first == c) carry[(int)(t & 1) * 64 + tk] = v;      // (another quarter may still read the previous tile's)
                else if (tok < a.n_tokens) a.tokmax[tok * a.n + c] = V::out(v);
            }
            prev_last = mt[TR - 1];
        }
        slot = slot + 1 == NBUF ? 0 : slot + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the phantom tiles land before the block's LDS is given back
}

// ---- the tokens as biased B operands, and their constants: one wave per token slot of the 64-token groups.  Per group: out[((tile * KS + s) * 64 +
// 16 kq + j)] = bytes 64 s + 16 kq .. + 15 of token 64 group + 16 tile + j, each xor 0x80; zeros (q' = 0) past the row's end and past the last token;
// then 64 x {128 Sq - 16384 dim, Sq2}
__global__ __launch_bounds__(64) void maxsim_u8_pack_kernel(const unsigned char *queries, uint32_t q_stride, uint32_t n_tokens, uint32_t dim, uint4 *out) {
    const uint32_t slot = blockIdx.x, lane = threadIdx.x, ks = (dim + 63) / 64;
    const uint32_t group_u4 = ks * 256 + 32;                 // uint4s per group: 4 ks 64 images, 64 x 8 bytes of constants
    const bool live = slot < n_tokens;
    uint32_t s1 = 0, s2 = 0;
    uint4 *gout = out + (uint64_t)(slot >> 6) * group_u4;
    if (lane < ks * 4) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (live && lane * 16 < dim) {
            v = *reinterpret_cast<const uint4 *>(queries + (uint64_t)slot * q_stride + (uint64_t)lane * 16);
            const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s1 = __builtin_amdgcn_udot4(wd[k], 0x01010101u, s1, false);
                s2 = __builtin_amdgcn_udot4(wd[k], wd[k], s2, false);
            }
            v = make_uint4(v.x ^ MSU_BIAS, v.y ^ MSU_BIAS, v.z ^ MSU_BIAS, v.w ^ MSU_BIAS);
        }
        const uint32_t tile = (slot >> 4) & 3u, j = slot & 15u, s = lane >> 2, kq = lane & 3u;
        gout[(tile * ks + s) * 64 + 16 * kq + j] = v;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        s1 += (uint32_t)__shfl_xor((int)s1, o, 64);
        s2 += (uint32_t)__shfl_xor((int)s2, o, 64);
    }
    if (lane == 0)
        reinterpret_cast<int2 *>(gout + ks * 256)[slot & 63u] = live ? make_int2(128 * (int32_t)s1 - 16384 * (int32_t)dim, (int32_t)s2) : make_int2(0, 0);
}

// ---------------------------------------------------------------------------------------------------------------------------
bool maxsim_u8_dim_ok(uint32_t dim) { return dim % 32 == 0 && dim >= 32 && dim <= (uint32_t)MSU_MAX_DIM; }
uint64_t maxsim_u8_pack_bytes(uint32_t dim, uint32_t n_tokens) { return (uint64_t)((n_tokens + 63) / 64) * (((dim + 63) / 64) * 4096ull + 512); }

template <int METRIC, int D32>
static int32_t launch_msu(hipStream_t st, const MsuArgs &a, int num_cus) {
    typedef MsuShape<D32> S;
    static thread_local DeviceOnce attr_once;
    if (attr_once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(maxsim_u8_kernel<METRIC, D32>), hipFuncAttributeMaxDynamicSharedMemorySize, S::LDS));
        attr_once.mark();
    }
    const uint32_t gy = (a.n_tokens + 63) / 64;
    // twice the resident blocks over all token groups (the tail of a long point then overlaps the next block), at least a few tiles each
    const uint64_t by_tiles = (a.total + 4 * S::TR - 1) / (4 * S::TR), by_cus = ((uint64_t)2 * S::BPC * num_cus + gy - 1) / gy;
    const uint32_t gx = (uint32_t)std::max<uint64_t>(1, std::min(by_tiles, by_cus));
    QMX_NOTE_KERNEL((maxsim_u8_kernel<METRIC, D32>));
    hipLaunchKernelGGL((maxsim_u8_kernel<METRIC, D32>), dim3(gx, gy), dim3(256), (size_t)S::LDS, st, a);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

template <int METRIC>
static int32_t launch_msu_dim(hipStream_t st, const MsuArgs &a, uint32_t d32, int num_cus) {
    switch (d32) {
        case 1: return launch_msu<METRIC, 1>(st, a, num_cus);
        case 2: return launch_msu<METRIC, 2>(st, a, num_cus);
        case 3: return launch_msu<METRIC, 3>(st, a, num_cus);
        case 4: return launch_msu<METRIC, 4>(st, a, num_cus);
        case 5: return launch_msu<METRIC, 5>(st, a, num_cus);
        case 6: return launch_msu<METRIC, 6>(st, a, num_cus);
        case 7: return launch_msu<METRIC, 7>(st, a, num_cus);
        default: return launch_msu<METRIC, 8>(st, a, num_cus);
    }
}

// The caller checked maxsim_u8_dim_ok(dim), 16-byte aligned rows and tokens and n < 2^32 - 1.  d_S / d_delta / s0 / total as for launch_maxsim_fused.
// Scratch: d_cmap [total] u32, d_pack maxsim_u8_pack_bytes, d_tokmax [n_tokens][n] f32.
int32_t launch_maxsim_u8(hipStream_t st, int distance, const void *d_rows, uint64_t row_stride, uint32_t dim, const void *d_tokens, uint32_t q_stride,
                         uint32_t n_tokens, const uint64_t *d_S, const uint64_t *d_delta, uint64_t n, uint64_t s0, uint64_t total, uint32_t *d_cmap,
                         void *d_pack, float *d_tokmax, const uint32_t *d_qfirst, uint32_t n_queries, float *d_out, int num_cus) {
    if (n == 0 || n_queries == 0) return QMX_OK;
    QMX_REQUIRE(maxsim_u8_dim_ok(dim) && row_stride % 16 == 0 && row_stride >= dim && q_stride % 16 == 0 && q_stride >= dim, QMX_ERR_BAD_ARG,
                "maxsim_u8: rows of %u bytes", dim);
    QMX_REQUIRE(distance == QMX_DISTANCE_DOT || distance == QMX_DISTANCE_COSINE || distance == QMX_DISTANCE_EUCLID, QMX_ERR_BAD_ARG,
                "maxsim_u8: distance %d has no contraction", distance);
    ::qmx::clear_stale_error();
    if (total && n_tokens) {
        hipLaunchKernelGGL(maxsim_u8_pack_kernel, dim3((n_tokens + 63) / 64 * 64), dim3(64), 0, st, (const unsigned char *)d_tokens, q_stride, n_tokens, dim,
                           (uint4 *)d_pack);
        QMX_HIP(hipGetLastError());
        QMX_TRY(launch_maxsim_map(st, d_S, n, s0, d_cmap));
        MsuArgs a;
        a.rows = (const unsigned char *)d_rows; a.row_stride = row_stride; a.S = d_S; a.cmap = d_cmap; a.delta = d_delta; a.bpack = (const uint4 *)d_pack;
        a.tokmax = d_tokmax; a.n = n; a.s0 = s0; a.total = total; a.n_tokens = n_tokens;
        if (distance == QMX_DISTANCE_DOT) QMX_TRY(launch_msu_dim<M_DOT>(st, a, dim / 32, num_cus));
        else if (distance == QMX_DISTANCE_EUCLID) QMX_TRY(launch_msu_dim<M_EUCLID>(st, a, dim / 32, num_cus));
        else QMX_TRY(launch_msu_dim<M_COSINE>(st, a, dim / 32, num_cus));
    } else {
        QMX_NOTE_KERNEL((maxsim_u8_kernel<M_DOT, 4>));      // (no rows or no tokens: the sums alone)
    }
    return launch_maxsim_sum(st, d_tokmax, d_S, n, d_qfirst, n_queries, d_out);
}

}  // namespace qmx
