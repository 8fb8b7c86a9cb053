// maxsim_f16.hip — Colbert MaxSim over dense f16 multi-vector points (`datatype: float16`) on v_mfma_f32_16x16x32_f16, without the [tokens][rows]
// similarity matrix and with the reference's bits (score_max_similarity over Metric<f16>; the f32 sibling: maxsim_fused.hip, whose row stream,
// work split, prefix / map / sum kernels this file reuses).  Taken for inner segments created with QMX_SEG_F16_WIDE, Dot / Cosine, dim a multiple of 32
// in 32 .. 256 (api_custom.hip multi_prepare).
//
// What it computes.  cq_scores[j * n + c] = sum over the tokens of multi-query j, in order from 0.0, of max over the rows of candidate c of
// R(token, row), R the reference's f16 score: 32 f32 fma chains over the converted halves, folded by hsum256_ps_avx (f16_avx_leaf.hpp).
//
// Two kernels.  The f16 matrix instruction contracts 32 elements per step into ONE accumulator in an order of its own: its score A is not R.  But a
// MaxSim needs only the maximum per (token, point), so:
//   1. maxsim_f16_kernel streams the candidates' rows once per 64 tokens and keeps, per (token, point), the triple (m1, r1, m2): the best A, the row
//      that gave it, the second best A (equal values: m2 = m1).  It writes m1 and r1 - or FLAG when m2 is not provably below m1 - band(token).
//   2. maxsim_f16_exact_kernel re-scores row r1 alone in the reference's order (unflagged pair), or every row of the point with `if x > max` from
//      -inf (flagged pair), and overwrites tokmax[token][candidate].  maxsim_sum_kernel then runs as for f32.
//
// Why r1 is the argmax of R.  band(token) = f16w_band(F16W_DOT, dim, token, rowmax, seg_subnormal) of f16w_band.hpp, verbatim: band >= 2 (eAR + eSub)
// + 4 u B, where |A - R| <= eAR + eSub for every row of the segment (its (1), (2), (5): any summation order of the exact products, subnormal operands
// possibly flushed) and B = |token| rowmax >= |A|, |R|.  A pair stays unflagged only if m2 < fl(m1 - band).  Every other row r of the point has
// A(r) <= m2, so R(r) <= A(r) + e < fl(m1 - band) + e <= m1 - band + u (1.001 B + band) + e <= m1 - e <= R(r1)   (e = eAR + eSub; the subtraction's
// rounding is paid by the 4 u B, as the selection's in (6)).  So R(r1) is the point's maximum, and its bits are what the reference's `if x > max`
// loop ends with (rows of equal R have equal bits; a +-0 disagreement cannot reach the sum, which starts at +0.0).  A token with an Inf / NaN
// element gets band = +inf: all its pairs are flagged (the compare is written so that a NaN flags).  The segment's elements are finite (checked at
// create: f16_maxsim_ok), so no other pair sees a NaN.
//
// Kernel 1, data movement.  The row stream, the blocks' shares and the tile ring are maxsim_fused.hip's.  What is f16's own:
//   * a row is dim x 2 bytes, a tile is TR = 64 rows at every dim (4 KiB per 32 coordinates), and the ring is as deep as the LDS left beside the
//     tokens and the scratch allows: 4 tiles up to dim 160, 3 at 192, 2 at 224 / 256;
//   * the A operand of K-step s is the lane's eight consecutive halves k = 32 s + 8 (lane >> 4) ..: ONE ds_read_b128 of piece e = 4 s + (lane >> 4)
//     of row m = lane & 15.  Piece e of tile row m sits in slot m (dim / 8) + (e ^ swz(m & 15)).  A ds_read_b128 is served sixteen lanes at a time -
//     {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 - i.e. two k-groups kq, kq + 1 with complementary rows; swz makes their sixteen
//     slots distinct mod 16 (the 64 banks) at every row length: bits 0-1 = {0, 2, 3, 1}[m >> 2] (with kq: four values per m & 3), bit 2 = bit 1 of
//     m, bit 3 = bit 0 of m, cut to the bits the row length does not already supply (a row of 4 (2 j + 1) pieces spreads m & 3 itself, one of
//     8 (2 j + 1) pieces m & 1);
//   * the tokens are packed once per call by maxsim_f16_pack_kernel as f16 B operands [token tile][K-step][64 lanes][8 halves], zeros past the last
//     token; a group's 64 tokens stay resident in LDS (4 KiB per 32 coordinates), read one ds_read_b128 per lane at 16 lane: conflict-free;
//   * wave w owns rows 16 w .. of the tile against all four token tiles: per K-step one A read, four B reads, four matrix instructions into four
//     accumulators - dim / 32 steps chained, no chain separation: 4 (dim / 32) instructions per 16 rows x 64 tokens (the f32 kernel: 128 (dim / 128)).
// Segmented max.  As in the f32 kernel - scratch tile, running values per (token, quarter of the tile's rows) that restart at point starts, then per
// point end the merge of the quarters and of the carry of a point that began in an earlier tile - but over triples, kept in three scratch planes
// (m1, m2, row).  msh_merge is associative; step 1, the quarters and the carry all use it.  A row is named by its position in the stream (u32: the
// caller keeps streams below 2^32 - 1 rows).
// LDS at dim 128: 16 (tokens) + 51 (planes) + 64 (ring) + 2.75 KiB = 133.75 KiB; at dim 256: 32 + 51 + 64 + 2.75 = 149.75 KiB; at dim 32: 73.75 KiB,
// two blocks per CU.
#include "maxsim_common.hpp"
#include "f16_avx_leaf.hpp"
#include "f16w_band.hpp"

namespace qmx {

typedef float msh_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 msh_half8 __attribute__((ext_vector_type(8)));

constexpr uint32_t MSH_FLAG = 0xFFFFFFFFu;      // ridx: the pair takes every row of the point in the exact kernel

template <int D32>
struct MshShape {
    static constexpr int DIM = 32 * D32;
    static constexpr int TR = 64;                            // rows per tile
    static constexpr int PPR = 4 * D32;                      // 16-byte pieces per row
    static constexpr int TILE_B = TR * DIM * 2;
    static constexpr int IPW = TILE_B / 4096;                // LDS-DMA instructions per wave and tile
    static constexpr int CH = TR / 4;                        // rows per quarter of the segmented max
    static constexpr int BPACK_B = 4 * D32 * 64 * 16;        // bytes of a token group's B operands
    static constexpr int PLANE_B = TR * MSF_SIM_P * 4;
    static constexpr int META_B = 5 * TR * 4;                // (ring + 1 tiles, for the deepest ring)
    static constexpr int CARRY_B = 2 * 3 * 64 * 4;           // the carry of the tile before, the carry of this one: three planes each
    static constexpr int FIXED_B = BPACK_B + 3 * PLANE_B + META_B + CARRY_B;
    static constexpr int FIT = (160 * 1024 - FIXED_B) / TILE_B;
    static constexpr int NBUF = FIT > 4 ? 4 : FIT;
    static constexpr int OFF_RING = BPACK_B;
    static constexpr int OFF_PLANES = OFF_RING + NBUF * TILE_B;
    static constexpr int OFF_META = OFF_PLANES + 3 * PLANE_B;
    static constexpr int OFF_CARRY = OFF_META + META_B;
    static constexpr int LDS = OFF_CARRY + CARRY_B;
    static constexpr uint32_t SWZ_MASK = msf_swz16_mask(PPR);
    static_assert(NBUF >= 2 && LDS <= 160 * 1024 && (NBUF - 1) * IPW < 64, "a ring of two tiles at least; the CU's LDS; the vmcnt field");
    static_assert(PPR % (SWZ_MASK + 1) == 0, "the swizzle stays inside the row");
};

struct MshTriple {
    float m1;          // the best similarity
    uint32_t r1;       // ... its row (MSF_NONE: none yet)
    float m2;          // the second best (a tie of the best: m2 = m1)
};
// the two best of x's rows and y's rows, x's first (a tie keeps x's row); a NaN in y.m1 is skipped
__device__ __forceinline__ MshTriple msh_merge(const MshTriple &x, const MshTriple &y) {
    MshTriple o;
    if (y.m1 > x.m1) { o.m1 = y.m1; o.r1 = y.r1; o.m2 = y.m2 > x.m1 ? y.m2 : x.m1; }
    else { o.m1 = x.m1; o.r1 = x.r1; o.m2 = y.m1 > x.m2 ? y.m1 : x.m2; }
    return o;
}

struct MshArgs {
    const unsigned char *rows;
    uint64_t row_stride;       // bytes
    const uint64_t *S;         // [n + 1]
    const uint32_t *cmap;      // [total]: candidate of stream row s0 + i
    const uint64_t *delta;     // [n] with a candidate list: (first storage row of candidate c) - S[c], wrapping; nullptr: the stream IS the storage
    const uint4 *bpack;        // [token groups][BPACK_B / 16]
    const float *band;         // [token groups][64]
    float *tokmax;             // [n_tokens][n]: m1
    uint32_t *ridx;            // [n_tokens][n]: r1 as a stream position counted from s0, or MSH_FLAG
    uint64_t n, s0, total;
    uint32_t n_tokens;
};

template <int D32>
__global__ __launch_bounds__(256) void maxsim_f16_kernel(const MshArgs a) {
    typedef MshShape<D32> S;
    constexpr int TR = S::TR, PPR = S::PPR, IPW = S::IPW, NBUF = S::NBUF, CH = S::CH, P = MSF_SIM_P;
    extern __shared__ __attribute__((aligned(16))) unsigned char msh_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *pl_m1 = reinterpret_cast<float *>(msh_smem + S::OFF_PLANES);
    float *pl_m2 = reinterpret_cast<float *>(msh_smem + S::OFF_PLANES + S::PLANE_B);
    uint32_t *pl_r = reinterpret_cast<uint32_t *>(msh_smem + S::OFF_PLANES + 2 * S::PLANE_B);
    uint32_t *meta = reinterpret_cast<uint32_t *>(msh_smem + S::OFF_META);
    float *carry_m1 = reinterpret_cast<float *>(msh_smem + S::OFF_CARRY);      // [2][64] each
    float *carry_m2 = carry_m1 + 128;
    uint32_t *carry_r = reinterpret_cast<uint32_t *>(carry_m1 + 256);
    const uint32_t ring0 = (uint32_t)(uintptr_t)(msf_lds_byte *)msh_smem + S::OFF_RING;

    // ---- the block's run of the stream: the candidates whose start falls in [lo, hi)
    const MsfRun run = msf_block_run(a.S, a.cmap, a.s0, a.total);
    const uint64_t b0 = run.b0, b1 = run.b1;
    if (b0 >= b1) return;
    const uint64_t n_tiles = (b1 - b0 + TR - 1) / TR;

    // ---- the token group's B operands
    {
        const uint4 *src = a.bpack + (size_t)blockIdx.y * (S::BPACK_B / 16);
        uint4 *dst = reinterpret_cast<uint4 *>(msh_smem);
        for (int i = tid; i < S::BPACK_B / 16; i += 256) dst[i] = src[i];
    }

    // position of this lane in tile t (every wave resolves the whole tile)
    auto tile_pos = [&](uint64_t t, bool *valid) -> uint64_t {  // the stream row, clamped into the block's run (phantom loads stay inside the storage)
        const uint64_t pos = b0 + t * TR + (uint32_t)lane;
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
            const uint32_t slo = (uint32_t)__shfl((int)blo, (int)m), shi = (uint32_t)__shfl((int)bhi, (int)m);
            const unsigned char *src = reinterpret_cast<const unsigned char *>(((uint64_t)shi << 32) | slo) + e * 16u;
            msf_glds16(src, ring0 + slot * (uint32_t)S::TILE_B + (uint32_t)(w * IPW + i) * 1024u);
        }
    };
    auto stage_tile = [&](uint64_t t, uint32_t cand, uint64_t d, uint32_t slot) {   // cand / d: cmap and delta of the lane's (clamped) position
        bool valid;
        const uint64_t pos = tile_pos(t, &valid);
        if (w == 0) meta[(uint32_t)(t % (NBUF + 1)) * TR + lane] = valid ? cand : MSF_NONE;
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

    const uint32_t mrow = (uint32_t)(w * 16 + (lane & 15)), kq = (uint32_t)lane >> 4;
    const uint32_t a_row = mrow * (uint32_t)(PPR * 16), sw = msf_swz16(mrow & 15u) & S::SWZ_MASK;
    const uint4 *lds_b = reinterpret_cast<const uint4 *>(msh_smem) + lane;
    uint32_t slot = 0;
    uint32_t prev_last = MSF_NONE;          // candidate of the previous tile's last row
    const int tk = tid & 63, qtr = tid >> 6;
    const uint64_t tok = (uint64_t)blockIdx.y * 64 + (uint32_t)tk;
    const float band = a.band[tok];

    for (uint64_t t = 0; t < n_tiles; ++t) {
        // B1: tile t has landed (this wave's share: at most the NBUF - 1 tiles issued after it are outstanding; the barrier: everyone's), and
        // every wave is done with the previous tile's scratch
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NBUF - 1) * IPW) : "memory");
        msf_barrier();
        // the rows of tile t + NBUF: delta of its candidates, and cmap of the tile after it - both arrive under the matrix work
        const uint64_t d_next = a.delta ? a.delta[c_cur] : 0ull;
        const uint32_t c_next = load_cand(t + NBUF + 1);

        // ---- approximate similarities of the wave's 16 rows x 64 tokens: dim / 32 chained steps
        const unsigned char *tile = msh_smem + S::OFF_RING + slot * S::TILE_B + a_row;
        msh_f32x4 acc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) acc[tt] = (msh_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < D32; ++s) {
            const msh_half8 av = *reinterpret_cast<const msh_half8 *>(tile + (((uint32_t)(4 * s) + kq) ^ sw) * 16u);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const uint4 bv = lds_b[(tt * D32 + s) * 64];
                acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, __builtin_bit_cast(msh_half8, bv), acc[tt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int j = 0; j < 4; ++j) pl_m1[(w * 16 + 4 * (int)kq + j) * P + 16 * tt + (lane & 15)] = acc[tt][j];
        // B2: the scratch tile is whole, and nobody reads ring slot `slot` any more: refill it
        msf_barrier();
        // (c_next is waited for here, where the tiles in flight were issued an iteration ago - not at the top of the next iteration, behind this
        // iteration's stores, where the compiler's vmcnt(0) would drain the ring)
        asm volatile("" :: "v"(c_next), "v"(d_next));
        stage_tile(t + NBUF, c_cur, d_next, slot);
        c_cur = c_next;

        // ---- segmented max, step 1: the running triple inside (point, quarter of the tile's rows); rows are named by their index in the tile
        const uint32_t *mt = meta + (uint32_t)(t % (NBUF + 1)) * TR;
        {
            uint32_t prev = MSF_NONE;
            MshTriple run{-__builtin_inff(), MSF_NONE, -__builtin_inff()};
#pragma unroll
            for (int r = qtr * CH; r < qtr * CH + CH; ++r) {
                const uint32_t c = mt[r];
                if (c != prev) { run = MshTriple{-__builtin_inff(), MSF_NONE, -__builtin_inff()}; prev = c; }
                run = msh_merge(run, MshTriple{pl_m1[r * P + tk], (uint32_t)r, -__builtin_inff()});
                pl_m1[r * P + tk] = run.m1;
                pl_m2[r * P + tk] = run.m2;
                pl_r[r * P + tk] = run.r1;
            }
        }
        msf_barrier();         // B3
        // ---- step 2: every point end of this quarter: merge the quarters the point spans and its carry; write or carry on.  From here on a row is
        // named by its position in the stream, counted from s0
        {
            const uint32_t first_c = mt[0];
            const bool cont_in = first_c == prev_last;
            const uint32_t next_first = meta[(uint32_t)((t + 1) % (NBUF + 1)) * TR];
            const uint32_t off0 = (uint32_t)(b0 + t * TR - a.s0);      // (no load here: a returning load in this step would wait for the whole ring)
            for (int r = qtr * CH; r < qtr * CH + CH; ++r) {
                const uint32_t c = mt[r];
                if (c == MSF_NONE) break;
                if (r != TR - 1 && mt[r + 1] == c) continue;
                auto plane = [&](int rr) -> MshTriple {
                    const uint32_t ri = pl_r[rr * P + tk];
                    return MshTriple{pl_m1[rr * P + tk], ri == MSF_NONE ? MSF_NONE : off0 + ri, pl_m2[rr * P + tk]};
                };
                MshTriple v = plane(r);
                for (int qq = qtr - 1; qq >= 0; --qq) {
                    const int re = qq * CH + CH - 1;
                    if (mt[re] != c) break;
                    v = msh_merge(plane(re), v);
                }
                if (cont_in && c == first_c) {
                    const int ci = (int)(~t & 1) * 64 + tk;
                    v = msh_merge(MshTriple{carry_m1[ci], carry_r[ci], carry_m2[ci]}, v);
                }
                if (r == TR - 1 && next_first == c) {      // (another quarter may still read the previous tile's)
                    const int ci = (int)(t & 1) * 64 + tk;
                    carry_m1[ci] = v.m1; carry_r[ci] = v.r1; carry_m2[ci] = v.m2;
                } else if (tok < a.n_tokens) {
                    const bool sure = v.m2 < v.m1 - band && v.r1 != MSF_NONE;      // (a NaN on either side: not sure)
                    a.tokmax[tok * a.n + c] = v.m1;
                    a.ridx[tok * a.n + c] = sure ? v.r1 : MSH_FLAG;
                }
            }
            prev_last = mt[TR - 1];
        }
        slot = slot + 1 == NBUF ? 0 : slot + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the phantom tiles land before the block's LDS is given back
}

// ---- the tokens as B operands, and their bands: one wave per token slot of the 64-token groups.  out[(((group * 4 + tile) * D32 + s) * 64 + 16 kq + j)]
// = halves 32 s + 8 kq .. + 7 of token 64 group + 16 tile + j; zeros past the last token.  band[slot] = f16w_band of the token; +inf for a token with
// an Inf / NaN element (and past the last token, where nobody reads it)
__global__ __launch_bounds__(64) void maxsim_f16_pack_kernel(const unsigned char *queries, uint32_t q_stride, uint32_t n_tokens, uint32_t dim, float rowmax,
                                                             uint32_t seg_subnormal, uint4 *out, float *band) {
    const uint32_t slot = blockIdx.x, lane = threadIdx.x, d32 = dim / 32;
    const bool live = slot < n_tokens;
    F16WQuery s{0.0, 0.0, 0u, 0u};
    if (lane < dim / 8) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (live) {
            v = *reinterpret_cast<const uint4 *>(queries + (uint64_t)slot * q_stride + (uint64_t)lane * 16);
            const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t h = (wd[e / 2] >> (16 * (e % 2))) & 0xFFFFu, ex = h & 0x7C00u;
                s.bad += ex == 0x7C00u;
                s.nsub += ex == 0 && (h & 0x3FFu) != 0;
                const double x = ex == 0x7C00u ? 0.0 : (double)fw_h2f(h);
                s.q2 += x * x;
                s.l1 += fabs(x);
            }
        }
        const uint32_t group = slot >> 6, tile = (slot >> 4) & 3u, j = slot & 15u, ks = lane >> 2, kq = lane & 3u;
        out[((uint64_t)(group * 4 + tile) * d32 + ks) * 64 + 16 * kq + j] = v;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        s.q2 += __shfl_xor(s.q2, o, 64);
        s.l1 += __shfl_xor(s.l1, o, 64);
        s.nsub += __shfl_xor(s.nsub, o, 64);
        s.bad += __shfl_xor(s.bad, o, 64);
    }
    if (lane == 0) band[slot] = live && s.bad == 0 ? f16w_band(F16W_DOT, dim, s, rowmax, seg_subnormal != 0) : __builtin_inff();
}

// ---- the reference's bits.  Items are candidate-major - (candidate, pair of tokens), a wave each, 32 lanes per token - so the waves that share a
// point run together and its rows come from HBM at most once more.  An unflagged pair: the exact score of row r1; a flagged one: of every row of the
// point, `if x > max` from -inf.  (The two halves of a wave walk the longer of their two row counts together: the leaf's shuffles want all lanes.)
struct MshExactArgs {
    const unsigned char *rows, *queries;
    uint64_t row_stride;
    const uint64_t *S, *delta;
    const uint32_t *ridx;
    float *tokmax;
    uint64_t n, s0;
    uint32_t n_tokens, q_stride, dim;
};
__global__ __launch_bounds__(256) void maxsim_f16_exact_kernel(const MshExactArgs a) {
    const uint32_t lane = threadIdx.x & 63u, l = lane & 31u;
    const uint64_t n_tp = (a.n_tokens + 1) / 2, n_items = a.n * n_tp;
    for (uint64_t item = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < n_items; item += (uint64_t)gridDim.x * 4) {
        const uint64_t c = item / n_tp;
        const uint32_t tok2 = (uint32_t)(item % n_tp) * 2, tok_h = tok2 + (lane >> 5);
        const uint64_t first = a.S[c], len64 = a.S[c + 1] - first;
        if (len64 == 0) continue;                                  // (maxsim_sum_kernel: -inf per token)
        const uint32_t len = (uint32_t)len64, rel = (uint32_t)(first - a.s0);      // (the stream is shorter than 2^32 - 1 rows)
        const bool valid = tok_h < a.n_tokens;
        const uint32_t tok = valid ? tok_h : tok2;
        const uint32_t r1 = a.ridx[(uint64_t)tok * a.n + c];
        const bool all = r1 - rel >= len;                          // MSH_FLAG (and nothing else: kernel 1 names rows of the point)
        const uint32_t cnt = all ? len : 1u, start = all ? 0u : r1 - rel;
        const uint32_t other = (uint32_t)__shfl_xor((int)cnt, 32, 64), n_it = cnt > other ? cnt : other;
        const uint64_t row0 = first + (a.delta ? a.delta[c] : 0ull) + start;
        const unsigned short *y = reinterpret_cast<const unsigned short *>(a.queries + (uint64_t)tok * a.q_stride) + l;
        float mx = -__builtin_inff();
        for (uint32_t i = 0; i < n_it; ++i) {
            const bool mine = i < cnt;
            const unsigned short *x = reinterpret_cast<const unsigned short *>(a.rows + (row0 + (mine ? i : 0u)) * a.row_stride) + l;
            const float v = f16_avx_pair<M_DOT>(x, y, a.dim, lane);
            if (mine && v > mx) mx = v;
        }
        if (valid && l == 0) a.tokmax[(uint64_t)tok * a.n + c] = mx;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
bool maxsim_f16_dim_ok(uint32_t dim) { return dim % 32 == 0 && dim >= 32 && dim <= 256; }
uint64_t maxsim_f16_pack_bytes(uint32_t dim, uint32_t n_tokens) { return (uint64_t)((n_tokens + 63) / 64) * (64ull * dim * 2 + 64 * 4); }

template <int D32>
static int32_t launch_msh(hipStream_t st, const MshArgs &a, int num_cus) {
    typedef MshShape<D32> S;
    static thread_local DeviceOnce attr_once;
    if (attr_once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(maxsim_f16_kernel<D32>), hipFuncAttributeMaxDynamicSharedMemorySize, S::LDS));
        attr_once.mark();
    }
    const uint32_t gy = (a.n_tokens + 63) / 64;
    // two blocks per CU over all token groups, at least a few tiles each (maxsim_fused.hip launch_msf)
    const uint64_t by_tiles = (a.total + 4 * S::TR - 1) / (4 * S::TR), by_cus = ((uint64_t)2 * num_cus + gy - 1) / gy;
    const uint32_t gx = (uint32_t)std::max<uint64_t>(1, std::min(by_tiles, by_cus));
    QMX_NOTE_KERNEL(maxsim_f16_kernel<D32>);
    hipLaunchKernelGGL(maxsim_f16_kernel<D32>, dim3(gx, gy), dim3(256), (size_t)S::LDS, st, a);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

// The caller checked maxsim_f16_dim_ok(dim), 16-byte aligned rows and tokens, a segment of finite elements, n < 2^32 - 1 and total < 2^32 - 1.  d_S / d_delta / s0 / total as for launch_maxsim_fused.  Scratch: d_cmap [total] u32, d_pack maxsim_f16_pack_bytes (the operands, then
// the bands), d_tokmax and d_ridx [n_tokens][n].
int32_t launch_maxsim_f16(hipStream_t st, const void *d_rows, uint64_t row_stride, uint32_t dim, float rowmax, bool seg_subnormal, const void *d_tokens,
                          uint32_t q_stride, uint32_t n_tokens, const uint64_t *d_S, const uint64_t *d_delta, uint64_t n, uint64_t s0, uint64_t total,
                          uint32_t *d_cmap, void *d_pack, float *d_tokmax, uint32_t *d_ridx, const uint32_t *d_qfirst, uint32_t n_queries, float *d_out,
                          int num_cus) {
    if (n == 0 || n_queries == 0) return QMX_OK;
    QMX_REQUIRE(maxsim_f16_dim_ok(dim) && row_stride % 16 == 0 && row_stride >= (uint64_t)dim * 2 && q_stride % 16 == 0 && q_stride >= dim * 2, QMX_ERR_BAD_ARG,
                "maxsim_f16: rows of %u halves", dim);
    ::qmx::clear_stale_error();
    if (total && n_tokens) {
        const uint32_t d32 = dim / 32, groups = (n_tokens + 63) / 64;
        float *d_band = reinterpret_cast<float *>((unsigned char *)d_pack + (size_t)groups * 64 * dim * 2);
        hipLaunchKernelGGL(maxsim_f16_pack_kernel, dim3(groups * 64), dim3(64), 0, st, (const unsigned char *)d_tokens, q_stride, n_tokens, dim, rowmax,
                           seg_subnormal ? 1u : 0u, (uint4 *)d_pack, d_band);
        QMX_HIP(hipGetLastError());
        QMX_TRY(launch_maxsim_map(st, d_S, n, s0, d_cmap));
        MshArgs a;
        a.rows = (const unsigned char *)d_rows; a.row_stride = row_stride; a.S = d_S; a.cmap = d_cmap; a.delta = d_delta; a.bpack = (const uint4 *)d_pack;
        a.band = d_band; a.tokmax = d_tokmax; a.ridx = d_ridx; a.n = n; a.s0 = s0; a.total = total; a.n_tokens = n_tokens;
        switch (d32) {
            case 1: QMX_TRY(launch_msh<1>(st, a, num_cus)); break;
            case 2: QMX_TRY(launch_msh<2>(st, a, num_cus)); break;
            case 3: QMX_TRY(launch_msh<3>(st, a, num_cus)); break;
            case 4: QMX_TRY(launch_msh<4>(st, a, num_cus)); break;
            case 5: QMX_TRY(launch_msh<5>(st, a, num_cus)); break;
            case 6: QMX_TRY(launch_msh<6>(st, a, num_cus)); break;
            case 7: QMX_TRY(launch_msh<7>(st, a, num_cus)); break;
            default: QMX_TRY(launch_msh<8>(st, a, num_cus)); break;
        }
        MshExactArgs x;
        x.rows = (const unsigned char *)d_rows; x.queries = (const unsigned char *)d_tokens; x.row_stride = row_stride; x.S = d_S; x.delta = d_delta;
        x.ridx = d_ridx; x.tokmax = d_tokmax; x.n = n; x.s0 = s0; x.n_tokens = n_tokens; x.q_stride = q_stride; x.dim = dim;
        const uint64_t items = n * ((n_tokens + 1) / 2);
        hipLaunchKernelGGL(maxsim_f16_exact_kernel, dim3((uint32_t)std::min<uint64_t>((items + 3) / 4, (uint64_t)num_cus * 32)), dim3(256), 0, st, x);
        QMX_HIP(hipGetLastError());
    } else {
        QMX_NOTE_KERNEL(maxsim_f16_kernel<4>);      // (no rows or no tokens: the sums alone)
    }
    return launch_maxsim_sum(st, d_tokmax, d_S, n, d_qfirst, n_queries, d_out);
}

}  // namespace qmx
