// scan_split.hip — f32 dot / cosine brute-force top-k for 65..256 queries per pass: a matrix-core PREFILTER with exact verification, over
// the f32 rows or over an f16 copy of them.
//
// Why.  The exact chain-major scan (scan_mfma16.hip) reproduces dot_similarity_avx bit for bit on v_mfma_f32_16x16x4_f32, which runs
// at the vector-ALU rate (155 TFLOP/s measured, profiles/r2_mfma_issue_rates.txt): 64 queries x 10 M x 768 cost 6.3 ms of matrix time at
// peak against a 4.5 ms HBM stream, and every further query costs another 0.1 ms.  The f16 matrix instruction is 16x faster.  An f32 value
// splits EXACTLY into two f16 values plus a residual below 2^-22 of it (x 2^e = h + l + r, h = f16(x 2^e), l = f16(x 2^e - h)), so
//     sum x_i y_i  =  2^-(ex + ey) [ sum h h' + sum h l' + sum l h' ]  +  O(2^-21) sum |x_i y_i|
// three v_mfma_f32_16x16x32_f16 per 16 x 16 x 32 block, f32 accumulation.  That approximate score is NOT returned to anybody: it only
// decides which rows are worth an exact look.
//   1. prescan   (api_search.hip)    exact scores of a strided sample of the block -> T_q = exact k-th best of the sample <= final k-th best
//   2. a scan of this file           approximate score A(r, q) of EVERY row; rows with A >= T_q - b_q become candidates (~1000 k per query)
//   3. select    (split_select.hip)  A_k = k-th best approximate score among the candidates; keep those with A >= A_k - 2 b_q  (~k rows)
//   4. verify    (api_search.hip)    exact scores of the kept rows with the gather kernel of qmx_rescore (the reference's bits), sort, top k
// With |A - E| <= b_q for the exact score E (b_q = 1e-4 |q| max|row|, two orders above the split error and above the worst-case f32
// accumulation bound of both sides for dim <= 1600) every member of the exact top k survives 2. and 3., so the result is the exact
// scan's result, bit for bit — ids, scores, ties — and the parity tests run against this path unchanged.  Anything unexpected (a
// candidate buffer or a verification list that overflows: masses of equal scores, a sample that is all deleted) raises a device-side
// flag and the exact scan runs after all in the same stream (its kernels start, read the flag and return when it is clear).
//
// Here, in the file's order: the queries' statistics, split f16 images and thresholds (once per batch); scan_f32_split_kernel over the f32 rows
// themselves (768 threads: 8 consumer waves on the matrix cores + 4 producer waves that stream the rows from HBM and split them on the fly;
// candidates straight into the per-query lists); scan_f16pair_kernel<HALF> over a pre-split copy (the staged scan of split_common.hpp with
// the f16 instruction; candidates into per-wave lists); scan_f16half256_kernel, the half copy against 256 queries, with a ring and a schedule
// of its own; the copy and the row statistics (once per segment); the launchers.  The int8 copy is scan_i8copy.hip; what turns the lists of
// either into rows to verify is split_select.hip.  All scans are GEMMs with the stored block as the streamed operand, C[rows x queries] over
// K = dim, on the operand layout of split_common.hpp (16-byte units of 8 consecutive k of one row, swizzled against LDS bank conflicts).
// Roofline of the f32-rows kernel: HBM (3072 B per row at d = 768, once); matrix time 3 x 2 x 128 x 768 flop per row = 2.4 ms per 10 M rows at the f16 peak.
#include "split_common.hpp"

namespace qmx {

constexpr int SP_THREADS = 768;          // 8 consumer waves (matrix cores) + 4 producer waves (HBM stream, f32 -> f16 pairs): 2 + 1 per SIMD
constexpr int SP_CONSUMERS = 8;
constexpr int SP_BRING = 4;           // LDS buffers of the queries' chunks: an LDS-DMA copy lands ~1.1 us after its issue (MI355X guide, ldsdma-fill),
                                      // longer than a stage lasts, so chunk g + 3 is requested while chunk g is multiplied
constexpr int SP_LDS = (2 * SP_A_UNITS + SP_BRING * SP_B_UNITS) * 16;

// x * scale = h + l (+ a residual below 2^-22 |x * scale|); round to nearest even both times
// (scale is a power of two, so x * scale is exact and fma(x, scale, -h) == x * scale - h: two v_fma_mix instructions per value)
__device__ __forceinline__ void sp_split4(const f32x4s v, float scale, half4 &h, half4 &l) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h[i] = (_Float16)__builtin_fmaf(v[i], scale, 0.0f);
        l[i] = (_Float16)__builtin_fmaf(v[i], scale, -(float)h[i]);
    }
}

// ---- once per query batch: preprocessed f32 queries -> split f16 in the B-operand layout, per-query norms, the scale of the batch ----
// stats[0] = max |q| over the batch (uint bits of a non-negative float order like the float)
__global__ void sp_query_stats_kernel(const float *q, uint32_t nq, uint32_t dim, float *qmax, float *qnorm) {
    const uint32_t qi = blockIdx.x;
    float mx = 0.0f, ss = 0.0f;
    for (uint32_t i = threadIdx.x; i < dim; i += blockDim.x) {
        const float v = q[(uint64_t)qi * dim + i];
        mx = __builtin_fmaxf(mx, __builtin_fabsf(v));
        ss = __builtin_fmaf(v, v, ss);
    }
    __shared__ float smx[256], sss[256];
    smx[threadIdx.x] = mx;
    sss[threadIdx.x] = ss;
    __syncthreads();
    for (uint32_t o = blockDim.x / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            smx[threadIdx.x] = __builtin_fmaxf(smx[threadIdx.x], smx[threadIdx.x + o]);
            sss[threadIdx.x] += sss[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        qmax[qi] = smx[0];
        qnorm[qi] = __builtin_sqrtf(sss[0]);
    }
}
// power of two that brings a magnitude bound to [8192, 16384): headroom below the f16 maximum, the low part stays a normal number
__device__ __forceinline__ float sp_pow2_scale(float maxabs) {
    if (!(maxabs > 0.0f) || !(maxabs < 3.0e38f)) return 1.0f;
    int e;
    (void)__builtin_frexpf(maxabs, &e);          // maxabs = m * 2^e, m in [0.5, 1)
    int s = 14 - e;
    s = s > 100 ? 100 : (s < -100 ? -100 : s);
    return __builtin_ldexpf(1.0f, s);
}
// scales[0] = query scale, scales[1] = row scale * query scale (accumulator units per score unit), scales[2] = its inverse
// the batch's query scale from the per-query maxima (at most 256 of them), by every thread of a block of a multiple of 64 threads (<= 256); `sh`: 4 floats of LDS
__device__ __forceinline__ float sp_batch_scale(const float *qmax, uint32_t nq, float *sh) {
    float mx = 0.0f;
    for (uint32_t i = threadIdx.x; i < nq; i += blockDim.x) mx = __builtin_fmaxf(mx, qmax[i]);
    for (int o = 32; o >= 1; o >>= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = sh[0];
    for (uint32_t w = 1; w < blockDim.x / 64; ++w) mx = __builtin_fmaxf(mx, sh[w]);
    return sp_pow2_scale(mx);
}
// one thread per 16-byte unit: bq[kc][nt][hl][kq][n ^ 2 kq] = 8 halfs, k = 32 kc + 8 kq + e, query 16 nt + n (zero beyond nq)
// half != 0 (the one-product mode): a chunk is 64 floats, the two unit planes hold the high parts of its two 32-float halves
__global__ __launch_bounds__(256) void sp_pack_queries_kernel(const float *q, uint32_t nq, uint32_t dim, const float *qmax, uint4 *bq, int half, uint32_t qt) {
    __shared__ float sh_mx[4];
    const float scale = sp_batch_scale(qmax, nq, sh_mx);
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (dim / 32) * qt * 4) return;
    const uint32_t b_units = qt * 8;                                    // 16-byte units of one chunk of the tile (128 queries: SP_B_UNITS)
    const uint32_t k32 = gid / (qt * 4), r = gid % (qt * 4);            // 32-float group of the row
    const uint32_t nt = r / 64, kq = (r / 16) % 4, n = r % 16;
    const uint32_t qi = nt * 16 + n;
    half8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = qi < nq ? q[(uint64_t)qi * dim + k32 * 32 + kq * 8 + e] * scale : 0.0f;
        h[e] = (_Float16)x;
        l[e] = (_Float16)(x - (float)h[e]);
    }
    if (half) {
        bq[(uint64_t)(k32 / 2) * b_units + sp_unit(nt, k32 & 1u, kq, n)] = *reinterpret_cast<const uint4 *>(&h);
        return;
    }
    uint4 *chunk = bq + (uint64_t)k32 * b_units;
    chunk[sp_unit(nt, 0, kq, n)] = *reinterpret_cast<const uint4 *>(&h);
    chunk[sp_unit(nt, 1, kq, n)] = *reinterpret_cast<const uint4 *>(&l);
}
// thr[q] in accumulator units: (exact k-th best of the sample - band) * scale.  band[q] = rel_band * row_norm_max * |q| + abs_band * (row_norm_max /
// query scale + |q| / row scale) (score units; split_rel_band and split_abs_band in api_search.hip say what each term covers); a band that reaches
// row_norm_max * |q| - the whole range of the query's scores - rejects nothing, and is infinite.
// Also: the batch's scales (scales[0] = query scale, [1] = row scale x query scale = accumulator units per score unit, [2] = its inverse) and the
// zeroed candidate counters of the pass.
__global__ __launch_bounds__(256) void sp_thresholds_kernel(const uint64_t *gthr, const float *qnorm, const float *qmax, uint32_t nq, float rel_band,
                                                            float abs_band, float row_norm_max, float row_scale, float *scales, float *thr, float *band, uint32_t *cand_cnt,
                                                            uint32_t n_cnt) {
    __shared__ float sh_mx[4];
    const float qs = sp_batch_scale(qmax, nq, sh_mx);
    const uint32_t q = threadIdx.x;                   // blockDim.x = queries of the tile (128 | 256)
    if (q == 0) {
        scales[0] = qs;
        scales[1] = row_scale * qs;
        scales[2] = 1.0f / (row_scale * qs);
    }
    for (uint32_t i = q; i < n_cnt; i += blockDim.x) cand_cnt[i] = 0;
    if (q >= nq) { thr[q] = __builtin_inff(); band[q] = 0.0f; return; }
    const float range = row_norm_max * qnorm[q];
    const float b = rel_band * range + abs_band * (row_norm_max / qs + qnorm[q] / row_scale);
    const uint64_t k = gthr[q];
    // no bound (the sample holds fewer than k live rows), or no band that selects (a query too small beside the batch's largest, a zero query, a
    // norm that is not finite): no candidates for this query, and its infinite band sends it - alone - to the exact scan
    const bool ok = k != 0 && b < range;
    band[q] = ok ? b : __builtin_inff();
    thr[q] = ok ? (key_score(k) - b) * (row_scale * qs) : __builtin_inff();
}

__global__ __launch_bounds__(SP_THREADS, 1) void scan_f32_split_kernel(const ScanArgs a, const SplitArgs s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned char *rows = reinterpret_cast<const unsigned char *>(a.rows);
    const uint64_t n_tiles = (a.n_cand + SP_BM - 1) / SP_BM;
    const uint32_t nch = s.nchunks;                       // a multiple of 4 (the host takes this path for dim % 128 == 0)
    const uint64_t my_tiles = blockIdx.x < n_tiles ? (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    const uint64_t G = my_tiles * nch;                    // stages of this block = its (tile, K-chunk) pairs, in order
    if (G == 0) return;

    if (w >= SP_CONSUMERS) {
        // ================= producers (4 waves): HBM -> registers -> split -> LDS, one K-chunk per stage, three chunks of rows in flight ==========
        // rows 64 pw + 8 rr + (lane >> 3), rr = 0..7, 16-byte piece p = lane & 7 of the chunk's 128 bytes: a wave instruction reads 8 rows x one
        // full 128-byte line, every byte once
        const uint32_t pw = (uint32_t)w - SP_CONSUMERS;
        const uint32_t p = (uint32_t)lane & 7u, lrow0 = pw * 64u + ((uint32_t)lane >> 3);
        const float rscale = s.row_scale;
        // byte offset of this thread's 8-byte stores inside an A buffer: row rl = lrow0 + 8 rr -> tile rl >> 4 = 4 pw + (rr >> 1), row-in-tile
        // (lane >> 3) + 8 (rr & 1); h half (l is + 64 units)
        const uint32_t kq_w = p >> 1;
        uint32_t a_wr[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) a_wr[e] = sp_unit(pw * 4u, 0, kq_w, ((uint32_t)lane >> 3) + 8u * (uint32_t)e) * 16u + (p & 1u) * 8u;
        f32x4s areg[3][8];                                // [slot = chunk % 3][rr]
        // the tile's first row through SGPRs + one 32-bit lane offset per row group: no 64-bit vector address arithmetic per load
        typedef const __attribute__((address_space(1))) unsigned char *sp_gptr;   // (an explicit global pointer: rebuilt from SGPR halves, it would be "flat")
        sp_gptr tile_base = (sp_gptr)(uintptr_t)rows;     // wave-uniform: row 0 of the tile being requested
        uint32_t voff[8];                                 // lane part: (row-in-tile) * stride + 16 p, clamped to the rows that exist
        uint64_t ld_g = 0, ld_it = 0;                     // next chunk to request: global index, its tile iteration
        uint32_t ld_kc = 0;
        auto set_tile = [&](uint64_t it) {
            const uint64_t tile = blockIdx.x + it * gridDim.x;
            const uint64_t first = tile * SP_BM;
            const uint64_t left = a.n_cand - first;       // rows of the tile that exist (> 0: the tile is one of this block's)
            const uint64_t tb = (uint64_t)(uintptr_t)(rows + first * a.row_stride);
            tile_base = (sp_gptr)(uintptr_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(tb >> 32)) << 32) |
                                             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tb));
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {              // rows past the end of the block re-read its last row: results masked
                const uint64_t rl = lrow0 + 8u * (uint32_t)rr;
                voff[rr] = (uint32_t)((rl < left ? rl : left - 1) * a.row_stride) + p * 16u;
            }
        };
        auto issue = [&](int slot) {                      // request the next chunk into register slot `slot`
            if (ld_g >= G) return;
            sp_gptr cb = tile_base + ld_kc * 128u;
#pragma unroll
            for (int rr = 0; rr < 8; ++rr)
                areg[slot][rr] = __builtin_nontemporal_load(reinterpret_cast<const __attribute__((address_space(1))) f32x4s *>(cb + voff[rr]));
            ++ld_g;
            if (++ld_kc == nch) {
                ld_kc = 0;
                ++ld_it;
                if (ld_g < G) set_tile(ld_it);
            }
        };
        auto convert = [&](int slot, uint32_t buf) {      // slot -> A buffer `buf`
            unsigned char *ab = reinterpret_cast<unsigned char *>(lds + buf * SP_A_UNITS);
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                half4 h, l;
                sp_split4(areg[slot][rr], rscale, h, l);
                const uint32_t off = a_wr[rr & 1] + (uint32_t)(rr >> 1) * (128u * 16u);   // + one 16-row tile (128 units) per two rr
                *reinterpret_cast<half4 *>(ab + off) = h;
                *reinterpret_cast<half4 *>(ab + off + 64 * 16) = l;
            }
        };
        set_tile(0);
#pragma unroll
        for (int sl = 0; sl < 3; ++sl) issue(sl);
        convert(0, 0);
        issue(0);
        sp_stage_barrier();                                  // stage 0 may start
        for (uint64_t g = 0; g < G; g += 6) {             // (unrolled by 6: the register slot is g % 3, the LDS buffer g % 2)
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                if (g + u >= G) break;
                // stage g + u: the consumers multiply buffer (g + u) & 1 while chunk g + u + 1 is prepared in the other one
                if (g + u + 1 < G) {
                    convert((u + 1) % 3, (uint32_t)(u + 1) & 1u);
                    issue((u + 1) % 3);
                }
                sp_stage_barrier();
            }
        }
        return;
    }

    // ================= consumers (8 waves = 4 row quarters x 2 query halves): LDS -> matrix cores, candidates of every finished tile ==========
    const uint32_t wm = (uint32_t)w & 3u, wn = (uint32_t)w >> 2;
    const uint32_t kq_r = (uint32_t)lane >> 4, m_r = (uint32_t)lane & 15u;
    const uint32_t a_rd = sp_unit(wm * 4, 0, kq_r, m_r), b_rd = sp_unit(wn * 4, 0, kq_r, m_r);   // + 128 units per tile, + 64 for the l half
    float thr[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) thr[nt] = s.thr[wn * 64 + nt * 16 + m_r];
    const float inv_scale = s.scales[2];
    const uint32_t lds0 = (uint32_t)(uintptr_t)(sp_lds_byte *)smem_raw;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    // the queries' chunk kc -> LDS buffer `bbuf` directly (this wave's 2 KiB of its 16 KiB): the only vector-memory traffic of a consumer
    auto load_b = [&](uint32_t kc, uint32_t bbuf) {
        const unsigned char *bsrc = reinterpret_cast<const unsigned char *>(s.bq + (uint64_t)kc * SP_B_UNITS) + (uint32_t)w * 2048u;
        const uint32_t dst = lds0 + (2u * SP_A_UNITS + bbuf * SP_B_UNITS) * 16u + (uint32_t)w * 2048u;
        // (wave-uniform base through SGPRs; readfirstlane returns a signed int: widen the halves as unsigned)
        const uint64_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)bsrc);
        const uint64_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uintptr_t)bsrc >> 32));
        const unsigned char *ub = reinterpret_cast<const unsigned char *>((hi << 32) | lo);
        sp_glds16(ub, lane_off, dst);
        sp_glds16(ub + 1024u, lane_off, dst + 1024u);
    };
    // chunks 0, 1, 2 are on their way before stage 0; every stage requests one more (indices wrap: the queries are the same for every tile;
    // the requests past the last stage land in buffers nobody reads) so that the count of outstanding copies is the same at every wait
    uint32_t b_kc = 0;                                    // K-chunk of the next request
    uint32_t b_slot = 0;                                  // ... and its ring slot
    auto request_b = [&]() {
        load_b(b_kc, b_slot);
        b_kc = b_kc + 1 == nch ? 0 : b_kc + 1;
        b_slot = (b_slot + 1) & (SP_BRING - 1);
    };
    request_b();
    request_b();
    request_b();
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");      // chunk 0 has landed (2 copies per chunk and wave; chunks 1 and 2 may still travel)
    sp_stage_barrier();
    uint32_t buf = 0, bbuf = 0;
    for (uint64_t it = 0; it < my_tiles; ++it) {
        const uint64_t tile = blockIdx.x + it * gridDim.x;
        f32x4s acc[4][4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = (f32x4s){0.f, 0.f, 0.f, 0.f};
        for (uint32_t kc = 0; kc < nch; ++kc) {
            request_b();                                  // chunk g + 3 -> the slot chunk g - 1 was read from (everybody is past that stage's barrier)
            const uint4 *ab = lds + buf * SP_A_UNITS + a_rd;
            const uint4 *bb = lds + 2 * SP_A_UNITS + bbuf * SP_B_UNITS + b_rd;
            half8 bh[4], bl[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                bh[nt] = *reinterpret_cast<const half8 *>(bb + nt * 128);
                bl[nt] = *reinterpret_cast<const half8 *>(bb + nt * 128 + 64);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const half8 ah = *reinterpret_cast<const half8 *>(ab + mt * 128);
                const half8 al = *reinterpret_cast<const half8 *>(ab + mt * 128 + 64);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[nt], acc[mt][nt], 0, 0, 0);
            }
            buf ^= 1;
            bbuf = (bbuf + 1) & (SP_BRING - 1);
            if (kc + 1 == nch) {
                // ---- candidates of the tile: accumulator register j of (mt, nt) = row 64 wm + 16 mt + 4 (lane >> 4) + j, query 64 wn + 16 nt + (lane & 15)
                const uint32_t row0 = (uint32_t)(tile * SP_BM) + wm * 64 + 4 * kq_r;      // (row ids are u32: PointOffsetType)
                const uint32_t n_rows32 = (uint32_t)a.n_cand;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float v = acc[mt][nt][j];
                            const uint32_t row = row0 + (uint32_t)mt * 16 + (uint32_t)j;
                            const bool c = !(v < thr[nt]) && row < n_rows32;           // NaN (greatest in OrderedFloat) is a candidate; thr = +inf past nq
                            if (__ballot(c)) {
                                uint32_t q = wn * 64 + (uint32_t)nt * 16 + m_r;
                                asm volatile("" : "+v"(q));                            // (keeps the buffer addresses out of the registers of the main loop)
                                if (c && q < s.nq && a.del.live(row, q)) {
                                    const uint32_t slot = atomicAdd(&s.cand_cnt[q], 1u);
                                    if (slot < s.cap) s.cand[(uint64_t)q * s.cap + slot] = make_key(v * inv_scale, row);
                                }
                            }
                        }
                    }
            }
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");     // the queries' NEXT chunk has landed (the two behind it may still travel)
            sp_stage_barrier();
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // nothing may land in LDS after the block is gone
}

// =====================================================================================================================================
// The same scan over a PRE-SPLIT copy of the block (QMX_SEG_SPLIT_COPY): the f16 pairs are made once, when the segment is created, and laid
// out in HBM as the LDS images the multiplication wants — [256-row tile][K-chunk][2048 16-byte units] — so a stage's 32 KiB of rows are ONE
// contiguous run that the waves copy straight into LDS (LDS-DMA, 1 KiB per wave instruction, no registers, no vector-ALU work at all).
// The vector ALU shares its issue port with the matrix instructions (measured on the converting kernel above: 33 % VALU + 36 % MFMA busy,
// not overlapped), so taking the conversion out of the scan is what lets the pass run at the HBM stream.  Costs a second copy of the
// block in HBM (4 bytes per element, like the f32 original, which stays: the verification gathers from it).
// block = 512 threads = 8 waves (4 row quarters x 2 query halves), every wave multiplies and copies; three-deep rings for rows and queries
// (a copy lands ~1.1 us after its issue, a stage lasts ~0.7 us): stage g requests stage g + 2 and multiplies stage g.
// =====================================================================================================================================
constexpr int SP3_BRING = 4;                                 // query stages: one being multiplied, three requested
constexpr int SP3_LDS = (SP3_ARING * SP3_A_UNITS + SP3_BRING * SP_B_UNITS) * 16;      // 96 + 64 = 160 KiB: the whole LDS of the CU

// what sp_staged_scan (split_common.hpp) takes for the f16 copies: the f16 instruction, one scale for the whole batch, the flat f32 epilogue
template <bool HALF /* one product per element (high parts only, 64-float chunks) instead of three */>
struct F16PairOps {
    using operand = half8;
    using accum = f32x4s;
    static constexpr bool CROSS = !HALF;
    static constexpr int BRING = SP3_BRING;
    static __device__ __forceinline__ accum mfma(operand x, operand y, accum c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(x, y, c, 0, 0, 0); }
    struct Bounds {
        float thr[4], inv_scale;
        __device__ __forceinline__ void load(const SplitArgs &s, uint32_t wn, uint32_t m_r) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) thr[nt] = s.thr[wn * 64 + nt * 16 + m_r];
            inv_scale = s.scales[2];
        }
    };
    static __device__ __forceinline__ void epilogue(const accum (&acc)[4][4], const Bounds &b, uint64_t tile, uint32_t wm, uint32_t wn, uint32_t kq_r, uint32_t m_r,
                                                    const ScanArgs &a, const SplitArgs &s, SpWaveList &list) {
        sp_f32_epilogue<SP3_BM>(acc, b.thr, b.inv_scale, tile, wm, wn, kq_r, m_r, a, s, list);
    }
};
template <bool HALF>
__global__ __launch_bounds__(SP3_THREADS, 1) void scan_f16pair_kernel(const ScanArgs a, const SplitArgs s) {
    sp_staged_scan<F16PairOps<HALF>>(a, s);
}

// =====================================================================================================================================
// 256 queries per pass over the HALF copy.  The pass above is HBM-bound (6.05 TB/s of the ~6.3 the part delivers): the only way to more
// queries per second is fewer bytes per query, i.e. more queries per pass.  Here a stage is 128 rows (16 KiB from HBM: half of a 256-row
// tile of the copy, whose image is tile-of-16 major) against 256 queries (32 KiB from L2): the same 64 x 64 block of accumulators and the same
// 32 matrix instructions per wave and stage as above for half the HBM bytes.  8 waves = 2 (row halves) x 4 (query quarters); rings of three
// stages each (rows 48 KiB + queries 96 KiB = 144 KiB of LDS); per stage a wave requests [4 KiB of the queries, 2 KiB of the rows] of
// stage g + 2: six copies as above, so the same `s_waitcnt vmcnt(6)` means "stage g + 1 has landed".
// =====================================================================================================================================
#ifndef SP4_DBG
#define SP4_DBG 0          // QMX_TUNING builds: 1 = no copies at all (matrix loop alone), 3 = no query copies (wrong results)
#endif
constexpr int SP4_A_UNITS = SP4_BM * 2 * 4;                  // 1024 units = 16 KiB
constexpr int SP4_B_UNITS = SP4_QT * 2 * 4;                  // 2048 units = 32 KiB
constexpr int SP4_RING = 3;
constexpr int SP4_LDS = SP4_RING * (SP4_A_UNITS + SP4_B_UNITS) * 16;      // 144 KiB

__global__ __launch_bounds__(SP3_THREADS, 1) void scan_f16half256_kernel(const ScanArgs a, const SplitArgs s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t n_tiles = split_phase_tiles((a.n_cand + SP4_BM - 1) / SP4_BM, s.phase);
    const uint32_t nch = s.nchunks;
    const uint64_t my_tiles = split_block_tiles(n_tiles, blockIdx.x, gridDim.x);
    const SplitTileWalk walk(s.phase);
    if (my_tiles == 0) {
        SpWaveList::none(s.wcnt, blockIdx.x * (SP3_THREADS / 64) + (uint32_t)w, lane);
        return;
    }
    const uint32_t wm = (uint32_t)w & 1u, wn = (uint32_t)w >> 1;
    const uint32_t kq_r = (uint32_t)lane >> 4, m_r = (uint32_t)lane & 15u;
    const uint32_t a_rd = sp_unit(wm * 4, 0, kq_r, m_r), b_rd = sp_unit(wn * 4, 0, kq_r, m_r);
    float thr[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) thr[nt] = s.thr[wn * 64 + nt * 16 + m_r];
    const float inv_scale = s.scales[2];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // from here on the kernel counts its vector-memory traffic itself
    const uint32_t lds0 = (uint32_t)(uintptr_t)(sp_lds_byte *)smem_raw;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    uint4 *b_lds = lds + SP4_RING * SP4_A_UNITS;
    // The two copy streams advance by plain pointer increments (a stage of the rows is 32 KiB further in the copy, the tile's image being
    // contiguous over the K-chunks; the queries wrap after nch stages); the tile's address is computed once per tile.  The scalar unit
    // shares the issue port with the matrix instructions: ~90 scalar instructions per stage cost as much as the 32 MFMAs themselves.
    uint64_t ra_it = 0;
    uint32_t ra_kc = 0, ra_slot = 0, rb_kc = 0, rb_slot = 0;
    auto tile_ptr = [&](uint64_t j) {      // first stage of the j-th tile of this block: half (tile & 1) of the copy's 256-row tile tile / 2
        const uint64_t tile = walk.tile(blockIdx.x + j * gridDim.x);
        return sp_uniform_ptr((uint64_t)(uintptr_t)(s.rows_split + (tile >> 1) * nch * SP3_A_UNITS + (tile & 1) * SP4_A_UNITS) + (uint32_t)w * 2048u);
    };
    const unsigned char *ra_cur = tile_ptr(0);
    const unsigned char *const rb_first = sp_uniform_ptr((uint64_t)(uintptr_t)s.bq + (uint32_t)w * 4096u);
    const unsigned char *rb_cur = rb_first;
    const unsigned char *ra_src = nullptr, *rb_src = nullptr;
    uint32_t ra_dst = 0, rb_dst = 0;
    const uint32_t ra_dst0 = lds0 + (uint32_t)w * 2048u, rb_dst0 = lds0 + SP4_RING * SP4_A_UNITS * 16u + (uint32_t)w * 4096u;
    auto rows_begin = [&]() {
        ra_src = ra_cur;
        ra_dst = ra_dst0 + ra_slot * (SP4_A_UNITS * 16u);
        ra_slot = ra_slot + 1 == SP4_RING ? 0 : ra_slot + 1;
        if (ra_kc + 1 < nch) { ++ra_kc; ra_cur += SP3_A_UNITS * 16; }
        else if (ra_it + 1 < my_tiles) { ra_kc = 0; ++ra_it; ra_cur = tile_ptr(ra_it); }
    };
    auto rows_piece = [&](int i) {
#if SP4_DBG != 1
        sp_glds16_m0_nt(ra_src + i * 1024, lane_off, ra_dst + i * 1024);
#endif
    };
    auto queries_begin = [&]() {
        rb_src = rb_cur;
        rb_dst = rb_dst0 + rb_slot * (SP4_B_UNITS * 16u);
        rb_slot = rb_slot + 1 == SP4_RING ? 0 : rb_slot + 1;
        if (rb_kc + 1 == nch) { rb_kc = 0; rb_cur = rb_first; }
        else { ++rb_kc; rb_cur += SP4_B_UNITS * 16; }
    };
    auto queries_piece = [&](int i) {
#if SP4_DBG != 1 && SP4_DBG != 3
        sp_glds16_m0(rb_src + i * 1024, lane_off, rb_dst + i * 1024);
#endif
    };
    auto request_stage = [&]() {
        queries_begin();
#pragma unroll
        for (int i = 0; i < 4; ++i) queries_piece(i);
        rows_begin();
        rows_piece(0);
        rows_piece(1);
    };
    request_stage();                                      // stage 0
    request_stage();                                      // stage 1
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");      // stage 0 has landed
    sp_stage_barrier();
    uint32_t slot = 0;
    f32x4s acc[4][4];
    SpWaveList list(s.wlist, s.wcap, blockIdx.x * (SP3_THREADS / 64) + (uint32_t)w);
    auto epilogue = [&](uint64_t tile) { sp_f32_epilogue<SP4_BM>(acc, thr, inv_scale, tile, wm, wn, kq_r, m_r, a, s, list); };
    // Operands are read ONE STAGE AHEAD: a stage's barrier sits after its third row tile (when the copies of stage g + 1 are known to have landed:
    // everything but the five requests this stage has issued by then), and the fourth tile is multiplied while the operands of stage g + 1
    // are already being read - the burst of 8 waves x 12 ds_read_b128 after a barrier no longer stands in front of idle matrix pipes.
    // Slot (g + 2) % 3 is free for the requests of stage g: its last readers finished before the barrier of stage g - 1.
    half8 bh[2][4], bl[2][4], ah[2], al[2];
    auto read_b = [&](auto Pc, uint32_t from_slot) {
        constexpr int P = decltype(Pc)::value;
        const uint4 *bb = b_lds + from_slot * SP4_B_UNITS + b_rd;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) bl[P][nt] = *reinterpret_cast<const half8 *>(bb + nt * 128 + 64);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) bh[P][nt] = *reinterpret_cast<const half8 *>(bb + nt * 128);
    };
    auto read_a = [&](int set, uint32_t from_slot, int mt) {
        const uint4 *ab = lds + from_slot * SP4_A_UNITS + a_rd + mt * 128;
        al[set] = *reinterpret_cast<const half8 *>(ab + 64);
        ah[set] = *reinterpret_cast<const half8 *>(ab);
    };
    read_a(0, 0, 0);
    read_b(std::integral_constant<int, 0>{}, 0);
    auto stage = [&](auto Pc) {
        constexpr int P = decltype(Pc)::value;
        queries_begin();                                  // stage g + 2 -> the slots stage g - 1 was read from
        rows_begin();
        const uint32_t next_slot = slot + 1 == SP4_RING ? 0 : slot + 1;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int cur = mt & 1, nxt = cur ^ 1;
            if (mt < 3) read_a(nxt, slot, mt + 1);
            else {
                read_a(nxt, next_slot, 0);                // (mt = 3 uses set 1: set 0 is free for the next stage's first tile)
                read_b(std::integral_constant<int, P ^ 1>{}, next_slot);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[cur], bl[P][nt], acc[mt][nt], 0, 0, 0);
            if (mt == 0) { queries_piece(0); queries_piece(1); }
            if (mt == 1) { queries_piece(2); queries_piece(3); }
            if (mt == 2) rows_piece(0);
            if (mt == 3) rows_piece(1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[cur], bh[P][nt], acc[mt][nt], 0, 0, 0);
            if (mt == 2) {
                asm volatile("s_waitcnt vmcnt(5)" ::: "memory");     // stage g + 1 has landed (this stage has requested five copies so far)
                sp_stage_barrier();
            }
        }
        slot = next_slot;
    };
    for (uint64_t it = 0; it < my_tiles; ++it) {
        if (it) epilogue(walk.tile(blockIdx.x + (it - 1) * gridDim.x));
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = (f32x4s){0.f, 0.f, 0.f, 0.f};
        for (uint32_t kc = 0; kc < nch; kc += 2) {        // (dim is a multiple of 128: an even number of 64-float stages)
            stage(std::integral_constant<int, 0>{});
            stage(std::integral_constant<int, 1>{});
        }
    }
    epilogue(walk.tile(blockIdx.x + (my_tiles - 1) * gridDim.x));
    list.finish(s.wcnt, blockIdx.x * (SP3_THREADS / 64) + (uint32_t)w, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // nothing may land in LDS after the block is gone
}

// the pre-split copy: one thread per 16-byte unit of the OUTPUT, out[(tile * nch + kc) * 2048 + unit(row, h / l, kq)], in the output's order (whole
// lines written, as sp_i8_copy_kernel); rows past n are zero
__global__ __launch_bounds__(256) void sp_split_copy_kernel(const unsigned char *rows, uint64_t row_stride, uint64_t n, uint32_t dim, float scale, uint4 *out,
                                                            int half) {
    const uint32_t nch = half ? dim / 64 : dim / 32;
    const uint64_t n_tiles = (n + SP3_BM - 1) / SP3_BM;
    const uint64_t total = n_tiles * nch * SP3_A_UNITS;
    for (uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (uint64_t)gridDim.x * 256) {
        const uint32_t u = (uint32_t)(gid % SP3_A_UNITS);
        const uint64_t blk = gid / SP3_A_UNITS, tile = blk / nch;
        const uint32_t kc = (uint32_t)(blk % nch);
        // sp_unit(t, hl, kq, m) = ((t * 2 + hl) * 4 + kq) * 16 + (m ^ 2 kq), inverted
        const uint32_t kq = (u >> 4) & 3u, hl = (u >> 6) & 1u, t = u >> 7, m = (u & 15u) ^ (2u * kq);
        const uint64_t r = tile * SP3_BM + t * 16u + m;
        // half: a plane pair per 64 floats = the high parts of its two 32-float halves; else the high (hl = 0) and low (hl = 1) parts of 32 floats
        const uint32_t k32 = half ? kc * 2u + hl : kc;
        half8 h, l;
        if (r < n) {
            const float *v = reinterpret_cast<const float *>(rows + r * row_stride) + k32 * 32 + kq * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                h[e] = (_Float16)__builtin_fmaf(v[e], scale, 0.0f);
                l[e] = (_Float16)__builtin_fmaf(v[e], scale, -(float)h[e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) { h[e] = (_Float16)0.0f; l[e] = (_Float16)0.0f; }
        }
        out[gid] = (half || hl == 0) ? *reinterpret_cast<const uint4 *>(&h) : *reinterpret_cast<const uint4 *>(&l);
    }
}

// ---- row statistics of an f32 block (once per segment): stats[0] = max |x|, stats[1] = max row sum of squares (uint bits) ----
// (the squares are those of x * scale, a power of two: a block far from unit scale neither underflows nor overflows them; stats[1] is in units of scale^2)
__global__ __launch_bounds__(256) void sp_row_stats_kernel(const unsigned char *rows, uint64_t row_stride, uint64_t n, uint32_t dim, float scale, uint32_t *stats) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    float mx = 0.0f, mss = 0.0f;
    for (uint64_t r = wave; r < n; r += nwaves) {
        const float *v = reinterpret_cast<const float *>(rows + r * row_stride);
        float ss = 0.0f;
        for (uint32_t i = lane; i < dim; i += 64) {
            const float x = v[i];
            mx = __builtin_fmaxf(mx, __builtin_fabsf(x));
            ss = __builtin_fmaf(x * scale, x * scale, ss);
        }
        for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
        mss = __builtin_fmaxf(mss, ss);
    }
    for (int o = 32; o >= 1; o >>= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) {
        atomicMax(&stats[0], __float_as_uint(mx));
        atomicMax(&stats[1], __float_as_uint(mss));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
bool split_scan_ok(const ScanArgs &a) {
    return a.dim % 128 == 0 && a.dim >= 128 && a.rem_pieces == 0 && a.tail_start == a.dim && a.row_stride % 16 == 0 && a.ids == nullptr && a.top <= 64 &&
           !option(OPT_NO_SPLIT_SCAN);
}
size_t split_wlists_bytes(int num_cus) { return split_wlists_counts_bytes(num_cus) + (size_t)num_cus * (SP3_THREADS / 64) * SP_WCAP * 16; }
size_t split_query_bytes(uint32_t dim) { return (size_t)(dim / 32) * SP4_B_UNITS * 16; }   // (sized for the 256-query tile; the half mode needs half of it)

int32_t launch_split_row_stats(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, float scale, uint32_t *d_stats) {
    if (n == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_row_stats_kernel, dim3(2048), dim3(256), 0, st, (const unsigned char *)rows, row_stride, n, dim, scale, d_stats);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
float split_row_scale(float row_maxabs) {
    if (!(row_maxabs > 0.0f) || !(row_maxabs < 3.0e38f)) return 1.0f;
    int e;
    (void)frexpf(row_maxabs, &e);
    int s = 14 - e;
    s = s > 100 ? 100 : (s < -100 ? -100 : s);
    return ldexpf(1.0f, s);
}

// queries (preprocessed f32, [nq][dim] contiguous) -> bq, qnorm, qmax (per query: the scale of the batch is derived from them where it is needed)
int32_t launch_split_pack_queries(hipStream_t st, const float *d_q, uint32_t nq, uint32_t dim, float *d_qmax, float *d_qnorm, void *d_bq, int half, uint32_t qt) {
    QMX_REQUIRE(nq <= SP_QT_MAX, QMX_ERR_BAD_ARG, "split tile of %u queries", nq);
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_query_stats_kernel, dim3(nq), dim3(256), 0, st, d_q, nq, dim, d_qmax, d_qnorm);
    const uint32_t units = (dim / 32) * qt * 4;
    hipLaunchKernelGGL(sp_pack_queries_kernel, dim3((units + 255) / 256), dim3(256), 0, st, d_q, nq, dim, d_qmax, (uint4 *)d_bq, half, qt);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_split_thresholds(hipStream_t st, const uint64_t *d_gthr, const float *d_qnorm, const float *d_qmax, uint32_t nq, float rel_band, float abs_band,
                                float row_norm_max, float row_scale, float *d_scales, float *d_thr, float *d_band, uint32_t qt, uint32_t *d_cand_cnt, uint32_t n_cnt) {
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_thresholds_kernel, dim3(1), dim3(qt), 0, st, d_gthr, d_qnorm, d_qmax, nq, rel_band, abs_band, row_norm_max, row_scale, d_scales, d_thr,
                       d_band, d_cand_cnt, n_cnt);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
size_t split_copy_bytes(uint64_t n, uint32_t dim, int half) { return (size_t)((n + SP3_BM - 1) / SP3_BM) * (dim / (half ? 64 : 32)) * SP3_A_UNITS * 16; }
int32_t launch_split_copy(hipStream_t st, const void *rows, uint64_t row_stride, uint64_t n, uint32_t dim, float row_scale, void *d_out, int half) {
    if (n == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_split_copy_kernel, dim3(8192), dim3(256), 0, st, (const unsigned char *)rows, row_stride, n, dim, row_scale, (uint4 *)d_out, half);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_scan_f32_split(hipStream_t st, const ScanArgs &a, const void *d_bq, float row_scale, const float *d_scales, const float *d_thr,
                              uint64_t *d_cand, uint32_t *d_cand_cnt, uint32_t cap, int num_cus, const void *d_rows_split, int half, void *d_wlists, uint32_t phase,
                              uint32_t qt) {
    auto kfn = scan_f32_split_kernel;
    auto kfn3 = scan_f16pair_kernel<false>;
    auto kfn3h = scan_f16pair_kernel<true>;
    auto kfn4 = scan_f16half256_kernel;
    QMX_REQUIRE(qt == SP_QT || (qt == SP4_QT && half && d_rows_split), QMX_ERR_BAD_ARG, "the 256-query shape scans the half copy");
    static thread_local DeviceOnce attr_once;
    if (attr_once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, SP_LDS));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn3), hipFuncAttributeMaxDynamicSharedMemorySize, SP3_LDS));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn3h), hipFuncAttributeMaxDynamicSharedMemorySize, SP3_LDS));
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn4), hipFuncAttributeMaxDynamicSharedMemorySize, SP4_LDS));
        attr_once.mark();
    }
    QMX_REQUIRE(!half || d_rows_split, QMX_ERR_BAD_ARG, "the one-product mode scans the half copy only");
    SplitArgs s;
    s.rows_split = (const uint4 *)d_rows_split;
    s.bq = (const uint4 *)d_bq;
    s.nchunks = a.dim / (half ? 64 : 32);
    s.nq = a.nq;
    s.row_scale = row_scale;
    s.scales = d_scales;
    s.thr = d_thr;
    s.cand = d_cand;
    s.cand_cnt = d_cand_cnt;
    s.cap = cap;
    s.wcap = SP_WCAP;
    const SplitWlists wl(d_wlists, num_cus);
    s.wcnt = wl.counts;
    s.wlist = wl.lists;
    QMX_REQUIRE(!d_rows_split || d_wlists, QMX_ERR_BAD_ARG, "the scan over a derived copy writes per-wave candidate lists");
    QMX_REQUIRE(phase == 0 || d_rows_split, QMX_ERR_BAD_ARG, "phases exist for the scan over a derived copy");
    s.phase = phase;
    const uint32_t bm = qt == SP4_QT ? SP4_BM : d_rows_split ? SP3_BM : SP_BM;
    const SplitGrid g = split_scan_grid(a.n_cand, bm, phase, num_cus);              // (phase 0 over the f32 rows themselves: every tile)
    if (g.n_tiles == 0) return QMX_OK;
    const uint32_t grid = g.grid;
    ::qmx::clear_stale_error();
    if (qt == SP4_QT) {
        QMX_NOTE_KERNEL(kfn4);
        hipLaunchKernelGGL(kfn4, dim3(grid), dim3(SP3_THREADS), (size_t)SP4_LDS, st, a, s);
    } else if (d_rows_split && half) {
        QMX_NOTE_KERNEL(kfn3h);
        hipLaunchKernelGGL(kfn3h, dim3(grid), dim3(SP3_THREADS), (size_t)SP3_LDS, st, a, s);
    } else if (d_rows_split) {
        QMX_NOTE_KERNEL(kfn3);
        hipLaunchKernelGGL(kfn3, dim3(grid), dim3(SP3_THREADS), (size_t)SP3_LDS, st, a, s);
    } else {
        QMX_NOTE_KERNEL(kfn);
        hipLaunchKernelGGL(kfn, dim3(grid), dim3(SP_THREADS), (size_t)SP_LDS, st, a, s);
    }
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

}  // namespace qmx
