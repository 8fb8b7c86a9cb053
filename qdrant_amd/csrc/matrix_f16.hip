// matrix_f16.hip — the exact top-k scan of qmx_search_matrix over f16 rows of 32 and more elements: the tiled kernel of scan_common.hpp with a lane
// policy that keeps the 32 running sums of the reference's f16 AVX leaf apart (lib/segment/src/spaces/metric_f16/avx/dot.rs:13-69, euclid.rs:13-75,
// manhattan.rs:13-77), so its scores are the reference's bits.  RowF16 (dense_policies.hpp) cannot: in the stored layout the two iterations of a
// 128-byte segment feed the same sums from different lanes.  The block of a matrix call is the library's own (matrix.hip gathers it), so it is laid out
// for this policy - matrix_plan.hpp matrix_f16_avx_source: a lane's piece holds, for four of the sums, the terms of both iterations side by side.
// Batches of 8 and more queries do not go to the matrix cores here (scan_sq_mfma.hip F16Ops sums in their order).
#include "dense_policies.hpp"

namespace qmx {

// lane (h = t >> 2, r = t & 3) of a row's 8 lanes holds AVX register r, SIMD lanes 4 h .. 4 h + 3 = a[0 .. 3] (lane_piece: piece 2 r + h)
template <int METRIC>
struct RowF16Avx {
    static constexpr int NACC = 4;
    static constexpr int NRAUX = 0;
    static constexpr int R16 = 1;      // (16 queries x 2 rows x 4 sums beside the widened halfs do not fit the registers: 240 - 536 bytes of scratch per lane)
    typedef float acc_t;

    static __device__ __forceinline__ void row_aux(acc_t (&)[1], const uint4 &) {}
    // a dword = one sum's terms of iterations 2 s (low half) and 2 s + 1 (high half): RowF16::mac2 takes them in that order
    static __device__ __forceinline__ void mac(acc_t (&a)[NACC], const uint4 &q, const uint4 &v) {
        RowF16<METRIC>::mac2(a[0], q.x, v.x);
        RowF16<METRIC>::mac2(a[1], q.y, v.y);
        RowF16<METRIC>::mac2(a[2], q.z, v.z);
        RowF16<METRIC>::mac2(a[3], q.w, v.w);
    }
    // hsum256_ps_avx of each register (simple_avx.rs:10-16), the four results added left to right (avx/dot.rs:58-61), then the scalar tail (:64-66)
    static __device__ __forceinline__ float finish(acc_t (&a)[NACC], acc_t (&)[1], const unsigned char *q_lds, const unsigned char *row, uint32_t,
                                                   const ScanArgs &args) {
        float lr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // the same register's other half: lane t ^ 4 = row_half_mirror (t -> 7 - t), then the quad reversed (t -> t ^ 3)
            const float other = dpp_f32<0x1B>(dpp_f32<DPP_ROW_HALF_MIRROR>(a[k]));      // quad_perm:[3,2,1,0]
            lr[k] = a[k] + other;                                                         // lr_sum = hi128 + lo128
        }
        const float reg = (lr[0] + lr[1]) + (lr[2] + lr[3]);                              // hadd, then p1 + p2: register (t & 3)
        float result = ((dpp_f32<DPP_QUAD_BCAST0>(reg) + dpp_f32<DPP_QUAD_BCAST1>(reg)) + dpp_f32<DPP_QUAD_BCAST2>(reg)) + dpp_f32<DPP_QUAD_BCAST3>(reg);
        if (args.tail_start < args.dim) {
            const _Float16 *qh = reinterpret_cast<const _Float16 *>(q_lds);
            const _Float16 *vh = reinterpret_cast<const _Float16 *>(row);
            for (uint32_t i = args.tail_start; i < args.dim; ++i) {
                const float x = (float)qh[i], y = (float)vh[i];
                if (METRIC == M_DOT) result += x * y;
                else if (METRIC == M_EUCLID) { const float d = x - y; result += d * d; }
                else result += __builtin_fabsf(x - y);
            }
        }
        return METRIC == M_DOT ? result : -result;
    }
};

template <class P>
static int32_t launch_f16_avx(hipStream_t st, int qt, const ScanArgs &a, int num_cus, uint32_t *grid) {
    switch (qt) {      // (rows per lane and unrolling as launch_policy picks them)
        case 1: return launch_scan_inst<P, 1, 4, 4, false, SCAN_TOPK>(st, a, num_cus, grid);
        case 2: return launch_scan_inst<P, 2, 4, 2, false, SCAN_TOPK>(st, a, num_cus, grid);
        case 4: return launch_scan_inst<P, 4, 2, 4, false, SCAN_TOPK>(st, a, num_cus, grid);
        case 8: return launch_scan_inst<P, 8, 2, 2, false, SCAN_TOPK>(st, a, num_cus, grid);
        case 16: return launch_scan_inst<P, 16, P::R16, 2, false, SCAN_TOPK>(st, a, num_cus, grid);
    }
    set_error("unsupported query tile %d", qt);
    return QMX_ERR_BAD_ARG;
}

int32_t launch_scan_f16_avx(hipStream_t st, int distance, int qt, ScanMode mode, const ScanArgs &a, int num_cus, uint32_t *grid_out) {
    QMX_REQUIRE(mode == SCAN_TOPK && !a.ids, QMX_ERR_NOT_SUPPORTED, "the f16 block of a matrix call is searched whole");
    QMX_REQUIRE(a.dim >= 64 && a.rem_pieces == 0 && a.tail_start == a.nseg * 64 && a.row_stride % 16 == 0, QMX_ERR_BAD_ARG,
                "not a block of whole two-iteration segments: %u elements", a.dim);
    switch (distance) {
        case QMX_DISTANCE_COSINE:      // CosineMetric::similarity == DotProductMetric::similarity on normalised vectors (simple.rs:174-176)
        case QMX_DISTANCE_DOT: return launch_f16_avx<RowF16Avx<M_DOT>>(st, qt, a, num_cus, grid_out);
        case QMX_DISTANCE_EUCLID: return launch_f16_avx<RowF16Avx<M_EUCLID>>(st, qt, a, num_cus, grid_out);
        case QMX_DISTANCE_MANHATTAN: return launch_f16_avx<RowF16Avx<M_MANHATTAN>>(st, qt, a, num_cus, grid_out);
    }
    set_error("bad distance %d", distance);
    return QMX_ERR_BAD_ARG;
}

}  // namespace qmx
