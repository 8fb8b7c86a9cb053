// f16_avx_leaf.hpp — the reference's score of one (f16 row, f16 query) pair, bit for bit, on 32 lanes: what f16w_pairs_kernel (scan_f16w.hip) and
// maxsim_f16_exact_kernel (maxsim_f16.hip) share.
//
// half_avx (metric_f16/avx/{dot,euclid}.rs) keeps 32 running f32 sums: element i feeds sum i % 32 - register (i % 32) / 8, SIMD lane i % 8 - by one fma per
// 32-element iteration (Euclid: d = a - b rounded, then fma(d, d, s)); hsum256_ps_avx of each register is
// ((s[0] + s[4]) + (s[1] + s[5])) + ((s[2] + s[6]) + (s[3] + s[7])), the four results are added left to right.  dim is a multiple of 32 here: no tail.
#pragma once
#include "dense_policies.hpp"

namespace qmx {

__device__ __forceinline__ float fw_h2f(uint32_t bits16) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16); }

template <int METRIC>
__device__ __forceinline__ float fw_term(float acc, float qv, float xv) {
    if constexpr (METRIC == M_EUCLID) {
        const float d = qv - xv;
        return __builtin_fmaf(d, d, acc);
    } else return __builtin_fmaf(qv, xv, acc);
}

// 32 lanes per pair (a wave holds two pairs; all 64 lanes call this together): lane l = lane & 31 owns sum l and takes elements l, l + 32, ... in order -
// x and y point at element l of the row and of the query.  Every lane of the pair's half returns the pair's sum (Euclid: not yet negated).
template <int METRIC>
__device__ __forceinline__ float f16_avx_pair(const unsigned short *x, const unsigned short *y, uint32_t dim, uint32_t lane) {
    float sum = 0.0f;
#pragma unroll 8
    for (uint32_t i = 0; i < dim; i += 32) sum = fw_term<METRIC>(sum, fw_h2f(y[i]), fw_h2f(x[i]));
    // hsum256_ps_avx inside each group of eight lanes (lane j < 4: s[j + 4] + s[j]; lane 0: (lr0 + lr1) + (lr2 + lr3)), then the four registers
    sum = __shfl_xor(sum, 4, 64) + sum;
    sum = sum + __shfl_xor(sum, 1, 64);
    sum = sum + __shfl_xor(sum, 2, 64);
    const uint32_t g0 = lane & 32u;
    return ((__shfl(sum, g0, 64) + __shfl(sum, g0 + 8, 64)) + __shfl(sum, g0 + 16, 64)) + __shfl(sum, g0 + 24, 64);
}

}  // namespace qmx
