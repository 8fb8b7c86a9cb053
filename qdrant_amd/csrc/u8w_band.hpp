// u8w_band.hpp — the band and the compare of the 128-query pass over a dense u8 block (scan_u8w.hip), as plain arithmetic that the device pack kernel,
// the host and a CPU test all compile (no HIP header; tools/u8w_band_check.cpp, tests/test_u8w_band.py).
//
// The pass knows the EXACT integers of a (query, row) pair: with x' = x - 128, q' = q - 128 (the bytes ^ 0x80 read as int8) and I = sum q' x'
//     Dot     S = q.x        = I + 128 sum(q') + 128 sum(x)
//     Euclid  -D = -|q - x|^2 = 2 I + (256 sum(x) - sum(x^2)) + (256 sum(q') - sum(q^2))
//     Cosine  S / sqrt(N1 N2),  N1 = sum(q^2), N2 = sum(x^2)
// (x = x' + 128, q = q' + 128: q.x = I + 128 sum(q') + 128 sum(x') + 128^2 dim, and 128 sum(x) = 128 sum(x') + 128^2 dim; |q - x|^2 = N1 + N2 - 2 q.x.)
// Its score A is that integer as one f32 number (Dot, Euclid negated), or the quotient of the exact integers evaluated in f64 and rounded once (Cosine).
//
// The reference's score R is not always a function of the integer.  Its AVX2 leaf (metric_uint/avx2/*.rs) converts eight i32 lane totals to f32 and adds
// them in hsum256_ps_avx order; rows of a multiple of 32 bytes have no remainder loop.  For dim <= 2048 a lane total is at most 65025 dim / 8 < 2^24 and
// converts exactly, so R is the result of SEVEN correctly rounded additions of non-negative numbers whose exact sum is the integer Z (S, D, N1 or N2):
// every partial sum is at most Z (1 + u)^k, u = 2^-24, so |R - Z| <= g7 Z with g7 = 7 u / (1 - 7 u), whatever the order of the additions.
//     (1) Dot / Euclid, AVX2 order:    |R - Z| <= g7 Z
//     (2) A itself:                    |A - Z| <= u Z          (one rounding of an integer below 2^27)
//     (3) the selection's arithmetic:  the cut max(T - band, A_k - 2 band) is two f32 subtractions of numbers of at most Z's size: <= 2 u Z
//   band = (g7 + 3 u) Zmax, Zmax a per-query bound of the total: 255 sum(q) for Dot, sum_i max(q_i, 255 - q_i)^2 for Euclid.
//     Under scalar order (QMX_SEG_U8_SCALAR_ORDER, metric_uint/simple_*.rs) the reference casts ONE i32: R = A, bit for bit, the subtractions of a zero
//   band are exact, and the band is zero (ties in f32 already pass: the selection keeps A >= cut).
//     (4) Cosine: R = fl(s / fl(sqrt(fl(n1 n2)))) with s, n1, n2 each within g7 of their integers (AVX2 order; one cast each within u under scalar order):
//   relative to c = S / sqrt(N1 N2): g7 (s) + (2 g7 + u) / 2 (the radicand, halved by the root) + u (root) + u (quotient), A's rounding u, the
//   selection's 2 u; second-order terms are below 1e-12 relative and one more u pays for them and for the f64 evaluation of A:
//   band = (2 g7 + 7 u) 1.0001 (|c| <= 1 by Cauchy-Schwarz, R <= 1.0001).  Either order: the scalar order's roundings are a subset.
//
// The integer compare (Dot, Euclid).  The scan holds V = I + C[row] (Dot) or 2 I + C[row] (Euclid); Z' = V + qoff is the integer score (S or -D) and
// A = fl32(Z').  |Z'| < 2^27, so |A - Z'| <= 4 and A >= cut implies Z' >= cut - 4: with bound = floor(cut) - 8 - qoff every pair the cut admits has
// V >= bound.  The float compare (Cosine).  A >= cut > 0 implies S >= cut (1 - 2 u) sqrt(N1) sqrt(N2).  The row's column F is an f32 number below sqrt(N2)
// (u8w_row_f), the query's coefficient k an f32 number below cut (1 - 3 u) sqrt(N1) (u8w_cos_coefs), so V - k F >= -qoff in exact arithmetic; the scan
// evaluates fma(-k, F, fl32(V)): the convert is within 4 of V and the fma within 8 of its exact value (both below 2^27 in magnitude), so the compare
// against a = -qoff - 16 (rounded down) admits the pair.  A cut that is not positive admits every pair (k = 0: all u8 cosines are >= 0 anyway).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QMX_U8W_HD __host__ __device__
#else
#define QMX_U8W_HD
#endif

namespace qmx {

enum { U8W_DOT = 0, U8W_EUCLID = 1, U8W_COSINE = 3 };      // (dense_policies.hpp M_*)
constexpr double U8W_U = 5.9604644775390625e-8;           // 2^-24
constexpr double U8W_G7 = 7.0 * U8W_U / (1.0 - 7.0 * U8W_U);

// f64 -> f32, never below the argument (moved up by more than the rounding to nearest can take back: no nextafter on either side of the compiler)
QMX_U8W_HD inline float u8w_up(double x) { return (float)(x + fabs(x) * 3.0 * U8W_U + 1.0e-45); }

// the sums of a query's bytes the pass needs
struct U8WQuery {
    int64_t sum_q;      // sum q_i
    int64_t sum_q2;     // N1 = sum q_i^2
    int64_t far2;       // sum_i max(q_i, 255 - q_i)^2: no row is farther
};
QMX_U8W_HD inline void u8w_query_add(U8WQuery &s, uint32_t q) {
    const int64_t v = (int64_t)q, f = v > 255 - v ? v : 255 - v;
    s.sum_q += v;
    s.sum_q2 += v * v;
    s.far2 += f * f;
}
// the query's term of the integer score: Z' = V + qoff (Dot, Cosine: 128 sum(q'), Euclid: 256 sum(q') - sum(q^2))
QMX_U8W_HD inline int64_t u8w_qoff(int metric, const U8WQuery &s, uint32_t dim) {
    const int64_t sum_qp = s.sum_q - 128 * (int64_t)dim;
    return metric == U8W_EUCLID ? 256 * sum_qp - s.sum_q2 : 128 * sum_qp;
}
// |A - R| <= band for every row, the selection's own roundings included (see above)
QMX_U8W_HD inline float u8w_band(int metric, bool scalar_order, const U8WQuery &s) {
    if (metric == U8W_COSINE) return u8w_up((2.0 * U8W_G7 + 7.0 * U8W_U) * 1.0001);
    if (scalar_order) return 0.0f;
    const double zmax = metric == U8W_DOT ? 255.0 * (double)s.sum_q : (double)s.far2;
    return u8w_up((U8W_G7 + 3.0 * U8W_U) * zmax);
}
// Dot / Euclid: every pair with A >= cut has V >= the bound (INT32_MAX: no finite cut - nothing passes)
QMX_U8W_HD inline int32_t u8w_int_bound(double cut, int64_t qoff) {
    if (!(cut == cut) || cut > 2147483000.0) return 0x7FFFFFFF;
    const double b = floor(cut) - 8.0 - (double)qoff;
    return b <= -2147483647.0 ? (int32_t)0x80000000 : b >= 2147483000.0 ? 0x7FFFFFFF : (int32_t)b;
}
// Cosine: the row's f32 column, below sqrt(N2) (0 for a zero row)
QMX_U8W_HD inline float u8w_row_f(int64_t n2) { return (float)(sqrt((double)n2) * (1.0 - 2.0 * U8W_U)); }
// ... and the query's terms: every pair with A >= cut has fma(-k, F, fl32(V)) >= a
QMX_U8W_HD inline void u8w_cos_coefs(double cut, const U8WQuery &s, int64_t qoff, float *k_out, float *a_out) {
    *k_out = cut > 0.0 ? (float)(cut * (1.0 - 4.0 * U8W_U) * sqrt((double)s.sum_q2)) : 0.0f;
    *a_out = -u8w_up((double)qoff + 16.0);
}
// the pass's score of a pair from its exact integers: z = S (Dot, Cosine) or -D (Euclid)
QMX_U8W_HD inline float u8w_score(int metric, int64_t z, int64_t n1, int64_t n2) {
    if (metric != U8W_COSINE) return (float)z;
    if (n1 == 0 || n2 == 0) return 0.0f;      // (cosine.rs: a zero denominator scores 0)
    return (float)((double)z / sqrt((double)n1 * (double)n2));
}

}  // namespace qmx
