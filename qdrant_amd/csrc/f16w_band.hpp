// f16w_band.hpp — the band of the 128-query pass over a dense f16 block (scan_f16w.hip), as plain arithmetic that the device pack kernel and the host
// both compile (no HIP header).
//
// Notation.  q, x: a query and a row, dim f16 numbers each, all finite (the segment is checked at create, a query with an Inf / NaN takes no bound).
// Every product q_i x_i is EXACT in f32 (11 x 11 significand bits; no smaller than 2^-48).  S = sum q_i x_i, N = |x|^2, Q = |q|^2, E = |q - x|^2 =
// Q + N - 2 S, all exact.  u = 2^-24.  rowmax: an f32 number not below the largest |x|_2 of the segment (f16w_up of the f64 root, made at create).
//     P = sqrt(Q) rowmax  >= sum |q_i x_i| (Cauchy-Schwarz)  >= |S|
//     M = (sqrt(Q) + rowmax)^2  >= each of N, Q, 2 P, E, 2 |S| + N
// R: the reference's score, half_avx (metric_f16/avx/*.rs): 32 running f32 sums, element i in register (i % 32) / 8 lane i % 8, one fma per 32
// elements, hsum256_ps_avx per register, the four results added left to right.  A: the pass's score - Dot / Cosine A = D, Euclid
// A = fl(fl(2 D - Nf) - Qf) with D the matrix cores' f32 accumulator, Nf = fl32(N in f64) the row's column, Qf = fl32(Q in f64).
//
// (1) The matrix cores (v_mfma_f32_16x16x32_f16, dim / 32 steps chained through the accumulator).  Assumed: D is SOME summation of the dim exact
//     products, every intermediate result within a relative 2^-22 of its exact value (round-to-nearest is 2^-24, truncation 2^-23: a factor two spare),
//     in any order; and, should a step align its products to the largest one, no more than 2^-24 of that product lost per term (32 terms: 2^-19 of the
//     step's sum of magnitudes).  Then |D - S| <= ((1 + 2^-22)^dim - 1 + 2^-19) sum |q_i x_i| <= acc P, acc = 1.001 dim 2^-22 + 2^-18
//     (dim 2^-22 <= 2^-12 for dim <= 1024: the first-order form holds with the 1.001).  The f32 split route's 1e-4 |q| max |row| (scan_split.hip) is
//     the precedent; this is 2.5e-4 at dim 1024.
// (2) R itself.  A term passes dim / 32 fma roundings of its chain, three of the hsum and three of the final additions: |R - S| <=
//     g(dim / 32 + 6) P (g(k) = k u / (1 - k u)) <= 38 u 1.001 P.  Euclid: d_i = fl(q_i - x_i) is rounded once (two f16 numbers may lie 40 binades
//     apart), its square enters the fma exactly: two more roundings, |R + E| <= 40 u 1.001 E <= 40 u 1.001 M.
// (3) Euclid's column and epilogue: Nf and Qf are within u (1 + 2^-20) of N and Q (the f64 sums of at most 1024 exact squares err by 2^-43
//     relative), t = fl(2 D - Nf) (one fma: one rounding, |t| <= 1.001 M), A = fl(t - Qf) (|A| <= 1.001 M): four roundings, 4 u 1.002 M, and
//     2 |D - S| <= 2 acc P <= acc M.
//     So |A - R| <= eAR = (acc + 38 u 1.001) P for Dot / Cosine, (acc + 45 u 1.002) M for Euclid.
// (4) The sample's bound T_q is the k-th best of scores the existing f16 scans made (bound_enqueue): the same exact products - for Euclid the same
//     squares of once-rounded differences - summed in f32 in the device's order, on the VALU (round to nearest: dim roundings at most, dim u <= acc / 4)
//     or, from 8 queries on, on the same matrix cores (1).  Each is within eTR = eAR of the reference's score of its pair, so the reference's k-th best of
//     the sample, a lower bound of the final k-th best, is >= T_q - eTR, every result row has A >= T_q - eTR - eAR, and k rows with R >= A_k - eAR
//     exist: the selection's max(T_q - band, A_k - 2 band) is safe with band >= eTR + eAR = 2 eAR.
// (5) Subnormal f16 operands.  The ISA documents at hand do not say what the f16 matrix instruction does with them: the band ASSUMES THEY MAY BE FLUSHED TO
//     ZERO, in the pass and in the scans behind T_q alike.  A flushed row element (|x_i| < 2^-14) loses |q_i x_i| < 2^-14 |q_i|: at most 2^-14 sum |q_i|
//     per pair, and only if the segment holds a subnormal (the create-time flag).  A flushed query element loses < 2^-14 |x_i|: at most
//     2^-14 sqrt(nsub) rowmax over the query's nsub subnormal elements.  Euclid's 2 D doubles both.  eSub = 0 when neither side holds one.  The f32
//     RESULTS cannot be subnormal: every partial sum is a multiple of 2^-48, far above 2^-126.
// (6) The selection's own arithmetic: T - band and A_k - 2 band are f32 subtractions of numbers of at most 1.001 B + band: 3 u 1.01 B pays.
//     band = 2 (eAR + eSub) + 4 u B,   B = P (Dot / Cosine) or M (Euclid); the cut T_q - band is rounded DOWN (f16w_up of its negation).
// The compare needs no proof of its own: the scan evaluates A in exactly the f32 operations named above (-ffp-contract=off; the fma is explicit), lists
// the pairs with A >= cut and hands the same A to the selection.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QMX_F16W_HD __host__ __device__
#else
#define QMX_F16W_HD
#endif

namespace qmx {

enum { F16W_DOT = 0, F16W_EUCLID = 1 };      // (Cosine is Dot over normalised vectors)
constexpr uint32_t F16W_MAX_DIM = 1024;      // where the derivation ends
constexpr double F16W_U = 5.9604644775390625e-8;      // 2^-24
static_assert(F16W_MAX_DIM * 4 * F16W_U <= 1.0 / 4096, "(1): (1 + 2^-22)^dim - 1 <= 1.001 dim 2^-22");
static_assert((F16W_MAX_DIM / 32 + 8) * F16W_U < 1.0e-3 / 40, "(2): g(dim / 32 + 8) <= 1.001 (dim / 32 + 8) u, and dim / 32 + 8 <= 40");
static_assert(4.0 * 65504.0 * 65504.0 * F16W_MAX_DIM < 3.0e38, "M of the longest row of the largest finite f16 numbers is a finite f32 number");

// f64 -> f32, never below the argument
QMX_F16W_HD inline float f16w_up(double x) { return (float)(x + fabs(x) * 3.0 * F16W_U + 1.0e-45); }

// what the pass needs of a query
struct F16WQuery {
    double q2;          // Q = sum q_i^2 (exact products, f64 sum)
    double l1;          // sum |q_i|
    uint32_t nsub;      // subnormal elements
    uint32_t bad;       // Inf / NaN elements: no bound for this query
};
QMX_F16W_HD inline double f16w_acc(uint32_t dim) { return 1.001 * (double)dim / 4194304.0 + 1.0 / 262144.0; }
// band >= eTR + eAR + the selection's roundings, for every row of a segment whose largest norm is <= rowmax
QMX_F16W_HD inline float f16w_band(int metric, uint32_t dim, const F16WQuery &s, float rowmax, bool seg_subnormal) {
    const double qn = sqrt(s.q2) * (1.0 + 1.0e-15), rm = (double)rowmax;
    const bool euclid = metric == F16W_EUCLID;
    const double b = euclid ? (qn + rm) * (qn + rm) : qn * rm;
    const double e_ar = (f16w_acc(dim) + (euclid ? 45.0 * 1.002 : 38.0 * 1.001) * F16W_U) * b;
    const double e_sub = ((seg_subnormal ? s.l1 : 0.0) + sqrt((double)s.nsub) * rm) / 16384.0 * (euclid ? 2.0 : 1.0);
    return f16w_up(2.0 * (e_ar + e_sub) + 4.0 * F16W_U * b);
}
// the cut: T_q - band, rounded down
QMX_F16W_HD inline float f16w_cut(float t, float band) { return -f16w_up(-((double)t - (double)band)); }

}  // namespace qmx
