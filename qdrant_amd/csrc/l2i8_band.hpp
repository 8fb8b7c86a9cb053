// l2i8_band.hpp — the error band of the Euclid int8 prefilter (scan_l2i8.hip), as plain arithmetic that the device pack kernel, the host and a CPU
// test all compile (no HIP header; tools/l2i8_band_check.cpp, tests/test_l2i8_band.py).
//
// What is compared.  The reference's score of a pair is R = -fl32( sum_i (q_i - x_i)^2 ) in the AVX order (dense_policies.hpp RowF32<M_EUCLID>).  The scan
// delivers  A = fl32( 2 t I - N_r - Q )  from
//   mu      any f32 vector (the column means; the identity below holds for EVERY mu, so its own rounding costs nothing)
//   y = x - mu, p = q - mu      formed in f64 from f32 operands: exact, or within 2^-53 of the larger operand
//   y_i = s_i (c_i + e_i),      c_i = rint(y_i / s_i) in [-127, 127], |e_i| <= 1/2       (s_i >= max_r |y_ri| / 127: the columns' scales)
//   p_i s_i = t (d_i + f_i),    d_i = rint(p_i s_i / t) in [-127, 127], |f_i| <= 1/2      (t >= max_i |p_i s_i| / 127, an f32 number: the query's scale)
//   I = sum_i c_i d_i           the integer of v_mfma_i32_16x16x64_i8, exact; the epilogue converts it to f32: fl32(I), see (6)
//   N_r = |y_r|^2, Q = |p|^2    f64 sums, stored as f32
// and  -|q - x|^2 = -|p - y|^2 = 2 y.p - N_r - Q  exactly.  So |A - R| is at most the sum of
//   (1) 2 |y.p - t I| <= 2 t [ min(C1 / 2, C2 |f|_2) + (sum_i |d_i|) / 2 + dim / 4 ]          C1 = max_r sum_i |c_ri|, C2 = max_r |c_r|_2
//       (scan_i8copy.hip's band_dot, twice; x 1.001 for the f64 roundings of y / s, p s, p s / t)
//   (2) the f32 storage of N_r and Q: 2^-24 (N_r + Q)
//   (3) the f64 centring and the f64 sums of N_r, Q: (dim + 4) 2^-52 of sum (|y_i| + |p_i|)^2 <= 2 (N_r + Q): below 2^-36 (N_r + Q) for dim <= 4096
//   (4) the reference's own f32 value: every term passes through one rounded subtraction (squared: 2 u), one fused multiply-add and the additions of its
//       AVX lane and of the horizontal sums - fewer than dim / 32 + 8 of them -, u = 2^-24: a relative (dim / 32 + 10) u (1 + ...) of |q - x|^2.  Taken as
//       (dim + 16) 2^-23, the issue's "about dim 2^-23", of |q - x|^2 <= 2 (N_r + Q) - for EVERY row, not only for those near the result
//   (5) the epilogue's f32 evaluation  fma(2 t, I, -N_r) - Q : two roundings of results below 2 t |I| + N_r + Q, the f32 value 2 t is exact;
//       2 t |I| <= 2 |y.p| + term (1) <= N_r + Q + term (1):  2^-23 (2 (N_r + Q) + term (1))
//   (6) the conversion fl32(I): |I| <= 127^2 dim.  Below 2^24 (dim <= 1024) every integer is an f32 number and the term is 0.  In [2^24, 2^25) - rows of
//       1 152 .. 2 048 coordinates, 127^2 2048 = 33 032 192 < 2^25 - the f32 numbers are the even integers, so |fl32(I) - I| <= e_I = 1, half the spacing
//       (in general half the spacing of the binade of 127^2 dim: l2i8_int_rounding).  The score moves by 2 t e_I, and the 2 t |fl32(I)| of (5) grows by as much.
// with N_r <= n_max = max_r N_r (as stored, rounded up).  Every term is rounded up; none is tuned.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QMX_L2I8_HD __host__ __device__
#else
#define QMX_L2I8_HD
#endif

namespace qmx {

// the terms of a query the band needs (the pack kernel's sums; the CPU test's numpy restatement)
struct L2I8Query {
    double t;          // the query's scale (an f32 value)
    double sum_abs_d;  // sum_i |d_i|
    double f_norm;     // |f|_2
    double q_norm2;    // Q = |q - mu|^2
};
// ... and of the segment
struct L2I8Rows {
    double c1;         // max_r sum_i |c_ri|
    double c2;         // max_r |c_r|_2
    double n_max;      // max_r N_r
    uint32_t dim;
};

QMX_L2I8_HD inline double l2i8_band_dot(const L2I8Query &q, const L2I8Rows &r) {
    const double cf = 0.5 * r.c1 < r.c2 * q.f_norm ? 0.5 * r.c1 : r.c2 * q.f_norm;
    return q.t * (cf + 0.5 * q.sum_abs_d + 0.25 * (double)r.dim) * 1.001;
}

// e_I of (6): the most fl32(I) differs from I for |I| <= 127^2 dim - 0 below 2^24, 1 below 2^25, doubling per binade
QMX_L2I8_HD inline double l2i8_int_rounding(uint32_t dim) {
    double e = 0.5;
    for (double m = 16129.0 * (double)dim; m >= 16777216.0; m *= 0.5) e *= 2.0;
    return e >= 1.0 ? e : 0.0;
}

// |A - R| <= l2i8_band for every row of the segment (an f32 number, rounded up)
QMX_L2I8_HD inline float l2i8_band(const L2I8Query &q, const L2I8Rows &r) {
    const double u = 5.9604644775390625e-8;                     // 2^-24
    const double dot2 = 2.0 * l2i8_band_dot(q, r);              // (1)
    const double s = r.n_max + q.q_norm2;
    const double store = u * s;                                 // (2)
    const double centre = 1.4551915228366852e-11 * s;           // (3) 2^-36
    const double ref = ((double)r.dim + 16.0) * 2.0 * u * 2.0 * s;   // (4)
    const double conv = 2.0 * q.t * l2i8_int_rounding(r.dim);  // (6): 0 for dim <= 1024, where every sum below keeps its bits
    const double epi = 2.0 * u * (2.0 * s + dot2 + conv);       // (5)
    const double b = (dot2 + store + centre + ref + epi + conv) * (1.0 + 1.0e-6);
    float f = (float)b;
    if ((double)f < b) f = nextafterf(f, INFINITY);
    return f;
}

// The epilogue's compare.  A pair is a candidate when A >= cut (cut = T_q - band).  In integers' units:  I >= (cut + Q) / (2 t) + N_r / (2 t) = a + b N_r.  The
// kernel evaluates  fl32(I) - fl32(b) N_r  by one fused multiply-add and compares with fl32(a) - slack:
// slack covers the roundings of a, of b (times N_r) and of the fused result - 2^-24 of |a|, b n_max, and 127^2 dim + b n_max -, doubled, plus one, plus e_I:
// fl32(I) >= I - e_I (term (6); 0 for dim <= 1024, where I is exact in f32).
QMX_L2I8_HD inline void l2i8_compare_coefs(double cut, const L2I8Query &q, const L2I8Rows &r, float *a_out, float *b_out) {
    const double u = 5.9604644775390625e-8;
    const double b = 1.0 / (2.0 * q.t);
    const double a = (cut + q.q_norm2) * b;
    const double slack = 2.0 * u * (fabs(a) + 2.0 * b * r.n_max + 16129.0 * (double)r.dim) + 1.0 + l2i8_int_rounding(r.dim);
    float af = (float)(a - slack);
    if ((double)af > a - slack) af = nextafterf(af, -INFINITY);
    *a_out = af;
    *b_out = (float)b;
}

}  // namespace qmx
