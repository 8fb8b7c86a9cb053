// l2i8_band_check.cpp — the host restatement of the Euclid int8 prefilter's band (qdrant_amd/csrc/l2i8_band.hpp) outside the library: C entry points for
// tests/test_l2i8_band.py (built as a shared object), and a stand-alone run of the same arithmetic on a small block for a sanitizer build:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iqdrant_amd/csrc tools/l2i8_band_check.cpp -o /tmp/l2i8_band_check
//   /tmp/l2i8_band_check
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "l2i8_band.hpp"

extern "C" float qmx_l2i8_band(double t, double sum_abs_d, double f_norm, double q_norm2, double c1, double c2, double n_max, uint32_t dim) {
    return qmx::l2i8_band(qmx::L2I8Query{t, sum_abs_d, f_norm, q_norm2}, qmx::L2I8Rows{c1, c2, n_max, dim});
}
extern "C" void qmx_l2i8_compare_coefs(double cut, double t, double q_norm2, double n_max, uint32_t dim, float *a, float *b) {
    qmx::l2i8_compare_coefs(cut, qmx::L2I8Query{t, 0.0, 0.0, q_norm2}, qmx::L2I8Rows{0.0, 0.0, n_max, dim}, a, b);
}

// a block of n rows shifted by `shift`, quantised as scan_l2i8.hip does it; every (query, row) pair: |A - R| <= band, and the compare admits every
// pair with A >= cut.  R here is the f32 sum in plain order - any order is inside term (4)
static int check_block(uint32_t n, uint32_t dim, uint32_t nq, float shift, unsigned seed) {
    srand(seed);
    auto unit = []() { return (float)rand() / (float)RAND_MAX - 0.5f; };
    std::vector<float> x((size_t)n * dim), q((size_t)nq * dim), mu(dim), s(dim);
    for (auto &v : x) v = unit() + shift;
    for (auto &v : q) v = unit() + shift;
    for (uint32_t i = 0; i < dim; ++i) {
        double sum = 0.0, mx = 0.0;
        for (uint32_t r = 0; r < n; ++r) sum += x[(size_t)r * dim + i];
        mu[i] = (float)(sum / n);
        for (uint32_t r = 0; r < n; ++r) mx = fmax(mx, fabs((double)x[(size_t)r * dim + i] - (double)mu[i]));
        s[i] = nextafterf((float)mx, INFINITY) / 127.0f;
    }
    std::vector<int> c((size_t)n * dim);
    std::vector<float> nr(n);
    qmx::L2I8Rows rows{0.0, 0.0, 0.0, dim};
    for (uint32_t r = 0; r < n; ++r) {
        double c1 = 0.0, c2 = 0.0, nn = 0.0;
        for (uint32_t i = 0; i < dim; ++i) {
            const double y = (double)x[(size_t)r * dim + i] - (double)mu[i];
            double k = rint(y / (double)s[i]);
            k = k > 127.0 ? 127.0 : (k < -127.0 ? -127.0 : k);
            c[(size_t)r * dim + i] = (int)k;
            c1 += fabs(k);
            c2 += k * k;
            nn += y * y;
        }
        nr[r] = (float)nn;
        rows.c1 = fmax(rows.c1, c1);
        rows.c2 = fmax(rows.c2, sqrt(c2));
        rows.n_max = fmax(rows.n_max, (double)nextafterf((float)nn, INFINITY));
    }
    int bad = 0;
    for (uint32_t j = 0; j < nq; ++j) {
        std::vector<double> u(dim);
        std::vector<int> d(dim);
        qmx::L2I8Query qq{0.0, 0.0, 0.0, 0.0};
        double mx = 0.0;
        for (uint32_t i = 0; i < dim; ++i) {
            const double p = (double)q[(size_t)j * dim + i] - (double)mu[i];
            u[i] = p * (double)s[i];
            mx = fmax(mx, fabs(u[i]));
            qq.q_norm2 += p * p;
        }
        const float t_f = nextafterf((float)(mx / 127.0), INFINITY);
        qq.t = t_f;
        for (uint32_t i = 0; i < dim; ++i) {
            double k = rint(u[i] / qq.t);
            k = k > 127.0 ? 127.0 : (k < -127.0 ? -127.0 : k);
            d[i] = (int)k;
            qq.sum_abs_d += fabs(k);
            qq.f_norm += (u[i] / qq.t - k) * (u[i] / qq.t - k);
        }
        qq.f_norm = sqrt(qq.f_norm);
        const float band = qmx::l2i8_band(qq, rows);
        const double cut = -(double)rows.n_max * 0.25 - (double)band;      // some cut inside the scores' range
        float ca, cb;
        qmx::l2i8_compare_coefs(cut, qq, rows, &ca, &cb);
        for (uint32_t r = 0; r < n; ++r) {
            long long dot = 0;
            float ref = 0.0f;
            for (uint32_t i = 0; i < dim; ++i) {
                dot += (long long)c[(size_t)r * dim + i] * d[i];
                const float df = q[(size_t)j * dim + i] - x[(size_t)r * dim + i];
                ref = fmaf(df, df, ref);
            }
            const float fi = (float)dot;
            const float a = fmaf(2.0f * t_f, fi, -nr[r]) - (float)qq.q_norm2;
            if (!(fabs((double)a - (double)-ref) <= (double)band)) ++bad;
            if ((double)a >= cut && !(fmaf(-cb, nr[r], fi) >= ca)) ++bad;
        }
    }
    return bad;
}

int main() {
    int bad = 0;
    bad += check_block(300, 128, 8, 0.0f, 1);
    bad += check_block(300, 128, 8, 50.0f, 2);
    bad += check_block(70, 256, 3, -7.0f, 3);
    if (bad) {
        printf("l2i8_band_check: %d pairs outside the band\n", bad);
        return 1;
    }
    printf("l2i8_band_check: ok\n");
    return 0;
}
