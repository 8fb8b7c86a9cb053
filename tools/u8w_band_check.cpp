// u8w_band_check.cpp — the host restatement of the dense-u8 128-query pass's band and compare (qdrant_amd/csrc/u8w_band.hpp) outside the library: C entry
// points for tests/test_u8w_band.py (built as a shared object), and a stand-alone run of the same arithmetic on small adversarial blocks for a sanitizer build:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iqdrant_amd/csrc tools/u8w_band_check.cpp -o /tmp/u8w_band_check
//   /tmp/u8w_band_check
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "u8w_band.hpp"

static qmx::U8WQuery query_sums(const uint8_t *q, uint32_t dim) {
    qmx::U8WQuery s{0, 0, 0};
    for (uint32_t i = 0; i < dim; ++i) qmx::u8w_query_add(s, q[i]);
    return s;
}
// what the device computes for one query against a block, from the same header: per row the pass's score A and whether the compare admits the pair at `cut`
extern "C" float qmx_u8w_band(int metric, int scalar_order, const uint8_t *q, uint32_t dim) { return qmx::u8w_band(metric, scalar_order != 0, query_sums(q, dim)); }
extern "C" void qmx_u8w_pass(int metric, const uint8_t *q, const uint8_t *rows, uint32_t n, uint32_t dim, double cut, float *a_out, uint8_t *admit_out) {
    const qmx::U8WQuery s = query_sums(q, dim);
    const int64_t qoff = qmx::u8w_qoff(metric, s, dim);
    const int32_t bound = qmx::u8w_int_bound(cut, qoff);
    float k = 0.0f, a = 0.0f;
    qmx::u8w_cos_coefs(cut, s, qoff, &k, &a);
    for (uint32_t r = 0; r < n; ++r) {
        const uint8_t *x = rows + (size_t)r * dim;
        int64_t dot = 0, s1 = 0, s2 = 0;      // I over the biased bytes, the row's column sums
        for (uint32_t i = 0; i < dim; ++i) {
            dot += (int64_t)(int8_t)(q[i] ^ 0x80) * (int8_t)(x[i] ^ 0x80);
            s1 += x[i];
            s2 += (int64_t)x[i] * x[i];
        }
        const int64_t col = metric == qmx::U8W_EUCLID ? 256 * s1 - s2 : 128 * s1;
        const int64_t v = (metric == qmx::U8W_EUCLID ? 2 * dot : dot) + col;
        a_out[r] = qmx::u8w_score(metric, v + qoff, s.sum_q2, s2);
        admit_out[r] = metric == qmx::U8W_COSINE ? fmaf(-k, qmx::u8w_row_f(s2), (float)(int32_t)v) >= a : (int32_t)v >= bound;
    }
}

// the reference's AVX2 leaf in plain C (dim a multiple of 32): eight i32 lanes (bytes 4 j .. 4 j + 3 of every 32-byte block land in lane j), converted and
// added in hsum256_ps_avx order
static float hsum8(const int64_t (&l)[8]) {
    float f[4];
    for (int j = 0; j < 4; ++j) f[j] = (float)l[j] + (float)l[j + 4];
    return (f[0] + f[2]) + (f[1] + f[3]);
}
static float reference(int metric, const uint8_t *q, const uint8_t *x, uint32_t dim) {
    int64_t l[8] = {0}, n1[8] = {0}, n2[8] = {0};
    for (uint32_t i = 0; i < dim; ++i) {
        const int j = (int)(i % 32) / 4;
        const int64_t a = q[i], b = x[i];
        l[j] += metric == qmx::U8W_EUCLID ? (a - b) * (a - b) : a * b;
        n1[j] += a * a;
        n2[j] += b * b;
    }
    const float s = hsum8(l);
    if (metric == qmx::U8W_DOT) return s;
    if (metric == qmx::U8W_EUCLID) return -s;
    const float den = hsum8(n1) * hsum8(n2);
    return den == 0.0f ? 0.0f : s / sqrtf(den);
}

// rows and queries from [lo, 255] with the extremes planted; every (query, row) pair: |A - R| <= band, and the compare admits every pair with A >= cut
static int check_block(int metric, uint32_t n, uint32_t dim, uint32_t nq, int lo, unsigned seed) {
    srand(seed);
    std::vector<uint8_t> x((size_t)n * dim), q((size_t)nq * dim);
    for (auto &v : x) v = (uint8_t)(lo + rand() % (256 - lo));
    for (auto &v : q) v = (uint8_t)(lo + rand() % (256 - lo));
    for (uint32_t i = 0; i < dim; ++i) {
        x[i] = 0;
        x[dim + i] = 255;
        x[2 * dim + i] = (uint8_t)(127 + (i & 1));
        q[i] = 255;
    }
    std::vector<float> a(n);
    std::vector<uint8_t> admit(n);
    int bad = 0;
    for (uint32_t j = 0; j < nq; ++j) {
        const uint8_t *qj = q.data() + (size_t)j * dim;
        const float band = qmx_u8w_band(metric, 0, qj, dim);
        const double cut = (double)reference(metric, qj, x.data() + (size_t)(3 + j) * dim, dim) - (double)band;      // some row's score as T
        qmx_u8w_pass(metric, qj, x.data(), n, dim, cut, a.data(), admit.data());
        for (uint32_t r = 0; r < n; ++r) {
            const float ref = reference(metric, qj, x.data() + (size_t)r * dim, dim);
            if (!(fabs((double)a[r] - (double)ref) <= (double)band)) ++bad;
            if ((double)a[r] >= cut && !admit[r]) ++bad;
        }
    }
    return bad;
}

int main() {
    int bad = 0;
    const int metrics[3] = {qmx::U8W_DOT, qmx::U8W_EUCLID, qmx::U8W_COSINE};
    for (int m = 0; m < 3; ++m) {
        bad += check_block(metrics[m], 200, 64, 6, 0, 1 + m);
        bad += check_block(metrics[m], 60, 1024, 4, 200, 4 + m);      // totals past 2^24
        // the staged scan's rows: its shortest (a last stage of one 64-byte chunk) and the derivation's limit (lane totals just under 2^24, totals under 2^27)
        for (uint32_t dim : {1088u, 2048u}) {
            bad += check_block(metrics[m], 60, dim, 4, 0, 7 + m + dim);
            bad += check_block(metrics[m], 60, dim, 4, 200, 10 + m + dim);
        }
    }
    if (bad) {
        printf("u8w_band_check: %d pairs outside the band or the compare\n", bad);
        return 1;
    }
    printf("u8w_band_check: ok\n");
    return 0;
}
