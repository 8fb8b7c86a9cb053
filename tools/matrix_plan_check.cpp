// matrix_plan_check.cpp — a stand-alone host run of the integer logic of the distance matrix API (qdrant_amd/csrc/matrix_plan.hpp): the sampler's key
// and its radix select driven level by level the way api_matrix.hip drives the kernels, against a sort; the chunk sizes for every limit against the
// staging bound; the validation of a sample on random lists; the clipping of the lists.  Meant for the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iqdrant_amd/csrc tools/matrix_plan_check.cpp -o /tmp/matrix_plan_check
//   /tmp/matrix_plan_check
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "matrix_plan.hpp"

using namespace qmx;

namespace {

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

// the select as the device runs it: per level a histogram of the candidates in the prefix, then the decision
uint32_t select_levels(const std::vector<uint32_t> &cand, uint64_t seed, uint32_t n, SampleState *out) {
    SampleState s{};
    s.need = n;
    uint32_t levels = 0;
    for (uint32_t level = 0; level < SAMPLE_LEVELS && !s.done; ++level, ++levels) {
        std::vector<uint32_t> hist(SAMPLE_BINS, 0), groups(SAMPLE_BINS / SAMPLE_GROUP, 0);
        for (uint32_t o : cand) {
            const uint64_t k = sample_key(seed, o);
            if (sample_in_prefix(k, s.prefix, level)) ++hist[sample_bin(k, level)];
        }
        for (uint32_t b = 0; b < SAMPLE_BINS; ++b) groups[b / SAMPLE_GROUP] += hist[b];
        sample_level_step(s, hist.data(), groups.data(), level);
    }
    *out = s;
    return levels;
}

void check_select(const std::vector<uint32_t> &cand, uint64_t seed, uint32_t n, uint32_t min_levels) {
    SampleState s{};
    const uint32_t levels = select_levels(cand, seed, n, &s);
    CHECK(s.done);
    CHECK(levels >= min_levels);
    CHECK(s.count == std::min<size_t>(n, cand.size()));
    std::vector<uint64_t> keys;
    for (uint32_t o : cand) keys.push_back(sample_key(seed, o));
    std::vector<uint64_t> sorted = keys;
    std::sort(sorted.begin(), sorted.end());
    CHECK(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end());      // the keys of distinct offsets differ
    size_t taken = 0;
    for (uint64_t k : keys) taken += k <= s.threshold;
    CHECK(taken == s.count);      // exactly the count smallest keys lie at or below the threshold
    if (s.count) CHECK(sorted[s.count - 1] <= s.threshold);
    if (s.count < sorted.size()) CHECK(sorted[s.count] > s.threshold);
}

void check_sampler() {
    CHECK(sample_key(0, 0) == 0xE220A8397B1DCDAFull);      // splitmix64's first output from state 0
    CHECK(sample_key(0x5EED, 12345) == 0xCBC84078A7339C6Aull);
    CHECK(sample_key(~0ull, 0xFFFFFFFEu) == 0xB079DC1E4A436403ull);
    for (uint32_t level = 0; level < SAMPLE_LEVELS; ++level) {      // the digits tile the key
        CHECK(sample_level_shift(level) + sample_level_bits(level) == (level ? sample_level_shift(level - 1) : 64u));
        CHECK(sample_bin(~0ull, level) == (1u << sample_level_bits(level)) - 1);
    }
    CHECK(sample_level_shift(SAMPLE_LEVELS - 1) == 0);
    std::mt19937_64 rng(1);
    std::vector<uint32_t> all(50000);
    for (uint32_t i = 0; i < all.size(); ++i) all[i] = i * 3 + (uint32_t)(rng() % 3);
    for (uint32_t n : {1u, 2u, 10u, 64u, 65u, 1000u, 49999u, 50000u, 50005u, 65536u}) check_select(all, rng(), n, 1);
    check_select({}, 3, 5, 1);
    check_select({7}, 3, 1, 1);
    check_select({7}, 3, 2, 1);
    // a crowded boundary bin: only offsets whose key has one top digit (and then one top two digits), so that the later levels decide
    for (uint32_t digits = 1; digits <= 2; ++digits) {
        const uint64_t seed = 99 + digits;
        std::vector<uint32_t> crowded;
        const uint32_t above = 64 - 12 * digits;
        const uint64_t want = sample_key(seed, 12345) >> above;
        for (uint32_t o = 0; crowded.size() < (digits == 1 ? 3000u : 10u) && o < 0xFFFFFFF0u; ++o)
            if ((sample_key(seed, o) >> above) == want) crowded.push_back(o);
        CHECK(crowded.size() >= 10);
        for (uint32_t n : {1u, 7u, (uint32_t)crowded.size() - 1}) check_select(crowded, seed, n, digits + 1);
        check_select(crowded, seed, (uint32_t)crowded.size(), 1);
    }
}

void check_chunks() {
    for (uint32_t n_sample : {2u, 3u, 63u, 64u, 65u, 4095u, 4096u, 4097u, 4099u, 8200u, 65535u, 65536u})
        for (uint32_t limit = 1; limit <= 65535; ++limit) {
            const uint32_t top = matrix_top(n_sample, limit), chunk = matrix_chunk(n_sample, limit);
            CHECK(top >= 1 && top <= n_sample && top <= limit + 1);
            CHECK(top == std::min<uint64_t>((uint64_t)limit + 1, n_sample));
            CHECK(chunk >= 1 && chunk <= MATRIX_MAX_CHUNK && chunk <= n_sample);
            CHECK((uint64_t)chunk * top * 8 <= MATRIX_STAGE_BYTES);
            // ... and no smaller than it has to be: twice the chunk (the rounding to whole tiles costs less than half) would break a bound
            if (chunk < n_sample && chunk < MATRIX_MAX_CHUNK) CHECK((uint64_t)chunk * 2 * top * 8 > MATRIX_STAGE_BYTES);
        }
    CHECK(matrix_chunk(65536, 3) == 4096);
    CHECK(matrix_chunk(65536, 65535) == 512);
    CHECK(matrix_chunk(10, 3) == 10);
    CHECK(matrix_top(10, 0xFFFFFFFFu) == 10);      // (limit + 1 must not wrap)
}

void check_validation() {
    std::mt19937 rng(2);
    uint32_t bad = 0;
    CHECK(matrix_validate_sample(nullptr, 0, 10, &bad) == 0);
    for (int round = 0; round < 2000; ++round) {
        const uint32_t n = 1 + rng() % 40, n_rows = 1 + rng() % 200;
        std::vector<uint32_t> ids(n);
        for (uint32_t &x : ids) x = rng() % (n_rows + (round % 4 == 0 ? 20 : 0));
        if (round % 2) std::sort(ids.begin(), ids.end());
        if (round % 3 == 0) ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        // the statement itself: the first position that breaks either rule, the order rule first at a position
        int want = 0;
        uint32_t want_at = 0;
        for (uint32_t i = 0; i < ids.size() && !want; ++i) {
            if (i && ids[i] <= ids[i - 1]) want = 1, want_at = i;
            else if (ids[i] >= n_rows) want = 2, want_at = i;
        }
        bad = 0;
        const int got = matrix_validate_sample(ids.data(), (uint32_t)ids.size(), n_rows, &bad);
        CHECK(got == want);
        if (want) CHECK(bad == want_at);
    }
    const uint32_t rep[3] = {1, 5, 5}, uns[3] = {1, 9, 5}, far[3] = {1, 5, 10};
    CHECK(matrix_validate_sample(rep, 3, 10, &bad) == 1 && bad == 2);
    CHECK(matrix_validate_sample(uns, 3, 10, &bad) == 1 && bad == 2);
    CHECK(matrix_validate_sample(far, 3, 10, &bad) == 2 && bad == 2);
    CHECK(matrix_validate_sample(far, 3, 11, &bad) == 0);
}

void check_clipping() {
    for (uint32_t count = 0; count <= 70; ++count)
        for (uint32_t self_at = 0; self_at <= count; ++self_at)
            for (uint32_t limit : {1u, 2u, 3u, 64u, 69u, 70u, 71u, 1000u}) {
                std::vector<uint32_t> want;      // the list without its entry at self_at, cut
                for (uint32_t k = 0; k < count && want.size() < limit; ++k)
                    if (k != self_at) want.push_back(k);
                const uint32_t kept = matrix_clip(count, self_at, limit);
                CHECK(kept == want.size());
                for (uint32_t k = 0; k < kept; ++k) {
                    CHECK(matrix_src(k, self_at) == want[k]);
                    CHECK(matrix_src(k, self_at) < count);
                }
            }
    // the reference's two rules on a list of limit + 1: remove self when it is there, pop the last one otherwise - both leave `limit` entries
    CHECK(matrix_clip(4, 1, 3) == 3 && matrix_clip(4, 4, 3) == 3 && matrix_src(2, 4) == 2 && matrix_src(2, 1) == 3);
}

// the f16 block layout: every stored element lands exactly once, the rest is zeros, and position (segment s, piece 2 r + h, dword k, half b) holds
// element 32 (2 s + b) + 8 r + 4 h + k - register r, SIMD lane 4 h + k of AVX iteration 2 s + b
void check_f16_layout() {
    for (uint32_t dim = 32; dim <= 1100; ++dim) {
        const uint32_t block_dim = matrix_f16_avx_dim(dim), iters = dim / 32;
        CHECK(block_dim >= dim && block_dim <= dim + 32 && block_dim % 64 == dim % 32);
        std::vector<uint32_t> seen(dim, 0);
        for (uint32_t o = 0; o < block_dim + 16; ++o) {      // (the gather asks up to the row's 16-byte pitch)
            const uint32_t from = matrix_f16_avx_source(o, dim);
            if (from == MATRIX_NO_SOURCE) continue;
            CHECK(from < dim && o < block_dim);
            ++seen[from];
            if (from >= iters * 32) CHECK(o == block_dim - dim % 32 + (from - iters * 32));
            else {
                const uint32_t it = from / 32, r = from % 32 / 8, h = from % 8 / 4, k = from % 4;
                CHECK(o == (it / 2) * 64 + (2 * r + h) * 8 + k * 2 + it % 2);
            }
        }
        for (uint32_t x : seen) CHECK(x == 1);
    }
    CHECK(matrix_f16_avx_dim(32) == 64 && matrix_f16_avx_dim(33) == 65 && matrix_f16_avx_dim(64) == 64 && matrix_f16_avx_dim(768) == 768);
}

}  // namespace

int main() {
    check_f16_layout();
    check_sampler();
    check_chunks();
    check_validation();
    check_clipping();
    printf("matrix_plan_check: ok\n");
    return 0;
}
