// group_logic_check.cpp — a stand-alone host run of the integer logic of grouped search (qdrant_amd/csrc/group_logic.hpp): the key table, the
// aggregation step, the done rule, the page bound and the fallback's tiling, driven page by page the way api_groups.hip drives the kernels, against a
// brute-force statement of the contract.  Meant for the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iqdrant_amd/csrc tools/group_logic_check.cpp -o /tmp/group_logic_check
//   /tmp/group_logic_check
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <random>
#include <vector>

#include "group_logic.hpp"

using namespace qmx;

namespace {

constexpr uint32_t PAGE = 64;
struct Hit { uint32_t idx; uint32_t rank; };      // rank 0 = best; the stream is ascending rank
struct Slots {
    uint32_t limit, group_size, n_slots = 0, n_full = 0;
    std::vector<uint32_t> key, cnt, last;
    std::vector<std::vector<uint32_t>> hits;
    Slots(uint32_t l, uint32_t g) : limit(l), group_size(g), key(l), cnt(l), last(l), hits(l) {}
};

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

// one aggregate launch over a page of ranked points; returns done
bool aggregate(Slots &s, const std::vector<uint32_t> &page, const std::vector<std::vector<uint32_t>> &keys_of) {
    std::fill(s.last.begin(), s.last.end(), 0xFFFFFFFFu);
    for (size_t h = 0; h < page.size() && s.n_full < s.limit; ++h) {
        const uint32_t idx = page[h];
        uint64_t prev = 0;
        for (;;) {      // the point's keys ascending, each once
            uint32_t key = GROUP_NONE;
            for (uint32_t k : keys_of[idx])
                if (k != GROUP_NONE && (uint64_t)k + 1 > prev && k < key) key = k;
            if (key == GROUP_NONE) break;
            prev = (uint64_t)key + 1;
            int32_t found = -1;
            for (uint32_t i = 0; i < s.n_slots; ++i)
                if (s.key[i] == key) { found = (int32_t)i; break; }
            const GroupStep st = group_step(found, found >= 0 ? s.cnt[found] : 0u, found >= 0 ? s.last[found] : 0u, idx, s.n_slots, s.limit, s.group_size);
            if (st.slot < 0) continue;
            CHECK((uint32_t)st.slot < s.limit && st.pos < s.group_size);
            s.key[st.slot] = key;
            s.cnt[st.slot] = st.pos + 1;
            s.last[st.slot] = idx;
            s.hits[st.slot].push_back(idx);
            s.n_slots += st.opened;
            s.n_full += st.filled;
        }
    }
    return group_done(s.n_full, s.limit, (uint32_t)page.size(), PAGE, false);
}

// one selection launch: the 64 best eligible points ranked below `bound_rank`
std::vector<uint32_t> select(const Slots &s, const std::vector<uint32_t> &stream, size_t first, const std::vector<std::vector<uint32_t>> &keys_of) {
    std::vector<uint32_t> table(GROUP_TABLE, GROUP_NONE);
    const bool filling = group_filling(s.n_slots, s.limit);
    for (uint32_t i = 0; i < s.n_slots; ++i)
        if (group_slot_in_table(s.cnt[i], s.group_size, filling)) group_table_insert_host(table.data(), s.key[i]);
    for (uint32_t i = 0; i < s.n_slots; ++i)
        CHECK(group_table_has(table.data(), s.key[i]) == group_slot_in_table(s.cnt[i], s.group_size, filling));
    std::vector<uint32_t> page;
    for (size_t r = first; r < stream.size() && page.size() < PAGE; ++r) {
        bool eligible = false;
        for (uint32_t k : keys_of[stream[r]]) eligible = eligible || group_key_eligible(table.data(), k, filling);
        if (eligible) page.push_back(stream[r]);
    }
    return page;
}

void one_case(std::mt19937 &rng, uint32_t n, uint32_t n_groups, uint32_t limit, uint32_t group_size, int layout) {
    std::vector<uint32_t> stream(n);
    for (uint32_t i = 0; i < n; ++i) stream[i] = i;
    std::shuffle(stream.begin(), stream.end(), rng);
    std::vector<std::vector<uint32_t>> keys_of(n);
    for (uint32_t r = 0; r < n; ++r) {
        const uint32_t i = stream[r];
        if (layout == 0) keys_of[i] = {(uint32_t)(rng() % n_groups)};
        else if (layout == 1) { for (uint32_t c = rng() % 4; c; --c) keys_of[i].push_back((uint32_t)(rng() % n_groups) * 2654435761u % 0xFFFFFFF0u); }
        else if (layout == 2) keys_of[i] = {r < n / 2 ? 0u : 1u + (uint32_t)(rng() % n_groups)};      // one group owns the best half
        else keys_of[i] = {rng() % 3 ? GROUP_NONE : (uint32_t)(rng() % n_groups)};
    }
    // the contract, brute force
    std::vector<uint32_t> order;
    std::map<uint32_t, std::vector<uint32_t>> want;
    for (uint32_t r = 0; r < n; ++r) {
        std::vector<uint32_t> ks = keys_of[stream[r]];
        std::sort(ks.begin(), ks.end());
        ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
        for (uint32_t k : ks) {
            if (k == GROUP_NONE) continue;
            if (!want.count(k)) order.push_back(k);
            if (want[k].size() < group_size) want[k].push_back(stream[r]);
        }
    }
    if (order.size() > limit) order.resize(limit);
    // the driver: stage 0 = the first 64 of the whole stream, then selection pages under the last rank consumed
    Slots s(limit, group_size);
    std::vector<uint32_t> rank_of(n);
    for (uint32_t r = 0; r < n; ++r) rank_of[stream[r]] = r;
    std::vector<uint32_t> page(stream.begin(), stream.begin() + std::min<uint32_t>(n, PAGE));
    bool done = aggregate(s, page, keys_of);
    uint64_t pages = 0;
    while (!done) {
        CHECK(pages <= group_page_bound(limit, group_size));
        const size_t first = (size_t)rank_of[page.back()] + 1;
        page = select(s, stream, first, keys_of);
        const uint32_t before = s.n_full;
        uint32_t hits_before = 0, hits_after = 0;
        for (uint32_t i = 0; i < s.n_slots; ++i) hits_before += s.cnt[i];
        done = aggregate(s, page, keys_of);
        for (uint32_t i = 0; i < s.n_slots; ++i) hits_after += s.cnt[i];
        CHECK(page.empty() || hits_after > hits_before);      // every page's first row is eligible by construction
        CHECK(s.n_full >= before);
        ++pages;
    }
    CHECK(s.n_slots == order.size());
    for (uint32_t i = 0; i < s.n_slots; ++i) {
        CHECK(s.key[i] == order[i]);
        CHECK(s.hits[i] == want[order[i]]);
    }
}

}  // namespace

int main() {
    std::mt19937 rng(12345);
    // the table at its fullest: 1024 keys that collide in the hash's low probes
    {
        std::vector<uint32_t> table(GROUP_TABLE, GROUP_NONE);
        std::vector<uint32_t> keys;
        for (uint32_t i = 0; i < 1024; ++i) keys.push_back(i % 2 ? i * 2048u : (uint32_t)rng());
        for (uint32_t k : keys) if (k != GROUP_NONE) group_table_insert_host(table.data(), k);
        for (uint32_t k : keys) CHECK(k == GROUP_NONE || group_table_has(table.data(), k));
        uint32_t misses = 0;
        for (uint32_t i = 0; i < 100000; ++i) {
            const uint32_t k = (uint32_t)rng();
            if (std::find(keys.begin(), keys.end(), k) == keys.end()) { CHECK(!group_table_has(table.data(), k)); ++misses; }
        }
        CHECK(misses > 0);
        for (uint32_t k = 0; k < 4096; ++k) CHECK(group_hash(k) < GROUP_TABLE);
        CHECK(group_hash(0xFFFFFFFEu) < GROUP_TABLE);
    }
    // the driver's arithmetic
    CHECK(group_page_bound(1024, 64) == 65537 && group_page_bound(1, 1) == 2);
    CHECK(group_score_stride(0) == 0 && group_score_stride(1) == 4 && group_score_stride(4096) == 4096 && group_score_stride(4097) == 4100);
    CHECK(group_tile_queries(5, 4096, 2 * 4096 * 4) == 2 && group_tile_queries(5, 4096, 1) == 1 && group_tile_queries(5, 4096, 1ull << 30) == 5);
    CHECK(group_tile_queries(3, 0, 0) == 3 && group_tile_queries(0, 100, 1 << 20) == 0);
    CHECK(group_select_blocks(1, 1) == 1 && group_select_blocks(10000000, 16) == 64 && group_select_blocks(10000000, 5000) == 1 && group_select_blocks(0, 0) == 1);
    {
        const uint64_t bound[5] = {0, 7, 0, ~0ull, 1};
        uint32_t list[5];
        CHECK(group_pack_unfinished(bound, 5, list) == 3 && list[0] == 1 && list[1] == 3 && list[2] == 4);
    }
    CHECK(!group_done(1, 2, 64, 64, false) && group_done(2, 2, 64, 64, false) && group_done(0, 2, 63, 64, false) && group_done(0, 2, 64, 64, true));
    // the pipeline on the host against the contract
    uint32_t cases = 0;
    for (int layout = 0; layout < 4; ++layout)
        for (int rep = 0; rep < 60; ++rep) {
            const uint32_t n = 1 + rng() % 1500, n_groups = 1 + rng() % 200;
            const uint32_t limit = rep % 7 == 0 ? 1024 : 1 + rng() % 40, group_size = rep % 5 == 0 ? 1 + rng() % 100 : 1 + rng() % 6;
            one_case(rng, n, n_groups, limit, std::min<uint32_t>(group_size, 65536 / limit), layout);
            ++cases;
        }
    printf("group_logic_check: %u cases ok\n", cases);
    return 0;
}
