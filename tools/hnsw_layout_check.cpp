// hnsw_layout_check.cpp — a stand-alone host run of the walk's LDS layout (qdrant_amd/csrc/hnsw_layout.hpp) over the combinations a launch can have:
// every region starts on a 16-byte boundary, the regions follow one another without overlap in the documented order, and the offsets and the total
// are the sums the kernel, the launcher and the occupancy query used to spell out each for itself (written out longhand below).  Meant for the
// sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iqdrant_amd/csrc tools/hnsw_layout_check.cpp -o /tmp/hnsw_layout_check
//   /tmp/hnsw_layout_check
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hnsw_layout.hpp"

using namespace qmx;

namespace {

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

size_t pad16(size_t v) { return (v + 15) / 16 * 16; }

struct Region {
    size_t start, bytes;
};

uint64_t check_one(int E, bool QLDS, uint32_t hop_cap, uint32_t acorn, uint32_t explore_cap, uint32_t lds_query_bytes, uint32_t ef, uint32_t vis_lds,
                   bool has_pq8, uint32_t pq8_stride) {
    const HnswLds l = hnsw_lds_layout(E, QLDS, hop_cap, acorn, explore_cap, lds_query_bytes, ef, vis_lds, has_pq8, pq8_stride);
    // the sums as they stood in the launcher ...
    const size_t longhand = 8 * (size_t)hop_cap + hnsw_acorn_lds(acorn, explore_cap) + (QLDS ? ((size_t)lds_query_bytes + 15) / 16 * 16 : 0) +
                            (E <= 0 ? hnsw_beam_lds(ef) : 0) + (E == HNSW_E_REF ? (size_t)HNSW_REF_CAND_LDS * 8 : 0) + vis_lds + (has_pq8 ? pq8_stride : 0);
    CHECK(l.total == longhand);
    // ... in the occupancy query (hop_lds + the padded entry) ...
    const size_t hop_lds = E == HNSW_E_REF ? 8 * (size_t)hop_cap + hnsw_acorn_lds(acorn, explore_cap) + hnsw_beam_lds(ef) + (size_t)HNSW_REF_CAND_LDS * 8 + vis_lds + (has_pq8 ? pq8_stride : 0)
                           : E == 0        ? 8 * (size_t)hop_cap + hnsw_acorn_lds(acorn, explore_cap) + hnsw_beam_lds(ef) + vis_lds + (has_pq8 ? pq8_stride : 0)
                                           : 8 * (size_t)hop_cap + hnsw_acorn_lds(acorn, explore_cap) + vis_lds + (has_pq8 ? pq8_stride : 0);
    CHECK(l.total == hop_lds + (QLDS ? ((size_t)lds_query_bytes + 15) / 16 * 16 : 0));
    // ... and in the kernel's carve-up
    CHECK(l.hop_ids == 0 && l.hop_scores == 4 * (size_t)hop_cap && l.explore == 8 * (size_t)hop_cap);
    CHECK(hnsw_hop_lds(hop_cap) == l.explore - l.hop_ids);                    // what the walk adds to hop_ids to find ACORN's explore list
    if (E == HNSW_E_REF) CHECK(hnsw_beam_lds(ef) == l.ref_cands - l.beam);    // ... and to `nearest` to find the reference candidates
    const size_t q_lds = 8 * (size_t)hop_cap + hnsw_acorn_lds(acorn, explore_cap);
    const size_t beam_lds = q_lds + (QLDS ? ((size_t)lds_query_bytes + 15) / 16 * 16 : 0);
    CHECK(l.query == q_lds && l.beam == beam_lds);
    CHECK(l.ref_cands == beam_lds + (E <= 0 ? hnsw_beam_lds(ef) : 0));
    CHECK(l.visited == beam_lds + (E <= 0 ? hnsw_beam_lds(ef) : 0) + (E == HNSW_E_REF ? (size_t)HNSW_REF_CAND_LDS * 8 : 0));
    if (E != HNSW_E_REF) CHECK(l.pq8 == beam_lds + (E <= 0 ? hnsw_beam_lds(ef) : 0) + vis_lds);      // (the reference-heap mode never carries the image)
    // what each region holds, in the documented order: aligned, back to back, inside the total
    const Region regions[] = {
        {l.hop_ids, 4 * (size_t)hop_cap},
        {l.hop_scores, 4 * (size_t)hop_cap},
        {l.explore, acorn ? 4 * (size_t)(explore_cap < 64 ? 64 : explore_cap) : 0},                      // explore_cap ids, 64 at least (rounded up to whole passes)
        {l.query, QLDS ? (size_t)lds_query_bytes : 0},
        {l.beam, E <= 0 ? (size_t)ef * 9 : 0},                                                          // ef keys + ef flag bytes (`nearest`: ef entries of 8)
        {l.ref_cands, E == HNSW_E_REF ? (size_t)HNSW_REF_CAND_LDS * 8 : 0},
        {l.visited, vis_lds},
        {l.pq8, has_pq8 ? (size_t)pq8_stride : 0},
    };
    size_t end = 0;
    for (const Region &r : regions) {
        CHECK(r.start % 16 == 0);
        CHECK(r.start >= end);                  // no overlap with what lies before
        CHECK(r.start - end < 64 * 4 + 16);     // ... and no hole beyond padding (the explore list is rounded up to whole 64-lane passes)
        end = r.start + r.bytes;
    }
    CHECK(end <= l.total && pad16(end) == pad16(l.total));
    CHECK(l.total % 16 == 0);
    return l.total;
}

}  // namespace

int main() {
    uint64_t n = 0, sum = 0;
    const std::vector<uint32_t> hop_caps = {64, 320, 1088, 4160};                         // 64; m0 (m0 + 1) rounded up to 64 for ACORN, capped
    const std::vector<uint32_t> entries = {0, 16, 32, 48, 100, 1000, 4096, 16384, 16400, 32 * 1024, 64 * 1024 + 16, 96 * 1024};
    const std::vector<uint32_t> efs = {1, 2, 63, 64, 65, 128, 129, 512, 513, 600, 1000, 4095, 4096};
    for (int E : {HNSW_E_REF, 0, 2, 8})
        for (bool QLDS : {false, true})
            for (uint32_t acorn : {0u, 1u})
                for (uint32_t hop_cap : hop_caps)
                    for (uint32_t explore_cap : {1u, 32u, 64u, 65u, 96u, 128u, 1000u, 8192u})
                        for (uint32_t q : entries)
                            for (uint32_t ef : efs)
                                for (uint32_t vis_lds : {0u, 16384u})
                                    for (uint32_t pq8_stride : {0u, 32u + 256u, 32u + 96u * 256u, 32u + 128u * 256u}) {
                                        sum += check_one(E, QLDS, hop_cap, acorn, explore_cap, q, ef, vis_lds, pq8_stride != 0, pq8_stride);
                                        ++n;
                                    }
    // a stride that the launch does not use takes no room
    CHECK(hnsw_lds_layout(2, true, 64, 0, 0, 512, 64, 16384, false, 4096).total == 512 + 512 + 16384);
    CHECK(hnsw_lds_layout(HNSW_E_REF, true, 64, 0, 0, 512, 64, 0, false, 0).total == 512 + 512 + 576 + 8192);
    CHECK(hnsw_lds_layout(0, true, 64, 1, 96, 132, 600, 0, false, 0).total == 512 + 4 * 128 + 144 + 5408);
    CHECK(hnsw_beam_lds(600) == 5408 && hnsw_acorn_lds(1, 8192) == 32768 && hnsw_acorn_lds(0, 8192) == 0);
    printf("hnsw_layout_check: ok (%llu combinations, %llu bytes in all)\n", (unsigned long long)n, (unsigned long long)sum);
    return 0;
}
