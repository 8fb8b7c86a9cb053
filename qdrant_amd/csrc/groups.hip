// groups.hip — grouped search on the device (qmx_group_search, api_groups.hip): "the best `limit` groups by a payload key, `group_size` hits each" =
// what `group_by` (lib/collection/src/grouping/group_by.rs:263-356) converges to when its searches are exact and its request budget suffices
// (DESIGN 3.12).  The reference's backend only returns a top-k, so its GroupByDriver (lib/shard/src/grouping/driver.rs) repeats whole searches under a
// growing filter and feeds GroupsAggregator (aggregator.rs); here the ranked stream stays on the device and is consumed in pages of 64 hits:
//
//   group_aggregate_kernel : one wave per query walks a page in rank order and fills the query's slots {key, count, hits}
//                            (GroupsAggregator::add_points, aggregator.rs:57-105; array values: :63-85)
//   group_select_kernel    : the fallback's next page - the 64 best keys of a query's SCORE ROW among the rows under its bound that can still
//                            contribute (the driver's `except_on` / `match_on` key filters and its `has_id` exclusion, in <= limit keys of state)
//   group_final_kernel     : slots ordered by their best hit (ties: ascending key index), written out
//
// The integer logic the three share with the host (and with the sanitized host check) is group_logic.hpp.
#include "kernels.hpp"
#include "group_logic.hpp"

namespace qmx {

static_assert(GROUP_NONE == QMX_GROUP_NONE, "the empty table entry is the no-key value");
static_assert(GROUP_TABLE >= 2 * GROUP_MAX_LIMIT, "the key table is at most half full");
static_assert(GROUP_PAGE == WAVE, "a page is one wave list");

// ---- the key column at create: values in range, CSR offsets that never decrease -----------------------------------------------------------
__global__ __launch_bounds__(256) void group_keys_check_kernel(const uint32_t *keys, uint64_t n_keys, uint32_t n_distinct, const uint64_t *offsets,
                                                               uint64_t n_points, uint32_t *bad) {
    uint32_t flags = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_keys; i += (uint64_t)gridDim.x * 256) {
        const uint32_t k = keys[i];
        if (k != GROUP_NONE && k >= n_distinct) flags |= 1u;
    }
    if (offsets)
        for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n_points; p += (uint64_t)gridDim.x * 256)
            if (offsets[p] > offsets[p + 1]) flags |= 2u;
    if (flags) atomicOr(bad, flags);
}

// ---- the aggregator ---------------------------------------------------------------------------------------------------------------------------
// One wave per query.  The query's slot keys, counts and the point each slot took last sit in LDS for the page; the hits themselves go straight to
// HBM.  Everything below is wave-uniform (the hit, its key, the slot found), lane 0 writes.
// A point's keys are taken in ASCENDING key order whatever order the column lists them in, and a repeated key once: the next key is the smallest one
// above the previous.  That pins which of a multi-valued point's groups open when slots run out (the contract: ties by ascending key index).
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(WAVE) void group_aggregate_kernel(GroupKeysDev gk, GroupState gs, const qmx_scored_point *pages, const uint32_t *counts,
                                                               const uint32_t *list, int has_threshold, float threshold) {
    __shared__ uint32_t sh_key[GROUP_MAX_LIMIT], sh_cnt[GROUP_MAX_LIMIT], sh_last[GROUP_MAX_LIMIT];
    const uint32_t q = list ? list[blockIdx.x] : blockIdx.x;
    const int lane = threadIdx.x;
    if (gs.bound[q] == 0) return;      // done by an earlier page
    const uint32_t limit = gs.limit, group_size = gs.group_size;
    uint32_t n_slots = gs.n_slots[q], n_full = gs.n_full[q];
    uint32_t *slot_key = gs.slot_key + (uint64_t)q * limit, *slot_cnt = gs.slot_cnt + (uint64_t)q * limit;
    uint64_t *slot_hits = gs.slot_hits + (uint64_t)q * limit * group_size;
    for (uint32_t i = lane; i < n_slots; i += WAVE) {
        sh_key[i] = slot_key[i];
        sh_cnt[i] = slot_cnt[i];
        sh_last[i] = 0xFFFFFFFFu;      // (an earlier page's points are all above this page's: none repeats)
    }
    __syncthreads();
    const uint32_t page_hits = counts[q] < GROUP_PAGE ? counts[q] : GROUP_PAGE;
    const qmx_scored_point *page = pages + (uint64_t)q * GROUP_PAGE;
    bool below = false;
    uint64_t last_key = 0;
    for (uint32_t h = 0; h < page_hits && n_full < limit; ++h) {
        const qmx_scored_point p = page[h];
        if (has_threshold && p.score < threshold) {      // hits under the threshold do not exist, and the stream only descends
            below = true;
            break;
        }
        last_key = make_key(p.score, p.idx);
        if (p.idx >= gk.n_points) continue;
        const uint64_t kb = gk.offsets ? gk.offsets[p.idx] : p.idx, ke = gk.offsets ? gk.offsets[p.idx + 1] : (uint64_t)p.idx + 1;
        uint64_t prev = 0;      // key + 1 of the key taken last
        for (;;) {
            uint32_t key = GROUP_NONE;
            if (ke - kb == 1) {
                key = prev ? GROUP_NONE : gk.keys[kb];
            } else {
                for (uint64_t j = kb + lane; j < ke; j += WAVE) {
                    const uint32_t k = gk.keys[j];
                    if (k != GROUP_NONE && (uint64_t)k + 1 > prev && k < key) key = k;
                }
                key = wave_min_u32(key);
            }
            if (key == GROUP_NONE) break;
            prev = (uint64_t)key + 1;
            int32_t found = -1;
            for (uint32_t base = 0; base < n_slots; base += WAVE) {
                const uint32_t i = base + lane;
                const uint64_t m = __ballot(i < n_slots && sh_key[i] == key);
                if (m) {
                    found = (int32_t)(base + __builtin_ctzll(m));
                    break;
                }
            }
            const GroupStep s = group_step(found, found >= 0 ? sh_cnt[found] : 0u, found >= 0 ? sh_last[found] : 0u, p.idx, n_slots, limit, group_size);
            if (s.slot >= 0) {
                if (lane == 0) {
                    sh_key[s.slot] = key;
                    sh_cnt[s.slot] = s.pos + 1;
                    sh_last[s.slot] = p.idx;
                    slot_hits[(uint64_t)s.slot * group_size + s.pos] = last_key;
                }
                n_slots += s.opened ? 1u : 0u;
                n_full += s.filled ? 1u : 0u;
                __syncthreads();      // (one wave: orders lane 0's LDS writes before the next lookup)
            }
        }
    }
    for (uint32_t i = lane; i < n_slots; i += WAVE) {
        slot_key[i] = sh_key[i];
        slot_cnt[i] = sh_cnt[i];
    }
    if (lane == 0) {
        gs.n_slots[q] = n_slots;
        gs.n_full[q] = n_full;
        atomicAdd(&gs.stats->pages, 1ull);
        const bool done = group_done(n_full, limit, page_hits, GROUP_PAGE, below);
        // (a page cut short by n_full == limit is done; otherwise every hit of a full page was walked and last_key is its last)
        gs.bound[q] = done ? 0ull : last_key;
        if (!done) atomicAdd(&gs.stats->unfinished, 1u);
    }
}

// ---- the selection of a fallback page ---------------------------------------------------------------------------------------------------------
// grid (blocks, packed queries): block (b, u) walks its grid-stride share of the score row of query list[u] and leaves the 64 best eligible keys under
// the query's bound in partial[b][u][0..64); merge_keys_kernel (topk_merge.hip) merges the blocks' lists into the page.
// 8 bytes per row and query: the f32 score and the row's key index, both as 16-byte loads where the candidates are the rows themselves and each
// carries one key (VEC); candidate lists and CSR keys take one row per lane.
// The key table (group_logic.hpp) is read once per row at a hashed address: lanes spread over the 32 banks of ds_read_b32 at random, a few LDS cycles
// per lookup beside the two global loads - the kernel stays a stream over the score row.
constexpr int GS_BLOCK = 256;
constexpr int GS_NW = GS_BLOCK / WAVE;

template <bool VEC>
__global__ __launch_bounds__(GS_BLOCK) void group_select_kernel(GroupKeysDev gk, GroupState gs, const float *scores, uint64_t stride, uint64_t n_cand,
                                                                const uint32_t *ids, DeletedView del, const uint32_t *list, uint64_t *partial) {
    __shared__ uint32_t table[GROUP_TABLE];
    __shared__ uint64_t sh[GS_NW][WAVE];
    const uint32_t u = blockIdx.y, q = list[u];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t *out = partial + ((uint64_t)blockIdx.x * gridDim.y + u) * GROUP_PAGE;
    const uint64_t bound = gs.bound[q];
    if (bound == 0) {      // done: an empty list
        if (threadIdx.x < GROUP_PAGE) out[threadIdx.x] = 0;
        return;
    }
    const uint32_t n_slots = gs.n_slots[q];
    const bool filling = group_filling(n_slots, gs.limit);
    for (uint32_t i = threadIdx.x; i < GROUP_TABLE; i += GS_BLOCK) table[i] = GROUP_NONE;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_slots; i += GS_BLOCK) {
        if (!group_slot_in_table(gs.slot_cnt[(uint64_t)q * gs.limit + i], gs.group_size, filling)) continue;
        const uint32_t key = gs.slot_key[(uint64_t)q * gs.limit + i];
        uint32_t h = group_hash(key);
        for (;;) {
            const uint32_t old = atomicCAS(&table[h], GROUP_NONE, key);
            if (old == GROUP_NONE || old == key) break;
            h = (h + 1) & (GROUP_TABLE - 1);
        }
    }
    __syncthreads();
    const float *row = scores + (uint64_t)u * stride;
    constexpr int R = VEC ? 4 : 1;
    uint64_t list64 = 0;
    for (uint64_t base = ((uint64_t)blockIdx.x * GS_BLOCK + (uint64_t)wave * WAVE) * R; base < n_cand; base += (uint64_t)gridDim.x * GS_BLOCK * R) {
        uint64_t key[R];
        if (VEC) {
            // (n_cand <= n_points; the score rows and the key column are padded to whole 16-byte pieces)
            const uint64_t c = base + (uint64_t)lane * 4;
            const bool in = c < n_cand;
            const uint64_t cc = in ? c : 0;
            const float4 s4 = *reinterpret_cast<const float4 *>(row + cc);
            const uint4 k4 = *reinterpret_cast<const uint4 *>(gk.keys + cc);
            const float s[4] = {s4.x, s4.y, s4.z, s4.w};
            const uint32_t k[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t id = (uint32_t)(cc + e);
                const bool ok = in && c + e < n_cand && del.live(id) && group_key_eligible(table, k[e], filling);
                const uint64_t kk = make_key(s[e], id);
                key[e] = kk & (0ull - (uint64_t)(ok && kk < bound));
            }
        } else {
            const uint64_t c = base + lane;
            const bool in = c < n_cand;
            const uint64_t cc = in ? c : 0;
            const uint32_t id = ids ? ids[cc] : (uint32_t)cc;
            bool ok = in && id < gk.n_points && del.live(id);
            bool eligible = false;
            if (ok) {
                const uint64_t kb = gk.offsets ? gk.offsets[id] : id, ke = gk.offsets ? gk.offsets[id + 1] : (uint64_t)id + 1;
                for (uint64_t j = kb; j < ke; ++j) eligible = eligible || group_key_eligible(table, gk.keys[j], filling);
            }
            const uint64_t kk = make_key(row[cc], id);
            key[0] = kk & (0ull - (uint64_t)(ok && eligible && kk < bound));
        }
#pragma unroll
        for (int e = 0; e < R; ++e) {
            if (key[e] <= readlane_u64(list64, GROUP_PAGE - 1)) key[e] = 0;
            uint64_t m = __ballot(key[e] != 0);
            while (m) {
                const int src = __builtin_ctzll(m);
                m &= m - 1;
                const uint64_t nk = readlane_u64(key[e], src);
                if (nk > readlane_u64(list64, GROUP_PAGE - 1)) wave_list_insert(list64, nk, lane);
            }
        }
    }
    sh[wave][lane] = list64;
    __syncthreads();
    if (wave == 0) {
        uint64_t merged = sh[0][lane];
        for (int w = 1; w < GS_NW; ++w) wave_offer(merged, sh[w][lane], GROUP_PAGE, lane);
        out[lane] = merged;
    }
}

// ---- the result ---------------------------------------------------------------------------------------------------------------------------------
// One block per query: slot i goes to rank = the number of slots whose best hit is better, or the same point under a lower key index.
constexpr int GF_BLOCK = 256;
__global__ __launch_bounds__(GF_BLOCK) void group_final_kernel(GroupState gs, uint32_t *out_keys, uint32_t *out_sizes, qmx_scored_point *out_hits,
                                                               uint32_t *out_n_groups) {
    __shared__ uint64_t sh_best[GROUP_MAX_LIMIT];
    __shared__ uint32_t sh_key[GROUP_MAX_LIMIT];
    const uint32_t q = blockIdx.x, limit = gs.limit, group_size = gs.group_size;
    const uint32_t n_slots = gs.n_slots[q];
    const uint64_t *slot_hits = gs.slot_hits + (uint64_t)q * limit * group_size;
    for (uint32_t i = threadIdx.x; i < n_slots; i += GF_BLOCK) {
        sh_best[i] = slot_hits[(uint64_t)i * group_size];
        sh_key[i] = gs.slot_key[(uint64_t)q * limit + i];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < limit; i += GF_BLOCK) {
        if (i >= n_slots) {      // ranks n_slots .. limit stay empty
            out_keys[(uint64_t)q * limit + i] = GROUP_NONE;
            out_sizes[(uint64_t)q * limit + i] = 0;
            for (uint32_t j = 0; j < group_size; ++j) out_hits[((uint64_t)q * limit + i) * group_size + j] = qmx_scored_point{0u, 0.0f};
            continue;
        }
        const uint64_t best = sh_best[i];
        const uint32_t key = sh_key[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n_slots; ++j) rank += (sh_best[j] > best || (sh_best[j] == best && sh_key[j] < key)) ? 1u : 0u;
        const uint32_t cnt = gs.slot_cnt[(uint64_t)q * limit + i];
        out_keys[(uint64_t)q * limit + rank] = key;
        out_sizes[(uint64_t)q * limit + rank] = cnt;
        qmx_scored_point *dst = out_hits + ((uint64_t)q * limit + rank) * group_size;
        for (uint32_t j = 0; j < group_size; ++j) {
            const uint64_t k = j < cnt ? slot_hits[(uint64_t)i * group_size + j] : 0ull;
            dst[j] = j < cnt ? qmx_scored_point{key_idx(k), key_score(k)} : qmx_scored_point{0u, 0.0f};
        }
    }
    if (threadIdx.x == 0) out_n_groups[q] = n_slots;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------
int32_t launch_group_keys_check(hipStream_t st, const uint32_t *keys, uint64_t n_keys, uint32_t n_distinct, const uint64_t *offsets, uint64_t n_points,
                                uint32_t *bad) {
    const uint64_t work = n_keys > n_points ? n_keys : n_points;
    if (work == 0) return QMX_OK;
    const uint32_t grid = (uint32_t)(work / 256 + 1 < 2048 ? work / 256 + 1 : 2048);
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(group_keys_check_kernel, dim3(grid), dim3(256), 0, st, keys, n_keys, n_distinct, offsets, n_points, bad);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_group_aggregate(hipStream_t st, const GroupKeysDev &gk, const GroupState &gs, const qmx_scored_point *pages, const uint32_t *counts,
                               const uint32_t *list, uint32_t n_queries, const float *threshold) {
    if (n_queries == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(group_aggregate_kernel, dim3(n_queries), dim3(WAVE), 0, st, gk, gs, pages, counts, list, threshold ? 1 : 0,
                       threshold ? *threshold : 0.0f);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_group_select(hipStream_t st, const GroupKeysDev &gk, const GroupState &gs, const float *scores, uint64_t stride, uint64_t n_cand,
                            const uint32_t *ids, const DeletedView &del, const uint32_t *list, uint32_t n_queries, uint32_t blocks, uint64_t *partial) {
    if (n_queries == 0 || blocks == 0) return QMX_OK;
    QMX_REQUIRE(n_queries <= 65535, QMX_ERR_NOT_SUPPORTED, "%u queries in one selection launch", n_queries);
    // 16-byte loads: the candidates are the rows themselves, one key each, and both arrays are made of whole pieces
    const bool vec = !ids && !gk.offsets && stride % 4 == 0 && ((uintptr_t)scores % 16) == 0 && ((uintptr_t)gk.keys % 16) == 0 && n_cand <= gk.n_points;
    ::qmx::clear_stale_error();
    if (vec) {
        QMX_NOTE_KERNEL(group_select_kernel<true>);
        hipLaunchKernelGGL(group_select_kernel<true>, dim3(blocks, n_queries), dim3(GS_BLOCK), 0, st, gk, gs, scores, stride, n_cand, ids, del, list, partial);
    } else {
        QMX_NOTE_KERNEL(group_select_kernel<false>);
        hipLaunchKernelGGL(group_select_kernel<false>, dim3(blocks, n_queries), dim3(GS_BLOCK), 0, st, gk, gs, scores, stride, n_cand, ids, del, list, partial);
    }
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_group_final(hipStream_t st, const GroupState &gs, uint32_t nq, uint32_t *out_keys, uint32_t *out_sizes, qmx_scored_point *out_hits,
                           uint32_t *out_n_groups) {
    if (nq == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(group_final_kernel, dim3(nq), dim3(GF_BLOCK), 0, st, gs, out_keys, out_sizes, out_hits, out_n_groups);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

}  // namespace qmx
