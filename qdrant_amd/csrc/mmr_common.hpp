// mmr_common.hpp — the selection machinery of maximal marginal relevance that mmr.hip (dense rows) and sparse_mmr.hip (sparse rows) share: the
// per-candidate arrays in LDS, the id check, unique-by-id, the order array (`remaining_indices`), OrderedFloat keys, the work-group arg-max and the
// pick with its swap_remove.  What differs between the two kernels is only where relevance(c) and sim(c, s) come from.
//
//  mmr_from_points_with_vector   lib/shard/src/query/mmr/mod.rs:42-100    (unique by id, < 2 candidates returned as they are)
//  maximal_marginal_relevance    lib/shard/src/query/mmr/mod.rs:198-279   (first pick by relevance, then lambda * rel - (1 - lambda) * max sim)
//
// Ties are the reference's: `max_by_key` returns the LAST maximal element of the iteration, i.e. "greatest score, then greatest position in the
// current order"; the running maximum takes a later equal similarity (>=); comparisons are OrderedFloat's (NaN greatest, -0.0 == 0.0).
#pragma once
#include "kernels.hpp"

namespace qmx {

constexpr int MMR_BLOCK = 1024;
constexpr int MMR_NW = MMR_BLOCK / WAVE;
constexpr uint32_t MMR_CAND_BYTES = 20;      // LDS per candidate: the five arrays of MmrLists

// OrderedFloat as one u32 (lib/common/common/src/types.rs: NaN greatest, -0.0 == 0.0)
__device__ __forceinline__ uint32_t ordered_float(float s) { return score_to_ord(s == 0.0f ? 0.0f : s); }

// block-wide maximum of one u64 key per thread (0 = none), returned to every thread
__device__ __forceinline__ uint64_t mmr_block_max(uint64_t key, uint64_t *s_best) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor((int)(uint32_t)key, off, 64), hi = __shfl_xor((int)(uint32_t)(key >> 32), off, 64);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        key = other > key ? other : key;
    }
    __syncthreads();      // the previous round's readers are done with s_best
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = key;
    __syncthreads();
    uint64_t best = s_best[0];
#pragma unroll
    for (int w = 1; w < MMR_NW; ++w) best = s_best[w] > best ? s_best[w] : best;
    return best;
}

// the per-candidate arrays, S = the stride rounded up to 4 entries each, one behind the other from the start of the dynamic LDS (a kernel fills the
// five pointers itself and passes the struct by value: through a factory function or a reference the dense kernel's u8 instantiations came out
// one VGPR above their earlier allocation)
struct MmrLists {
    uint32_t *id;       // [S] id of every input position
    uint32_t *src;      // [S] input position of unique candidate c
    uint32_t *order;    // [S] remaining_indices: candidate at every position of the current order
    float *rel;         // [S] relevance of candidate c
    float *max;         // [S] max_similarity_to_selected of candidate c
};
// the ids of the request's candidates into LDS; false (for every thread) when one lies past the segment's rows: no row is read through an id the
// segment does not hold, the request is dropped and the caller gets QMX_ERR_OUT_OF_BOUNDS
__device__ __forceinline__ bool mmr_load_ids(const MmrLists l, const qmx_scored_point *cand, uint32_t cnt, uint64_t n_rows, uint32_t limit, qmx_scored_point *out,
                                             uint32_t *out_count, int *err_flag, uint32_t *s_bad) {
    const uint32_t tid = threadIdx.x;
    if (tid == 0) *s_bad = 0;
    __syncthreads();
    for (uint32_t j = tid; j < cnt; j += MMR_BLOCK) {
        const uint32_t id = cand[j].idx;
        l.id[j] = id;
        if (id >= n_rows) *s_bad = 1;
    }
    __syncthreads();
    if (*s_bad) {
        if (tid == 0) {
            *err_flag = 1;
            *out_count = 0;
        }
        for (uint32_t i = tid; i < limit; i += MMR_BLOCK) out[i] = qmx_scored_point{0u, 0.0f};
        return false;
    }
    return true;
}

// unique_by(|p| p.id): the first occurrence stays, the order is kept; returns the number of unique candidates (l.src filled, *s_n as scratch)
__device__ __forceinline__ uint32_t mmr_unique(const MmrLists l, uint32_t cnt, uint32_t *s_n) {
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63;
    for (uint32_t j = tid; j < cnt; j += MMR_BLOCK) {
        const uint32_t id = l.id[j];
        bool dup = false;
        for (uint32_t e = 0; e < j; ++e) dup = dup || (l.id[e] == id);
        l.order[j] = dup ? 0u : 1u;
    }
    __syncthreads();
    if (tid < 64) {
        uint32_t running = 0;
        for (uint32_t base = 0; base < cnt; base += 64) {
            const uint32_t j = base + (uint32_t)lane;
            const bool keep = j < cnt && l.order[j] != 0u;
            const uint64_t m = __ballot(keep);
            if (keep) l.src[running + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = j;
            running += (uint32_t)__popcll(m);
        }
        if (lane == 0) *s_n = running;
    }
    __syncthreads();
    return *s_n;
}

// the arg-max key of the candidate at position p of the current order
__device__ __forceinline__ uint64_t mmr_key(float score, uint32_t p) { return ((uint64_t)ordered_float(score) << 32) | p; }

// folds sim(c, selected last) into candidate c's running maximum and returns the key of its MMR score at position p
__device__ __forceinline__ uint64_t mmr_fold(const MmrLists l, uint32_t c, uint32_t p, float sim, bool first, float lambda, float one_minus) {
    const float m = first || ordered_float(sim) >= ordered_float(l.max[c]) ? sim : l.max[c];
    l.max[c] = m;
    const float mmr = lambda * l.rel[c] - one_minus * m;
    return mmr_key(mmr, p);
}

// thread 0 takes the winner out of the order - swap_remove: the last element moves into the freed slot - and writes it with its INPUT score
// (candidates[idx].clone()); every thread leaves through the barrier
__device__ __forceinline__ void mmr_pick(const MmrLists l, uint64_t best, uint32_t R, const qmx_scored_point *cand, qmx_scored_point *out, uint32_t n_sel,
                                         uint32_t *s_sel) {
    if (threadIdx.x == 0) {
        const uint32_t p = (uint32_t)best;
        const uint32_t c = l.order[p];
        l.order[p] = l.order[R - 1];
        *s_sel = c;
        out[n_sel] = cand[l.src[c]];
    }
    __syncthreads();
}

}  // namespace qmx
