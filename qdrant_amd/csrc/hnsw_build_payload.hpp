// hnsw_build_payload.hpp — the payload-block sub-graphs of an HNSW build on the device (qmx_hnsw_build_payload_links).
//
// For every payload block of an indexed field the reference builds a second, FLAT graph over the block's points only
// (hnsw/build.rs:408-531, build_filtered_graph :631-716: GraphLayersBuilder::new_with_params(total, payload_m, ef_construct, 1, ..) - every point on
// level 0, capacity payload_m0, the block's first point its entry point) and appends its links to the main graph's level 0 (merge_from_other,
// graph_layers_builder.rs:346-381).  Blocks share nothing, so all of them are built here side by side: the per-point work is the main build's
// (hnsw_build.hpp: phase 1 = search_on_level(ef_construct) + heuristic, phase 2 = publish + back links under the neighbour's lock), over a WORK LIST
// instead of an id range.  An item = (block, position in block); one launch pair inserts the next batch of every block that still has points.
//
// Storage is block-local: a block's points occupy the membership slots blk_off[b] .. blk_off[b + 1] (live points only, insertion order); link rows,
// counts and locks are indexed by slot, links are POSITIONS within the block (the id of position i of block b = points[blk_off[b] + i]), and the
// visited bitmap of an insertion search has one bit per position of the largest block.  These are kernels of their own: the instantiations of
// hnsw_build.hpp are what they were.
#pragma once
#include "hnsw_build.hpp"
#include "hnsw_payload_args.hpp"

namespace qmx {

// heuristic_fill over positions of one block: pts[pos] is the point id (the rows scored)
template <class H>
__device__ __forceinline__ uint32_t payload_heuristic_fill(const ScanArgs &a, const uint32_t *pts, const uint32_t *cand_pos, const float *cand_scores, uint32_t n_cand,
                                                           uint32_t lm, uint32_t *sel_pos, float *sel_scores, uint32_t *hop_ids, float *hop_scores, int lane) {
    uint32_t n_sel = 0;
    for (uint32_t c = 0; c < n_cand && n_sel < lm; ++c) {
        const uint32_t cpos = cand_pos[c];
        const uint32_t cid = pts[cpos];
        const float cs = cand_scores[c];
        bool skip = false;
        for (uint32_t base = 0; base < n_sel && !skip; base += 64) {
            const uint32_t k = n_sel - base < 64 ? n_sel - base : 64;
            __syncthreads();
            if ((uint32_t)lane < k) hop_ids[lane] = pts[sel_pos[base + lane]];
            hop_score<H>(query_args<H>(a, cid), stored_query<H>(a, cid), hop_ids, hop_scores, k, lane);   // score(candidate, kept link)
            const bool bad = (uint32_t)lane < k && hop_scores[lane] > cs;
            skip = __ballot(bad) != 0;
        }
        if (skip) continue;
        __syncthreads();
        if (lane == 0) {
            sel_pos[n_sel] = cpos;
            sel_scores[n_sel] = cs;
        }
        ++n_sel;
    }
    __syncthreads();
    return n_sel;
}

constexpr uint32_t HNSW_PAYLOAD_LDS_HEAD = 768;     // hop ids, hop scores, hop positions: 64 entries each

// ---- phase 1: one wavefront per item, every block graph READ-ONLY ---------------------------------------------------------------------------------------
template <class H, class HI, int E>
__global__ __launch_bounds__(64) void hnsw_payload_search_kernel(const ScanArgs a0, const HnswPayloadArgs h) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    const uint32_t ccap = hnsw_build_cand_cap(E, h.ef_construct);
    uint32_t *hop_ids = reinterpret_cast<uint32_t *>(smem);
    float *hop_scores = reinterpret_cast<float *>(smem + 256);
    uint32_t *hop_pos = reinterpret_cast<uint32_t *>(smem + 512);
    uint32_t *cand_pos = reinterpret_cast<uint32_t *>(smem + HNSW_PAYLOAD_LDS_HEAD);                     // [ccap]
    float *cand_scores = reinterpret_cast<float *>(smem + HNSW_PAYLOAD_LDS_HEAD + 4 * (size_t)ccap);
    uint32_t *sel_pos = reinterpret_cast<uint32_t *>(smem + HNSW_PAYLOAD_LDS_HEAD + 8 * (size_t)ccap);   // [HNSW_BUILD_MAX_M0]
    float *sel_scores = reinterpret_cast<float *>(smem + HNSW_PAYLOAD_LDS_HEAD + 8 * (size_t)ccap + 4 * HNSW_BUILD_MAX_M0);
    unsigned char *q_lds = smem + HNSW_PAYLOAD_LDS_HEAD + 8 * (size_t)ccap + 8 * HNSW_BUILD_MAX_M0;
    unsigned char *beam_lds = q_lds + ((size_t)h.lds_query_bytes + 15) / 16 * 16;
    uint32_t *vis = h.visited + (uint64_t)blockIdx.x * h.vis_words;
    uint32_t *vlog = h.vis_log + (uint64_t)blockIdx.x * h.log_cap;
    const unsigned char *rows = reinterpret_cast<const unsigned char *>(a0.rows);
    const uint32_t ef = h.ef_construct;

    auto next_item = [&](uint32_t bi) -> uint32_t {      // (as the main build: the items of a round are handed out one at a time)
        uint32_t v = 0;
        if (lane == 0) v = atomicAdd(&h.next[0], 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    };
    for (uint32_t bi = blockIdx.x; bi < h.count; bi = next_item(bi)) {
        const uint32_t blk = h.item_block[h.first_item + bi];
        const uint32_t pos = h.item_pos[h.first_item + bi];
        const uint64_t slot0 = h.blk_off[blk];
        const uint32_t blk_n = (uint32_t)(h.blk_off[blk + 1] - slot0);
        const uint32_t *pts = h.points + slot0;
        const uint32_t p = pts[pos];
        const ScanArgs a = query_args<H>(a0, p);     // the new point is the query of every score below
        if (lane == 0) h.sel_cnt[bi] = 0;

        // the query entry of the new point (hnsw_build.hpp): made from its original vector before this launch, or its own stored row staged in LDS
        const unsigned char *qp = q_lds;
        __syncthreads();
        if (h.batch_queries && h.lds_query_bytes) {
            const unsigned char *src = h.batch_queries + (uint64_t)bi * h.batch_q_stride;
            const uint32_t q_bytes = h.lds_query_bytes < h.batch_q_stride ? h.lds_query_bytes : (uint32_t)h.batch_q_stride;
            for (uint32_t i = (uint32_t)lane * 16; i < q_bytes; i += 64 * 16)
                *reinterpret_cast<uint4 *>(q_lds + i) = *reinterpret_cast<const uint4 *>(src + i);
        } else if (h.batch_queries) {
            qp = h.batch_queries + (uint64_t)bi * h.batch_q_stride;
        } else {
            const unsigned char *src = rows + (uint64_t)p * a.row_stride;
            for (uint32_t i = (uint32_t)lane * 16; i < h.lds_query_bytes; i += 64 * 16) {
                uint4 v = make_uint4(0, 0, 0, 0);
                if (i + 16 <= h.row_bytes) v = *reinterpret_cast<const uint4 *>(src + i);
                else if (i < h.row_bytes) {
                    unsigned char tmp[16];
                    for (uint32_t b = 0; b < 16; ++b) tmp[b] = i + b < h.row_bytes ? src[i + b] : 0;
                    v = *reinterpret_cast<const uint4 *>(tmp);
                }
                *reinterpret_cast<uint4 *>(q_lds + i) = v;
            }
        }
        __syncthreads();

        // ---- the block's entry point: its first point, on level 0 like every point (graph_layers_builder.rs:441-447: score_internal(p, entry)) ----
        uint32_t cur_pos = 0;
        float cur_score;
        {
            if (lane == 0) hop_ids[0] = pts[0];
            if (is_asymmetric<HI>::value)
                hop_score<HI>(query_args<HI>(a0, p), stored_query<HI>(a0, p), hop_ids, hop_scores, 1, lane);
            else
                hop_score<H>(a, qp, hop_ids, hop_scores, 1, lane);
            cur_score = hop_scores[0];
        }

        // ---- search_on_level(ef_construct) on level 0 of the block graph -> heuristic -> sel ----
        Beam<E> beam;
        if constexpr (E == 0) {
            __syncthreads();
            beam.init(beam_lds, ef);
        }
        beam.clear();
        uint32_t log_cnt = 1;
        if (lane == 0) {
            atomicOr(&vis[cur_pos >> 5], 1u << (cur_pos & 31));
            vlog[0] = cur_pos >> 5;
        }
        beam.insert(make_key(cur_score, cur_pos), ef, lane);
        while (true) {
            const uint64_t ck = beam.pop_best(lane);
            if (ck == 0) break;
            const uint32_t cand = key_idx(ck);
            const uint32_t *lst = h.links + (slot0 + cand) * h.pm0;
            uint32_t len = h.cnt[slot0 + cand];
            len = len < h.pm0 ? len : h.pm0;
            for (uint32_t base = 0; base < len; base += 64) {
                const uint32_t i = base + (uint32_t)lane;
                const bool on = i < len;
                const uint32_t lp = on ? lst[i] : 0;
                const bool live = on && lp < blk_n;
                const uint32_t bit = 1u << (lp & 31);
                const uint32_t old = live ? atomicOr(&vis[lp >> 5], bit) : bit;
                const bool keep = live && !(old & bit);
                const uint64_t mask = __ballot(keep);
                const uint32_t rank = (uint32_t)__popcll(mask & lt_mask);
                const uint32_t k = (uint32_t)__popcll(mask);
                __syncthreads();
                if (keep) {
                    hop_pos[rank] = lp;
                    hop_ids[rank] = pts[lp];
                    if (log_cnt + rank < h.log_cap) vlog[log_cnt + rank] = lp >> 5;
                }
                log_cnt += k;
                hop_score<H>(a, qp, hop_ids, hop_scores, k, lane);
                const uint64_t mykey = (uint32_t)lane < k ? make_key(hop_scores[lane], hop_pos[lane]) : 0;
                uint64_t mm = __ballot(mykey > beam.at(ef - 1));
                while (mm) {
                    const int src = __builtin_ctzll(mm);
                    mm &= mm - 1;
                    const uint64_t nk = readlane_u64(mykey, src);
                    if (nk > beam.at(ef - 1)) beam.insert(nk, ef, lane);
                }
            }
        }
        // candidates, best first
        __syncthreads();
        uint32_t n_cand = 0;
        if constexpr (E == 0) {
            for (uint32_t base = 0; base < ef; base += 64) {
                const uint32_t idx = base + (uint32_t)lane;
                const uint64_t k = idx < ef ? beam.at(idx) : 0ull;
                const bool ok = k != 0;
                if (ok) {
                    cand_pos[idx] = key_idx(k);
                    cand_scores[idx] = key_score(k);
                }
                n_cand += (uint32_t)__popcll(__ballot(ok));
            }
        } else {
#pragma unroll
            for (int e = 0; e < (E ? E : 1); ++e) {
                const uint32_t idx = (uint32_t)e * 64 + (uint32_t)lane;
                const bool ok = beam.key[e] != 0;
                if (ok) {
                    cand_pos[idx] = key_idx(beam.key[e]);
                    cand_scores[idx] = key_score(beam.key[e]);
                }
                n_cand += (uint32_t)__popcll(__ballot(ok));
            }
        }
        __syncthreads();
        // give the visited bitmap back all-zero
        if (log_cnt <= h.log_cap) {
            for (uint32_t i = (uint32_t)lane; i < log_cnt; i += 64) vis[vlog[i]] = 0;
        } else {
            for (uint64_t w = (uint64_t)lane; w < h.vis_words; w += 64) vis[w] = 0;
        }
        __threadfence();
        const uint32_t n_sel = payload_heuristic_fill<HI>(a0, pts, cand_pos, cand_scores, n_cand, h.pm0, sel_pos, sel_scores, hop_ids, hop_scores, lane);
        const uint64_t so = (uint64_t)bi * h.pm0;
        for (uint32_t i = (uint32_t)lane; i < n_sel; i += 64) {
            h.sel_pos[so + i] = sel_pos[i];
            h.sel_scores[so + i] = sel_scores[i];
        }
        if (lane == 0) h.sel_cnt[bi] = n_sel;
        __syncthreads();
    }
}

// ---- phase 2: publish the item's links, then connect_with_heuristic(p, q) under q's lock for every selected neighbour q of its block ------------------
template <class H>
__global__ __launch_bounds__(64) void hnsw_payload_link_kernel(const ScanArgs a, const HnswPayloadArgs h) {
    __shared__ uint32_t hop_ids[64];
    __shared__ float hop_scores[64];
    __shared__ uint32_t cand_pos[HNSW_BUILD_MAX_M0 + 16];
    __shared__ float cand_scores[HNSW_BUILD_MAX_M0 + 16];
    __shared__ uint32_t srt_pos[HNSW_BUILD_MAX_M0 + 16];
    __shared__ float srt_scores[HNSW_BUILD_MAX_M0 + 16];
    __shared__ uint32_t sel_pos[HNSW_BUILD_MAX_M0];
    __shared__ float sel_scores[HNSW_BUILD_MAX_M0];
    const int lane = threadIdx.x;
    auto next_item = [&](uint32_t bi) -> uint32_t {
        uint32_t v = 0;
        if (lane == 0) v = atomicAdd(&h.next[1], 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    };
    const uint32_t lm = h.pm0;
    for (uint32_t bi = blockIdx.x; bi < h.count; bi = next_item(bi)) {
        const uint32_t blk = h.item_block[h.first_item + bi];
        const uint32_t pos = h.item_pos[h.first_item + bi];
        const uint64_t slot0 = h.blk_off[blk];
        const uint32_t *pts = h.points + slot0;
        const uint32_t p = pts[pos];
        uint32_t n_sel = h.sel_cnt[bi];
        n_sel = n_sel < lm ? n_sel : lm;
        if (n_sel == 0) continue;
        const uint64_t so = (uint64_t)bi * h.pm0;
        // the item's own list: nobody else touches it during this phase (it was not in its graph in phase 1)
        uint32_t *mine = h.links + (slot0 + pos) * h.pm0;
        for (uint32_t i = (uint32_t)lane; i < n_sel; i += 64) st_agent(mine + i, h.sel_pos[so + i]);
        if (lane == 0) st_agent(h.cnt + slot0 + pos, n_sel);
        for (uint32_t k = 0; k < n_sel; ++k) {
            const uint32_t qpos = h.sel_pos[so + k];
            const uint32_t q = pts[qpos];
            float s_qp = h.sel_scores[so + k];
            if constexpr (is_asymmetric<H>::value) {
                __syncthreads();
                if (lane == 0) hop_ids[0] = p;
                hop_score<H>(query_args<H>(a, q), stored_query<H>(a, q), hop_ids, hop_scores, 1, lane);
                s_qp = hop_scores[0];
            }
            uint32_t *lockp = h.lock + slot0 + qpos;
            if (lane == 0) {
                while (atomicCAS(lockp, 0u, 1u) != 0u) __builtin_amdgcn_s_sleep(8);
            }
            __syncthreads();
            __threadfence();
            uint32_t *lst = h.links + (slot0 + qpos) * h.pm0;
            uint32_t *cntp = h.cnt + slot0 + qpos;
            uint32_t len = ld_agent(cntp);
            len = len < lm ? len : lm;
            if (len < lm) {
                if (lane == 0) {
                    st_agent(lst + len, pos);
                    st_agent(cntp, len + 1);
                }
            } else {
                const uint32_t n_c = len + 1;               // <= pm0 + 1 <= HNSW_BUILD_MAX_M0 + 1
                for (uint32_t base = 0; base < len; base += 64) {
                    const uint32_t kk = len - base < 64 ? len - base : 64;
                    __syncthreads();
                    if ((uint32_t)lane < kk) {
                        const uint32_t lp = ld_agent(lst + base + lane);
                        hop_ids[lane] = pts[lp];
                        cand_pos[base + lane] = lp;
                    }
                    hop_score<H>(query_args<H>(a, q), stored_query<H>(a, q), hop_ids, hop_scores, kk, lane);
                    if ((uint32_t)lane < kk) cand_scores[base + lane] = hop_scores[lane];
                }
                if (lane == 0) {
                    cand_pos[len] = pos;
                    cand_scores[len] = s_qp;
                }
                __syncthreads();
                for (uint32_t i = (uint32_t)lane; i < n_c; i += 64) {
                    const uint32_t oi = score_to_ord(cand_scores[i]);
                    uint32_t rank = 0;
                    for (uint32_t j = 0; j < n_c; ++j) {
                        const uint32_t oj = score_to_ord(cand_scores[j]);
                        rank += (oj > oi || (oj == oi && j < i)) ? 1u : 0u;
                    }
                    srt_pos[rank] = cand_pos[i];
                    srt_scores[rank] = cand_scores[i];
                }
                __syncthreads();
                const uint32_t n_new = payload_heuristic_fill<H>(a, pts, srt_pos, srt_scores, n_c, lm, sel_pos, sel_scores, hop_ids, hop_scores, lane);
                for (uint32_t i = (uint32_t)lane; i < n_new; i += 64) st_agent(lst + i, sel_pos[i]);
                if (lane == 0) st_agent(cntp, n_new);
            }
            __threadfence();
            __syncthreads();
            if (lane == 0) atomicExch(lockp, 0u);
        }
    }
}

template <class H, class HI = H>
int32_t launch_hnsw_payload_hop(hipStream_t st, const ScanArgs &a, const HnswPayloadArgs &h, int phase, uint32_t grid, int *per_cu) {
    QMX_REQUIRE(h.ef_construct >= 1 && h.ef_construct <= HNSW_MAX_EF, QMX_ERR_BAD_ARG, "ef_construct %u not in 1..%u", h.ef_construct, HNSW_MAX_EF);
    QMX_REQUIRE(h.pm0 >= 1 && h.pm0 <= HNSW_BUILD_MAX_M0, QMX_ERR_BAD_ARG, "payload_m0 %u not in 1..%u", h.pm0, HNSW_BUILD_MAX_M0);
    const int e_sel = h.ef_construct <= 128 ? 2 : h.ef_construct <= HNSW_MAX_EF_REG ? 8 : 0;
    const size_t lds1 = HNSW_PAYLOAD_LDS_HEAD + 8 * (size_t)hnsw_build_cand_cap(e_sel, h.ef_construct) + 8 * HNSW_BUILD_MAX_M0 + ((size_t)h.lds_query_bytes + 15) / 16 * 16 +
                        (e_sel == 0 ? hnsw_beam_lds(h.ef_construct) : 0);
    if (phase == 1) {
        auto k2 = hnsw_payload_search_kernel<H, HI, 2>;
        auto k8 = hnsw_payload_search_kernel<H, HI, 8>;
        auto k0 = hnsw_payload_search_kernel<H, HI, 0>;
        QMX_REQUIRE(lds1 <= 160 * 1024, QMX_ERR_NOT_SUPPORTED, "payload links: ef_construct %u needs %zu bytes of LDS per insertion", h.ef_construct, lds1);
        auto allow = [](const void *kfn) -> int32_t {
            hipFuncAttributes fa;
            QMX_HIP(hipFuncGetAttributes(&fa, kfn));
            QMX_HIP(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (int)fa.sharedSizeBytes));
            return QMX_OK;
        };
        if (lds1 > 48 * 1024) {
            static thread_local DeviceOnce attr_once;
            if (attr_once.need()) {
                QMX_TRY(allow(reinterpret_cast<const void *>(k0)));
                QMX_TRY(allow(reinterpret_cast<const void *>(k2)));
                QMX_TRY(allow(reinterpret_cast<const void *>(k8)));
                attr_once.mark();
            }
        }
        if (grid == 0) {
            int n = 0;
            if (e_sel == 8) QMX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k8, 64, lds1));
            else if (e_sel == 2) QMX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k2, 64, lds1));
            else QMX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k0, 64, lds1));
            *per_cu = n < 1 ? 1 : n;
            return QMX_OK;
        }
        ::qmx::clear_stale_error();
        if (e_sel == 8) hipLaunchKernelGGL(k8, dim3(grid), dim3(64), lds1, st, a, h);
        else if (e_sel == 2) hipLaunchKernelGGL(k2, dim3(grid), dim3(64), lds1, st, a, h);
        else hipLaunchKernelGGL(k0, dim3(grid), dim3(64), lds1, st, a, h);
        QMX_HIP(hipGetLastError());
        return QMX_OK;
    }
    if (grid == 0) {
        int n = 0;
        QMX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, hnsw_payload_link_kernel<HI>, 64, 0));
        *per_cu = n < 1 ? 1 : n;
        return QMX_OK;
    }
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL((hnsw_payload_link_kernel<HI>), dim3(grid), dim3(64), 0, st, a, h);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

struct HnswPayloadLauncher {
    hipStream_t st;
    const HnswPayloadArgs *h;
    int phase;
    uint32_t grid;
    int *per_cu;
    template <class P> int32_t row(const ScanArgs &a) const { return launch_hnsw_payload_hop<HopRow<P>>(st, a, *h, phase, grid, per_cu); }
    template <class S> int32_t small(const ScanArgs &a) const { return launch_hnsw_payload_hop<HopSmall<S>>(st, a, *h, phase, grid, per_cu); }
};

}  // namespace qmx
