// split_select.hip — from the candidates of a prefilter scan to the rows worth an exact score.  The scans over a derived copy (scan_split.hip,
// scan_i8copy.hip), the wide scans (scan_sqw.hip, scan_tq4w.hip) and the PQ prefilter (pq_prefilter.hip) leave per-wave candidate lists
// (split_common.hpp SpWaveList).  Here: sp_regroup_kernel (per-wave -> per-query lists: the one reader of the wave-list format), the k-th best key
// of a list by a whole block, sp_refine_kernel (the second launch's threshold), sp_select_kernel (the cut, the rows to verify), sp_i8_probe_kernel
// (the k best so far, whose exact scores renew the int8 passes' bound: scan_i8copy.hip sp_i8_bound_kernel), sp_plan_kernel, the launchers.
#include "split_common.hpp"

namespace qmx {

// per-wave candidate lists -> per-query lists (what sp_select_kernel reads), deleted rows dropped.  One block per RG_LISTS wave lists: count per
// query in LDS, reserve the block's range of every query's list with ONE global atomic per query, then place.
constexpr int RG_LISTS = 16;
__global__ __launch_bounds__(256) void sp_regroup_kernel(const uint4 *wlist, const uint32_t *wcnt, uint32_t wcap, uint32_t n_lists, DeletedView del,
                                                         uint64_t *cand, uint32_t *cand_cnt, uint32_t cap, int *overflow /* of the tile: every query of it */) {
    __shared__ uint32_t hist[SP_QT_MAX], base[SP_QT_MAX];
    __shared__ uint32_t pre[RG_LISTS + 1];        // entries of the block's lists in front of list j
    if (threadIdx.x < SP_QT_MAX) hist[threadIdx.x] = 0;
    const uint32_t l0 = blockIdx.x * RG_LISTS, l1 = l0 + RG_LISTS < n_lists ? l0 + RG_LISTS : n_lists;
    if (threadIdx.x < 64) {                       // the lists' lengths in one load, their prefix sums across the wave
        const uint32_t l = l0 + threadIdx.x;
        uint32_t cnt = threadIdx.x < RG_LISTS && l < l1 ? wcnt[l] : 0;
        if (cnt > wcap) {
            *overflow = 1;
            cnt = wcap;
        }
        uint32_t inc = cnt;
        for (int o = 1; o < RG_LISTS; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o, 64);
            if ((int)threadIdx.x >= o) inc += up;
        }
        if (threadIdx.x < RG_LISTS) pre[threadIdx.x + 1] = inc;
        if (threadIdx.x == 0) pre[0] = 0;
    }
    __syncthreads();
    const uint32_t total = pre[RG_LISTS];
    // the block's entries as one sequence: every trip of the loops below has 256 independent loads in flight (the lists are short - a few
    // dozen entries each - and walking them one after the other was a chain of dependent round trips: 25 us per launch, twice per step)
    auto entry = [&](uint32_t i) -> uint4 {
        uint32_t j = 0;
#pragma unroll
        for (int s2 = RG_LISTS / 2; s2 >= 1; s2 >>= 1)
            if (pre[j + s2] <= i) j += s2;
        return wlist[(uint64_t)(l0 + j) * wcap + (i - pre[j])];
    };
    for (uint32_t i = threadIdx.x; i < total; i += 256) {
        const uint4 e = entry(i);
        if (e.z < (uint32_t)SP_QT_MAX && del.live(e.x ^ 0xFFFFFFFFu, e.z)) atomicAdd(&hist[e.z], 1u);      // (e.z = 0xFFFFFFFF: an entry tq4w_finish_kernel withdrew)
    }
    __syncthreads();
    if (threadIdx.x < SP_QT_MAX) {
        const uint32_t c = hist[threadIdx.x];
        base[threadIdx.x] = c ? atomicAdd(&cand_cnt[threadIdx.x], c) : 0;
        hist[threadIdx.x] = 0;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < total; i += 256) {
        const uint4 e = entry(i);
        if (e.z >= (uint32_t)SP_QT_MAX || !del.live(e.x ^ 0xFFFFFFFFu, e.z)) continue;
        const uint32_t at = base[e.z] + atomicAdd(&hist[e.z], 1u);
        if (at < cap) cand[(uint64_t)e.z * cap + at] = ((uint64_t)e.y << 32) | e.x;
    }
}

// ---- candidates -> the rows worth an exact score: A_k = k-th best approximate key, keep A >= A_k - 2 band (at most vcap per query) ----
constexpr int SEL_BLOCK = 512;
// k-th best of raw keys (0 when there are fewer than k), whole block; the result is valid in wave 0 (and broadcast through *sh_out after the sync)
__device__ __forceinline__ void block_kth_key(const uint64_t *c, uint32_t raw, int ptop, uint64_t (*sh)[WAVE], uint64_t *sh_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t list = 0;
    for (uint32_t base = wave * WAVE; base < raw; base += SEL_BLOCK) {
        const uint32_t i = base + lane;
        uint64_t key = i < raw ? c[i] : 0;
        if (key <= readlane_u64(list, ptop - 1)) key = 0;
        uint64_t m = __ballot(key != 0);
        while (m) {
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const uint64_t nk = readlane_u64(key, src);
            if (nk > readlane_u64(list, ptop - 1)) wave_list_insert(list, nk, lane);
        }
    }
    sh[wave][lane] = list;
    __syncthreads();
    if (wave == 0) {
        uint64_t merged = sh[0][lane];
        for (int w2 = 1; w2 < SEL_BLOCK / WAVE; ++w2) {
            const uint64_t key = sh[w2][lane];
            uint64_t m = __ballot(key > readlane_u64(merged, ptop - 1));
            while (m) {
                const int src = __builtin_ctzll(m);
                m &= m - 1;
                const uint64_t nk = readlane_u64(key, src);
                if (nk > readlane_u64(merged, ptop - 1)) wave_list_insert(merged, nk, lane);
            }
        }
        if (lane == 0) *sh_out = readlane_u64(merged, ptop - 1);
    }
    __syncthreads();
}

// The same for lists of up to 8 keys per thread (the usual ~1 000 candidates of a query) without serial insertions, as custom_topk_small_kernel does it:
// the k-th largest of a wave's 64 lane maxima bounds the k-th best key from below, the largest such bound over the waves prunes the list to a few
// times k survivors in LDS, and the survivor with k - 1 larger ones is the answer (keys are distinct: they carry the row id).
constexpr int SEL_E = 3;       // (8 until round 5: 32 KiB of scratch; 3: 12 KiB - a selection block fits the 16 KiB the int8 scan leaves free on a CU)
constexpr int SEL_SURV = SEL_BLOCK * SEL_E;
struct SelScratch {
    uint64_t surv[SEL_SURV];
    uint64_t t[SEL_BLOCK / WAVE];
    uint32_t cnt;
};
// the serial-insertion path (block_kth_key) and the ranked one (block_kth_key_ranked) never run in the same block: one LDS area for both
union SelShared {
    uint64_t sh[SEL_BLOCK / WAVE][WAVE];
    SelScratch scratch;
};
__device__ __forceinline__ void block_kth_key_ranked(const uint64_t *c, uint32_t raw, uint32_t ptop, SelScratch *sc, uint64_t *sh_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t kreg[SEL_E];
    uint64_t m = 0;
#pragma unroll
    for (int e = 0; e < SEL_E; ++e) {
        const uint32_t i = (uint32_t)e * SEL_BLOCK + threadIdx.x;
        kreg[e] = i < raw ? c[i] : 0ull;
        m = kreg[e] > m ? kreg[e] : m;
    }
    uint32_t rank = 0;
    for (int j = 0; j < WAVE; ++j) rank += readlane_u64(m, j) > m ? 1u : 0u;
    const uint64_t sel = __ballot(rank == ptop - 1 && m != 0);
    const uint64_t tw = sel ? readlane_u64(m, __builtin_ctzll(sel)) : 0ull;
    if (lane == 0) sc->t[wave] = tw;
    if (threadIdx.x == 0) { sc->cnt = 0; *sh_out = 0; }
    __syncthreads();
    uint64_t t = 0;
#pragma unroll
    for (int w = 0; w < SEL_BLOCK / WAVE; ++w) t = sc->t[w] > t ? sc->t[w] : t;
#pragma unroll
    for (int e = 0; e < SEL_E; ++e)
        if (kreg[e] != 0 && kreg[e] >= t) sc->surv[atomicAdd(&sc->cnt, 1u)] = kreg[e];
    __syncthreads();
    const uint32_t cnt = sc->cnt;
    for (uint32_t i = threadIdx.x; i < cnt; i += SEL_BLOCK) {
        const uint64_t my = sc->surv[i];
        uint32_t r = 0;
        for (uint32_t j = 0; j < cnt; ++j) r += (sc->surv[j] > my || (sc->surv[j] == my && j < i)) ? 1u : 0u;
        if (r == ptop - 1) *sh_out = my;
    }
    __syncthreads();
}

// After the strided sixteenth of the block: the k-th best APPROXIMATE score A among its rows proves k rows with an exact score >= A - band,
// so a result row has an approximate score >= A - 2 band: the threshold of the other fifteen sixteenths (never lowered).
__global__ __launch_bounds__(SEL_BLOCK) void sp_refine_kernel(const uint64_t *cand, const uint32_t *cand_cnt, uint32_t cap, const float *band, uint32_t top,
                                                              const float *scales, float *thr) {
    __shared__ SelShared sel_sh;
    uint64_t (*const sh)[WAVE] = sel_sh.sh;
    SelScratch &scratch = sel_sh.scratch;
    __shared__ uint64_t sh_kth;
    const uint32_t q = blockIdx.x;
    const uint32_t raw = cand_cnt[q];
    if (raw > cap || raw < top || !(band[q] < 3.0e38f)) return;   // overflow is sp_select_kernel's to report; fewer than k rows prove nothing
    if (raw <= (uint32_t)SEL_SURV) block_kth_key_ranked(cand + (uint64_t)q * cap, raw, top, &scratch, &sh_kth);
    else block_kth_key(cand + (uint64_t)q * cap, raw, (int)top, sh, &sh_kth);
    if (threadIdx.x == 0 && sh_kth) {
        const float t = (key_score(sh_kth) - 2.0f * band[q]) * scales[1];
        if (t > thr[q]) thr[q] = t;
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void sp_select_kernel(const uint64_t *cand, const uint32_t *cand_cnt, uint32_t cap, const float *band, uint32_t top,
                                                              const VerifyPool pool, uint32_t q_base, const int *tile_overflow, uint32_t *ovf_q,
                                                              SplitStats *stats, const float *t_exact /* or nullptr: an exact lower bound of the k-th best score per query */,
                                                              bool tighten /* with t_exact: the k-th best approximate score's bound as well */) {
    __shared__ SelShared sel_sh;
    uint64_t (*const sh)[WAVE] = sel_sh.sh;
    SelScratch &scratch = sel_sh.scratch;
    __shared__ uint64_t sh_kth;
    __shared__ float sh_cut;
    __shared__ uint32_t sh_n, sh_off;
    const uint32_t q = blockIdx.x;
    const uint32_t raw = cand_cnt[q];
    // a wave list of the scan overflowed (its dropped entries could be anybody's), or this query's candidate buffer did: the pass cannot be
    // trusted for this query, which takes the exact scan (the other queries of the batch keep their lists)
    if (*tile_overflow || raw > cap || !(band[q] < 3.0e38f)) {      // (an infinite band: the query had no usable threshold)
        if (threadIdx.x == 0) { ovf_q[q] = 1; pool.cnt[q_base + q] = 0; pool.off[q_base + q] = 0; }
        return;
    }
    const uint64_t *c = cand + (uint64_t)q * cap;
    if (threadIdx.x == 0) sh_n = 0;
    // with an exact bound T (the int8 copy's passes): a result row's approximate score is >= T - band; without: the k-th best approximate score A_k
    // proves k rows with an exact score >= A_k - band, so >= A_k - 2 band
    const bool have_t = t_exact != nullptr && t_exact[q] > -__builtin_inff();
    if (have_t && tighten) {
        // both bounds (the 128-query TurboQuant pass: T comes from a sample alone, so A_k - 2 band is usually the tighter cut)
        if (raw <= (uint32_t)SEL_SURV) block_kth_key_ranked(c, raw, top, &scratch, &sh_kth);
        else block_kth_key(c, raw, (int)top, sh, &sh_kth);
        if (threadIdx.x == 0) {
            const float by_t = t_exact[q] - band[q], by_k = sh_kth ? key_score(sh_kth) - 2.0f * band[q] : -__builtin_inff();
            sh_cut = by_k > by_t ? by_k : by_t;
        }
    } else if (have_t) {
        if (threadIdx.x == 0) sh_cut = t_exact[q] - band[q];
    } else {
        if (raw <= (uint32_t)SEL_SURV) block_kth_key_ranked(c, raw, top, &scratch, &sh_kth);
        else block_kth_key(c, raw, (int)top, sh, &sh_kth);
        // fewer than k candidates: keep all of them (cut = -inf)
        if (threadIdx.x == 0) sh_cut = sh_kth ? key_score(sh_kth) - 2.0f * band[q] : -__builtin_inff();
    }
    __syncthreads();
    const float cut = sh_cut;
    // how many rows the query verifies, then its range of the pool (one global atomic per query), then the rows
    uint32_t mine = 0;
    for (uint32_t i = threadIdx.x; i < raw; i += SEL_BLOCK) mine += !(key_score(c[i]) < cut) ? 1u : 0u;
    if (mine) atomicAdd(&sh_n, mine);
    __syncthreads();
    const uint32_t n = sh_n;
    if (threadIdx.x == 0) {
        const bool too_many = n > pool.max_per_query;                     // (more rows than a query may verify: it reserves nothing)
        const uint32_t off = (n && !too_many) ? atomicAdd(pool.used, n) : 0u;
        const bool over = too_many || (n != 0 && ((uint64_t)off + n > pool.cap));     // (or the pool is full: this query - alone - takes the exact scan)
        sh_off = over ? 0xFFFFFFFFu : off;
        sh_kth = too_many ? (uint64_t)pool.cap : (uint64_t)off;           // (the raw offset: what a query that ran over the pool's end must fill, below)
        ovf_q[q] = over ? 1u : 0u;
        pool.off[q_base + q] = over ? 0u : off;
        pool.cnt[q_base + q] = over ? 0u : n;
        atomicAdd(&stats->candidates, (unsigned long long)raw);
        if (!over) atomicAdd(&stats->verified, (unsigned long long)n);
        sh_n = 0;
    }
    __syncthreads();
    const uint32_t off = sh_off;
    if (off == 0xFFFFFFFFu) {
        // what this query reserved inside the pool before it ran over stays in front of `used`: the gather visits those entries, so they name a row
        // that exists (row 0: its score is dropped - the query's count is zero)
        const uint64_t lo = sh_kth;
        for (uint64_t i = lo + threadIdx.x; i < pool.cap; i += SEL_BLOCK) {
            pool.ids[i] = 0;
            pool.qsel[i] = q_base + q;
        }
        return;
    }
    if (n == 0) return;
    for (uint32_t i = threadIdx.x; i < raw; i += SEL_BLOCK) {
        const uint64_t key = c[i];
        if (!(key_score(key) < cut)) {
            const uint32_t slot = off + atomicAdd(&sh_n, 1u);
            pool.ids[slot] = key_idx(key);
            pool.qsel[slot] = q_base + q;
        }
    }
}

// ---- the queries whose lists overflowed, packed: list[j] = j-th such query (0xFFFFFFFF behind the last), its pre-scan bound next to it; the run flags of
// the conditional exact passes (api_*.hip: one 16-query pass when 1..16 queries overflowed, else passes of 64) ----
__global__ __launch_bounds__(256) void sp_plan_kernel(const uint32_t *ovf_q, uint32_t nq, const uint64_t *gthr, uint32_t *list, uint64_t *gthr_packed,
                                                       uint32_t list_cap, uint32_t *count, int *run16, int *run64, uint32_t n_run64, SplitStats *stats,
                                                       const uint4 *queries, uint32_t units_per_query, uint4 *packed_queries, const uint32_t *filter_of,
                                                       uint32_t *filter_of_packed) {
    __shared__ uint32_t sh_cnt;
    const uint32_t lane = threadIdx.x & 63;
    if (threadIdx.x < 64) {
        uint32_t cnt = 0;
        for (uint32_t base = 0; base < nq; base += 64) {
            const uint32_t i = base + lane;
            const bool f = i < nq && ovf_q[i] != 0;
            const uint64_t m = __ballot(f);
            if (f) {
                const uint32_t at = cnt + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                list[at] = i;
                gthr_packed[at] = gthr[i];
            }
            cnt += (uint32_t)__popcll(m);
        }
        for (uint32_t i = cnt + lane; i < list_cap; i += 64) { list[i] = 0xFFFFFFFFu; gthr_packed[i] = 0; }
        if (lane == 0) {
            *count = cnt;
            *run16 = cnt >= 1 && cnt <= 16;
            const uint32_t fqt = n_run64 ? list_cap / n_run64 : 64u;      // queries per conditional pass: 64, or 32 for rows the 64-query shape does not take
            for (uint32_t p = 0; p < n_run64; ++p) run64[p] = cnt > (p ? fqt * p : 16u);
            stats->fallback_queries = cnt;
            sh_cnt = cnt;
        }
    }
    __syncthreads();
    const uint32_t cnt = sh_cnt;
    if (cnt == 0) return;
    // their query entries, packed the same way (slots behind the last repeat the first: valid operands, results dropped); a rare path, one block does it
    __threadfence_block();
    for (uint64_t gid = threadIdx.x; gid < (uint64_t)list_cap * units_per_query; gid += 256) {
        const uint32_t j = (uint32_t)(gid / units_per_query), u = (uint32_t)(gid % units_per_query);
        const uint32_t src = list[j < cnt ? j : 0];
        packed_queries[gid] = queries[(uint64_t)src * units_per_query + u];
    }
    // per-request filters follow their queries into the packed passes
    if (filter_of)
        for (uint32_t j = threadIdx.x; j < list_cap; j += 256) filter_of_packed[j] = filter_of[list[j < cnt ? j : 0]];
}

// ---- after a launch: the k best candidates (by approximate score) of every query, for an exact look.  k of them are enough: approximate and exact
// scores differ by a hundredth of the band in practice, so the worst exact score among the k best approximate ones is the k-th best exact score so far
// or next to it - and finding k keys is what the bound-and-rank selection is quick at (the 64 best of ~5 000 took 100 - 190 us, these take ~15) ----
__global__ __launch_bounds__(SEL_BLOCK) void sp_i8_probe_kernel(const uint64_t *cand, const uint32_t *cand_cnt, uint32_t cap, const float *band,
                                                                const int *tile_overflow, uint32_t top, uint32_t *probe_ids, uint32_t *probe_cnt) {
    __shared__ SelShared sel_sh;
    uint64_t (*const sh)[WAVE] = sel_sh.sh;
    SelScratch &scratch = sel_sh.scratch;
    __shared__ uint64_t sh_kth;
    __shared__ uint32_t sh_n;
    const uint32_t q = blockIdx.x;
    const uint32_t raw = cand_cnt[q];
    if (*tile_overflow || raw > cap || raw == 0 || !(band[q] < 3.0e38f)) {       // (sp_select_kernel reports; nothing to learn here)
        if (threadIdx.x == 0) probe_cnt[q] = 0;
        return;
    }
    const uint64_t *c = cand + (uint64_t)q * cap;
    const uint32_t k = top < SP_I8_PROBE ? top : SP_I8_PROBE;
    const uint32_t want = raw < k ? raw : k;
    if (threadIdx.x == 0) sh_n = 0;
    if (raw <= (uint32_t)SEL_SURV) block_kth_key_ranked(c, raw, want, &scratch, &sh_kth);
    else block_kth_key(c, raw, (int)want, sh, &sh_kth);
    const uint64_t kth = sh_kth;                                                  // (keys are distinct - they carry the row -: exactly `want` keys are >= it)
    for (uint32_t base = 0; base < raw; base += SEL_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        if (i < raw) {
            const uint64_t key = c[i];
            if (kth != 0 && key >= kth) {                                          // (`k` is taken: the candidate's key)
                const uint32_t slot = atomicAdd(&sh_n, 1u);
                if (slot < SP_I8_PROBE) probe_ids[(uint64_t)q * SP_I8_PROBE + slot] = key_idx(key);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) probe_cnt[q] = sh_n < SP_I8_PROBE ? sh_n : SP_I8_PROBE;
}

// ---------------------------------------------------------------------------------------------------------------------------
// per-wave lists of launch_scan_f32_split (over a derived copy) -> d_cand / d_cand_cnt; d_cand_cnt zeroed by the caller before the scan
int32_t launch_split_regroup(hipStream_t st, const ScanArgs &a, const void *d_wlists, int num_cus, uint64_t *d_cand, uint32_t *d_cand_cnt, uint32_t cap,
                             int *d_overflow, uint32_t phase, uint32_t qt) {
    const SplitGrid g = split_scan_grid(a.n_cand, qt == SP4_QT ? SP4_BM : SP3_BM, phase, num_cus);      // the scan's own grid: its blocks' lists are the ones written
    if (g.n_tiles == 0) return QMX_OK;
    const uint32_t n_lists = g.grid * (SP3_THREADS / 64);
    const SplitWlists wl(d_wlists, num_cus);
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_regroup_kernel, dim3((n_lists + RG_LISTS - 1) / RG_LISTS), dim3(256), 0, st, (const uint4 *)wl.lists, (const uint32_t *)wl.counts,
                       (uint32_t)SP_WCAP, n_lists, a.del, d_cand, d_cand_cnt, cap, d_overflow);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
// any set of per-wave candidate lists (the PQ prefilter's, pq_prefilter.hip) -> per-query lists
int32_t launch_regroup_lists(hipStream_t st, const DeletedView &del, const void *d_wlist, const uint32_t *d_wcnt, uint32_t wcap, uint32_t n_lists, uint64_t *d_cand,
                             uint32_t *d_cand_cnt, uint32_t cap, int *d_overflow) {
    if (n_lists == 0) return QMX_OK;
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_regroup_kernel, dim3((n_lists + RG_LISTS - 1) / RG_LISTS), dim3(256), 0, st, (const uint4 *)d_wlist, d_wcnt, wcap, n_lists, del, d_cand,
                       d_cand_cnt, cap, d_overflow);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_split_refine(hipStream_t st, const uint64_t *d_cand, const uint32_t *d_cand_cnt, uint32_t cap, const float *d_band, uint32_t nq, uint32_t top,
                            const float *d_scales, float *d_thr) {
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_refine_kernel, dim3(nq), dim3(SEL_BLOCK), 0, st, d_cand, d_cand_cnt, cap, d_band, top, d_scales, d_thr);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_split_select(hipStream_t st, const uint64_t *d_cand, const uint32_t *d_cand_cnt, uint32_t cap, const float *d_band, uint32_t nq, uint32_t top,
                            const VerifyPool &pool, uint32_t q_base, const int *d_tile_overflow, uint32_t *d_ovf_q, SplitStats *d_stats, const float *d_t_exact,
                            bool tighten) {
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_select_kernel, dim3(nq), dim3(SEL_BLOCK), 0, st, d_cand, d_cand_cnt, cap, d_band, top, pool, q_base, d_tile_overflow, d_ovf_q, d_stats,
                       d_t_exact, tighten);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_split_plan(hipStream_t st, const uint32_t *d_ovf_q, uint32_t nq, const uint64_t *d_gthr, uint32_t *d_list, uint64_t *d_gthr_packed, uint32_t list_cap,
                          uint32_t *d_count, int *d_run16, int *d_run64, uint32_t n_run64, SplitStats *d_stats, const void *d_queries, uint32_t q_stride,
                          void *d_packed_queries, const uint32_t *d_filter_of, uint32_t *d_filter_of_packed) {
    QMX_REQUIRE(q_stride % 16 == 0, QMX_ERR_OTHER, "query entries are whole 16-byte units");
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_plan_kernel, dim3(1), dim3(256), 0, st, d_ovf_q, nq, d_gthr, d_list, d_gthr_packed, list_cap, d_count, d_run16, d_run64, n_run64, d_stats,
                       (const uint4 *)d_queries, q_stride / 16, (uint4 *)d_packed_queries, d_filter_of, d_filter_of_packed);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}
int32_t launch_split_i8_probe(hipStream_t st, const uint64_t *d_cand, const uint32_t *d_cand_cnt, uint32_t cap, const float *d_band, uint32_t nq, uint32_t top,
                              const int *d_tile_overflow, uint32_t *d_probe_ids, uint32_t *d_probe_cnt) {
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(sp_i8_probe_kernel, dim3(nq), dim3(SEL_BLOCK), 0, st, d_cand, d_cand_cnt, cap, d_band, d_tile_overflow, top, d_probe_ids, d_probe_cnt);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

}  // namespace qmx
