// sparse_mmr.hip — maximal marginal relevance re-ranking over sparse vectors, on device (qmx_sparse_mmr_select*).
//
//  mmr_from_points_with_vector   lib/shard/src/query/mmr/mod.rs:42-100, :103-140 (the temporary storage: VectorStorageEnum::SparseVolatile)
//  SparseMetricQueryScorer       lib/segment/src/vector_storage/query_scorer/sparse_metric_query_scorer.rs:37-44  (a.score(b).unwrap_or_default())
//  score_vectors                 lib/sparse/src/common/sparse_vector.rs:66-90
//
// The selection is mmr_common.hpp's, the one of the dense kernel (mmr.hip): one work-group per request, every step inside the one launch, no
// C x C matrix and no [candidates] similarity array outside LDS.  What is sparse is the pair score, for relevance(c) = score(query, c) and for
// sim(c, s) alike: the products of the shared dimensions, each rounded, added from +0.0 in ascending ORIGINAL index order, each add rounded; 0.0
// without a shared dimension (never -0.0: a sum that starts at +0.0 cannot reach it).  The reference scores the vectors as they come off the
// points - the IndicesTracker never sees them - while the segment stores its rows sorted by REMAPPED id.  Without a map, or under a monotone one,
// the two orders are one (MAPPED = false); under any other map the kernel needs the original index of a remapped id (`inv_*`, MAPPED = true).
//
// A step stages ONE list - step 0 the request's query, step k the row picked last - and scores every remaining candidate against it, 8 lanes per
// candidate.  A lane takes one entry of the WALKED list and binary-searches the other list for its dimension; the hits of the 8 lanes are then
// added serially in lane order (ballot + shuffle), which is the walked list's order.
//   MAPPED = false: the candidate's row is walked (coalesced loads of the CSR row), the staged list is searched in LDS.  Both are in stored order.
//   MAPPED = true:  the staged list is walked; it was put into ascending original index when it was staged (the query's lists come that way, a
//                   row is ranked by the original index of its dimensions), and the candidate's row is searched by remapped id.
// A list of more than `stage_cap` entries is not staged: the unmapped kernel searches it where it lies, the mapped kernel ranks a row into the
// request's slice of a device buffer (sized from the segment's longest row) and walks it there.  Nothing is refused for length.
#include "mmr_common.hpp"

namespace qmx {

// Walks list a (lane t of the group takes entries t, t + 8, ...), looks each dimension up in list b (ascending) and adds the products in a's
// order.  Every lane of the group returns the sum.  Groups of a wave may run different trip counts; the fold's branches depend on the ballot of
// the active lanes only, so they are uniform among them and every shuffle reads a lane of the reader's own group.
__device__ __forceinline__ float sparse_mmr_pair(const uint32_t *ai, const float *av, uint32_t na, const uint32_t *bi, const float *bv, uint32_t nb, int t,
                                                 int lane) {
    float acc = 0.0f;
    const int gbase = lane & ~7;
    for (uint32_t base = 0; base < na; base += 8) {
        const uint32_t i = base + (uint32_t)t;
        float prod = 0.0f;
        bool hit = false;
        if (i < na && nb != 0) {
            const uint32_t x = ai[i];
            uint32_t lo = 0, n = nb;
            while (n > 1) {
                const uint32_t half = n >> 1;
                lo = bi[lo + half] <= x ? lo + half : lo;
                n -= half;
            }
            if (bi[lo] == x) {
                hit = true;
                prod = __fmul_rn(av[i], bv[lo]);
            }
        }
        const uint64_t m = __ballot(hit);
        if (m == 0) continue;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (m & (0x0101010101010101ull << k)) {      // lane k of some group has a hit
                const float p = __shfl(prod, gbase + k, 64);
                acc = __fadd_rn(acc, p);      // (+0.0 where this group's lane k has none: the sum is never -0.0, so that add changes no bit)
            }
        }
    }
    return acc;
}

struct SparseMmrStep {
    uint32_t R, n_sel;
    float lambda, one_minus;
};

// one step's sweep over the remaining candidates against the staged list (si, sv, sn): step 0 writes the relevance, later steps fold the
// similarity into the running maximum; returns this thread's best key
template <bool MAPPED>
__device__ __forceinline__ uint64_t sparse_mmr_sweep(const MmrLists l, const SparseRows &rows, const uint32_t *si, const float *sv, uint32_t sn,
                                                     const SparseMmrStep &st) {
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, t = lane & 7;
    const uint32_t g = tid >> 3;
    uint64_t best = 0;
    for (uint32_t base = 0; base < st.R; base += MMR_BLOCK / 8) {
        const uint32_t p = base + g;
        const bool valid = p < st.R;
        const uint32_t c = l.order[valid ? p : 0];
        const uint32_t id = l.id[l.src[c]];
        const uint64_t ro = rows.off[id];
        const uint32_t cn = valid ? (uint32_t)(rows.off[id + 1] - ro) : 0u;
        const float sim = MAPPED ? sparse_mmr_pair(si, sv, valid ? sn : 0u, rows.idx + ro, rows.val + ro, cn, t, lane)
                                 : sparse_mmr_pair(rows.idx + ro, rows.val + ro, cn, si, sv, sn, t, lane);
        if (valid && t == 0) {
            uint64_t key;
            if (st.n_sel == 0) {
                l.rel[c] = sim;
                key = mmr_key(sim, p);
            } else {
                key = mmr_fold(l, c, p, sim, st.n_sel == 1, st.lambda, st.one_minus);
            }
            best = key > best ? key : best;
        }
    }
    return best;
}

// the original index of remapped id x (inv_vals ascending; every stored id is one of them)
__device__ __forceinline__ uint32_t sparse_mmr_original(const SparseMmrArgs &a, uint32_t x) {
    uint32_t lo = 0, n = a.n_inv;
    while (n > 1) {
        const uint32_t half = n >> 1;
        lo = a.inv_vals[lo + half] <= x ? lo + half : lo;
        n -= half;
    }
    return a.inv_keys[lo];
}

// a row (stored order) into ascending original index: every entry's original index, then its rank among them (keys are distinct; the entry's
// position breaks a tie so that the ranks stay a permutation whatever the map holds)
__device__ __forceinline__ void sparse_mmr_rank_row(const SparseMmrArgs &a, const uint32_t *ri, const float *rv, uint32_t n, uint32_t *key, uint32_t *oi,
                                                    float *ov) {
    for (uint32_t i = threadIdx.x; i < n; i += MMR_BLOCK) key[i] = sparse_mmr_original(a, ri[i]);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += MMR_BLOCK) {
        const uint32_t k = key[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t kj = key[j];
            rank += (kj < k || (kj == k && j < i)) ? 1u : 0u;
        }
        oi[rank] = ri[i];
        ov[rank] = rv[i];
    }
}

template <bool MAPPED>
__global__ __launch_bounds__(MMR_BLOCK) void sparse_mmr_select_kernel(const SparseMmrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sparse_mmr_smem[];
    const uint32_t S = (a.stride + 3) & ~3u;
    MmrLists l;
    l.id = reinterpret_cast<uint32_t *>(sparse_mmr_smem);
    l.src = l.id + S;
    l.order = l.src + S;
    l.rel = reinterpret_cast<float *>(l.order + S);
    l.max = l.rel + S;
    uint32_t *s_ridx = reinterpret_cast<uint32_t *>(l.max + S);     // [stage_cap] the staged list: remapped ids ...
    float *s_rval = reinterpret_cast<float *>(s_ridx + a.stage_cap);  // [stage_cap] ... and weights
    uint32_t *s_rkey = s_ridx + 2 * (size_t)a.stage_cap;             // [stage_cap] MAPPED: the original indices while a row is ranked
    __shared__ uint64_t s_best[MMR_NW];
    __shared__ uint32_t s_bad, s_n, s_sel;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const qmx_scored_point *cand = a.cand + (uint64_t)q * a.stride;
    qmx_scored_point *out = a.out + (uint64_t)q * a.limit;
    const uint32_t cnt = a.counts[q] < a.stride ? a.counts[q] : a.stride;

    if (!mmr_load_ids(l, cand, cnt, a.rows.n, a.limit, out, a.out_counts + q, a.err_flag, &s_bad)) return;
    const uint32_t C = mmr_unique(l, cnt, &s_n);
    for (uint32_t c = tid; c < C; c += MMR_BLOCK) {
        l.order[c] = c;
        l.max[c] = 0.0f;
    }
    __syncthreads();

    uint32_t n_sel = 0;
    if (C < 2) {      // "can't compute MMR for less than 2 points, return with original score" (mod.rs:77-80)
        if (tid == 0 && C == 1) out[0] = cand[l.src[0]];
        n_sel = C;
    } else {
        const uint32_t L = a.limit < C ? a.limit : C;
        SparseMmrStep st;
        st.R = C;
        st.lambda = a.lambda;
        st.one_minus = 1.0f - a.lambda;
        while (n_sel < L) {
            st.n_sel = n_sel;
            // the list of this step: the request's query in original order (step 0: the sweep gives every candidate's relevance and the first pick
            // is the greatest), then the row picked last
            const uint32_t *gi;
            const float *gv;
            uint32_t sn;
            if (n_sel == 0) {
                const uint64_t qo = a.qs.off[q];
                gi = a.qs.idx + qo;
                gv = a.qs.val + qo;
                sn = (uint32_t)(a.qs.off[q + 1] - qo);
            } else {
                const uint32_t sel_id = l.id[l.src[s_sel]];
                const uint64_t ro = a.rows.off[sel_id];
                gi = a.rows.idx + ro;
                gv = a.rows.val + ro;
                sn = (uint32_t)(a.rows.off[sel_id + 1] - ro);
            }
            const bool in_lds = sn <= a.stage_cap;
            if (MAPPED && n_sel != 0) {
                if (in_lds) {
                    sparse_mmr_rank_row(a, gi, gv, sn, s_rkey, s_ridx, s_rval);
                } else {      // a.spill != nullptr: the segment's longest row exceeds stage_cap
                    uint32_t *sp = a.spill + (uint64_t)q * 3 * a.spill_stride;
                    sparse_mmr_rank_row(a, gi, gv, sn, sp + 2 * a.spill_stride, sp, reinterpret_cast<float *>(sp + a.spill_stride));
                    gi = sp;
                    gv = reinterpret_cast<const float *>(sp + a.spill_stride);
                }
            } else if (in_lds) {
                for (uint32_t e = tid; e < sn; e += MMR_BLOCK) {
                    s_ridx[e] = gi[e];
                    s_rval[e] = gv[e];
                }
            }
            __syncthreads();
            uint64_t best = in_lds ? sparse_mmr_sweep<MAPPED>(l, a.rows, s_ridx, s_rval, sn, st) : sparse_mmr_sweep<MAPPED>(l, a.rows, gi, gv, sn, st);
            best = mmr_block_max(best, s_best);
            mmr_pick(l, best, st.R, cand, out, n_sel, &s_sel);
            --st.R;
            ++n_sel;
        }
    }
    if (tid == 0) a.out_counts[q] = n_sel;
    for (uint32_t i = n_sel + tid; i < a.limit; i += MMR_BLOCK) out[i] = qmx_scored_point{0u, 0.0f};
}

template <bool MAPPED>
static int32_t launch_sparse_mmr_inst(hipStream_t st, const SparseMmrArgs &a, uint32_t nq) {
    const size_t S = ((size_t)a.stride + 3) & ~(size_t)3;
    const size_t lds = S * MMR_CAND_BYTES + (size_t)a.stage_cap * (MAPPED ? 12 : 8);
    QMX_REQUIRE(a.stage_cap <= SPARSE_MMR_STAGE_CAP && lds <= 160 * 1024 - 256, QMX_ERR_NOT_SUPPORTED,
                "sparse MMR over %u candidates staging %u entries needs %zu B of LDS (> 160 KiB)", a.stride, a.stage_cap, lds);
    auto kfn = sparse_mmr_select_kernel<MAPPED>;
    static thread_local DeviceOnce attr_once;
    if (attr_once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
        attr_once.mark();
    }
    ::qmx::clear_stale_error();
    QMX_NOTE_KERNEL(kfn);
    hipLaunchKernelGGL(kfn, dim3(nq), dim3(MMR_BLOCK), lds, st, a);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_sparse_mmr_select(hipStream_t st, const SparseMmrArgs &a, uint32_t nq) {
    if (nq == 0) return QMX_OK;
    return a.inv_vals ? launch_sparse_mmr_inst<true>(st, a, nq) : launch_sparse_mmr_inst<false>(st, a, nq);
}

}  // namespace qmx
