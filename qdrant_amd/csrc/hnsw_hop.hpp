// hnsw_hop.hpp — the hop scorers of the walk (hnsw.hpp): lane policies that score one stored row against the staged query entry, their wrappers (MaxSim,
// custom queries, per-request filters) and hop_score, which scores the ids of one hop into LDS.
#pragma once
#include "custom_combine.hpp"
#include "scan_common.hpp"

namespace qmx {

// trait<T>::value = T::FLAG where a policy declares that static constexpr bool, false where it does not
#define QMX_HOP_TRAIT(trait, FLAG)                                                   \
    template <class T, class = void>                                                 \
    struct trait { static constexpr bool value = false; };                           \
    template <class T>                                                               \
    struct trait<T, decltype((void)T::FLAG)> { static constexpr bool value = T::FLAG; }

// ---- hop scorers: LPI lanes score one stored row; the score is valid in the lane with sub == 0 ----
// a policy whose query offset comes from ScanArgs::sq_qoff instead of the query entry's aux block (a stored SQ row as the query)
QMX_HOP_TRAIT(has_internal_qoff, INTERNAL_QOFF);
// ... or whose query norm comes from ScanArgs::u8_qnorm_* (a stored u8 row as the query of the per-pair cosine)
QMX_HOP_TRAIT(has_internal_norm, INTERNAL_NORM);
// a hop scorer whose stored <-> stored score is NOT the score of the search (PQ: LUT of the original vector vs centroid <-> centroid)
QMX_HOP_TRAIT(is_asymmetric, ASYMMETRIC);
// a row policy whose score lacks the row's offset (RowSQX): HopRow hands that on as ADDS_OFFSET
QMX_HOP_TRAIT(offset_by_caller, OFFSET_BY_CALLER);

template <class P>
struct HopRow {
    static constexpr int LPI = 8;
    static constexpr bool ADDS_OFFSET = offset_by_caller<P>::value;      // the policy's score lacks the row's offset: hop_score adds hop_scores[j]'s prefilled value
    static constexpr bool INTERNAL_QOFF = has_internal_qoff<P>::value;
    static constexpr bool INTERNAL_NORM = has_internal_norm<P>::value;
    static constexpr bool MULTI = true;     // score_multi<R>: R rows per 8-lane group in one pass
    static __device__ __forceinline__ float score(const ScanArgs &a, const unsigned char *qp, uint32_t id, int sub) {
        return group_score<P>(a, qp, id, sub);
    }
    template <int R>
    static __device__ __forceinline__ void score_multi(const ScanArgs &a, const unsigned char *qp, const uint32_t (&ids)[R], int sub, float (&out)[R]) {
        group_score_multi<P, R>(a, qp, ids, sub, out);
    }
};
template <class S>
struct HopSmall {
    static constexpr int LPI = 1;
    static constexpr bool INTERNAL_QOFF = false;
    static constexpr bool INTERNAL_NORM = false;
    static constexpr bool MULTI = false;
    static __device__ __forceinline__ float score(const ScanArgs &a, const unsigned char *qp, uint32_t id, int) {
        return S::score(qp, reinterpret_cast<const unsigned char *>(a.rows) + (uint64_t)id * a.row_stride, id, a);
    }
};

// Multi-vector points with the MaxSim comparator (MultiMetricQueryScorer, query_scorer/multi_metric_query_scorer.rs + score_max_similarity,
// query_scorer/mod.rs:70-97; quantized: QuantizedMultivectorStorage::score_point_max_similarity, quantized_multivector_storage/mod.rs:339-363):
// the graph's points are multi-vectors, a hop candidate's score is the sum over the query's inner vectors (in order, from 0.0) of the max
// over the point's inner vectors (`if max_sim < sim`, from -inf) of the inner policy's score.  The query entry in LDS is
// [16-byte header: number of inner query vectors, pad, pointer to the first entry][the entries, when they fit the launch's LDS share - else the header points
// at them in global memory (PQ: every inner query vector is a LUT)]; qp points behind the header.
QMX_HOP_TRAIT(is_maxsim, MAXSIM);
template <class HI>
struct HopMaxSim {
    static constexpr int LPI = HI::LPI;
    static constexpr bool INTERNAL_QOFF = false;
    static constexpr bool INTERNAL_NORM = false;
    static constexpr bool MULTI = false;
    static constexpr bool MAXSIM = true;
    static __device__ __forceinline__ float score(const ScanArgs &a, const unsigned char *qp, uint32_t id, int sub) {
        const uint32_t n_tokens = *reinterpret_cast<const uint32_t *>(qp - 16);
        const unsigned char *toks = *reinterpret_cast<const unsigned char *const *>(qp - 8);
        const uint64_t b0 = a.mv_offsets[id], b1 = a.mv_offsets[id + 1];
        float sum = 0.0f;
        for (uint32_t t = 0; t < n_tokens; ++t) {
            const unsigned char *qe = toks + (size_t)t * a.q_stride;
            float max_sim = -__builtin_inff();
            for (uint64_t b = b0; b < b1; ++b) {
                const float sim = HI::score(a, qe, (uint32_t)b, sub);
                if (max_sim < sim) max_sim = sim;
            }
            sum += max_sim;
        }
        return sum;
    }
};

// The insertion searches of a build over multi-vector points whose inner storage cannot turn a stored row into a query (PQ, TurboQuant:
// QuantizedMultivectorStorage::encode_internal_vector -> None, quantized_multivector_storage/mod.rs:458-470; point_scorer.rs:183-218 then takes the query
// scorer of the point's ORIGINAL multi-vector): HopMaxSim over the batch's query entries - the new point's tokens are a.mv_q_tokens entries, a.q_stride
// apart, from `qp` on (hnsw_build.hpp points it at the first; no header).
QMX_HOP_TRAIT(is_maxsim_q, MAXSIM_Q);
template <class HI>
struct HopMaxSimQ {
    static constexpr int LPI = HI::LPI;
    static constexpr bool INTERNAL_QOFF = false;
    static constexpr bool INTERNAL_NORM = false;
    static constexpr bool MULTI = false;
    static constexpr bool MAXSIM_Q = true;
    static __device__ __forceinline__ float score(const ScanArgs &a, const unsigned char *qp, uint32_t id, int sub) {
        const uint32_t n_tokens = a.mv_q_tokens;
        const uint64_t b0 = a.mv_offsets[id], b1 = a.mv_offsets[id + 1];
        float sum = 0.0f;
        for (uint32_t t = 0; t < n_tokens; ++t) {
            const unsigned char *qe = qp + (size_t)t * a.q_stride;
            float max_sim = -__builtin_inff();
            for (uint64_t b = b0; b < b1; ++b) {
                const float sim = HI::score(a, qe, (uint32_t)b, sub);
                if (max_sim < sim) max_sim = sim;
            }
            sum += max_sim;
        }
        return sum;
    }
};

// The same points scored stored <-> stored (HNSW build over multi-vector points, hnsw/build.rs:334-341 through FilteredScorer::new_internal:
// MultiMetricQueryScorer::score_internal, multi_metric_query_scorer.rs; quantized: score_internal_max_similarity,
// quantized_multivector_storage/mod.rs:366-393): sum over the inner vectors of point a (in order, from 0.0) of the max over the inner vectors of
// point b (`if sim > max_sim`, from -inf) of the inner storage's score_internal.  The "query entry" of a stored multi-vector is its point id
// (stored_query in hnsw_build.hpp hands it over in the pointer); the inner rows are read from HBM / L2 on every pair.  Not symmetric.
QMX_HOP_TRAIT(is_maxsim_internal, MAXSIM_INTERNAL);
template <class HI>
struct HopMaxSimInternal {
    static constexpr int LPI = HI::LPI;
    static constexpr bool INTERNAL_QOFF = false;     // the inner rows' offsets / norms are looked up per inner row below
    static constexpr bool INTERNAL_NORM = false;
    static constexpr bool MULTI = false;
    static constexpr bool ASYMMETRIC = true;
    static constexpr bool MAXSIM_INTERNAL = true;
    static __device__ __forceinline__ float score(const ScanArgs &a, const unsigned char *qp, uint32_t id, int sub) {
        const uint32_t p = (uint32_t)reinterpret_cast<uintptr_t>(qp);
        const unsigned char *rows = reinterpret_cast<const unsigned char *>(a.rows);
        const uint64_t a0 = a.mv_offsets[p], a1 = a.mv_offsets[p + 1];
        const uint64_t b0 = a.mv_offsets[id], b1 = a.mv_offsets[id + 1];
        float sum = 0.0f;
        for (uint64_t i = a0; i < a1; ++i) {
            ScanArgs b = a;
            if constexpr (HI::INTERNAL_QOFF) b.sq_qoff = a.row_offsets[i] - a.sq_shift;
            if constexpr (HI::INTERNAL_NORM) {
                b.u8_qnorm_f = a.row_norms_f[i];
                b.u8_qnorm_i = a.row_norms_i[i];
            }
            const unsigned char *qe = rows + i * a.row_stride;
            float max_sim = -__builtin_inff();
            for (uint64_t j = b0; j < b1; ++j) {
                const float sim = HI::score(b, qe, (uint32_t)j, sub);
                if (sim > max_sim) max_sim = sim;
            }
            sum += max_sim;
        }
        return sum;
    }
};

// a hop policy whose score lacks the row's offset: hop_score adds it (HopRow over RowSQX)
QMX_HOP_TRAIT(hop_adds_offset, ADDS_OFFSET);
// a hop policy that can drop candidates on an upper bound of their score before the exact scoring (H::prefilter): HopPQ's 8-bit LUT image, pq.hip
QMX_HOP_TRAIT(has_hop_prefilter, HOP_PREFILTER);

// a hop policy that scores a whole hop itself, wave-cooperatively (H::hop): TurboQuant over Manhattan, tq_l1_policy.hpp
QMX_HOP_TRAIT(is_tql1, TQL1);

// Custom queries as the scorer of the walk (raw_scorer.rs:228-333 builds a CustomQueryScorer / QuantizedCustomQueryScorer / TurboCustomQueryScorer for
// whatever storage the segment has; graph_layers.rs:108-149 walks with whatever scorer it gets): a hop candidate's score is
// query.score_by(|example| inner policy's score(example, candidate)) - the examples of ONE custom query, in flat_iter() order, are what the search stages.
// The query block in LDS is [32-byte CustomHeader][the examples' entries, when they fit: else the header points at them in global memory]; qp points
// behind the header.
struct CustomHeader {
    uint32_t kind, n_a, n_b, coef_first;
    const unsigned char *entries;       // the examples' query entries, a.q_stride apart (LDS or global) ...
    const uint32_t *ex_off;             // ... or, when the examples are multi-vectors of different lengths: byte offset of example e's first token from `entries`
};
static_assert(sizeof(CustomHeader) == 32, "the custom walk's LDS header");
QMX_HOP_TRAIT(is_custom, CUSTOM);

// Per-request payload filters (qmx_query_set_filters) in the walk: the same hop policy under another name, instantiated beside the plain one and launched
// only for a batch that carries such filters (launch_hnsw_hop).  The walks of every other batch are the instantiations they were: their liveness test does
// not know of a second index.
template <class H>
struct HopPerQuery : H { static constexpr bool PER_QUERY_FILTER = true; };
QMX_HOP_TRAIT(per_query_filter, PER_QUERY_FILTER);
// filters().check_vector(id) of search qi
template <class H>
__device__ __forceinline__ bool walk_live(const DeletedView &d, uint32_t id, uint32_t qi) {
    if constexpr (per_query_filter<H>::value) return d.live(id, qi);
    else return d.live(id);
}
template <class HI>
struct HopCustom {
    static constexpr int LPI = HI::LPI;
    static constexpr bool INTERNAL_QOFF = false;
    static constexpr bool INTERNAL_NORM = false;
    static constexpr bool MULTI = false;
    static constexpr bool CUSTOM = true;
    static constexpr bool MULTI_EXAMPLES = is_maxsim<HI>::value;      // MultiCustomQueryScorer: every example is a multi-vector scored by MaxSim
    static __device__ __forceinline__ float score(const ScanArgs &a, const unsigned char *qp, uint32_t id, int sub) {
        const CustomHeader *hd = reinterpret_cast<const CustomHeader *>(qp - sizeof(CustomHeader));
        const unsigned char *ent = hd->entries;
        const uint32_t *off = hd->ex_off;
        return custom_score_by(hd->kind, hd->n_a, hd->n_b, a.cq_coefs + hd->coef_first, [&](uint32_t e) {
            return HI::score(a, MULTI_EXAMPLES ? ent + off[e] : ent + (size_t)e * a.q_stride, id, sub);
        });
    }
    // an inner policy that scores a hop as a wave (TurboQuant over Manhattan): the hop against every example in turn - scores parked per example in LDS -
    // then lane j combines candidate j's.  The examples are always staged; behind them [the inner policy's hop scratch][n_examples x 64 floats]
    // (custom_tql1_lds_bytes sizes it; instantiated for such policies only)
    static constexpr bool TQL1 = is_tql1<HI>::value;
    static __device__ __forceinline__ void hop(const ScanArgs &a, const unsigned char *qp, const uint32_t *hop_ids, float *hop_scores, uint32_t k, int lane) {
        const CustomHeader *hd = reinterpret_cast<const CustomHeader *>(qp - sizeof(CustomHeader));
        const uint32_t ne = hd->kind <= QMX_CUSTOM_RECO_SUM_SCORES ? hd->n_a + hd->n_b : hd->n_a + 2 * hd->n_b;
        unsigned char *scratch = const_cast<unsigned char *>(qp) + (size_t)ne * a.q_stride;
        float *ex = reinterpret_cast<float *>(scratch + HI::scratch_bytes(a));
        for (uint32_t e = 0; e < ne; ++e) HI::hop_at(a, hd->entries + (size_t)e * a.q_stride, scratch, hop_ids, ex + (size_t)e * 64, k, lane);
        if ((uint32_t)lane < k)
            hop_scores[lane] = custom_score_by(hd->kind, hd->n_a, hd->n_b, a.cq_coefs + hd->coef_first, [&](uint32_t e) { return ex[(size_t)e * 64 + (uint32_t)lane]; });
        __syncthreads();
    }
};

// scores hop_ids[0..k) into hop_scores[0..k); uniform control flow, k <= 64
template <class H, int R>
__device__ __forceinline__ void hop_score_pass(const ScanArgs &a, const unsigned char *qp, const uint32_t *hop_ids, float *hop_scores,
                                               uint32_t base, uint32_t k, int sub, int g) {
    constexpr int IPP = 64 / H::LPI;
    uint32_t ids[R];
    float sc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t j = base + (uint32_t)(r * IPP + g);
        ids[r] = hop_ids[j < k ? j : 0];
    }
    H::template score_multi<R>(a, qp, ids, sub, sc);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t j = base + (uint32_t)(r * IPP + g);
        if (j < k && sub == 0) hop_scores[j] = hop_adds_offset<H>::value ? sc[r] + hop_scores[j] : sc[r];
    }
}

// (policies whose score lacks the row's offset - hop_adds_offset: RowSQX - find it in hop_scores[j]: put there by the caller with the links
// (`have_offsets`), or gathered here from the offsets column)
template <class H>
__device__ __forceinline__ void hop_score(const ScanArgs &a, const unsigned char *qp, const uint32_t *hop_ids,
                                          float *hop_scores, uint32_t k, int lane, bool have_offsets = false) {
    constexpr int IPP = 64 / H::LPI;
    const int sub = lane % H::LPI, g = lane / H::LPI;
    __syncthreads();   // hop_ids written by other lanes
    if constexpr (hop_adds_offset<H>::value) {
        if (!have_offsets) {
            for (uint32_t j = (uint32_t)lane; j < k; j += 64) hop_scores[j] = a.row_offsets[hop_ids[j]];
            __syncthreads();
        }
    }
    if constexpr (is_tql1<H>::value) {      // the policy scores the hop as a wave (it ends on a barrier, like the loop below)
        H::hop(a, qp, hop_ids, hop_scores, k, lane);
        return;
    }
    uint32_t base = 0;
    if constexpr (H::MULTI) {
        // the usual hop (9..32 fresh neighbours) in ONE pass with 2 or 4 rows per lane group: one round of gathers
        for (; base + 2 * IPP < k; base += 4 * IPP) hop_score_pass<H, 4>(a, qp, hop_ids, hop_scores, base, k, sub, g);
        for (; base + IPP < k; base += 2 * IPP) hop_score_pass<H, 2>(a, qp, hop_ids, hop_scores, base, k, sub, g);
    }
    for (; base < k; base += IPP) {
        const uint32_t j = base + (uint32_t)g;
        const bool on = j < k;
        const uint32_t id = hop_ids[on ? j : 0];
        const float s = H::score(a, qp, id, sub);
        if (on && sub == 0) hop_scores[j] = hop_adds_offset<H>::value ? s + hop_scores[j] : s;
    }
    __syncthreads();
}

}  // namespace qmx
