// formula.hip — formula rescoring ("score boosting") of prefetch lists on device.
//
//  do_rescore_with_formula     lib/segment/src/segment/read_view/formula_rescore.rs:29-104
//  FormulaScorer::score        lib/segment/src/index/query_optimization/rescore_formula/formula_scorer.rs:76-343
//
// One work-group per request.  The first half is fusion.hip's: entry j = source * stride + position gets the key (id << 32 | j), the keys are sorted
// in LDS, the entries of one id sit side by side in ascending j and the first entry of a run is the candidate (the reference's `points_to_rescore`
// set).  $score[s] of a candidate is the score of its run's LAST entry from source s (`collect::<AHashMap>` keeps the last duplicate).  One lane
// per candidate interprets the formula's linear program (api_formula.hip compiles it) over an f64 stack: the top in a register, the rest
// [depth - 1][lane] in LDS, so nothing is indexed at run time but LDS.  Every step is one rounded f64 operation (-ffp-contract=off; IEEE division
// and square root); exp / ln / log10 / pow / sin / cos / asin are the device library's.  The (score, id) keys of the candidates that pass the
// threshold are sorted once more and the best `limit` written; a request with a failing candidate reports the error of its lowest failing offset
// instead.
#include "kernels.hpp"
#include "sort_lds.hpp"

namespace qmx {

constexpr int FORMULA_BLOCK = 256;
constexpr uint64_t FORMULA_DEAD = ~0ull;      // a slot behind its list's count: sorts behind every live entry
constexpr uint64_t FORMULA_NO_ERROR = ~0ull;

// 0 = the point has no value, 1 = exactly one value, 2 = a value of the wrong type or several (`invalid` wins over `present`)
__device__ __forceinline__ int formula_value_state(const FormulaColumnDev &c, uint32_t id, uint64_t n_points) {
    if (id >= n_points) return 0;
    if (c.invalid && bit_get(c.invalid, id)) return 2;
    return c.present ? (bit_get(c.present, id) ? 1 : 0) : 1;
}

// Haversine.distance of the geo crate over f64: radians as x * (pi / 180), a = sin^2(dphi / 2) + cos phi1 * cos phi2 * sin^2(dlambda / 2),
// 6371008.8 * (2 * asin(sqrt(a)))
__device__ __forceinline__ double formula_haversine(double lat1, double lon1, double lat2, double lon2) {
    const double to_rad = 3.14159265358979323846 / 180.0;
    const double theta1 = lat1 * to_rad, theta2 = lat2 * to_rad;
    const double delta_theta = (lat2 - lat1) * to_rad, delta_lambda = (lon2 - lon1) * to_rad;
    const double st = sin(delta_theta / 2.0), sl = sin(delta_lambda / 2.0);
    const double a = st * st + cos(theta1) * cos(theta2) * (sl * sl);
    return 6371008.8 * (2.0 * asin(__builtin_sqrt(a)));
}

// FormulaScorer::eval_expression for point `id`: `score_of(s, out)` = whether prefetch s holds the point, and its score.  `stk` is the lane's
// column of the LDS stack (entries FORMULA_BLOCK apart).  Stops at the first error in evaluation order: `status` = its qmx_formula_status.
template <class ScoreOf>
__device__ __forceinline__ double formula_run(const FormulaProgram &p, uint32_t id, const ScoreOf &score_of, double *stk, uint32_t &status) {
    double tos = 0.0;
    uint32_t sp = 0, pc = 0;
    status = QMX_FORMULA_OK;
#define FORMULA_PUSH(v)                                         \
    do {                                                        \
        if (sp) stk[(sp - 1) * FORMULA_BLOCK] = tos;            \
        tos = (v);                                              \
        ++sp;                                                   \
    } while (0)
#define FORMULA_CHECKED(v)                                      \
    do {                                                        \
        const double r__ = (v);                                 \
        if (!__builtin_isfinite(r__)) {                         \
            status = QMX_FORMULA_NON_FINITE;                    \
            return r__;                                         \
        }                                                       \
        tos = r__;                                              \
    } while (0)
    while (pc < p.n_instrs) {
        const FormulaInstr *in = p.instrs + pc;
        ++pc;
        const uint32_t op = in->op, a = in->a;
        switch (op) {
        case FI_CONST:
            FORMULA_PUSH(in->c[0]);
            break;
        case FI_SCORE: {
            float s;
            const bool found = score_of(a, s);
            FORMULA_PUSH(found ? (double)s : in->c[0]);
            break;
        }
        case FI_CONDITION:
            FORMULA_PUSH(id < p.n_points && bit_get((const uint64_t *)p.cols[a].data, id) ? 1.0 : 0.0);
            break;
        case FI_PAYLOAD:
        case FI_GEO:
        case FI_DATETIME: {
            const FormulaColumnDev &c = p.cols[a];
            const int state = formula_value_state(c, id, p.n_points);
            if (state == 2 || (state == 0 && !in->b)) {
                status = state == 2 ? QMX_FORMULA_BAD_VALUE : QMX_FORMULA_NO_VALUE;
                return 0.0;
            }
            double v;
            if (op == FI_PAYLOAD) {
                v = state ? ((const double *)c.data)[id] : in->c[0];
            } else if (op == FI_DATETIME) {
                // datetime.timestamp() as f64, then / 1_000_000.0
                v = state ? (double)((const int64_t *)c.data)[id] / 1000000.0 : in->c[0];
            } else {
                const double lat = state ? ((const double *)c.data)[id] : in->c[2];
                const double lon = state ? ((const double *)c.data2)[id] : in->c[3];
                v = formula_haversine(in->c[0], in->c[1], lat, lon);
            }
            FORMULA_PUSH(v);
            break;
        }
        case FI_ADD:
            --sp;
            tos = stk[(sp - 1) * FORMULA_BLOCK] + tos;
            break;
        case FI_MUL_SC:
            --sp;
            if (tos == 0.0) {
                tos = 0.0;
                pc = a;
            } else {
                tos = stk[(sp - 1) * FORMULA_BLOCK] * tos;
            }
            break;
        case FI_DIV_SC:
            if (tos == 0.0) {
                tos = 0.0;
                pc = a;
            }
            break;
        case FI_DIV: {
            --sp;
            const double left = stk[(sp - 1) * FORMULA_BLOCK], right = tos;
            if (right == 0.0 && in->b) {
                tos = in->c[0];
            } else {
                FORMULA_CHECKED(left / right);
            }
            break;
        }
        case FI_NEG:
            tos = -tos;
            break;
        case FI_ABS:
            tos = __builtin_fabs(tos);
            break;
        case FI_SQRT:
            FORMULA_CHECKED(__builtin_sqrt(tos));
            break;
        case FI_POW:
            --sp;
            FORMULA_CHECKED(pow(stk[(sp - 1) * FORMULA_BLOCK], tos));
            break;
        case FI_EXP:
            FORMULA_CHECKED(exp(tos));
            break;
        case FI_LOG10:
            FORMULA_CHECKED(log10(tos));
            break;
        case FI_LN:
            FORMULA_CHECKED(log(tos));
            break;
        case FI_DECAY: {
            --sp;
            const double x = stk[(sp - 1) * FORMULA_BLOCK], target = tos, lambda = in->c[0];
            if (a == QMX_DECAY_EXP) {
                const double diff = __builtin_fabs(x - target);
                tos = exp(lambda * diff);
            } else if (a == QMX_DECAY_GAUSS) {
                const double diff = x - target;
                tos = exp(lambda * diff * diff);
            } else {
                const double diff = __builtin_fabs(x - target);
                tos = fmax(-lambda * diff + 1.0, 0.0);
            }
            break;
        }
        default:      // (the host emits no other op)
            status = QMX_FORMULA_BAD_VALUE;
            return 0.0;
        }
    }
#undef FORMULA_PUSH
#undef FORMULA_CHECKED
    return tos;
}

// FormulaScorer::score's cast: the f32 must be finite
__device__ __forceinline__ float formula_cast(double v, uint32_t &status) {
    const float s = (float)v;
    if (status == QMX_FORMULA_OK && !__builtin_isfinite(s)) status = QMX_FORMULA_NON_FINITE;
    return s;
}

// $score[s] of the candidate whose run starts at sorted slot x: the run's last entry from source s (its greatest position)
struct FormulaRunScores {
    const FormulaRescoreArgs &a;
    const uint64_t *keys;
    uint32_t n, x, q;
    __device__ __forceinline__ bool operator()(uint32_t s, float &out) const {
        const uint32_t id = (uint32_t)(keys[x] >> 32);
        bool found = false;
        for (uint32_t y = x; y < n; ++y) {
            const uint64_t key = keys[y];
            if (key == FORMULA_DEAD || (uint32_t)(key >> 32) != id) break;
            const uint32_t j = (uint32_t)key, src = j / a.stride;
            if (src > s) break;
            if (src == s) {
                out = a.lists[((uint64_t)s * a.nq + q) * a.stride + (j - src * a.stride)].score;
                found = true;
            }
        }
        return found;
    }
};

// (as fusion.hip) OrderedFloat holds -0.0 equal to 0.0, make_key's order does not: a zero keys as +0.0, so that the offset decides among zeros
__device__ __forceinline__ float formula_key_score(float s) { return s == 0.0f ? 0.0f : s; }

__global__ __launch_bounds__(FORMULA_BLOCK) void formula_rescore_kernel(const FormulaRescoreArgs a, uint32_t n, uint32_t stack_slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char formula_smem[];
    uint64_t *keys = reinterpret_cast<uint64_t *>(formula_smem);      // [n] (id, slot), sorted ascending
    uint64_t *rescored = keys + n;                                     // [n] (score, id) keys of the kept candidates, 0 elsewhere
    double *stack = reinterpret_cast<double *>(rescored + n);          // [stack_slots][FORMULA_BLOCK]
    uint32_t *neg_zero = reinterpret_cast<uint32_t *>(stack + (size_t)stack_slots * FORMULA_BLOCK);   // [max(n / 32, 1)] bit x: the candidate at slot x scored -0.0
    __shared__ uint32_t cnt[FUSE_MAX_SOURCES];
    __shared__ uint32_t n_kept;
    __shared__ unsigned long long first_error;      // (lowest failing offset << 32) | its status
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t total = a.n_sources * a.stride;

    if (tid < a.n_sources) {
        const uint32_t c = a.counts[(uint64_t)tid * a.nq + q];
        cnt[tid] = c < a.stride ? c : a.stride;
    }
    if (tid == 0) {
        n_kept = 0;
        first_error = FORMULA_NO_ERROR;
    }
    for (uint32_t w = tid; w < (n + 31) / 32; w += FORMULA_BLOCK) neg_zero[w] = 0;
    __syncthreads();

    for (uint32_t j = tid; j < n; j += FORMULA_BLOCK) {
        uint64_t key = FORMULA_DEAD;
        if (j < total) {
            const uint32_t s = j / a.stride, i = j - s * a.stride;
            if (i < cnt[s]) key = ((uint64_t)a.lists[((uint64_t)s * a.nq + q) * a.stride + i].idx << 32) | j;
        }
        keys[j] = key;
    }
    __syncthreads();
    bitonic_sort_lds<FORMULA_BLOCK>(keys, n);

    for (uint32_t x = tid; x < n; x += FORMULA_BLOCK) {
        const uint64_t key = keys[x];
        uint64_t f = 0;
        if (key != FORMULA_DEAD && (x == 0 || (uint32_t)(keys[x - 1] >> 32) != (uint32_t)(key >> 32))) {
            const uint32_t id = (uint32_t)(key >> 32);
            uint32_t status;
            const double precise = formula_run(a.prog, id, FormulaRunScores{a, keys, n, x, q}, stack + tid, status);
            const float s = formula_cast(precise, status);
            if (status != QMX_FORMULA_OK) {
                atomicMin(&first_error, ((unsigned long long)id << 32) | status);
            } else if (!a.has_threshold || s >= a.threshold) {
                f = make_key(formula_key_score(s), id);
                atomicAdd(&n_kept, 1u);
                if (__float_as_uint(s) == 0x80000000u) atomicOr(&neg_zero[x >> 5], 1u << (x & 31));
            }
        }
        rescored[x] = f;
    }
    __syncthreads();
    const unsigned long long err = first_error;      // (the same for every lane: the branch below is taken by the whole group)
    if (err == FORMULA_NO_ERROR) bitonic_sort_lds<FORMULA_BLOCK>(rescored, n);

    const uint32_t found = err != FORMULA_NO_ERROR ? 0u : (n_kept < a.limit ? n_kept : a.limit);
    for (uint32_t r = tid; r < a.limit; r += FORMULA_BLOCK) {
        qmx_scored_point p{0u, 0.0f};
        if (r < found) {
            const uint64_t f = rescored[n - 1 - r];
            p.idx = key_idx(f);
            p.score = key_score(f);
            if (p.score == 0.0f) {
                // the key carries +0.0, the result the score's own sign: the bit of the id's first sorted slot
                uint32_t lo = 0, hi = n;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (keys[mid] < ((uint64_t)p.idx << 32)) lo = mid + 1; else hi = mid;
                }
                if (lo < n && ((neg_zero[lo >> 5] >> (lo & 31)) & 1u)) p.score = -0.0f;
            }
        }
        a.out[(uint64_t)q * a.limit + r] = p;
    }
    if (tid == 0) {
        a.out_counts[q] = found;
        a.out_status[q] = err == FORMULA_NO_ERROR ? (uint32_t)QMX_FORMULA_OK : (uint32_t)err;
        a.out_error_point[q] = err == FORMULA_NO_ERROR ? 0u : (uint32_t)(err >> 32);
    }
}

// FormulaScorer::score for explicit points: one lane per point, $score[s] from the caller's rows
struct FormulaGivenScores {
    const FormulaEvalArgs &a;
    uint64_t i;
    __device__ __forceinline__ bool operator()(uint32_t s, float &out) const {
        if (s >= a.n_score_vars || !a.scores) return false;
        const uint64_t at = (uint64_t)s * a.n + i;
        if (a.score_missing && a.score_missing[at]) return false;
        out = a.scores[at];
        return true;
    }
};

__global__ __launch_bounds__(FORMULA_BLOCK) void formula_eval_kernel(const FormulaEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char formula_smem[];
    double *stack = reinterpret_cast<double *>(formula_smem);      // [depth - 1][FORMULA_BLOCK]
    const uint64_t i = (uint64_t)blockIdx.x * FORMULA_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    uint32_t status;
    const double precise = formula_run(a.prog, a.ids[i], FormulaGivenScores{a, i}, stack + threadIdx.x, status);
    const float s = formula_cast(precise, status);
    if (a.out_precise) a.out_precise[i] = precise;
    if (a.out_scores) a.out_scores[i] = s;
    a.out_status[i] = status;
}

static uint32_t formula_stack_slots(const FormulaProgram &p) { return p.depth > 1 ? p.depth - 1 : 1; }

int32_t launch_formula_rescore(hipStream_t st, const FormulaRescoreArgs &a) {
    if (a.nq == 0) return QMX_OK;
    const uint64_t total = (uint64_t)a.n_sources * a.stride;
    uint32_t n = 2;
    while (n < total) n <<= 1;
    const uint32_t slots = formula_stack_slots(a.prog);
    auto lds_of = [](uint32_t n_, uint32_t slots_) {
        return (size_t)n_ * 2 * sizeof(uint64_t) + (size_t)slots_ * FORMULA_BLOCK * sizeof(double) + (size_t)((n_ + 31) / 32) * sizeof(uint32_t);
    };
    static thread_local DeviceOnce attr_once;
    if (attr_once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(formula_rescore_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_of(FUSE_MAX_ENTRIES, FORMULA_MAX_DEPTH - 1)));
        attr_once.mark();
    }
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(formula_rescore_kernel, dim3(a.nq), dim3(FORMULA_BLOCK), lds_of(n, slots), st, a, n, slots);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

int32_t launch_formula_eval(hipStream_t st, const FormulaEvalArgs &a) {
    if (a.n == 0) return QMX_OK;
    const uint64_t blocks = (a.n + FORMULA_BLOCK - 1) / FORMULA_BLOCK;
    const size_t lds = (size_t)formula_stack_slots(a.prog) * FORMULA_BLOCK * sizeof(double);
    ::qmx::clear_stale_error();
    hipLaunchKernelGGL(formula_eval_kernel, dim3((uint32_t)blocks), dim3(FORMULA_BLOCK), lds, st, a);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

}  // namespace qmx
