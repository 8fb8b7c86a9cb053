// api_formula.hip — the C-ABI of include/qdrant_amd.h, formula rescoring: payload columns (qmx_payload_columns_*), the formula handle with its
// validation and its compilation to the stack program of formula.hip (qmx_formula_*), and the entry points qmx_formula_rescore* / qmx_formula_eval.
// (One of the api_*.hip translation units; what they share: api_internal.hpp.)
#include "api_internal.hpp"

struct qmx_payload_columns {
    int device = 0;
    uint64_t n_points = 0;
    std::vector<uint32_t> kinds;
    std::vector<DevBuf> allocs;            // every column array and the descriptor table d_cols points into: freed with the handle
    FormulaColumnDev *d_cols = nullptr;
    // a column array (host or device memory) copied into an allocation of this handle; a null array stays null
    int32_t upload(const void *src, size_t bytes, const void **dst) {
        *dst = nullptr;
        if (!src) return QMX_OK;
        DevBuf b;
        QMX_TRY(b.reserve(bytes));
        if (bytes) QMX_HIP(hipMemcpy(b.p, src, bytes, hipMemcpyDefault));
        *dst = b.p;
        allocs.push_back(std::move(b));
        return QMX_OK;
    }
};

constexpr int FORMULA_MAX_DEVICES = 64;
struct qmx_formula {
    std::vector<FormulaInstr> prog;
    uint32_t depth = 0, n_score_vars = 0;
    struct Use { uint32_t col, kind; };
    std::vector<Use> uses;                              // the columns the program reads and the kind each read expects
    mutable std::mutex mu;
    mutable FormulaInstr *d_prog[FORMULA_MAX_DEVICES] = {};   // the program on every device that ran it
    qmx_formula() = default;
    qmx_formula(const qmx_formula &) = delete;
    qmx_formula &operator=(const qmx_formula &) = delete;
    ~qmx_formula() {
        int before = 0;
        const bool have = hipGetDevice(&before) == hipSuccess;
        for (int d = 0; d < FORMULA_MAX_DEVICES; ++d)
            if (d_prog[d] && hipSetDevice(d) == hipSuccess) dev_free(d_prog[d]);
        if (have) (void)hipSetDevice(before);
    }
};

namespace {

struct FormulaCompiler {
    const qmx_formula_node *nodes;
    uint32_t n_nodes;
    const qmx_formula_default *defaults;
    uint32_t n_defaults;
    qmx_formula *f;
    std::vector<uint8_t> on_path;
    uint32_t max_depth = 0;
    int32_t rc = QMX_OK;

    bool fail(int32_t code, const char *fmt, ...) __attribute__((format(printf, 3, 4))) {
        if (rc == QMX_OK) {
            char buf[256];
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(buf, sizeof(buf), fmt, ap);
            va_end(ap);
            set_error("%s", buf);
            rc = code;
        }
        return false;
    }
    const qmx_formula_default *default_of(bool column, uint32_t index) const {
        const qmx_formula_default *found = nullptr;
        for (uint32_t i = 0; i < n_defaults; ++i)
            if ((defaults[i].is_column != 0) == column && defaults[i].index == index) found = &defaults[i];      // (a map: the last insert stays)
        return found;
    }
    uint32_t emit(uint32_t op, uint32_t a = 0, uint32_t b = 0, double c0 = 0.0, double c1 = 0.0, double c2 = 0.0, double c3 = 0.0) {
        FormulaInstr in{};
        in.op = op;
        in.a = a;
        in.b = b;
        in.c[0] = c0;
        in.c[1] = c1;
        in.c[2] = c2;
        in.c[3] = c3;
        f->prog.push_back(in);
        return (uint32_t)f->prog.size() - 1;
    }
    void pushed(uint32_t depth_before) { max_depth = std::max(max_depth, depth_before + 1); }

    // emits the code that leaves the value of node `at` on a stack that holds `depth` values
    bool node(uint32_t at, uint32_t depth) {
        if (rc != QMX_OK) return false;
        if (at >= n_nodes) return fail(QMX_ERR_BAD_ARG, "formula node index %u out of range (%u nodes)", at, n_nodes);
        if (on_path[at]) return fail(QMX_ERR_BAD_ARG, "formula node %u is its own descendant (a cycle)", at);
        if (f->prog.size() > FORMULA_MAX_INSTRS) return fail(QMX_ERR_NOT_SUPPORTED, "formula compiles to more than %u instructions", FORMULA_MAX_INSTRS);
        if (depth + 1 > FORMULA_MAX_DEPTH) return fail(QMX_ERR_NOT_SUPPORTED, "formula needs more than %u values on the evaluation stack", FORMULA_MAX_DEPTH);
        const qmx_formula_node &n = nodes[at];
        if (n.n_children && !n.children) return fail(QMX_ERR_BAD_ARG, "formula node %u: children is NULL", at);
        auto arity = [&](uint32_t lo, uint32_t hi) {
            return n.n_children >= lo && n.n_children <= hi ? true
                   : fail(QMX_ERR_BAD_ARG, "formula node %u (op %u) has %u children, expected %u..%u", at, n.op, n.n_children, lo, hi);
        };
        on_path[at] = 1;
        bool ok = true;
        switch (n.op) {
        case QMX_FORMULA_CONSTANT:
            ok = arity(0, 0);
            emit(FI_CONST, 0, 0, n.value);
            pushed(depth);
            break;
        case QMX_FORMULA_SCORE: {
            ok = arity(0, 0);
            const qmx_formula_default *d = default_of(false, n.var);
            if (d && d->kind != QMX_PAYLOAD_NUMBER) ok = fail(QMX_ERR_BAD_ARG, "the default of $score[%u] must be a number", n.var);
            emit(FI_SCORE, n.var, 0, d ? d->value : 0.0);      // DEFAULT_SCORE = 0.0
            f->n_score_vars = std::max(f->n_score_vars, n.var + 1);
            pushed(depth);
            break;
        }
        case QMX_FORMULA_CONDITION:
            ok = arity(0, 0);
            emit(FI_CONDITION, n.var);
            f->uses.push_back({n.var, QMX_PAYLOAD_CONDITION});
            pushed(depth);
            break;
        case QMX_FORMULA_PAYLOAD:
        case QMX_FORMULA_GEO_DISTANCE:
        case QMX_FORMULA_DATETIME_KEY: {
            ok = arity(0, 0);
            const uint32_t kind = n.op == QMX_FORMULA_PAYLOAD ? QMX_PAYLOAD_NUMBER : n.op == QMX_FORMULA_GEO_DISTANCE ? QMX_PAYLOAD_GEO : QMX_PAYLOAD_DATETIME;
            const qmx_formula_default *d = default_of(true, n.var);
            if (d && d->kind != kind)
                ok = fail(QMX_ERR_BAD_ARG, "the default of column %u is of kind %u, formula node %u reads kind %u", n.var, d->kind, at, kind);
            if (kind == QMX_PAYLOAD_NUMBER) emit(FI_PAYLOAD, n.var, d ? 1 : 0, d ? d->value : 0.0);
            else if (kind == QMX_PAYLOAD_GEO) emit(FI_GEO, n.var, d ? 1 : 0, n.value, n.value2, d ? d->value : 0.0, d ? d->value2 : 0.0);
            else emit(FI_DATETIME, n.var, d ? 1 : 0, d ? (double)d->micros / 1000000.0 : 0.0);
            f->uses.push_back({n.var, kind});
            pushed(depth);
            break;
        }
        case QMX_FORMULA_DATETIME:
            ok = arity(0, 0);
            emit(FI_CONST, 0, 0, (double)n.micros / 1000000.0);      // timestamp() as f64 / 1_000_000.0: the device's two operations, done here
            pushed(depth);
            break;
        case QMX_FORMULA_SUM:
            emit(FI_CONST, 0, 0, 0.0);
            pushed(depth);
            for (uint32_t i = 0; ok && i < n.n_children; ++i) {
                ok = node(n.children[i], depth + 1);
                emit(FI_ADD);
            }
            break;
        case QMX_FORMULA_MULT: {
            emit(FI_CONST, 0, 0, 1.0);
            pushed(depth);
            std::vector<uint32_t> jumps;
            for (uint32_t i = 0; ok && i < n.n_children; ++i) {
                ok = node(n.children[i], depth + 1);
                jumps.push_back(emit(FI_MUL_SC));
            }
            for (uint32_t j : jumps) f->prog[j].a = (uint32_t)f->prog.size();
            break;
        }
        case QMX_FORMULA_DIV: {
            if (!(ok = arity(2, 2))) break;
            ok = node(n.children[0], depth);
            const uint32_t jump = emit(FI_DIV_SC);
            ok = ok && node(n.children[1], depth + 1);
            emit(FI_DIV, 0, n.flags & 1u, n.value);
            f->prog[jump].a = (uint32_t)f->prog.size();
            break;
        }
        case QMX_FORMULA_POW:
            if (!(ok = arity(2, 2))) break;
            ok = node(n.children[0], depth) && node(n.children[1], depth + 1);
            emit(FI_POW);
            break;
        case QMX_FORMULA_NEG:
        case QMX_FORMULA_SQRT:
        case QMX_FORMULA_EXP:
        case QMX_FORMULA_LOG10:
        case QMX_FORMULA_LN:
        case QMX_FORMULA_ABS: {
            if (!(ok = arity(1, 1))) break;
            ok = node(n.children[0], depth);
            const uint32_t op = n.op == QMX_FORMULA_NEG ? FI_NEG : n.op == QMX_FORMULA_SQRT ? FI_SQRT : n.op == QMX_FORMULA_EXP ? FI_EXP
                              : n.op == QMX_FORMULA_LOG10 ? FI_LOG10 : n.op == QMX_FORMULA_LN ? FI_LN : FI_ABS;
            emit(op);
            break;
        }
        case QMX_FORMULA_DECAY:
            if (!(ok = arity(1, 2))) break;
            if (n.var > QMX_DECAY_EXP) { ok = fail(QMX_ERR_BAD_ARG, "formula node %u: decay kind %u", at, n.var); break; }
            ok = node(n.children[0], depth);
            if (n.n_children == 2) {
                ok = ok && node(n.children[1], depth + 1);
            } else {
                if (depth + 2 > FORMULA_MAX_DEPTH) { ok = fail(QMX_ERR_NOT_SUPPORTED, "formula needs more than %u values on the evaluation stack", FORMULA_MAX_DEPTH); break; }
                emit(FI_CONST, 0, 0, 0.0);      // DEFAULT_DECAY_TARGET
                pushed(depth + 1);
            }
            emit(FI_DECAY, n.var, 0, n.value);
            break;
        default:
            ok = fail(QMX_ERR_BAD_ARG, "formula node %u: unknown op %u", at, n.op);
        }
        on_path[at] = 0;
        return ok && rc == QMX_OK;
    }
};

// the program of `f` in the memory of the current device `dev`
int32_t formula_on_device(const qmx_formula *f, int dev, const FormulaInstr **out) {
    QMX_REQUIRE(dev >= 0 && dev < FORMULA_MAX_DEVICES, QMX_ERR_NOT_SUPPORTED, "device %d", dev);
    std::lock_guard<std::mutex> lock(f->mu);
    if (!f->d_prog[dev]) QMX_TRY(dev_upload(&f->d_prog[dev], f->prog.data(), f->prog.size()));
    *out = f->d_prog[dev];
    return QMX_OK;
}

// column kinds against the ops that read them; fills `p` (the current device must be the columns')
int32_t formula_program(const qmx_formula *f, const qmx_payload_columns *cols, int dev, FormulaProgram &p) {
    for (const qmx_formula::Use &u : f->uses) {
        QMX_REQUIRE(cols && u.col < cols->kinds.size(), QMX_ERR_BAD_ARG, "the formula reads column %u, the columns handle holds %zu", u.col,
                    cols ? cols->kinds.size() : (size_t)0);
        QMX_REQUIRE(cols->kinds[u.col] == u.kind, QMX_ERR_BAD_ARG, "column %u is of kind %u, the formula reads it as kind %u", u.col, cols->kinds[u.col], u.kind);
    }
    memset(&p, 0, sizeof(p));
    QMX_TRY(formula_on_device(f, dev, &p.instrs));
    p.n_instrs = (uint32_t)f->prog.size();
    p.depth = f->depth;
    p.cols = cols ? cols->d_cols : nullptr;
    p.n_cols = cols ? (uint32_t)cols->kinds.size() : 0;
    p.n_points = cols ? cols->n_points : 0;
    return QMX_OK;
}

int32_t rescore_args(const qmx_formula *f, const qmx_scored_point *lists, const uint32_t *counts, uint32_t n_sources, uint32_t nq, uint32_t stride,
                     uint32_t limit, const float *thr, qmx_scored_point *out, uint32_t *oc, uint32_t *os, uint32_t *oe, FormulaRescoreArgs &a) {
    QMX_REQUIRE(f && out && oc && os && oe && (nq == 0 || n_sources == 0 || (lists && counts)), QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(limit >= 1 && limit <= MAX_TOP, QMX_ERR_NOT_SUPPORTED, "limit %u not in 1..%u", limit, MAX_TOP);
    QMX_REQUIRE(n_sources <= FUSE_MAX_SOURCES, QMX_ERR_NOT_SUPPORTED, "formula rescoring of %u sources (at most %u)", n_sources, FUSE_MAX_SOURCES);
    QMX_REQUIRE((uint64_t)n_sources * stride <= FUSE_MAX_ENTRIES, QMX_ERR_NOT_SUPPORTED,
                "formula rescoring of %u lists x %u entries exceeds %u entries per request", n_sources, stride, FUSE_MAX_ENTRIES);
    memset(&a, 0, sizeof(a));
    a.lists = lists;
    a.counts = counts;
    a.n_sources = n_sources;
    a.nq = nq;
    a.stride = stride;
    a.limit = limit;
    a.has_threshold = thr ? 1 : 0;
    a.threshold = thr ? *thr : 0.0f;
    a.out = out;
    a.out_counts = oc;
    a.out_status = os;
    a.out_error_point = oe;
    return QMX_OK;
}

int32_t columns_upload(qmx_payload_columns *h, const qmx_payload_column *cols, uint32_t n_cols) {
    const uint64_t n_points = h->n_points;
    const size_t words = (size_t)((n_points + 63) / 64) * 8;
    std::vector<FormulaColumnDev> dev(n_cols);
    for (uint32_t i = 0; i < n_cols; ++i) {
        const qmx_payload_column &c = cols[i];
        h->kinds.push_back(c.kind);
        dev[i].kind = c.kind;
        dev[i].pad_ = 0;
        dev[i].data = dev[i].data2 = nullptr;
        dev[i].present = dev[i].invalid = nullptr;
        if (c.kind == QMX_PAYLOAD_CONDITION) {
            QMX_TRY(h->upload(c.data, words, &dev[i].data));
            continue;
        }
        QMX_TRY(h->upload(c.data, (size_t)n_points * 8, &dev[i].data));
        if (c.kind == QMX_PAYLOAD_GEO) QMX_TRY(h->upload(c.data2, (size_t)n_points * 8, &dev[i].data2));
        QMX_TRY(h->upload(c.present, words, (const void **)&dev[i].present));
        QMX_TRY(h->upload(c.invalid, words, (const void **)&dev[i].invalid));
    }
    if (n_cols) QMX_TRY(h->upload(dev.data(), dev.size() * sizeof(FormulaColumnDev), (const void **)&h->d_cols));
    return QMX_OK;
}

}  // namespace

extern "C" {

int32_t qmx_payload_columns_create(int32_t device_id, uint64_t n_points, const qmx_payload_column *cols, uint32_t n_cols, qmx_payload_columns **out) {
    QMX_REQUIRE(out && (n_cols == 0 || cols), QMX_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    QMX_REQUIRE(n_points <= 0xFFFFFFFFull, QMX_ERR_NOT_SUPPORTED, "point offsets are 32-bit (%llu points)", (unsigned long long)n_points);
    for (uint32_t i = 0; i < n_cols; ++i) {
        QMX_REQUIRE(cols[i].kind <= QMX_PAYLOAD_CONDITION, QMX_ERR_BAD_ARG, "column %u: kind %u", i, cols[i].kind);
        QMX_REQUIRE(n_points == 0 || (cols[i].data && (cols[i].kind != QMX_PAYLOAD_GEO || cols[i].data2)), QMX_ERR_BAD_ARG, "column %u: data is NULL", i);
    }
    QMX_TRY(check_device(device_id, nullptr));
    qmx_payload_columns *h = new (std::nothrow) qmx_payload_columns();
    QMX_REQUIRE(h, QMX_ERR_OUT_OF_MEMORY, "host allocation failed");
    h->device = device_id;
    h->n_points = n_points;
    const int32_t rc = columns_upload(h, cols, n_cols);
    if (rc != QMX_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return QMX_OK;
}

int32_t qmx_payload_columns_destroy(qmx_payload_columns *columns) {
    if (!columns) return QMX_OK;
    (void)hipSetDevice(columns->device);
    delete columns;
    return QMX_OK;
}

int32_t qmx_formula_create(const qmx_formula_node *nodes, uint32_t n_nodes, uint32_t root, const qmx_formula_default *defaults, uint32_t n_defaults,
                           qmx_formula **out) {
    QMX_REQUIRE(out && nodes && n_nodes && (n_defaults == 0 || defaults), QMX_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    for (uint32_t i = 0; i < n_defaults; ++i)
        QMX_REQUIRE(defaults[i].kind <= QMX_PAYLOAD_DATETIME, QMX_ERR_BAD_ARG, "default %u: kind %u is no value kind", i, defaults[i].kind);
    qmx_formula *f = new (std::nothrow) qmx_formula();
    QMX_REQUIRE(f, QMX_ERR_OUT_OF_MEMORY, "host allocation failed");
    FormulaCompiler c{nodes, n_nodes, defaults, n_defaults, f, std::vector<uint8_t>(n_nodes, 0)};
    c.node(root, 0);
    if (c.rc == QMX_OK && f->prog.size() > FORMULA_MAX_INSTRS) c.fail(QMX_ERR_NOT_SUPPORTED, "formula compiles to more than %u instructions", FORMULA_MAX_INSTRS);
    if (c.rc != QMX_OK) {
        delete f;
        return c.rc;
    }
    f->depth = c.max_depth;
    *out = f;
    return QMX_OK;
}

int32_t qmx_formula_destroy(qmx_formula *formula) {
    if (!formula) return QMX_OK;
    delete formula;
    return QMX_OK;
}

int32_t qmx_formula_rescore(const qmx_formula *formula, const qmx_payload_columns *columns, const qmx_scored_point *lists, const uint32_t *counts,
                            uint32_t n_sources, uint32_t nq, uint32_t stride, uint32_t limit, const float *score_threshold, qmx_scored_point *out,
                            uint32_t *out_counts, uint32_t *out_status, uint32_t *out_error_point) {
    FormulaRescoreArgs a;
    QMX_TRY(rescore_args(formula, lists, counts, n_sources, nq, stride, limit, score_threshold, out, out_counts, out_status, out_error_point, a));
    const int dev = columns ? columns->device : 0;
    QMX_TRY(check_device(dev, nullptr));
    QMX_TRY(formula_program(formula, columns, dev, a.prog));
    if (nq == 0) return QMX_OK;
    Staging st;
    QMX_TRY(st.in(lists, (size_t)n_sources * nq * stride * sizeof(qmx_scored_point), &a.lists));
    QMX_TRY(st.in(counts, (size_t)n_sources * nq * 4, &a.counts));
    QMX_TRY(st.out(out, (size_t)nq * limit * sizeof(qmx_scored_point), &a.out));
    QMX_TRY(st.out(out_counts, (size_t)nq * 4, &a.out_counts));
    QMX_TRY(st.out(out_status, (size_t)nq * 4, &a.out_status));
    QMX_TRY(st.out(out_error_point, (size_t)nq * 4, &a.out_error_point));
    QMX_TRY(launch_formula_rescore(nullptr, a));
    QMX_HIP(hipDeviceSynchronize());
    return st.back();
}

int32_t qmx_formula_rescore_async(const qmx_formula *formula, const qmx_payload_columns *columns, void *hip_stream, const qmx_scored_point *lists_dev,
                                  const uint32_t *counts_dev, uint32_t n_sources, uint32_t nq, uint32_t stride, uint32_t limit,
                                  const float *score_threshold, qmx_scored_point *out_dev, uint32_t *out_counts_dev, uint32_t *out_status_dev,
                                  uint32_t *out_error_point_dev) {
    FormulaRescoreArgs a;
    QMX_TRY(rescore_args(formula, lists_dev, counts_dev, n_sources, nq, stride, limit, score_threshold, out_dev, out_counts_dev, out_status_dev,
                         out_error_point_dev, a));
    const int dev = columns ? columns->device : 0;
    QMX_HIP(hipSetDevice(dev));
    QMX_TRY(formula_program(formula, columns, dev, a.prog));
    return launch_formula_rescore((hipStream_t)hip_stream, a);
}

int32_t qmx_formula_eval(const qmx_formula *formula, const qmx_payload_columns *columns, const uint32_t *ids, uint64_t n, const float *scores,
                         const uint8_t *score_missing, qmx_precise_score *out_precise, float *out_scores, uint32_t *out_status) {
    QMX_REQUIRE(formula && out_status && (n == 0 || ids), QMX_ERR_BAD_ARG, "NULL argument");
    QMX_REQUIRE(n <= 0x7FFFFFFFull * 256, QMX_ERR_NOT_SUPPORTED, "%llu points in one call", (unsigned long long)n);
    FormulaEvalArgs a;
    memset(&a, 0, sizeof(a));
    const int dev = columns ? columns->device : 0;
    QMX_TRY(check_device(dev, nullptr));
    QMX_TRY(formula_program(formula, columns, dev, a.prog));
    if (n == 0) return QMX_OK;
    a.n = n;
    a.n_score_vars = formula->n_score_vars;
    Staging st;
    QMX_TRY(st.in(ids, (size_t)n * 4, &a.ids));
    QMX_TRY(st.in(scores, (size_t)a.n_score_vars * n * 4, &a.scores));
    QMX_TRY(st.in(score_missing, (size_t)a.n_score_vars * n, &a.score_missing));
    QMX_TRY(st.out(out_precise, (size_t)n * 8, &a.out_precise));
    QMX_TRY(st.out(out_scores, (size_t)n * 4, &a.out_scores));
    QMX_TRY(st.out(out_status, (size_t)n * 4, &a.out_status));
    QMX_TRY(launch_formula_eval(nullptr, a));
    QMX_HIP(hipDeviceSynchronize());
    return st.back();
}

}  // extern "C"
