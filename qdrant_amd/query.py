"""Hybrid queries on the device: fusion of prefetch lists (RRF, DBSF), formula rescoring and MMR re-ranking - the last steps of the reference's
Query API (`rrf_scoring`, `score_fusion`, `do_rescore_with_formula`, `mmr_from_points_with_vector`) over lists the dense and sparse searches of
this package return.

A list is a numpy array of ScoredPointOffset as the searches return it; `lists[s][qi]` is the list of source s for query qi.  Offsets are point
offsets of one shared id space (the named vectors of a segment share the id tracker)."""
import ctypes as C
import math
from typing import List, Optional, Sequence

import numpy as np

from . import _ffi as F
from .scorer import RawScorer, ScoredPointOffset, SparseVectorStorage, VectorStorage, new_raw_scorer


def _pack(lists):
    """[n_sources][nq] lists -> ([n_sources][nq][stride] entries, [n_sources][nq] counts)"""
    n_sources = len(lists)
    nq = len(lists[0]) if n_sources else 0
    if any(len(src) != nq for src in lists):
        raise ValueError("every source needs one list per query")
    stride = max([len(l) for src in lists for l in src] + [1])
    packed = np.zeros((n_sources, nq, stride), dtype=ScoredPointOffset)
    counts = np.zeros((n_sources, nq), dtype=np.uint32)
    for s, src in enumerate(lists):
        for qi, l in enumerate(src):
            packed[s, qi, :len(l)] = l
            counts[s, qi] = len(l)
    return packed, counts, nq, stride


def _fusion_params(kind: int, top: int, k: int, weights):
    p = F.FusionParams()
    p.kind, p.rrf_k, p.top = kind, int(k), int(top)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    p.weights, p.n_weights = (None, 0) if w is None else (w.ctypes.data, len(w))
    return p, w      # (w is kept alive by the caller)


def _fuse(lists, kind, top, k, weights, device_id) -> List[np.ndarray]:
    packed, counts, nq, stride = _pack(lists)
    params, keep = _fusion_params(kind, top, k, weights)
    out = np.zeros((nq, top), dtype=ScoredPointOffset)
    oc = np.zeros(nq, dtype=np.uint32)
    F.check(F.lib().qmx_fuse_topk(device_id, F.ptr(packed), F.ptr(counts), len(lists), nq, stride, C.byref(params), F.ptr(out), F.ptr(oc)))
    del keep
    return [out[i, :oc[i]].copy() for i in range(nq)]


def rrf(lists, top: int, k: int = 2, weights: Optional[Sequence[float]] = None, device_id: int = 0) -> List[np.ndarray]:
    """`rrf_scoring(responses, k, weights)` (reciprocal_rank_fusion.rs:54-99) per query, the best `top` kept: score descending, the lower offset
    first among equal scores.  `weights`: None or one per source (another length raises, as the reference rejects it)."""
    return _fuse(lists, F.FUSION_RRF, top, k, weights, device_id)


def dbsf(lists, top: int, weights: Optional[Sequence[float]] = None, device_id: int = 0) -> List[np.ndarray]:
    """`score_fusion(responses, ScoreFusion::dbsf())` (score_fusion.rs:46-94) per query; missing weights are 1.0."""
    return _fuse(lists, F.FUSION_DBSF, top, 0, weights, device_id)


def _mmr(select, scorer, candidates, lambda_, limit):
    if len(candidates) != scorer.nq:
        raise ValueError("one candidate list per request")
    packed, counts, nq, stride = _pack([candidates])
    out = np.zeros((nq, limit), dtype=ScoredPointOffset)
    oc = np.zeros(nq, dtype=np.uint32)
    F.check(select(scorer._h, F.ptr(packed), F.ptr(counts), stride, float(lambda_), int(limit), F.ptr(out), F.ptr(oc)))
    return [out[i, :oc[i]].copy() for i in range(nq)]


def mmr(storage: VectorStorage, vectors, candidates, lambda_: float, limit: int) -> List[np.ndarray]:
    """`mmr_from_points_with_vector` (shard/src/query/mmr/mod.rs:42-100): request qi re-ranks candidates[qi] (a ScoredPointOffset list over
    `storage`, a dense f32 / f16 / u8 storage) for diversity against `vectors[qi]`; the picked candidates in selection order, input scores kept.
    (Sparse storages: `sparse_mmr`.)"""
    scorer = vectors if isinstance(vectors, RawScorer) else new_raw_scorer(vectors, storage)
    try:
        return _mmr(F.lib().qmx_mmr_select, scorer, candidates, lambda_, limit)
    finally:
        if scorer is not vectors:
            scorer.close()


def sparse_mmr(storage: SparseVectorStorage, vectors, candidates, lambda_: float, limit: int, idf=None) -> List[np.ndarray]:
    """`mmr` over a SparseVectorStorage: `vectors` are the requests' sparse mmr vectors, (indices, values) pairs (or CSR arrays), or a RawScorer
    made over `storage`; `idf` as new_raw_scorer takes it.  Relevance and similarity are `score_vectors` sums in ascending ORIGINAL index order
    (0.0 without a shared dimension), over the stored f32 rows whatever the index weights are."""
    if not isinstance(storage, SparseVectorStorage):
        raise ValueError("sparse_mmr needs a SparseVectorStorage (dense storages: mmr)")
    scorer = vectors if isinstance(vectors, RawScorer) else new_raw_scorer(vectors, storage, idf=idf)
    try:
        return _mmr(F.lib().qmx_sparse_mmr_select, scorer, candidates, lambda_, limit)
    finally:
        if scorer is not vectors:
            scorer.close()


# ---- formula rescoring ("score boosting"): Query::Formula ----------------------------------------------------------------------------------

class FormulaError(RuntimeError):
    """The reference fails a formula request on the first point whose evaluation fails: `request` = its index in the batch, `point` = the lowest
    failing offset, `code` = F.FORMULA_NON_FINITE / FORMULA_NO_VALUE / FORMULA_BAD_VALUE."""

    def __init__(self, request: int, point: int, code: int):
        self.request, self.point, self.code = int(request), int(point), int(code)
        name = F.FORMULA_STATUS_NAMES[self.code] if 0 <= self.code < len(F.FORMULA_STATUS_NAMES) else str(self.code)
        super().__init__("formula request %d: point %d failed with %s" % (self.request, self.point, name))


def decay_params_to_lambda(kind: str, midpoint: Optional[float] = None, scale: Optional[float] = None) -> float:
    """`ParsedExpression::decay_params_to_lambda` (parsed_formula.rs:186-224) in float64: midpoint and scale arrive as f32 (defaults 0.5 and 1.0)
    and are widened; the reference's validation errors are ValueError."""
    midpoint = float(np.float32(0.5 if midpoint is None else midpoint))
    scale = float(np.float32(1.0 if scale is None else scale))
    if kind == "lin":
        if not 0.0 <= midpoint <= 1.0:
            raise ValueError("Linear decay midpoint should be in the range [0.0, 1.0], got %r." % midpoint)
    elif kind in ("gauss", "exp"):
        if midpoint <= 0.0 or midpoint >= 1.0 or midpoint != midpoint:
            raise ValueError("Decay midpoint should be in the range (0.0, 1.0), got %r." % midpoint)
    else:
        raise ValueError("decay kind %r" % (kind,))
    if scale <= 0.0:
        raise ValueError("Decay scale should be non-zero positive, got %r." % scale)
    if kind == "lin":
        return (1.0 - midpoint) / scale
    if kind == "exp":
        return math.log(midpoint) / scale
    return math.log(midpoint) / (scale * scale)      # powi(2)


# The expression builder: a ParsedExpression (parsed_formula.rs:55-92) as a plain tree of tuples, (op, ...).
def const(value):
    return ("const", float(value))


def score(index: int = 0):
    return ("score", int(index))


def payload(name: str):
    return ("payload", name)


def condition(name: str):
    return ("condition", name)


def geo_distance(origin, name: str):
    """Haversine metres between `origin` = (lat, lon) and geo column `name`."""
    return ("geo_distance", (float(origin[0]), float(origin[1])), name)


def datetime(value):
    """Seconds of a constant given as integer microseconds since the epoch, or of datetime column `value` (a name)."""
    return ("datetime_key", value) if isinstance(value, str) else ("datetime", int(value))


def sum_(*terms):
    return ("sum", list(terms))


def mult(*factors):
    return ("mult", list(factors))


def div(left, right, by_zero_default: Optional[float] = None):
    return ("div", left, right, None if by_zero_default is None else float(by_zero_default))


def neg(x):
    return ("neg", x)


def sqrt(x):
    return ("sqrt", x)


def pow_(base, exponent):
    return ("pow", base, exponent)


def exp(x):
    return ("exp", x)


def log10(x):
    return ("log10", x)


def ln(x):
    return ("ln", x)


def abs_(x):
    return ("abs", x)


def _decay(kind, x, target, midpoint, scale):
    return ("decay", kind, x, target, decay_params_to_lambda(kind, midpoint, scale))


def lin_decay(x, target=None, midpoint: Optional[float] = None, scale: Optional[float] = None):
    return _decay("lin", x, target, midpoint, scale)


def gauss_decay(x, target=None, midpoint: Optional[float] = None, scale: Optional[float] = None):
    return _decay("gauss", x, target, midpoint, scale)


def exp_decay(x, target=None, midpoint: Optional[float] = None, scale: Optional[float] = None):
    return _decay("exp", x, target, midpoint, scale)


def _bitmap(bits, n_points):
    """None, a bool array over the points, or u64 words as they are -> u64 words (BitSlice<u64, Lsb0>)."""
    if bits is None:
        return None
    bits = np.asarray(bits)
    n_words = (n_points + 63) // 64
    if bits.dtype == np.uint64:
        if len(bits) != n_words:
            raise ValueError("a bitmap over %d points holds %d words" % (n_points, n_words))
        return np.ascontiguousarray(bits)
    if len(bits) != n_points:
        raise ValueError("one flag per point")
    padded = np.zeros(n_words * 64, dtype=np.uint8)
    padded[:n_points] = bits.astype(bool)
    return np.packbits(padded, bitorder="little").view(np.uint64)


class PayloadColumns:
    """Payload as the device reads it (qmx_payload_columns): named columns over the point offsets 0..n_points.
      numbers   {name: values | (values, present, invalid)}            float64 values
      geo       {name: (lat, lon) | (lat, lon, present, invalid)}      float64 degrees
      datetimes {name: micros | (micros, present, invalid)}            int64 microseconds since the epoch
      conditions{name: flags}                                          what the condition's checker returned per point
    `present` / `invalid` / `flags`: bool arrays over the points (or u64 bitmap words); present None = every point has exactly one value, invalid =
    a value of the wrong type or several values.  A point in neither has no value and takes the formula's default."""

    def __init__(self, n_points: int, numbers=None, geo=None, datetimes=None, conditions=None, device_id: int = 0):
        self.n_points, self.device_id = int(n_points), device_id
        self.index, self.kinds = {}, []
        keep, cols = [], []

        def add(name, kind, data, data2, present, invalid):
            if name in self.index:
                raise ValueError("column %r given twice" % (name,))
            c = F.PayloadColumn()
            c.kind = kind
            arrays = [data, data2, _bitmap(present, self.n_points), _bitmap(invalid, self.n_points)]
            for a in arrays[:2]:
                if a is not None and kind != F.PAYLOAD_CONDITION and len(a) != self.n_points:
                    raise ValueError("column %r: one value per point" % (name,))
            c.data, c.data2, c.present, c.invalid = [None if a is None else a.ctypes.data for a in arrays]
            keep.extend(arrays)
            self.index[name] = len(cols)
            self.kinds.append(kind)
            cols.append(c)

        def split(v, n_values):
            v = v if isinstance(v, tuple) else (v,)
            if len(v) not in (n_values, n_values + 2):
                raise ValueError("a column is its value arrays, or those with (present, invalid)")
            return v + (None, None) if len(v) == n_values else v

        for name, v in (numbers or {}).items():
            values, present, invalid = split(v, 1)
            add(name, F.PAYLOAD_NUMBER, np.ascontiguousarray(values, dtype=np.float64), None, present, invalid)
        for name, v in (geo or {}).items():
            lat, lon, present, invalid = split(v, 2)
            add(name, F.PAYLOAD_GEO, np.ascontiguousarray(lat, dtype=np.float64), np.ascontiguousarray(lon, dtype=np.float64), present, invalid)
        for name, v in (datetimes or {}).items():
            micros, present, invalid = split(v, 1)
            add(name, F.PAYLOAD_DATETIME, np.ascontiguousarray(micros, dtype=np.int64), None, present, invalid)
        for name, flags in (conditions or {}).items():
            add(name, F.PAYLOAD_CONDITION, _bitmap(flags, self.n_points), None, None, None)
        arr = (F.PayloadColumn * max(len(cols), 1))(*cols)
        self._h = C.c_void_p()
        F.check(F.lib().qmx_payload_columns_create(device_id, self.n_points, arr, len(cols), C.byref(self._h)))
        del keep      # (the handle holds device copies)

    def close(self):
        if self._h:
            F.lib().qmx_payload_columns_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_UNARY = {"neg": F.FORMULA_NEG, "sqrt": F.FORMULA_SQRT, "exp": F.FORMULA_EXP, "log10": F.FORMULA_LOG10, "ln": F.FORMULA_LN, "abs": F.FORMULA_ABS}
_DECAYS = {"lin": F.DECAY_LIN, "gauss": F.DECAY_GAUSS, "exp": F.DECAY_EXP}


class CompiledFormula:
    """An expression tree handed to the library (qmx_formula): `defaults` = {("score", i) | column name: number | (lat, lon) | datetime micros}."""

    def __init__(self, expr, columns: Optional[PayloadColumns] = None, defaults=None):
        nodes, keep = [], []

        def column(name):
            if columns is None or name not in columns.index:
                raise KeyError("the formula names column %r, the payload columns do not hold it" % (name,))
            return columns.index[name]

        def add(op, var=0, children=(), flags=0, value=0.0, value2=0.0, micros=0):
            n = F.FormulaNode()
            n.op, n.var, n.n_children, n.flags, n.value, n.value2, n.micros = op, var, len(children), flags, value, value2, micros
            if children:
                kids = np.asarray(children, dtype=np.uint32)
                keep.append(kids)
                n.children = kids.ctypes.data
            nodes.append(n)
            return len(nodes) - 1

        def walk(e):
            op = e[0]
            if op == "const":
                return add(F.FORMULA_CONSTANT, value=e[1])
            if op == "score":
                return add(F.FORMULA_SCORE, var=e[1])
            if op == "payload":
                return add(F.FORMULA_PAYLOAD, var=column(e[1]))
            if op == "condition":
                return add(F.FORMULA_CONDITION, var=column(e[1]))
            if op == "geo_distance":
                return add(F.FORMULA_GEO_DISTANCE, var=column(e[2]), value=e[1][0], value2=e[1][1])
            if op == "datetime":
                return add(F.FORMULA_DATETIME, micros=e[1])
            if op == "datetime_key":
                return add(F.FORMULA_DATETIME_KEY, var=column(e[1]))
            if op in ("sum", "mult"):
                return add(F.FORMULA_SUM if op == "sum" else F.FORMULA_MULT, children=[walk(c) for c in e[1]])
            if op == "div":
                kids = [walk(e[1]), walk(e[2])]
                return add(F.FORMULA_DIV, children=kids, flags=0 if e[3] is None else 1, value=0.0 if e[3] is None else e[3])
            if op == "pow":
                return add(F.FORMULA_POW, children=[walk(e[1]), walk(e[2])])
            if op in _UNARY:
                return add(_UNARY[op], children=[walk(e[1])])
            if op == "decay":
                kids = [walk(e[2])] + ([] if e[3] is None else [walk(e[3])])
                return add(F.FORMULA_DECAY, var=_DECAYS[e[1]], children=kids, value=e[4])
            raise ValueError("unknown formula op %r" % (op,))

        root = walk(expr)
        ds = []
        for key, v in (defaults or {}).items():
            d = F.FormulaDefault()
            if isinstance(key, tuple) and key[0] == "score":
                d.is_column, d.index, d.kind, d.value = 0, int(key[1]), F.PAYLOAD_NUMBER, float(v)
            else:
                d.is_column, d.index, d.kind = 1, column(key), columns.kinds[column(key)]
                if d.kind == F.PAYLOAD_GEO:
                    d.value, d.value2 = float(v[0]), float(v[1])
                elif d.kind == F.PAYLOAD_DATETIME:
                    d.micros = int(v)
                elif d.kind == F.PAYLOAD_NUMBER:
                    d.value = float(v)
                else:
                    raise ValueError("there are no defaults for conditions")
            ds.append(d)
        self.columns = columns
        self._h = C.c_void_p()
        F.check(F.lib().qmx_formula_create((F.FormulaNode * len(nodes))(*nodes), len(nodes), root, (F.FormulaDefault * max(len(ds), 1))(*ds), len(ds),
                                           C.byref(self._h)))
        del keep

    def close(self):
        if self._h:
            F.lib().qmx_formula_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _compiled(formula, columns, defaults):
    if isinstance(formula, CompiledFormula):
        return formula, False
    return CompiledFormula(formula, columns, defaults), True


def _raise_first_error(status, points):
    bad = np.nonzero(status)[0]
    if len(bad):
        raise FormulaError(bad[0], points[bad[0]], status[bad[0]])


def formula_rescore(lists, formula, columns: Optional[PayloadColumns], limit: int, score_threshold: Optional[float] = None,
                    defaults=None) -> List[np.ndarray]:
    """`do_rescore_with_formula` (formula_rescore.rs:29-104) per request: the distinct ids of the request's lists are scored by `formula` (an
    expression tree of this module's builders, or a CompiledFormula) over `columns`, those with score >= score_threshold kept, the best `limit`
    returned: score descending, the lower offset first among equal scores.  Raises FormulaError for the first request with a failing point."""
    packed, counts, nq, stride = _pack(lists)
    f, mine = _compiled(formula, columns, defaults)
    try:
        out = np.zeros((nq, limit), dtype=ScoredPointOffset)
        oc, status, points = (np.zeros(nq, dtype=np.uint32) for _ in range(3))
        thr = None if score_threshold is None else C.byref(C.c_float(score_threshold))
        F.check(F.lib().qmx_formula_rescore(f._h, columns._h if columns is not None else None, F.ptr(packed), F.ptr(counts), len(lists), nq, stride,
                                            int(limit), thr, F.ptr(out), F.ptr(oc), F.ptr(status), F.ptr(points)))
    finally:
        if mine:
            f.close()
    _raise_first_error(status, points)
    return [out[i, :oc[i]].copy() for i in range(nq)]


def formula_eval(formula, columns: Optional[PayloadColumns], ids, scores=None, score_missing=None, defaults=None):
    """`FormulaScorer::score` for explicit points (qmx_formula_eval): `scores` [n_score_vars][n] float32 and `score_missing` (same shape, True =
    the point is not in that prefetch), both optional.  Returns (the float64 values before the cast, the float32 scores, the status per point)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    n = len(ids)
    scores = None if scores is None else np.ascontiguousarray(scores, dtype=np.float32).reshape(-1, n)
    score_missing = None if score_missing is None else np.ascontiguousarray(score_missing, dtype=np.uint8).reshape(-1, n)
    f, mine = _compiled(formula, columns, defaults)
    try:
        precise, out, status = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint32)
        F.check(F.lib().qmx_formula_eval(f._h, columns._h if columns is not None else None, F.ptr(ids), n, F.ptr(scores), F.ptr(score_missing),
                                         F.ptr(precise), F.ptr(out), F.ptr(status)))
    finally:
        if mine:
            f.close()
    return precise, out, status


class Formula:
    """The formula stage of hybrid_search (Query::Formula): `expr` over `columns`, kept when score >= score_threshold."""

    def __init__(self, expr, columns: Optional[PayloadColumns] = None, defaults=None, score_threshold: Optional[float] = None):
        self.compiled, self._mine = _compiled(expr, columns, defaults)
        self.columns, self.score_threshold = columns, score_threshold


class Rrf:
    """Fusion::Rrf of hybrid_search: `k` and optional per-source weights."""

    def __init__(self, k: int = 2, weights: Optional[Sequence[float]] = None):
        self.kind, self.k, self.weights = F.FUSION_RRF, k, weights


class Dbsf:
    """Fusion::Dbsf of hybrid_search: optional per-source weights."""

    def __init__(self, weights: Optional[Sequence[float]] = None):
        self.kind, self.k, self.weights = F.FUSION_DBSF, 0, weights


class Mmr:
    """The MMR stage of hybrid_search: `scorer` = the Nearest batch of the requests' mmr vectors (new_raw_scorer) over the dense storage, or over
    the SparseVectorStorage when `mmr.using` names the sparse vector."""

    def __init__(self, scorer: RawScorer, lambda_: float, limit: int):
        self.scorer, self.lambda_, self.limit = scorer, float(lambda_), int(limit)


def hybrid_search(sources, fusion, top: int, mmr: Optional[Mmr] = None, device_id: int = 0, sparse_idf=None) -> List[np.ndarray]:
    """One hybrid request batch without a host round trip between its stages.  `sources`: (scorer, prefetch limit) pairs - query batches of the
    same size made by new_raw_scorer over a dense VectorStorage or a SparseVectorStorage on one device; `fusion`: Rrf(...), Dbsf(...) or
    Formula(...) (whose first failing request raises FormulaError after the synchronisation); `mmr`: an optional Mmr stage over the fused list.  Every search, the fusion and the MMR selection are enqueued on one stream, which is synchronised
    once.  (All sources search the largest prefetch limit; a source with a smaller one has its counts clamped - a top list's head is the shorter
    top list.)  A sparse source may be given as ((SparseVectorStorage, queries), prefetch limit): its query batch is then made here, with
    `sparse_idf` as the IDF modifier (True, a corpus mask or merged statistics, as SparseVectorStorage.search takes them)."""
    import torch
    if not sources:
        raise ValueError("no sources")
    made = []
    for i, (s, limit) in enumerate(sources):
        if isinstance(s, tuple):
            storage, queries = s
            made.append(new_raw_scorer(queries, storage, idf=sparse_idf))
            sources = list(sources)
            sources[i] = (made[-1], limit)
    if sparse_idf is not None and not made:
        raise ValueError("sparse_idf needs a sparse source given as ((storage, queries), limit)")
    nq = sources[0][0].nq
    if any(s.nq != nq for s, _ in sources) or (mmr is not None and mmr.scorer.nq != nq):
        raise ValueError("every stage needs the same number of queries")
    limits = [int(l) for _, l in sources]
    stride = max(limits)
    dev = torch.device("cuda", device_id)
    stream = torch.cuda.Stream(dev)
    lib = F.lib()
    is_formula = isinstance(fusion, Formula)
    params, keep = (None, None) if is_formula else _fusion_params(fusion.kind, top, fusion.k, fusion.weights)
    scorers = [s for s, _ in sources] + ([mmr.scorer] if mmr is not None else [])
    with torch.cuda.stream(stream):
        lists = torch.empty((len(sources), nq, stride), dtype=torch.int64, device=dev)      # ScoredPointOffset entries (8 bytes)
        counts = torch.zeros((len(sources), nq), dtype=torch.int32, device=dev)
        fused = torch.empty((nq, top), dtype=torch.int64, device=dev)
        fcounts = torch.zeros(nq, dtype=torch.int32, device=dev)
        result, rcounts = fused, fcounts
        try:
            for s in scorers:
                F.check(lib.qmx_query_set_stream(s._h, C.c_void_p(stream.cuda_stream)))
            for i, (s, limit) in enumerate(sources):
                F.check(lib.qmx_search_topk_async(s._h, stride, None, 0, F.ptr(lists[i]), F.ptr(counts[i])))
                if limit < stride:
                    counts[i].clamp_(max=limit)
            if is_formula:
                fstatus = torch.zeros((2, nq), dtype=torch.int32, device=dev)      # status and failing offset per request
                thr = None if fusion.score_threshold is None else C.byref(C.c_float(fusion.score_threshold))
                F.check(lib.qmx_formula_rescore_async(fusion.compiled._h, fusion.columns._h if fusion.columns is not None else None,
                                                      C.c_void_p(stream.cuda_stream), F.ptr(lists), F.ptr(counts), len(sources), nq, stride, top, thr,
                                                      F.ptr(fused), F.ptr(fcounts), F.ptr(fstatus[0]), F.ptr(fstatus[1])))
                h_status = torch.empty(fstatus.shape, dtype=fstatus.dtype, pin_memory=True)
                h_status.copy_(fstatus, non_blocking=True)
            else:
                F.check(lib.qmx_fuse_topk_async(device_id, C.c_void_p(stream.cuda_stream), F.ptr(lists), F.ptr(counts), len(sources), nq, stride,
                                                C.byref(params), F.ptr(fused), F.ptr(fcounts)))
            if mmr is not None:
                result = torch.empty((nq, mmr.limit), dtype=torch.int64, device=dev)
                rcounts = torch.zeros(nq, dtype=torch.int32, device=dev)
                select = lib.qmx_sparse_mmr_select_async if isinstance(mmr.scorer.storage, SparseVectorStorage) else lib.qmx_mmr_select_async
                F.check(select(mmr.scorer._h, F.ptr(fused), F.ptr(fcounts), top, mmr.lambda_, mmr.limit, F.ptr(result), F.ptr(rcounts)))
            out = torch.empty(result.shape, dtype=result.dtype, pin_memory=True)
            oc = torch.empty(rcounts.shape, dtype=rcounts.dtype, pin_memory=True)
            out.copy_(result, non_blocking=True)
            oc.copy_(rcounts, non_blocking=True)
        finally:
            stream.synchronize()      # the one synchronisation of the request batch
            for s in scorers:
                lib.qmx_query_set_stream(s._h, None)
            for s in made:
                s.close()
    del keep
    if is_formula:
        h_status = h_status.numpy().view(np.uint32)
        _raise_first_error(h_status[0], h_status[1])
    # (a fused id past the MMR storage's rows empties that request's MMR list; the next synchronous call on mmr.scorer reports it)
    out = out.numpy().view(ScoredPointOffset).reshape(nq, -1)
    oc = oc.numpy()
    return [out[i, :oc[i]].copy() for i in range(nq)]
