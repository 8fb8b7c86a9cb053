"""A numpy restatement of the custom queries over sparse vectors (test infrastructure, CPU only).

* SparseCustomQueryScorer (lib/segment/src/vector_storage/query_scorer/sparse_custom_query_scorer.rs):
  `score(point) = query.score_by(|example| example.score(point).unwrap_or(0.0))`.  `new` sorts every example by index and scores it against the
  vector STORAGE: the IndicesTracker never sees it, so each example's sum runs in ascending ORIGINAL index order (Nearest, through the index,
  sums in remapped order - sparse_reference.Restatement.score_matrix).
* Query::score_by of the five kinds (reco_query.rs:68-92, 114-131; discover_query.rs:45-73; context_query.rs:53-62, 112-118;
  feedback_query.rs:198-226), vectorised over the points: `score_by(kind, n_a, n_b, sims [examples, n])`, float32 throughout, `total_cmp` through
  the int32 view, `fast_sigmoid` as x / (1 + |x|), sequential sums in example order.
* search_scored (sparse_vector_index/read_view/search.rs:99-151): peek_top_iter over every live point (or the id list), overlap or not.
"""
import numpy as np

from sparse_reference import ScoredPointOffset, sort_vector

BEST_SCORE, SUM_SCORES, DISCOVER, CONTEXT, FEEDBACK = range(5)
EPSILON = np.float32(1.1920929e-07)      # ScoreType::EPSILON


def total_cmp(a, b):
    """f32::total_cmp elementwise: -1 / 0 / 1 (int32)."""
    def key(x):
        k = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).copy()
        k ^= ((k >> 31).view(np.uint32) >> np.uint32(1)).view(np.int32)
        return k
    x, y = key(a), key(b)
    return (x > y).astype(np.int32) - (x < y).astype(np.int32)


def fast_sigmoid(x):
    return (x / (np.float32(1.0) + np.abs(x))).astype(np.float32)


def scaled_fast_sigmoid(x):
    return (np.float32(0.5) * (fast_sigmoid(x) + np.float32(1.0))).astype(np.float32)


def n_examples(kind, n_a, n_b):
    return n_a + n_b if kind <= SUM_SCORES else n_a + 2 * n_b


def score_by(kind, n_a, n_b, sims, coefs=None):
    """sims [examples, n] float32 in flat_iter() order (reco: positives, negatives; discover / feedback: target, then (positive, negative)
    per pair; context: pairs) -> scores [n] float32.  coefs (feedback): [a, partial_computation_0, ...]."""
    sims = np.asarray(sims, dtype=np.float32)
    ne = n_examples(kind, n_a, n_b)
    assert sims.shape[0] == ne, (sims.shape, ne)
    n = sims.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == BEST_SCORE:
            best = [np.full(n, -np.inf, dtype=np.float32), np.full(n, -np.inf, dtype=np.float32)]
            for e in range(ne):
                side = 0 if e < n_a else 1
                best[side] = np.where(total_cmp(sims[e], best[side]) > 0, sims[e], best[side])
            return np.where(best[0] > best[1], scaled_fast_sigmoid(best[0]), -scaled_fast_sigmoid(best[1])).astype(np.float32)
        if kind == SUM_SCORES:
            pos, neg = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
            for e in range(ne):
                if e < n_a:
                    pos = pos + sims[e]
                else:
                    neg = neg + sims[e]
            return pos - neg
        if kind == DISCOVER:
            rank = np.zeros(n, dtype=np.int32)
            for p in range(n_b):
                rank += total_cmp(sims[1 + 2 * p], sims[2 + 2 * p])
            return rank.astype(np.float32) + scaled_fast_sigmoid(sims[0])
        if kind == CONTEXT:
            acc = np.zeros(n, dtype=np.float32)
            for p in range(n_b):
                difference = sims[2 * p] - sims[2 * p + 1] - EPSILON
                acc = acc + fast_sigmoid(np.fmin(difference, np.float32(0.0)))
            return acc
        assert kind == FEEDBACK
        coefs = np.asarray(coefs, dtype=np.float32)
        score = coefs[0] * sims[0]
        for p in range(n_b):
            delta = sims[1 + 2 * p] - sims[2 + 2 * p]
            score = score + coefs[1 + p] * delta
        return score.astype(np.float32)


def original_order_sims(restatement, example, ids=None):
    """score_vectors of one example (indices, values; original indices) with every stored row (or rows `ids`), the example's dimensions in
    ascending ORIGINAL index; under the restatement's map the remapped postings are looked up, dimensions the map lacks contribute nothing;
    0.0 without overlap."""
    ix, vx = sort_vector(*example)
    sims = np.zeros(restatement.n, dtype=np.float32)
    for i, v in zip(ix, vx):
        d = int(i)
        if restatement.dim_map is not None:
            if d not in restatement.dim_map:
                continue
            d = restatement.dim_map[d]
        rows, pw = restatement.postings(d)
        if len(rows):
            sims[rows] = sims[rows] + pw * np.float32(v)
    return sims if ids is None else sims[np.asarray(ids, dtype=np.int64)]


def custom_scores(restatement, query, ids=None):
    """One custom query (an object with kind, n_a, n_b, examples = (indices, values) pairs in flat_iter() order, coefs) against the rows `ids`
    (every row when None): scores [n] float32."""
    n = restatement.n if ids is None else len(ids)
    sims = np.zeros((len(query.examples), n), dtype=np.float32)
    for e, ex in enumerate(query.examples):
        sims[e] = original_order_sims(restatement, ex, ids)
    return score_by(query.kind, query.n_a, query.n_b, sims, query.coefs)


def search(restatement, query, top, ids=None, live=None):
    """search_scored: the `top` best (score descending, lower offset first) among `ids` (every point when None) that `live` allows."""
    scores = custom_scores(restatement, query)
    cand = np.zeros(restatement.n, dtype=bool)
    if ids is None:
        cand[:] = True
    else:
        ids = np.asarray(ids, dtype=np.int64)
        cand[ids[ids < restatement.n]] = True
    if live is not None:
        cand &= live
    sel = np.flatnonzero(cand)
    order = np.lexsort((sel, -scores[sel].astype(np.float64)))[:top]
    r = np.zeros(len(order), dtype=ScoredPointOffset)
    r["idx"] = sel[order]
    r["score"] = scores[sel[order]]
    return r
