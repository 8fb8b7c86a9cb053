"""A numpy restatement of MMR re-ranking over sparse vectors (test infrastructure, CPU only).

* mmr_from_points_with_vector (lib/shard/src/query/mmr/mod.rs:42-100) builds a volatile sparse storage from the vectors that come off the
  points (:103-140) and scores through SparseMetricQueryScorer::score_sparse = a.score(b).unwrap_or_default()
  (query_scorer/sparse_metric_query_scorer.rs:37-44).  The IndicesTracker never sees these vectors: every sum runs in ascending ORIGINAL index
  order, whatever map the segment's index uses, and a pair without a shared dimension scores 0.0.
* The selection is fusion_reference.mmr_from_points, the pair score sparse_reference.score_pair.

`points[id]` and `query` are (indices, values) pairs with ORIGINAL indices.  `remapped_order=dim_map` restates the WRONG rule on purpose - both
vectors through IndicesTracker::remap_vector first, so that the sums run in ascending remapped id - for the tests that show the two differ."""
import numpy as np

import fusion_reference as FR
from sparse_reference import remap_vector, sort_vector, score_pair


def score(a, b, remapped_order=None):
    ai, av = sort_vector(*a)
    bi, bv = sort_vector(*b)
    if remapped_order is not None:
        ai, av = remap_vector(ai, av, remapped_order)
        bi, bv = remap_vector(bi, bv, remapped_order)
    s, overlap = score_pair(ai, av, bi, bv)
    return s if overlap else np.float32(0.0)


def mmr(points, query, candidates, lambda_, limit, remapped_order=None):
    """One request: `candidates` a ScoredPointOffset list of ids into `points`; the picks in selection order with their input scores."""
    return FR.mmr_from_points(candidates, lambda i: score(query, points[i], remapped_order),
                              lambda c, s: score(points[c], points[s], remapped_order), lambda_, limit)


class Dense:
    """The points as a dense [n, D] array over the ORIGINAL dimensions plus a presence mask: what `mmr_columns` sums column by column."""

    def __init__(self, points, n_dims):
        self.val = np.zeros((len(points), n_dims), dtype=np.float32)
        self.has = np.zeros((len(points), n_dims), dtype=bool)
        for r, (ix, vx) in enumerate(points):
            ix = np.asarray(ix, dtype=np.int64)
            self.val[r, ix] = np.asarray(vx, dtype=np.float32)
            self.has[r, ix] = True

    def scores(self, ids, vector):
        """score(vector, points[id]) for every id: the columns of `vector` in ascending original index, one rounded multiply and one rounded add
        per shared dimension.  Rows without the dimension add +0.0, which changes no bit of a sum that started at +0.0."""
        ix, vx = sort_vector(*vector)
        acc = np.zeros(len(ids), dtype=np.float32)
        with np.errstate(all="ignore"):
            for d, w in zip(ix.tolist(), vx):
                if d < self.val.shape[1]:
                    col = self.has[ids, d]
                    if col.any():
                        acc = acc + np.where(col, self.val[ids, d] * np.float32(w), np.float32(0.0))
        return acc

    def matrix(self, ids):
        """score(points[a], points[b]) for every pair of `ids`, column by column as `scores` (kept for the last `ids` asked)."""
        key = ids.tobytes()
        if getattr(self, "_key", None) != key:
            acc = np.zeros((len(ids), len(ids)), dtype=np.float32)
            with np.errstate(all="ignore"):
                for d in np.flatnonzero(self.has[ids].any(axis=0)).tolist():
                    col, v = self.has[ids, d], self.val[ids, d]
                    acc = acc + np.where(col[:, None] & col[None, :], v[:, None] * v[None, :], np.float32(0.0))
            self._key, self._matrix = key, acc
        return self._matrix

    def point(self, i):
        ix = np.flatnonzero(self.has[i])
        return ix, self.val[i, ix]


def mmr_columns(dense, query, candidates, lambda_, limit, matrix=None):
    """`mmr` for candidate lists too long for the pair-by-pair restatement: the same selection with a running maximum per candidate and whole
    columns of similarities per step (tests/test_sparse_mmr_reference.py holds the two equal).  The similarities come from the matrix of all
    pairs (`matrix`; the default for up to 1 024 candidates, where a request takes many steps) or from one pass over the columns per step.
    No NaN may occur: the vectorised arg-max orders plain floats."""
    candidates = np.asarray(candidates, dtype=FR.ScoredPointOffset)
    _, first = np.unique(candidates["idx"], return_index=True)
    uniq = candidates[np.sort(first)]
    if len(uniq) < 2:
        return uniq
    ids = uniq["idx"].astype(np.int64)
    if matrix is None:
        matrix = len(ids) <= 1024
    rel = dense.scores(ids, query)
    lam, one_minus = np.float32(lambda_), np.float32(1.0) - np.float32(lambda_)
    order = np.arange(len(ids))

    def take(scores):      # the LAST maximal element of the current order, then swap_remove
        nonlocal order
        assert not np.isnan(scores).any()
        p = np.flatnonzero(scores == scores.max())[-1]
        c = order[p]
        order[p] = order[-1]
        order = order[:-1]
        return c

    picked = [take(rel[order])]
    max_sim = None
    with np.errstate(all="ignore"):
        while len(picked) < limit and len(order):
            sim = dense.matrix(ids)[:, picked[-1]] if matrix else dense.scores(ids, dense.point(ids[picked[-1]]))
            max_sim = sim if max_sim is None else np.where(sim >= max_sim, sim, max_sim)
            picked.append(take(lam * rel[order] - one_minus * max_sim[order]))
    return uniq[picked]
