"""A numpy restatement of the reference's sparse-vector scoring and Nearest search (test infrastructure, CPU only).

* score_vectors (lib/sparse/src/common/sparse_vector.rs:66-90): both index lists ascending, `score += a * b` over the shared dimensions from
  0.0, the multiply and the add rounded separately (f32); no shared dimension -> None, which the raw scorer turns into 0.0
  (lib/segment/src/vector_storage/query_scorer/sparse_metric_query_scorer.rs:43).
* Vectors are sorted by index on the way in (lib/segment/src/data_types/vectors.rs:71-78); duplicate indices are invalid
  (sparse_vector.rs:302-323).
* IndicesTracker (lib/segment/src/index/sparse_index/indices_tracker.rs:39-73): `remap_vector` maps every index, drops the unknown ones and
  re-sorts, so the index paths sum in ascending REMAPPED id order.
* Nearest (lib/sparse/src/index/search_context.rs:92-143 plain_search, :146-187 advance_batch): only points that share a dimension with the
  query; TopK (lib/common/common/src/top_k.rs:21-64) orders by score only, the device breaks ties by the lower offset.

`Restatement.score_matrix` works dimension-major, as the issue describes it: per query, dimensions in ascending order, float32 arrays,
`score[rows_with_d] += w * q` plus an overlap mask.  `score_pair` is the per-pair sequential merge loop it must equal bit for bit.
"""
import numpy as np

ScoredPointOffset = np.dtype([("idx", np.uint32), ("score", np.float32)])


def sort_vector(indices, values):
    """(indices, values) sorted by index; ValueError on a duplicate index or a length mismatch."""
    idx = np.asarray(indices, dtype=np.uint32)
    val = np.asarray(values, dtype=np.float32)
    if len(idx) != len(val):
        raise ValueError("values must be the same length as indices")
    order = np.argsort(idx, kind="stable")
    idx, val = idx[order], val[order]
    if len(idx) > 1 and np.any(idx[1:] == idx[:-1]):
        raise ValueError("indices must be unique")
    return idx, val


def remap_vector(indices, values, dim_map):
    """IndicesTracker::remap_vector: known indices mapped, unknown ones dropped, re-sorted by the remapped id."""
    keep = [(dim_map[int(i)], v) for i, v in zip(indices, values) if int(i) in dim_map]
    if not keep:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32)
    return sort_vector([k for k, _ in keep], [v for _, v in keep])


def score_pair(ai, av, bi, bv):
    """score_vectors as the reference writes it: returns (score, overlap)."""
    s = np.float32(0.0)
    overlap = False
    i = j = 0
    while i < len(ai) and j < len(bi):
        if ai[i] < bi[j]:
            i += 1
        elif ai[i] > bi[j]:
            j += 1
        else:
            overlap = True
            s = np.float32(s + np.float32(np.float32(av[i]) * np.float32(bv[j])))
            i += 1
            j += 1
    return s, overlap


class Restatement:
    """Stored rows (sorted, remapped under `dim_map`) and a dimension-major index of them."""

    def __init__(self, rows, dim_map=None):
        """rows: (indices, values) pairs, or CSR arrays (offsets, indices, values) whose rows are sorted already (no map)."""
        self.dim_map = dict(dim_map) if dim_map is not None else None
        if isinstance(rows, tuple):
            self._init_csr(*rows)
            return
        self.rows = []
        for ix, vx in rows:
            ix, vx = sort_vector(ix, vx)
            if self.dim_map is not None:
                if any(int(i) not in self.dim_map for i in ix):
                    raise ValueError("stored index not in the map")
                ix, vx = remap_vector(ix, vx, self.dim_map)
            self.rows.append((ix, vx))
        self.n = len(self.rows)
        lens = np.array([len(r[0]) for r in self.rows], dtype=np.int64)
        all_idx = np.concatenate([r[0] for r in self.rows]) if lens.sum() else np.zeros(0, dtype=np.uint32)
        all_val = np.concatenate([r[1] for r in self.rows]) if lens.sum() else np.zeros(0, dtype=np.float32)
        all_row = np.repeat(np.arange(self.n, dtype=np.int64), lens)
        order = np.argsort(all_idx, kind="stable")
        self._dims, starts = np.unique(all_idx[order], return_index=True)
        self._starts = np.append(starts, len(order))
        self._post_rows, self._post_w = all_row[order], all_val[order]

    def _init_csr(self, off, idx, val):
        off = np.asarray(off, dtype=np.int64)
        self.n = len(off) - 1
        lens = np.diff(off)
        row = np.repeat(np.arange(self.n, dtype=np.int64), lens)
        assert not np.any((row[1:] == row[:-1]) & (idx[1:] <= idx[:-1])), "CSR rows must be sorted and unique"
        self.rows = None
        order = np.argsort(idx, kind="stable")
        self._dims, starts = np.unique(idx[order], return_index=True)
        self._starts = np.append(starts, len(order))
        self._post_rows, self._post_w = row[order], np.asarray(val, dtype=np.float32)[order]

    def prepare_query(self, indices, values):
        ix, vx = sort_vector(indices, values)
        if self.dim_map is not None:
            ix, vx = remap_vector(ix, vx, self.dim_map)
        return ix, vx

    def postings(self, d):
        k = np.searchsorted(self._dims, d)
        if k == len(self._dims) or self._dims[k] != d:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
        a, b = self._starts[k], self._starts[k + 1]
        return self._post_rows[a:b], self._post_w[a:b]

    def score_matrix(self, queries):
        """queries: prepared (indices, values) pairs -> (scores [nq, n] f32, overlap [nq, n] bool)."""
        scores = np.zeros((len(queries), self.n), dtype=np.float32)
        overlap = np.zeros((len(queries), self.n), dtype=bool)
        for qi, (ix, vx) in enumerate(queries):
            for d, w in zip(ix, vx):          # ascending dimension order
                rows, pw = self.postings(d)
                if len(rows):
                    scores[qi, rows] = scores[qi, rows] + pw * np.float32(w)
                    overlap[qi, rows] = True
        return scores, overlap

    def search(self, queries, top, ids=None, live=None):
        """Nearest: per query the `top` best (score desc, lower offset first) overlapping points among `ids` (all points when None) that `live` allows."""
        scores, overlap = self.score_matrix(queries)
        cand = np.zeros(self.n, dtype=bool)
        if ids is None:
            cand[:] = True
        else:
            ids = np.asarray(ids, dtype=np.int64)
            cand[ids[ids < self.n]] = True
        if live is not None:
            cand &= live
        out = []
        for qi in range(len(queries)):
            sel = np.flatnonzero(cand & overlap[qi])
            order = np.lexsort((sel, -scores[qi, sel].astype(np.float64)))[:top]
            r = np.zeros(len(order), dtype=ScoredPointOffset)
            r["idx"] = sel[order]
            r["score"] = scores[qi, sel[order]]
            out.append(r)
        return out
