"""Custom queries (recommend / discover / context / feedback) over sparse vectors on the device (qmx_sparse_custom_score_points,
qmx_sparse_custom_search_topk; sparse.hip) against the numpy restatement of tests/sparse_custom_reference.py.  Every comparison is on the
uint32 view of the scores and id for id (score descending, lower offset first): no tolerance anywhere."""
import numpy as np
import pytest

import qdrant_amd as qa
from qdrant_amd import _ffi as F
import sparse_reference as SR
import sparse_custom_reference as SCR

pytestmark = pytest.mark.gpu


def _zipf_rows(seed, n, n_dims, nnz, signed=False, integer=False, base=0):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_dims + 1) ** 1.1
    p /= p.sum()
    rows = []
    for _ in range(n):
        k = int(rng.integers(0, nnz + 1))
        ix = (rng.choice(n_dims, size=min(k, n_dims), replace=False, p=p) + base).astype(np.uint32)
        if integer:
            vx = rng.integers(1, 4, len(ix)).astype(np.float32)
        elif signed:
            vx = rng.standard_normal(len(ix)).astype(np.float32)
        else:
            vx = rng.lognormal(0.0, 1.0, len(ix)).astype(np.float32)
        rows.append((ix, vx))
    return rows


def _all_kinds(seed, n_dims, nnz, **kw):
    """Every kind in one batch: best score with positives only / negatives only / both, sum scores, discover with three pairs, context with four
    pairs and with none, feedback with six pairs and with none."""
    ex = _zipf_rows(seed, 40, n_dims, nnz, **kw)
    pairs = lambda a, k: [(ex[a + 2 * i], ex[a + 2 * i + 1]) for i in range(k)]
    return [
        qa.CustomQuery.recommend_best_score(ex[0:3], []),
        qa.CustomQuery.recommend_best_score([], ex[3:6]),
        qa.CustomQuery.recommend_best_score(ex[6:8], ex[8:10]),
        qa.CustomQuery.recommend_sum_scores(ex[10:13], ex[13:15]),
        qa.CustomQuery.discover(ex[15], pairs(16, 3)),
        qa.CustomQuery.context(pairs(22, 4)),
        qa.CustomQuery.context([]),
        qa.CustomQuery.feedback_naive(ex[30], [(ex[31], 0.9), (ex[32], 0.5), (ex[33], 0.2), (ex[34], -0.3)], a=0.7, b=1.5, c=0.4),
        qa.CustomQuery.feedback_naive(ex[35], [(ex[36], 0.5)], a=-1.25, b=1.0, c=1.0),
    ]


def _check_scores(got, ref, queries, ids):
    assert got.shape == (len(queries), len(ids)) and got.dtype == np.float32
    for qi, q in enumerate(queries):
        want = SCR.custom_scores(ref, q, ids)
        assert np.array_equal(got[qi].view(np.uint32), want.view(np.uint32)), qi


def _check_lists(got, ref, queries, top, ids=None, live=None):
    assert len(got) == len(queries)
    for qi, (g, q) in enumerate(zip(got, queries)):
        w = SCR.search(ref, q, top, ids=ids, live=live)
        assert g["idx"].tolist() == w["idx"].tolist(), qi
        assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32)), qi


def test_all_five_kinds_score_points_full_scan_and_id_list():
    rows = _zipf_rows(1, 5000, 400, 40, signed=True)
    queries = _all_kinds(2, 400, 14, signed=True)
    assert [q.n_b for q in queries[-2:]] == [6, 0] and queries[5].n_b == 4 and queries[6].n_b == 0
    st, ref = qa.SparseVectorStorage(rows), SR.Restatement(rows)
    scorer = qa.CustomRawScorer(queries, st)
    rng = np.random.default_rng(3)
    ids = rng.permutation(st.n)[:500].astype(np.uint32)
    _check_scores(scorer.score_points(ids), ref, queries, ids)
    deleted = rng.random(st.n) < 0.15
    st.set_deleted(deleted)
    for top in (10, 100):        # 100: two passes of the key lists
        _check_lists(scorer.peek_top(top), ref, queries, top, live=~deleted)
    assert scorer.counters.vectors_scored > 0 and scorer.counters.bytes_read == 8 * scorer.counters.vectors_scored
    allowed = rng.random(st.n) < 0.6
    cand = np.sort(rng.choice(st.n, 1500, replace=False)).astype(np.uint32)
    scorer.examples.set_filter(allowed)
    _check_lists(scorer.peek_top(10, cand), ref, queries, 10, ids=cand, live=~deleted & allowed)
    _check_lists(scorer.peek_top(100, cand), ref, queries, 100, ids=cand, live=~deleted & allowed)
    n_examples = sum(len(q.examples) for q in queries)
    assert scorer.counters.vectors_scored == n_examples * len(cand) * 2 and scorer.counters.bytes_read == 0
    _check_lists(scorer.peek_top(10), ref, queries, 10, live=~deleted & allowed)
    scorer.examples.set_filter(None)
    _check_lists(scorer.peek_top(10), ref, queries, 10, live=~deleted)


def test_points_without_overlap_are_returned():
    rows = _zipf_rows(4, 1000, 60, 8, base=10)
    for p, w in ((17, 2.0), (400, 3.0), (999, 0.5)):
        rows[p] = (np.append(rows[p][0], 1).astype(np.uint32), np.append(rows[p][1], w).astype(np.float32))
    st, ref = qa.SparseVectorStorage(rows), SR.Restatement(rows)
    queries = [qa.CustomQuery.recommend_sum_scores([([1], [1.0])], []), qa.CustomQuery.recommend_best_score([([1], [1.0])], [])]
    scorer = qa.CustomRawScorer(queries, st)
    got = scorer.peek_top(50)
    assert [len(g) for g in got] == [50, 50]
    assert got[0]["idx"].tolist() == [400, 17, 999] + [i for i in range(48) if i != 17][:47]
    assert got[0]["score"].tolist() == [3.0, 2.0, 0.5] + [0.0] * 47          # the tail: the no-overlap score, ascending ids
    assert got[1]["idx"][3:].tolist() == got[0]["idx"][3:].tolist() and set(got[1]["score"][3:].tolist()) == {0.5}     # scaled_fast_sigmoid(0.0)
    _check_lists(got, ref, queries, 50)
    deleted = np.zeros(st.n, dtype=bool)
    deleted[::3] = True
    st.set_deleted(deleted)
    got = scorer.peek_top(2000)
    assert [len(g) for g in got] == [int((~deleted).sum())] * 2             # counts = min(top, live candidates), never padded
    _check_lists(got, ref, queries, 2000, live=~deleted)
    cand = np.array([5, 6, 7, 400, 2000, 8], dtype=np.uint32)                # 2000: past the segment, skipped; 6: deleted
    got = scorer.peek_top(10, cand)
    assert got[0]["idx"].tolist() == [400, 5, 7, 8]
    _check_lists(got, ref, queries, 10, ids=cand, live=~deleted)


def test_examples_without_dimensions_or_with_unknown_ones_score_zero():
    rows = _zipf_rows(5, 700, 50, 10, signed=True)
    st, ref = qa.SparseVectorStorage(rows), SR.Restatement(rows)
    empty, unknown, real = ([], []), ([100000, 70000], [1.0, -2.0]), ([0, 1, 2], [1.0, 0.5, -1.0])
    queries = [qa.CustomQuery.recommend_sum_scores([empty], []), qa.CustomQuery.recommend_sum_scores([unknown], []),
               qa.CustomQuery.recommend_best_score([empty, real], [unknown]), qa.CustomQuery.discover(real, [(empty, unknown), (unknown, real)]),
               qa.CustomQuery.context([(empty, real), (real, unknown)])]
    scorer = qa.CustomRawScorer(queries, st)
    ids = np.arange(st.n, dtype=np.uint32)
    sc = scorer.score_points(ids)
    assert np.array_equal(sc[:2].view(np.uint32), np.zeros((2, st.n), dtype=np.uint32))      # +0.0 everywhere
    _check_scores(sc, ref, queries, ids)
    _check_lists(scorer.peek_top(20), ref, queries, 20)
    _check_lists(scorer.peek_top(20, ids[::2]), ref, queries, 20, ids=ids[::2])


def test_integer_weights_tie_masses():
    rows = _zipf_rows(6, 30000, 50, 6, integer=True)
    queries = _all_kinds(7, 50, 4, integer=True)
    st, ref = qa.SparseVectorStorage(rows), SR.Restatement(rows)
    scorer = qa.CustomRawScorer(queries, st)
    for top in (1, 10, 100):
        _check_lists(scorer.peek_top(top), ref, queries, top)
    cand = np.arange(0, st.n, 3, dtype=np.uint32)
    _check_lists(scorer.peek_top(70, cand), ref, queries, 70, ids=cand)


def test_non_monotone_map_sums_in_original_order():
    example = ([1, 2, 3], [1.0, 1.0, 1.0])
    rows = [([1, 2, 3], [1e8, 1.0, -1e8]), ([2], [5.0])]
    dim_map = {1: 0, 3: 1, 2: 2}
    st = qa.SparseVectorStorage(rows, dim_map=dim_map)
    scorer = qa.CustomRawScorer([qa.CustomQuery.recommend_sum_scores([example], [])], st)
    assert scorer.score_points([0, 1]).tolist() == [[0.0, 5.0]]                               # (1e8 + 1) - 1e8: original order
    assert [(int(r["idx"]), float(r["score"])) for r in scorer.peek_top(2)[0]] == [(1, 5.0), (0, 0.0)]
    assert [(int(r["idx"]), float(r["score"])) for r in scorer.peek_top(2, [0, 1])[0]] == [(1, 5.0), (0, 0.0)]
    assert qa.new_raw_scorer([example], st).score_points([0, 1]).tolist() == [[1.0, 5.0]]     # Nearest: remapped order, as before
    assert st.search([example], 2)[0]["score"].tolist() == [5.0, 1.0]

    n_dims = 64
    perm = np.random.default_rng(8).permutation(n_dims)
    dim_map = {int(d): int(perm[d]) for d in range(n_dims)}
    rows = _zipf_rows(9, 4000, n_dims, 30, signed=True)
    queries = _all_kinds(10, n_dims, 30, signed=True)
    queries.append(qa.CustomQuery.recommend_sum_scores([([1000, 3, 40], [1.0, 2.0, -1.0])], []))      # dimension 1000 is not in the map
    st, ref = qa.SparseVectorStorage(rows, dim_map=dim_map), SR.Restatement(rows, dim_map=dim_map)
    scorer = qa.CustomRawScorer(queries, st)
    ids = np.arange(st.n, dtype=np.uint32)
    _check_scores(scorer.score_points(ids), ref, queries, ids)
    for top in (10, 80):
        _check_lists(scorer.peek_top(top), ref, queries, top)
        _check_lists(scorer.peek_top(top, ids[1::2]), ref, queries, top, ids=ids[1::2])
    # the same examples as plain queries still sum in remapped order, and that order gives other floats somewhere in this data
    examples = queries[3].examples
    nearest = qa.new_raw_scorer(examples, st).score_points(ids)
    remapped, _ = ref.score_matrix([ref.prepare_query(*e) for e in examples])
    assert np.array_equal(nearest.view(np.uint32), remapped.view(np.uint32))
    original = np.stack([SCR.original_order_sims(ref, e) for e in examples])
    assert not np.array_equal(original.view(np.uint32), remapped.view(np.uint32))


def test_multi_tile_zipf_two_million_points():
    n, n_dims = 2_000_000, 5000
    rng = np.random.default_rng(21)
    p = 1.0 / np.arange(1, n_dims + 1) ** 1.05
    p /= p.sum()
    lens = rng.integers(1, 12, n)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    raw = rng.choice(n_dims, size=int(off[-1]), p=p).astype(np.uint32)
    # unique per row: sort (row, dim), drop repeats
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    key = np.unique(row * n_dims + raw)
    row, idx = key // n_dims, (key % n_dims).astype(np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(row, minlength=n))
    val = rng.lognormal(0.0, 1.0, len(idx)).astype(np.float32)
    st = qa.SparseVectorStorage(off, idx, val)
    ref = SR.Restatement((off, idx, val))
    ex = _zipf_rows(22, 10, 400, 6)           # popular dimensions: posting lists that span every tile
    queries = [qa.CustomQuery.discover(ex[0], [(ex[1], ex[2]), (ex[3], ex[4])]), qa.CustomQuery.recommend_best_score(ex[5:8], ex[8:10])]
    scorer = qa.CustomRawScorer(queries, st)
    for top in (10, 100):
        _check_lists(scorer.peek_top(top), ref, queries, top)
    c = scorer.counters
    assert c.vectors_scored > 0 and c.bytes_read == 8 * c.vectors_scored      # posting entries (id, weight) of every example, per pass


def test_results_into_device_buffers():
    import torch
    rows = _zipf_rows(11, 5000, 200, 20, signed=True)
    queries = _all_kinds(12, 200, 10, signed=True)
    st, ref = qa.SparseVectorStorage(rows), SR.Restatement(rows)
    scorer = qa.CustomRawScorer(queries, st)
    top, nq = 70, len(queries)
    for ids in (None, np.arange(0, st.n, 2, dtype=np.uint32)):
        out = torch.zeros((nq, top, 2), dtype=torch.int32, device="cuda")
        counts = torch.zeros(nq, dtype=torch.int32, device="cuda")
        F.check(F.lib().qmx_sparse_custom_search_topk(scorer.examples._h, scorer._descs, nq, top, F.ptr(ids), 0 if ids is None else len(ids),
                                                      F.ptr(out), F.ptr(counts), None, None))
        o, c = out.cpu().numpy(), counts.cpu().numpy()
        got = []
        for i in range(nq):
            r = np.zeros(int(c[i]), dtype=SR.ScoredPointOffset)
            r["idx"] = o[i, :c[i], 0].view(np.uint32)
            r["score"] = o[i, :c[i], 1].view(np.float32)
            got.append(r)
        _check_lists(got, ref, queries, top, ids=ids)


def test_refusals_and_errors():
    rows = _zipf_rows(13, 300, 40, 8)
    st = qa.SparseVectorStorage(rows)
    lib = F.lib()
    out = np.zeros(8, dtype=SR.ScoredPointOffset)
    cnt = np.zeros(2, dtype=np.uint32)
    sc = np.zeros(8, dtype=np.float32)
    ids = np.arange(4, dtype=np.uint32)

    def both(h, descs, n):
        a = lib.qmx_sparse_custom_score_points(h, descs, n, F.ptr(ids), 4, F.ptr(sc))
        b = lib.qmx_sparse_custom_search_topk(h, descs, n, 4, None, 0, F.ptr(out), F.ptr(cnt), None, None)
        assert a == b
        return a

    def desc(kind, first, n_a, n_b, coef_first=0):
        d = (F.CustomQuery * 1)()
        d[0].kind, d[0].first, d[0].n_a, d[0].n_b, d[0].coef_first = kind, first, n_a, n_b, coef_first
        return d

    ok = desc(F.CUSTOM_RECO_SUM_SCORES, 0, 1, 1)
    # the example batch: made by qmx_sparse_query_create over a sparse segment
    internal = qa.new_raw_scorer_internal([0, 1], st)
    assert both(internal._h, ok, 1) == F.ERR_NOT_SUPPORTED
    dense = qa.VectorStorage(np.eye(4, dtype=np.float32), qa.Distance.Dot)
    dense_batch = qa.new_raw_scorer(np.eye(4, dtype=np.float32)[:2], dense)
    assert both(dense_batch._h, ok, 1) == F.ERR_NOT_SUPPORTED
    ex = qa.new_raw_scorer(rows[:4], st)
    assert both(ex._h, ok, 1) == F.OK
    assert both(ex._h, ok, 0) == F.OK                                                         # nothing to do
    # the statuses of the dense custom calls' validation
    assert both(ex._h, desc(F.CUSTOM_RECO_SUM_SCORES, 2, 2, 1), 1) == F.ERR_OUT_OF_BOUNDS     # reaches past the 4 examples
    assert both(ex._h, desc(F.CUSTOM_DISCOVER, 0, 1, 2), 1) == F.ERR_OUT_OF_BOUNDS
    assert both(ex._h, desc(F.CUSTOM_FEEDBACK, 0, 1, 1), 1) == F.ERR_OUT_OF_BOUNDS            # no coefficients set
    assert both(ex._h, desc(5, 0, 1, 1), 1) == F.ERR_BAD_ARG
    assert both(ex._h, desc(F.CUSTOM_DISCOVER, 0, 2, 1), 1) == F.ERR_BAD_ARG
    assert both(ex._h, desc(F.CUSTOM_CONTEXT, 0, 1, 1), 1) == F.ERR_BAD_ARG
    cf = np.array([1.0, 0.5], dtype=np.float32)
    assert lib.qmx_custom_set_coefficients(ex._h, F.ptr(cf), 2) == F.OK
    assert both(ex._h, desc(F.CUSTOM_FEEDBACK, 0, 1, 1), 1) == F.OK
    assert both(ex._h, desc(F.CUSTOM_FEEDBACK, 0, 1, 1, coef_first=1), 1) == F.ERR_OUT_OF_BOUNDS
    # ids past the segment: an error for score_points, skipped by the search
    bad = np.array([0, 300, 1, 2], dtype=np.uint32)
    assert lib.qmx_sparse_custom_score_points(ex._h, ok, 1, F.ptr(bad), 4, F.ptr(sc)) == F.ERR_OUT_OF_BOUNDS
    assert lib.qmx_sparse_custom_search_topk(ex._h, ok, 1, 4, F.ptr(bad), 4, F.ptr(out), F.ptr(cnt), None, None) == F.OK and cnt[0] == 3
    assert lib.qmx_sparse_custom_search_topk(ex._h, ok, 1, 4, F.ptr(bad), 0, F.ptr(out), F.ptr(cnt), None, None) == F.OK and cnt[0] == 0
    assert lib.qmx_sparse_custom_search_topk(ex._h, ok, 1, 0, None, 0, F.ptr(out), F.ptr(cnt), None, None) == F.ERR_NOT_SUPPORTED
    assert lib.qmx_sparse_custom_search_topk(ex._h, ok, 1, 65537, None, 0, F.ptr(out), F.ptr(cnt), None, None) == F.ERR_NOT_SUPPORTED
    stop = np.ones(1, dtype=np.uint8)
    assert lib.qmx_sparse_custom_search_topk(ex._h, ok, 1, 4, None, 0, F.ptr(out), F.ptr(cnt), F.ptr(stop), None) == F.ERR_CANCELLED
    # the dense custom calls keep refusing a sparse batch
    assert lib.qmx_custom_search_topk(ex._h, ok, 1, 4, None, 0, F.ptr(out), F.ptr(cnt)) == F.ERR_NOT_SUPPORTED
    assert lib.qmx_custom_score_points(ex._h, ok, 1, F.ptr(ids), 4, F.ptr(sc)) == F.ERR_NOT_SUPPORTED


def test_python_layer_refusals():
    st = qa.SparseVectorStorage([([1, 2], [1.0, 2.0]), ([2], [3.0])])
    dense = qa.VectorStorage(np.eye(4, dtype=np.float32), qa.Distance.Dot)
    sparse_q = qa.CustomQuery.recommend_sum_scores([([2], [1.0])], [])
    dense_q = qa.CustomQuery.recommend_sum_scores([np.ones(4, dtype=np.float32)], [])
    assert sparse_q.sparse is True and dense_q.sparse is False and qa.CustomQuery.context([]).sparse is None
    with pytest.raises(ValueError):
        qa.CustomRawScorer([sparse_q, dense_q], st)
    with pytest.raises(ValueError):
        qa.CustomRawScorer([sparse_q], dense)
    with pytest.raises(ValueError):
        qa.CustomRawScorer([dense_q], st)
    with pytest.raises(ValueError):
        qa.CustomQuery.recommend_sum_scores([([2], [1.0]), np.ones(4, dtype=np.float32)], [])
    scorer = qa.CustomRawScorer([sparse_q, qa.CustomQuery.context([])], st)
    assert scorer.score_points([0, 1]).tolist() == [[2.0, 3.0], [0.0, 0.0]]
    with pytest.raises(NotImplementedError):
        scorer.search_hnsw(None, 1, 8)
    assert qa.CustomRawScorer([dense_q], dense).score_points([0, 3]).tolist() == [[1.0, 1.0]]     # the dense path is what it was
