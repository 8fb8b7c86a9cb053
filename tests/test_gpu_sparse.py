"""Sparse vectors on the device (QMX_DTYPE_SPARSE, sparse.hip / api_sparse.hip) against the numpy restatement of tests/sparse_reference.py:
score bits exact, Nearest lists exact (ties: lower offset first) and through parity_asserts.assert_reference_lists."""
import ctypes as C

import numpy as np
import pytest

import qdrant_amd as qa
from qdrant_amd import _ffi as F
import parity_asserts
import sparse_reference as SR

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


class _Adapter:
    """What parity_asserts.assert_reference_lists reads: peek_top and, for masses of ties, score_points over every row (NaN where a point is
    not a candidate: it can never join a tie group)."""

    def __init__(self, ref, queries, live=None):
        self.ref, self.queries, self.live = ref, queries, live
        self.rows = np.zeros((ref.n, 1))

    def peek_top(self, qidx, top, threads=None):
        return self.ref.search([self.queries[int(i)] for i in qidx], top, live=self.live)

    def score_points(self, qidx, ids):
        sc, ov = self.ref.score_matrix([self.queries[int(i)] for i in qidx])
        ok = ov if self.live is None else ov & self.live
        return np.where(ok, sc, np.float32(np.nan))[:, ids]


def _check_lists(got, ref, queries, top, ids=None, live=None):
    want = ref.search(queries, top, ids=ids, live=live)
    assert len(got) == len(want)
    for qi, (g, w) in enumerate(zip(got, want)):
        assert g["idx"].tolist() == w["idx"].tolist(), qi
        assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32)), qi
    if ids is None:
        parity_asserts.assert_reference_lists(got, _Adapter(ref, queries, live), np.arange(len(queries)), top, live=None, threads=None)


def _setup(rows, queries, dim_map=None):
    st = qa.SparseVectorStorage(rows, dim_map=dim_map)
    ref = SR.Restatement(rows, dim_map=dim_map)
    return st, ref, [ref.prepare_query(*q) for q in queries]


@pytest.mark.parametrize("nq", [1, 3, 8, 32, 128])
def test_score_points_and_search_all(nq):
    rows = _zipf_rows(1, 3000, 400, 40)
    queries = _zipf_rows(2, nq, 400, 12)
    st, ref, prep = _setup(rows, queries)
    sc = qa.new_raw_scorer(queries, st).score_points(np.arange(st.n))
    want, _ = ref.score_matrix(prep)
    assert np.array_equal(sc.view(np.uint32), want.view(np.uint32))
    for top in (1, 10):
        _check_lists(st.search(queries, top), ref, prep, top)


def test_unsorted_rows_are_sorted_and_bad_input_refused():
    rng = np.random.default_rng(3)
    rows = [(rng.permutation(np.arange(0, 200, 7)).astype(np.uint32), rng.standard_normal(29).astype(np.float32)) for _ in range(50)]
    queries = [(np.array([140, 7, 63], dtype=np.uint32), np.array([1.0, -2.0, 0.5], dtype=np.float32))]
    st, ref, prep = _setup(rows, queries)
    sc = qa.new_raw_scorer(queries, st).score_points(np.arange(50))
    assert np.array_equal(sc.view(np.uint32), ref.score_matrix(prep)[0].view(np.uint32))
    with pytest.raises(F.QmxError) as e:
        qa.SparseVectorStorage([([1, 2, 1], [1.0, 2.0, 3.0])])
    assert e.value.status == F.ERR_BAD_ARG
    with pytest.raises(F.QmxError) as e:
        qa.SparseVectorStorage(np.array([0, 3, 2], dtype=np.uint64), np.arange(3, dtype=np.uint32), np.ones(3, dtype=np.float32))
    assert e.value.status == F.ERR_BAD_ARG
    with pytest.raises(F.QmxError) as e:
        qa.new_raw_scorer([([4, 4], [1.0, 1.0])], st)
    assert e.value.status == F.ERR_BAD_ARG


def test_empty_rows_empty_query_and_zero_without_overlap():
    rows = [([], []), ([1, 5], [1.0, 2.0]), ([], []), ([9], [3.0])]
    queries = [([], []), ([5, 9], [2.0, 1.0]), ([100], [1.0])]
    st, ref, prep = _setup(rows, queries)
    scorer = qa.new_raw_scorer(queries, st)
    sc = scorer.score_points(np.arange(4))
    assert sc.tolist() == [[0.0] * 4, [0.0, 4.0, 0.0, 3.0], [0.0] * 4]
    ragged = scorer.score_points_ragged([[0, 1], [3, 2, 1], [1]])
    assert [r.tolist() for r in ragged] == [[0.0, 0.0], [3.0, 0.0, 4.0], [0.0]]
    assert scorer.score_point(3, query_index=1) == 3.0
    got = st.search(queries, 5)
    assert [len(g) for g in got] == [0, 2, 0]
    _check_lists(got, ref, prep, 5)
    assert [len(g) for g in st.search(queries, 0)] == [0, 0, 0]


def test_internal_scores_and_internal_queries():
    rows = _zipf_rows(4, 500, 100, 20, signed=True)
    st, ref, _ = _setup(rows, [])
    a = np.arange(0, 500, 3, dtype=np.uint32)
    b = (a * 7 + 11) % 500
    scorer = qa.new_raw_scorer_internal(a, st)
    got = scorer.score_internal(a, b)
    want = np.array([SR.score_pair(*ref.rows[int(x)], *ref.rows[int(y)])[0] for x, y in zip(a, b)], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    sc = scorer.score_points(np.arange(500))
    want_m, _ = ref.score_matrix([ref.rows[int(x)] for x in a])
    assert np.array_equal(sc.view(np.uint32), want_m.view(np.uint32))


def test_id_list_filter_and_deleted_flags():
    rows = _zipf_rows(5, 20000, 300, 30)
    queries = _zipf_rows(6, 8, 300, 10)
    st, ref, prep = _setup(rows, queries)
    rng = np.random.default_rng(7)
    deleted = rng.random(st.n) < 0.2
    allowed = rng.random(st.n) < 0.6
    st.set_deleted(deleted)
    ids = np.sort(rng.choice(st.n, 5000, replace=False)).astype(np.uint32)
    _check_lists(st.search(queries, 10, ids=ids), ref, prep, 10, ids=ids, live=~deleted)
    _check_lists(st.search(queries, 10, allowed=allowed), ref, prep, 10, live=~deleted & allowed)
    _check_lists(st.search(queries, 100, ids=ids, allowed=allowed), ref, prep, 100, ids=ids, live=~deleted & allowed)


@pytest.mark.parametrize("top", [65, 10000])
def test_large_top_and_fewer_overlapping_than_top(top):
    rows = _zipf_rows(8, 6000, 2000, 15)
    queries = _zipf_rows(9, 3, 2000, 6)
    st, ref, prep = _setup(rows, queries)
    got = st.search(queries, top)
    _check_lists(got, ref, prep, top)
    assert all(len(g) < top for g in got) or top == 65       # shorter lists, never padded


def test_integer_weights_tie_masses():
    rows = _zipf_rows(10, 30000, 50, 6, integer=True)
    queries = _zipf_rows(11, 8, 50, 4, integer=True)
    st, ref, prep = _setup(rows, queries)
    for top in (1, 10, 100):
        _check_lists(st.search(queries, top), ref, prep, top)


def test_mixed_signs_exact_zero_sum_is_returned():
    rows = [([1, 2], [1.0, -1.0]), ([1], [0.5]), ([3], [1.0])] + _zipf_rows(12, 1000, 40, 8, signed=True, base=10)
    queries = [([1, 2], [2.0, 2.0])]
    st, ref, prep = _setup(rows, queries)
    got = st.search(queries, 10)[0]
    assert 0 in got["idx"].tolist() and got["score"][got["idx"].tolist().index(0)] == 0.0
    _check_lists([got], ref, prep, 10)
    queries = _zipf_rows(13, 8, 40, 8, signed=True, base=10)
    st2, ref2, prep2 = _setup(rows, queries)
    _check_lists(st2.search(queries, 20), ref2, prep2, 20)


def test_dimension_ids_near_the_top_of_u32():
    top_id = 0xFFFFFFFF
    rows = _zipf_rows(14, 2000, 64, 10, base=top_id - 63)
    queries = _zipf_rows(15, 4, 64, 10, base=top_id - 63)
    st, ref, prep = _setup(rows, queries)
    sc = qa.new_raw_scorer(queries, st).score_points(np.arange(st.n))
    assert np.array_equal(sc.view(np.uint32), ref.score_matrix(prep)[0].view(np.uint32))
    _check_lists(st.search(queries, 10), ref, prep, 10)


def test_non_monotone_dimension_map_follows_the_remapped_order():
    n_dims = 64
    rng = np.random.default_rng(16)
    perm = rng.permutation(n_dims)
    dim_map = {int(d): int(perm[d]) for d in range(n_dims)}
    rows = _zipf_rows(17, 4000, n_dims, 30, signed=True)
    queries = _zipf_rows(18, 8, n_dims, 30, signed=True) + [([1000, 3], [1.0, 2.0])]      # dimension 1000 is unknown: dropped
    st, ref, prep = _setup(rows, queries, dim_map=dim_map)
    sc = qa.new_raw_scorer(queries, st).score_points(np.arange(st.n))
    want, _ = ref.score_matrix(prep)
    assert np.array_equal(sc.view(np.uint32), want.view(np.uint32))
    ident, _ = SR.Restatement(rows).score_matrix([SR.sort_vector(*q) for q in queries[:-1]])
    assert not np.array_equal(ident.view(np.uint32), want[:-1].view(np.uint32))      # the order matters somewhere in this data
    _check_lists(st.search(queries, 10), ref, prep, 10)
    with pytest.raises(F.QmxError) as e:
        qa.SparseVectorStorage([([1, 2000], [1.0, 1.0])], dim_map=dim_map)
    assert e.value.status == F.ERR_BAD_ARG


def test_async_search_into_device_buffers():
    import torch
    rows = _zipf_rows(19, 5000, 200, 20)
    queries = _zipf_rows(20, 5, 200, 8)
    st, ref, prep = _setup(rows, queries)
    scorer = qa.new_raw_scorer(queries, st)
    top = 70
    out = torch.zeros((len(queries), top, 2), dtype=torch.int32, device="cuda")
    counts = torch.zeros(len(queries), dtype=torch.int32, device="cuda")
    F.check(F.lib().qmx_search_topk_async(scorer._h, top, None, 0, F.ptr(out), F.ptr(counts)))
    F.check(F.lib().qmx_query_synchronize(scorer._h))
    o, c = out.cpu().numpy(), counts.cpu().numpy()
    got = []
    for i in range(len(queries)):
        r = np.zeros(int(c[i]), dtype=SR.ScoredPointOffset)
        r["idx"] = o[i, :c[i], 0].view(np.uint32)
        r["score"] = o[i, :c[i], 1].view(np.float32)
        got.append(r)
    _check_lists(got, ref, prep, top)


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
    queries = _zipf_rows(22, 4, 400, 6)       # popular dimensions: posting lists that span every tile
    ref = SR.Restatement((off, idx, val))
    prep = [ref.prepare_query(*q) for q in queries]
    for top in (10, 100):
        _check_lists(st.search(queries, top), ref, prep, top)
    c = st.counters
    assert c.vectors_scored > 0 and c.bytes_read == 8 * c.vectors_scored      # posting entries (id, weight) of the query's dimensions, per pass


def test_other_entry_points_refuse_a_sparse_segment():
    st = qa.SparseVectorStorage([([1, 2], [1.0, 2.0]), ([2], [3.0])])
    scorer = qa.new_raw_scorer([([2], [1.0])], st)
    out = np.zeros(4, dtype=SR.ScoredPointOffset)
    cnt = np.zeros(1, dtype=np.uint32)
    assert F.lib().qmx_hnsw_search(None, scorer._h, 1, 8, F.ptr(out), F.ptr(cnt), None, None) == F.ERR_NOT_SUPPORTED
    cq = (F.CustomQuery * 1)()
    assert F.lib().qmx_custom_search_topk(scorer._h, cq, 1, 1, None, 0, F.ptr(out), F.ptr(cnt)) == F.ERR_NOT_SUPPORTED
    h = C.c_void_p()
    assert F.lib().qmx_query_create(st._h, F.ptr(np.zeros(4, dtype=np.float32)), 1, C.byref(h)) == F.ERR_NOT_SUPPORTED
    assert F.lib().qmx_score_bytes(scorer._h, F.ptr(np.zeros(8, dtype=np.uint8)), 1, 8, F.ptr(np.zeros(1, dtype=np.float32))) == F.ERR_NOT_SUPPORTED
    with pytest.raises(NotImplementedError):
        qa.BatchFilteredSearcher([([2], [1.0])], st, 1)
