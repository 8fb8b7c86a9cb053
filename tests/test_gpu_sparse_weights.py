"""f16 / u8 index weights and the IDF modifier of sparse segments on the device (sparse.hip / api_sparse.hip) against the numpy restatement of
tests/sparse_weights_reference.py: score bits exact, lists id for id (ties: lower offset first - u8 weights make many)."""
import ctypes as C
import functools

import numpy as np
import pytest

import qdrant_amd as qa
from qdrant_amd import _ffi as F
import sparse_reference as SR
import sparse_custom_reference as SCR
import sparse_weights_reference as SW

pytestmark = pytest.mark.gpu

DT = {SW.F32: qa.VectorStorageDatatype.Float32, SW.F16: qa.VectorStorageDatatype.Float16, SW.U8: qa.VectorStorageDatatype.Uint8}
QUANTIZED = [SW.F16, SW.U8]


def _zipf_rows(seed, n, n_dims, nnz, signed=False, exact=None):
    """Rows as in tests/test_gpu_sparse.py; `exact`: that many dimensions in every row."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_dims + 1) ** 1.1
    p /= p.sum()
    rows = []
    for _ in range(n):
        k = exact if exact is not None else int(rng.integers(0, nnz + 1))
        ix = rng.choice(n_dims, size=min(k, n_dims), replace=False, p=p).astype(np.uint32)
        vx = (rng.standard_normal(len(ix)) if signed else rng.lognormal(0.0, 1.0, len(ix))).astype(np.float32)
        rows.append((ix, vx))
    return rows


@functools.lru_cache(maxsize=None)
def _rows(seed, n, n_dims=400, nnz=40, signed=False):
    return _zipf_rows(seed, n, n_dims, nnz, signed=signed)


@functools.lru_cache(maxsize=None)
def _ref(seed, n, weights, n_dims=400, nnz=40, signed=False):
    return SW.WeightsRestatement(_rows(seed, n, n_dims, nnz, signed), weights=weights)


def _check_lists(got, ref, prep, top, ids=None, live=None):
    want = ref.search(prep, top, ids=ids, live=live)
    assert len(got) == len(want)
    for qi, (g, w) in enumerate(zip(got, want)):
        assert g["idx"].tolist() == w["idx"].tolist(), qi
        assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32)), qi


def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["idx"].tolist() == y["idx"].tolist() and np.array_equal(x["score"].view(np.uint32), y["score"].view(np.uint32))


@pytest.mark.parametrize("n", [3000, 10245])      # 10245: past a work-group tile of 8192 and a wave sub-range of 2048, ragged end
@pytest.mark.parametrize("weights", QUANTIZED)
def test_full_search(weights, n):
    rows, ref = _rows(1, n), _ref(1, n, weights)
    assert max(len(ref.postings(d)[0]) for d in range(5)) > 64
    st = qa.SparseVectorStorage(rows, index_datatype=DT[weights])
    for nq in (1, 3, 128):
        queries = _zipf_rows(2 + nq, nq, 400, 12)
        if nq == 3:
            queries[1] = _zipf_rows(9, 1, 400, 0, exact=70)[0]      # more than one 64-entry plan chunk
        prep = [ref.prepare_query(*q) for q in queries]
        for top in (1, 10, 100):      # 100: two passes of 64
            _check_lists(st.search(queries, top), ref, prep, top)
    c = st.counters
    assert c.vectors_scored > 0 and c.bytes_read == (6 if weights == SW.F16 else 5) * c.vectors_scored


@pytest.mark.parametrize("weights", QUANTIZED)
def test_signed_weights(weights):
    rows, ref = _rows(3, 3000, signed=True), _ref(3, 3000, weights, signed=True)
    queries = _zipf_rows(4, 8, 400, 12, signed=True)
    st = qa.SparseVectorStorage(rows, index_datatype=DT[weights])
    _check_lists(st.search(queries, 20), ref, [ref.prepare_query(*q) for q in queries], 20)
    if weights == SW.U8:
        assert any(mn < 0 for mn, _ in ref.params)


@pytest.mark.parametrize("weights", QUANTIZED)
def test_with_an_indices_tracker_map(weights):
    n_dims = 64
    perm = np.random.default_rng(16).permutation(n_dims)
    dim_map = {int(d): int(perm[d]) for d in range(n_dims)}
    rows = _zipf_rows(17, 3000, n_dims, 30, signed=True)
    queries = _zipf_rows(18, 8, n_dims, 30, signed=True) + [([1000, 3], [1.0, 2.0])]      # dimension 1000 is unknown: dropped
    st = qa.SparseVectorStorage(rows, dim_map=dim_map, index_datatype=DT[weights])
    ref = SW.WeightsRestatement(rows, dim_map=dim_map, weights=weights)
    prep = [ref.prepare_query(*q) for q in queries]
    _check_lists(st.search(queries, 10), ref, prep, 10)
    ids = np.arange(0, 3000, 3, dtype=np.uint32)
    _check_lists(st.search(queries, 10, ids=ids), ref, prep, 10, ids=ids)


@pytest.mark.parametrize("weights", QUANTIZED)
def test_id_list_filter_and_deleted_flags(weights):
    rows, ref = _rows(1, 10245), _ref(1, 10245, weights)
    queries = _zipf_rows(6, 8, 400, 10)
    prep = [ref.prepare_query(*q) for q in queries]
    st = qa.SparseVectorStorage(rows, index_datatype=DT[weights])
    rng = np.random.default_rng(7)
    deleted = rng.random(st.n) < 0.2
    allowed = rng.random(st.n) < 0.6
    st.set_deleted(deleted)
    ids = np.sort(rng.choice(st.n, 3000, replace=False)).astype(np.uint32)
    _check_lists(st.search(queries, 10, ids=ids), ref, prep, 10, ids=ids, live=~deleted)
    _check_lists(st.search(queries, 10, allowed=allowed), ref, prep, 10, live=~deleted & allowed)
    _check_lists(st.search(queries, 100, ids=ids, allowed=allowed), ref, prep, 100, ids=ids, live=~deleted & allowed)
    assert [len(g) for g in st.search(queries, 5, ids=np.zeros(0, dtype=np.uint32))] == [0] * 8


def _custom_queries(seed):
    ex = _zipf_rows(seed, 12, 400, 10)
    return [qa.CustomQuery.recommend_best_score(ex[0:2], ex[2:3]), qa.CustomQuery.recommend_sum_scores(ex[3:5], ex[5:6]),
            qa.CustomQuery.discover(ex[6], [(ex[7], ex[8])]), qa.CustomQuery.context([(ex[9], ex[10])]),
            qa.CustomQuery.feedback_naive(ex[11], [(ex[0], 0.9), (ex[3], 0.2)], 0.5, 2.0, 0.25)]


@pytest.mark.parametrize("weights", QUANTIZED)
def test_storage_readers_have_the_bits_of_an_f32_twin(weights):
    """The raw scorer and the custom queries read the vector storage, which stays f32 whatever the index holds."""
    rows = _rows(1, 3000)
    twin = qa.SparseVectorStorage(rows)
    st = qa.SparseVectorStorage(rows, index_datatype=DT[weights])
    queries = _zipf_rows(21, 5, 400, 12)
    every = np.arange(3000)
    a, b = qa.new_raw_scorer(queries, st), qa.new_raw_scorer(queries, twin)
    assert np.array_equal(a.score_points(every).view(np.uint32), b.score_points(every).view(np.uint32))
    ragged = [[0, 5, 2999], [7], [], [10, 11], [2, 1, 0]]
    for x, y in zip(a.score_points_ragged(ragged), b.score_points_ragged(ragged)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    pa = np.arange(0, 3000, 3, dtype=np.uint32)
    pb = (pa * 7 + 11) % 3000
    ia, ib = qa.new_raw_scorer_internal(pa, st), qa.new_raw_scorer_internal(pa, twin)
    assert np.array_equal(ia.score_internal(pa, pb).view(np.uint32), ib.score_internal(pa, pb).view(np.uint32))
    cq = _custom_queries(22)
    ca, cb = qa.CustomRawScorer(cq, st), qa.CustomRawScorer(cq, twin)
    assert np.array_equal(ca.score_points(every).view(np.uint32), cb.score_points(every).view(np.uint32))
    ids = np.arange(1, 3000, 2, dtype=np.uint32)
    for top in (10, 100):
        _same_lists(ca.peek_top(top), cb.peek_top(top))                       # the row kernel over the implicit identity list == the fused posting scan
        _same_lists(ca.peek_top(top, ids), cb.peek_top(top, ids))
    deleted = np.random.default_rng(23).random(3000) < 0.3
    st.set_deleted(deleted)
    twin.set_deleted(deleted)
    _same_lists(ca.peek_top(10), cb.peek_top(10))
    assert "sparse_custom_topk_ids_kernel" in F.last_kernel(ca.examples._h) and "postings" in F.last_kernel(cb.examples._h)


def test_f32_flag_value_is_the_segment_of_flags_zero():
    rows = _rows(1, 3000)
    queries = _zipf_rows(24, 8, 400, 12)
    a = qa.SparseVectorStorage(rows)
    b = qa.SparseVectorStorage(rows, index_datatype=qa.VectorStorageDatatype.Float32)
    _same_lists(a.search(queries, 100), b.search(queries, 100))
    ref = _ref(1, 3000, SW.F32)
    _check_lists(b.search(queries, 10), ref, [ref.prepare_query(*q) for q in queries], 10)
    assert b.counters.bytes_read == 8 * b.counters.vectors_scored


def _idf_setup(weights, dim_map=None):
    n, n_dims = 10245, 400
    rows = _rows(1, n)
    st = qa.SparseVectorStorage(rows, dim_map=dim_map, index_datatype=DT[weights])
    ref = SW.WeightsRestatement(rows, dim_map=dim_map, weights=weights)
    rng = np.random.default_rng(31)
    pdel, vdel = rng.random(n) < 0.15, rng.random(n - 1000) < 0.1      # the vector flags end before the rows do
    st.set_deleted(pdel, vdel)
    live = ~pdel
    live[:len(vdel)] &= ~vdel
    return st, ref, pdel, vdel, live


@pytest.mark.parametrize("weights", [SW.F32, SW.U8])
def test_idf_statistics_global_and_corpus(weights):
    dim_map = {d: 1000 - d for d in range(451)}      # 400 .. 450: known to the map, in no row
    st, ref, pdel, vdel, _ = _idf_setup(weights, dim_map)
    dims = np.array(list(range(50)) + [5000, 450, 0], dtype=np.uint32)      # ... unknown to the map, no posting, a repeat
    df, n_docs = st.idf_statistics(dims)
    want_df, want_n = ref.global_statistics(dims)
    assert df.tolist() == want_df.tolist() and n_docs == want_n
    assert df[50] == 0 and df[51] == 0 and df[-1] == df[0] > 64
    mask = np.random.default_rng(32).random(10245 - 77) < 0.5       # the mask ends before the rows do
    member = ref.corpus_members(mask, pdel, vdel)
    df, n_docs = st.idf_statistics(dims, corpus=mask)
    want_df, want_n = ref.corpus_statistics_mask(dims, member)
    assert df.tolist() == want_df.tolist() and n_docs == want_n and 0 < n_docs < np.count_nonzero(mask)
    df, n_docs = st.idf_statistics(dims, corpus=np.zeros(10245, dtype=bool))
    assert df.tolist() == [0] * len(dims) and n_docs == 0


@pytest.mark.parametrize("weights", [SW.F32, SW.F16, SW.U8])
def test_search_with_idf(weights):
    st, ref, pdel, vdel, live = _idf_setup(weights)
    queries = _zipf_rows(33, 8, 400, 12) + [([3, 5000], [1.0, 2.0])]
    dims = np.unique(np.concatenate([np.asarray(q[0], dtype=np.uint32) for q in queries]))

    def scaled(stats):
        return [ref.prepare_query(q[0], SW.remap_idf_weights(q[0], q[1], dims, *stats)) for q in queries]
    plain = st.search(queries, 10)
    got = st.search(queries, 10, idf=True)
    _check_lists(got, ref, scaled(ref.global_statistics(dims)), 10, live=live)
    assert any(not np.array_equal(g["score"], p["score"]) for g, p in zip(got, plain))
    mask = np.random.default_rng(34).random(st.n) < 0.5
    stats = ref.corpus_statistics_mask(dims, ref.corpus_members(mask, pdel, vdel))
    _check_lists(st.search(queries, 10, idf=mask), ref, scaled(stats), 10, live=live)
    ids = np.arange(0, st.n, 3, dtype=np.uint32)
    _check_lists(st.search(queries, 10, ids=ids, idf=mask), ref, scaled(stats), 10, ids=ids, live=live)
    # the statistics of two segments, added before they are applied
    other_rows = _rows(35, 3000)
    other = qa.SparseVectorStorage(other_rows, index_datatype=DT[weights])
    merged = SW.merge_statistics(st.idf_statistics(dims), other.idf_statistics(dims))
    want = SW.merge_statistics(ref.global_statistics(dims), SW.WeightsRestatement(other_rows).global_statistics(dims))
    assert merged[0].tolist() == want[0].tolist() and merged[1] == want[1]
    _check_lists(st.search(queries, 10, idf=(dims, merged[0], merged[1])), ref, scaled(want), 10, live=live)
    sc = qa.new_raw_scorer(queries, st, idf=(dims, merged[0], merged[1])).score_points(np.arange(st.n))
    want_sc, _ = SR.Restatement(_rows(1, 10245)).score_matrix(scaled(want))      # the raw scorer: f32 rows
    assert np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))


@pytest.mark.parametrize("weights", [SW.F32, SW.U8])
def test_custom_query_with_idf_scales_every_example(weights):
    rows = _rows(1, 3000)
    st = qa.SparseVectorStorage(rows, index_datatype=DT[weights])
    ref = SR.Restatement(rows)      # the custom scorer reads the f32 rows
    cq = _custom_queries(41)
    dims = np.unique(np.concatenate([ix for q in cq for ix, _ in q.examples]))
    stats = SW.WeightsRestatement(rows).global_statistics(dims)
    scaled = [qa.CustomQuery(q.kind, [(ix, SW.remap_idf_weights(ix, vx, dims, *stats)) for ix, vx in q.examples], q.n_a, q.n_b, q.coefs) for q in cq]
    scorer = qa.CustomRawScorer(cq, st, idf=True)
    every = np.arange(3000)
    sc = scorer.score_points(every)
    lists = scorer.peek_top(10)
    unscaled = qa.CustomRawScorer(cq, st).score_points(every)
    for qi, q in enumerate(scaled):
        want = SCR.custom_scores(ref, q)
        assert np.array_equal(sc[qi].view(np.uint32), want.view(np.uint32)), qi
        w = SCR.search(ref, q, 10)
        assert lists[qi]["idx"].tolist() == w["idx"].tolist() and np.array_equal(lists[qi]["score"].view(np.uint32), w["score"].view(np.uint32))
    assert not np.array_equal(sc[1], unscaled[1])      # (the sum of scores moves with every example's scale)


def test_hybrid_search_with_idf_equals_the_two_step_path():
    import oracle_ffi as O
    n, dim, nq = 3000, 32, 8
    dense = qa.VectorStorage(O.preprocess(O.COSINE, O.synth(0x61, 0, n, dim)), qa.Distance.Cosine)
    sparse = qa.SparseVectorStorage(_rows(1, n), index_datatype=qa.VectorStorageDatatype.Uint8)
    dq = qa.new_raw_scorer(O.synth(0x62, 0, nq, dim), dense)
    queries = _zipf_rows(63, nq, 400, 12)
    mask = np.random.default_rng(64).random(n) < 0.5
    for idf in (True, mask):
        got = qa.hybrid_search([(dq, 50), ((sparse, queries), 40)], qa.Rrf(2), 20, sparse_idf=idf)
        two_step = qa.hybrid_search([(dq, 50), (qa.new_raw_scorer(queries, sparse, idf=idf), 40)], qa.Rrf(2), 20)
        _same_lists(got, two_step)
    without = qa.hybrid_search([(dq, 50), (qa.new_raw_scorer(queries, sparse), 40)], qa.Rrf(2), 20)
    assert any(g["idx"].tolist() != w["idx"].tolist() for g, w in zip(got, without))
    with pytest.raises(ValueError):
        qa.hybrid_search([(dq, 50)], qa.Rrf(2), 20, sparse_idf=True)


def test_unknown_flag_bits_are_refused_and_sparse_refusals_stay():
    off = np.array([0, 2, 3], dtype=np.uint64)
    idx, val = np.array([1, 2, 2], dtype=np.uint32), np.array([1.0, 2.0, 3.0], dtype=np.float32)
    for flags in (3, 4, 0x10, 0x80000001):
        desc = F.SparseSegmentDesc()
        desc.n, desc.offsets, desc.indices, desc.values, desc.flags = 2, F.ptr(off), F.ptr(idx), F.ptr(val), flags
        h = C.c_void_p()
        assert F.lib().qmx_sparse_segment_create(C.byref(desc), C.byref(h)) == F.ERR_BAD_ARG, flags
    st = qa.SparseVectorStorage([([1, 2], [1.0, 2.0]), ([2], [3.0])], index_datatype=qa.VectorStorageDatatype.Uint8)
    scorer = qa.new_raw_scorer([([2], [1.0])], st)
    tiny = SW.WeightsRestatement([([1, 2], [1.0, 2.0]), ([2], [3.0])], weights=SW.U8)
    _check_lists(st.search([([2], [1.0])], 5), tiny, [tiny.prepare_query([2], [1.0])], 5)
    out = np.zeros(4, dtype=SR.ScoredPointOffset)
    cnt = np.zeros(1, dtype=np.uint32)
    assert F.lib().qmx_hnsw_search(None, scorer._h, 1, 8, F.ptr(out), F.ptr(cnt), None, None) == F.ERR_NOT_SUPPORTED
    cq = (F.CustomQuery * 1)()
    assert F.lib().qmx_custom_search_topk(scorer._h, cq, 1, 1, None, 0, F.ptr(out), F.ptr(cnt)) == F.ERR_NOT_SUPPORTED
    h = C.c_void_p()
    assert F.lib().qmx_query_create(st._h, F.ptr(np.zeros(4, dtype=np.float32)), 1, C.byref(h)) == F.ERR_NOT_SUPPORTED
    assert F.lib().qmx_score_bytes(scorer._h, F.ptr(np.zeros(8, dtype=np.uint8)), 1, 8, F.ptr(np.zeros(1, dtype=np.float32))) == F.ERR_NOT_SUPPORTED
    dense = qa.VectorStorage(np.zeros((4, 8), dtype=np.float32), qa.Distance.Dot)
    n_docs = C.c_uint64(0)
    df = np.zeros(1, dtype=np.uint64)
    assert F.lib().qmx_sparse_idf_statistics(dense._h, F.ptr(np.zeros(1, dtype=np.uint32)), 1, None, 0, F.ptr(df), C.byref(n_docs)) == F.ERR_NOT_SUPPORTED
    with pytest.raises(ValueError):
        qa.new_raw_scorer(np.zeros((1, 8), dtype=np.float32), dense, idf=True)
