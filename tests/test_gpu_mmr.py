"""MMR re-ranking on the device (qmx_mmr_select, qmx_mmr_select_async; mmr.hip) against the numpy restatement of maximal_marginal_relevance in
tests/fusion_reference.py.  The pair scores of the expectation are the oracle's f32 scorer on the rows widened to f32 (the reference's
temporary MMR storage is f32 whatever the stored datatype); the relevance is the score the device gives the request's query for the
candidate's row.  The selection is compared id for id and on the uint32 view of the scores: no tolerance anywhere."""
import numpy as np
import pytest

import qdrant_amd as qa
from qdrant_amd import _ffi as F
import fusion_reference as FR
import oracle_ffi as O
from test_fusion_reference import TIE_EXPECTED, TIE_QUERY, TIE_ROWS

pytestmark = pytest.mark.gpu
SPO = FR.ScoredPointOffset
DIST = {O.COSINE: qa.Distance.Cosine, O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid, O.MANHATTAN: qa.Distance.Manhattan}
DT = {O.F32: qa.VectorStorageDatatype.Float32, O.F16: qa.VectorStorageDatatype.Float16, O.U8: qa.VectorStorageDatatype.Uint8}


def _storage(dtype, dist, rows_f32):
    """(device storage, the stored rows widened to f32) from f32 values: preprocessed and cast as at insert."""
    if dtype == O.U8:
        stored = O.to_u8(rows_f32)
        return qa.VectorStorage(stored, DIST[dist], DT[dtype]), stored.astype(np.float32)
    pre = O.preprocess(dist, rows_f32)
    if dtype == O.F16:
        stored = O.to_f16(pre)
        return qa.VectorStorage(stored.view(np.float16), DIST[dist], DT[dtype]), O.f16_to_f32(stored)
    return qa.VectorStorage(pre, DIST[dist], DT[dtype]), pre


def _rows(rng, dtype, n, dim, integer=False):
    if dtype == O.U8 or integer:
        return rng.integers(0, 4 if integer else 256, (n, dim)).astype(np.float32)
    return rng.standard_normal((n, dim)).astype(np.float32)


def _relevance(st, dtype, queries, ids):
    """rel[qi][id]: what qmx_score_points gives query qi for the row.  f16 scores of a batch of 8 and more queries come from the matrix cores in
    another summation order (within 1e-5): there the one-query batches are asked, whose bits the gather path shares."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    if dtype == O.F16 and len(queries) >= 8:
        scores = np.concatenate([qa.new_raw_scorer(queries[i:i + 1], st).score_points(ids) for i in range(len(queries))])
    else:
        scores = qa.new_raw_scorer(queries, st).score_points(ids)
    return [dict(zip(ids.tolist(), scores[qi])) for qi in range(len(queries))]


def _check(st, dtype, dist, rows32, queries, candidates, lambda_, limit):
    got = qa.mmr(st, queries, candidates, lambda_, limit)
    ids = np.unique(np.concatenate([c["idx"] for c in candidates] + [np.zeros(0, dtype=np.uint32)]))
    rel = _relevance(st, dtype, queries, ids) if len(ids) else [{} for _ in candidates]
    sim_dist = O.DOT if dist == O.COSINE else dist      # the f32 metric on the rows as stored
    assert len(got) == len(candidates)
    for qi, cand in enumerate(candidates):
        want = FR.mmr_from_points(cand, lambda i: rel[qi][i], lambda c, s: O.similarity(O.F32, sim_dist, rows32[c], rows32[s]), lambda_, limit)
        assert got[qi]["idx"].tolist() == want["idx"].tolist(), (qi, lambda_, limit)
        assert np.array_equal(got[qi]["score"].view(np.uint32), want["score"].view(np.uint32)), qi


def _candidates(rng, n, nq, c, duplicates=False):
    out = []
    for _ in range(nq):
        ids = rng.choice(n, size=c, replace=duplicates)
        cand = np.zeros(c, dtype=SPO)
        cand["idx"], cand["score"] = ids, np.sort(rng.standard_normal(c).astype(np.float32))[::-1]
        out.append(cand)
    return out


@pytest.mark.parametrize("dim", [2, 70, 768])
@pytest.mark.parametrize("dist", [O.COSINE, O.DOT, O.EUCLID, O.MANHATTAN])
@pytest.mark.parametrize("dtype", [O.F32, O.F16, O.U8])
def test_storage_types_distances_dims(dtype, dist, dim):
    rng = np.random.default_rng(dtype * 100 + dist * 10 + dim)
    n, nq = 1500, 2
    st, rows32 = _storage(dtype, dist, _rows(rng, dtype, n, dim))
    queries = _rows(rng, dtype, nq, dim)
    _check(st, dtype, dist, rows32, queries, _candidates(rng, n, nq, 100), 0.5, 12)


@pytest.mark.parametrize("c,limits", [(2, (1, 2, 5)), (5, (3, 5, 9)), (100, (7, 100, 130)), (1000, (10, 40))])
def test_candidate_counts_and_limits(c, limits):
    rng = np.random.default_rng(c)
    n, dim, nq = 3000, 70, 2
    st, rows32 = _storage(O.F32, O.COSINE, _rows(rng, O.F32, n, dim))
    queries = _rows(rng, O.F32, nq, dim)
    cand = _candidates(rng, n, nq, c)
    for i, limit in enumerate(limits):      # below, equal to and above the number of candidates (1 000: below only, the restatement is quadratic)
        _check(st, O.F32, O.COSINE, rows32, queries, cand, (0.5, 0.01, 1.0)[i % 3], limit)


@pytest.mark.parametrize("lambda_", [0.0, 0.01, 0.5, 1.0])
def test_lambdas(lambda_):
    rng = np.random.default_rng(17)
    n, dim, nq = 2000, 768, 2
    st, rows32 = _storage(O.F32, O.DOT, _rows(rng, O.F32, n, dim))
    _check(st, O.F32, O.DOT, rows32, _rows(rng, O.F32, nq, dim), _candidates(rng, n, nq, 100), lambda_, 15)


@pytest.mark.parametrize("nq", [1, 32, 128])
def test_batch_sizes_and_ragged_counts(nq):
    rng = np.random.default_rng(nq)
    n, dim = 2000, 70
    for dtype in (O.F32, O.F16):
        st, rows32 = _storage(dtype, O.COSINE, _rows(rng, dtype, n, dim))
        cand = [c[:int(rng.integers(0, 41))] for c in _candidates(rng, n, nq, 40)]      # ragged, some empty or with one entry
        cand[0] = cand[0][:1] if nq > 1 else cand[0]
        _check(st, dtype, O.COSINE, rows32, _rows(rng, dtype, nq, dim), cand, 0.5, 8)


def test_duplicate_candidate_ids():
    rng = np.random.default_rng(3)
    n, dim, nq = 60, 70, 4
    st, rows32 = _storage(O.F32, O.EUCLID, _rows(rng, O.F32, n, dim))
    cand = _candidates(rng, n, nq, 90, duplicates=True)      # 90 draws of 60 ids
    assert all(len(set(c["idx"].tolist())) < len(c) for c in cand)
    _check(st, O.F32, O.EUCLID, rows32, _rows(rng, O.F32, nq, dim), cand, 0.5, 200)


@pytest.mark.parametrize("dtype", [O.F32, O.F16, O.U8])
@pytest.mark.parametrize("dim", [2, 70])
def test_planted_exact_ties_follow_the_swap_remove_order(dtype, dim):
    """The hand-derived case of tests/test_fusion_reference.py (duplicate rows, integer coordinates: relevance and MMR scores tie exactly), its
    rows padded with zeros to 70 coordinates for the 8-lane leaf: the order rule decides three of the five picks."""
    rows = np.zeros((16, dim), dtype=np.float32)
    rows[10:16, :2] = TIE_ROWS      # candidates 0..5 are points 10..15
    query = np.zeros((1, dim), dtype=np.float32)
    query[0, :2] = TIE_QUERY
    stored = O.cast(dtype, rows)      # small integers: exact in every element type
    st = qa.VectorStorage(stored.view(np.float16) if dtype == O.F16 else stored, DIST[O.DOT], DT[dtype])
    cand = np.zeros(6, dtype=SPO)
    cand["idx"], cand["score"] = np.arange(10, 16), [6, 5, 4, 3, 2, 1]
    got = qa.mmr(st, query, [cand], 0.5, 5)[0]
    assert got["idx"].tolist() == [10 + c for c in TIE_EXPECTED]
    assert got["score"].tolist() == [cand["score"][c] for c in TIE_EXPECTED]      # the input scores, in selection order
    _check(st, dtype, O.DOT, rows, query, [cand], 0.5, 5)


@pytest.mark.parametrize("dtype", [O.F32, O.U8])
def test_ties_in_bulk_small_integer_rows(dtype):
    """Rows of small integers with many exact duplicates: relevance and MMR scores tie all the time, every score is exact."""
    rng = np.random.default_rng(29)
    n, dim, nq = 40, 70, 8
    base = rng.integers(0, 3, (8, dim)).astype(np.float32)
    rows = base[rng.integers(0, 8, n)]      # 40 points, 8 distinct rows
    for dist in (O.DOT, O.MANHATTAN):
        st, rows32 = _storage(dtype, dist, rows)
        queries = base[rng.integers(0, 8, nq)]
        _check(st, dtype, dist, rows32, queries, _candidates(rng, n, nq, 30), 0.5, 30)


@pytest.mark.parametrize("dist", [O.COSINE, O.DOT, O.EUCLID, O.MANHATTAN])
@pytest.mark.parametrize("dim", [2, 70, 768])
def test_pair_score_contract(dist, dim):
    """sim(c, s) of the expectation = candidate c as the query against stored row s: on an f32 segment the bits of
    new_raw_scorer_internal([c]).score_points([s])."""
    rng = np.random.default_rng(dim + dist)
    n = 300
    st, rows32 = _storage(O.F32, dist, _rows(rng, O.F32, n, dim))
    sim_dist = O.DOT if dist == O.COSINE else dist
    cs = rng.choice(n, 6, replace=False)
    ss = rng.choice(n, 20, replace=False).astype(np.uint32)
    got = qa.new_raw_scorer_internal(cs, st).score_points(ss)
    want = np.array([[O.similarity(O.F32, sim_dist, rows32[c], rows32[s]) for s in ss] for c in cs], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_refusals():
    rng = np.random.default_rng(1)
    st, _ = _storage(O.F32, O.DOT, _rows(rng, O.F32, 50, 70))
    q = _rows(rng, O.F32, 1, 70)
    cand = _candidates(rng, 50, 1, 10)
    bad = cand[0].copy()
    bad["idx"][4] = 50      # past the segment's rows
    with pytest.raises(qa.QmxError) as e:
        qa.mmr(st, q, [bad], 0.5, 5)
    assert e.value.status == F.ERR_OUT_OF_BOUNDS
    assert qa.mmr(st, q, cand, 0.5, 5)[0]["idx"].tolist() != []      # the batch is usable afterwards
    too_many = np.zeros(F.MMR_MAX_CANDIDATES + 1, dtype=SPO)
    with pytest.raises(qa.QmxError) as e:
        qa.mmr(st, q, [too_many], 0.5, 5)
    assert e.value.status == F.ERR_NOT_SUPPORTED
    sparse = qa.SparseVectorStorage([(np.array([1, 2], dtype=np.uint32), np.array([1.0, 2.0], dtype=np.float32))] * 4)
    sq = qa.new_raw_scorer([(np.array([1], dtype=np.uint32), np.array([1.0], dtype=np.float32))], sparse)
    with pytest.raises(qa.QmxError) as e:
        qa.mmr(sparse, sq, [np.array([(0, 1.0), (1, 0.5)], dtype=SPO)], 0.5, 2)
    assert e.value.status == F.ERR_NOT_SUPPORTED
    sqz = qa.ScalarQuantizer.from_min_max(_rows(rng, O.F32, 50, 70), 70, qa.Distance.Dot)
    quantized = qa.EncodedVectorsU8(sqz.encode(_rows(rng, O.F32, 50, 70)), sqz)
    with pytest.raises(qa.QmxError) as e:
        qa.mmr(quantized, q, cand, 0.5, 5)
    assert e.value.status == F.ERR_NOT_SUPPORTED


def test_the_candidate_cap_itself_runs():
    rng = np.random.default_rng(4096)
    n, dim = 5000, 32
    st, rows32 = _storage(O.F32, O.DOT, _rows(rng, O.F32, n, dim))
    cand = _candidates(rng, n, 1, F.MMR_MAX_CANDIDATES)
    _check(st, O.F32, O.DOT, rows32, _rows(rng, O.F32, 1, dim), cand, 0.5, 6)


def _sparse_rows(rng, n, n_dims, nnz):
    rows = []
    for _ in range(n):
        k = int(rng.integers(1, nnz + 1))
        rows.append((rng.choice(n_dims, size=k, replace=False).astype(np.uint32), rng.lognormal(0.0, 1.0, k).astype(np.float32)))
    return rows


@pytest.mark.parametrize("fusion", ["rrf", "dbsf"])
def test_hybrid_search_end_to_end_equals_the_stages_composed_by_hand(fusion):
    rng = np.random.default_rng(77)
    n, dim, nq, top = 20000, 70, 5, 30
    st, rows32 = _storage(O.F32, O.COSINE, _rows(rng, O.F32, n, dim))
    sparse = qa.SparseVectorStorage(_sparse_rows(rng, n, 300, 12))
    queries = _rows(rng, O.F32, nq, dim)
    sparse_queries = _sparse_rows(rng, nq, 300, 8)
    limits = (60, 100)      # each source its own prefetch limit
    f = qa.Rrf(k=2, weights=[1.0, 0.5]) if fusion == "rrf" else qa.Dbsf(weights=[2.0])
    sources = [(qa.new_raw_scorer(queries, st), limits[0]), (qa.new_raw_scorer(sparse_queries, sparse), limits[1])]
    fused = qa.hybrid_search(sources, f, top)
    reranked = qa.hybrid_search(sources, f, top, mmr=qa.Mmr(qa.new_raw_scorer(queries, st), 0.5, 10))
    # by hand: the two searches, the restatement of the fusion, the restatement of MMR over the fused list
    dense_lists = qa.BatchFilteredSearcher(queries, st, limits[0]).peek_top_all()
    sparse_lists = sparse.search(sparse_queries, limits[1])
    rel = _relevance(st, O.F32, queries, np.unique(np.concatenate([w["idx"] for w in fused])))
    for qi in range(nq):
        responses = [dense_lists[qi], sparse_lists[qi]]
        want = FR.rrf_scoring(responses, 2, [1.0, 0.5], top) if fusion == "rrf" else FR.score_fusion(responses, [2.0], top)
        assert fused[qi]["idx"].tolist() == want["idx"].tolist(), qi
        assert np.array_equal(fused[qi]["score"].view(np.uint32), want["score"].view(np.uint32)), qi
        picked = FR.mmr_from_points(want, lambda i: rel[qi][i], lambda c, s: O.similarity(O.F32, O.DOT, rows32[c], rows32[s]), 0.5, 10)
        assert reranked[qi]["idx"].tolist() == picked["idx"].tolist(), qi
        assert np.array_equal(reranked[qi]["score"].view(np.uint32), picked["score"].view(np.uint32)), qi
