"""MMR re-ranking over sparse vectors on the device (qmx_sparse_mmr_select, qmx_sparse_mmr_select_async; sparse_mmr.hip) against the numpy
restatement in tests/sparse_mmr_reference.py, itself pinned on the CPU by tests/test_sparse_mmr_reference.py.  Picks and output scores are
compared id for id and on the uint32 view: no tolerance anywhere.  On a segment without a dimension map the relevance of the restatement is
also compared with the bits of qmx_score_points."""
import numpy as np
import pytest

import qdrant_amd as qa
from qdrant_amd import _ffi as F
import fusion_reference as FR
import sparse_mmr_reference as SM
from test_sparse_mmr_reference import MAP, MAP_LAMBDA, MAP_POINTS, MAP_REQUESTS, candidates, literal_case

pytestmark = pytest.mark.gpu
SPO = FR.ScoredPointOffset
LENGTHS = [0, 1, 7, 8, 9, 31, 64, 65]      # around the 8-lane group and the 64-lane wave, and the empty row
COUNTS = [0, 1, 2, 63, 64, 65, 129, 500]   # 129: past one sweep of 128 candidates per 1 024 threads


def _rows(rng, n, n_dims, lengths, integer):
    rows = []
    for r in range(n):
        k = min(int(lengths[r % len(lengths)] if r < 2 * len(lengths) else rng.choice(lengths)), n_dims)
        ix = np.sort(rng.choice(n_dims, size=k, replace=False)).astype(np.uint32)
        vx = rng.choice([-2.0, -1.0, 1.0, 2.0], size=k) if integer else rng.standard_normal(k)
        rows.append((ix, vx.astype(np.float32)))
    return rows


def _permutation_map(rng, n_dims):
    perm = rng.permutation(n_dims)
    assert np.any(np.diff(perm) < 0)      # non-monotone
    return {d: int(perm[d]) for d in range(n_dims)}


def _storage(rows, dim_map=None, **kw):
    return qa.SparseVectorStorage(rows, dim_map=dim_map, **kw)


def _requests(rng, n, counts, duplicates=True):
    out = []
    for c in counts:
        ids = rng.choice(n, size=c, replace=duplicates and c > 2)
        cand = np.zeros(c, dtype=SPO)
        cand["idx"], cand["score"] = ids, np.sort(rng.standard_normal(c).astype(np.float32))[::-1]
        out.append(cand)
    return out


def _assert_equal(got, want, what):
    assert got["idx"].tolist() == want["idx"].tolist(), what
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32)), what


def _check(st, dense, queries, cands, lambda_, limit, what=()):
    got = qa.sparse_mmr(st, queries, cands, lambda_, limit)
    assert len(got) == len(cands)
    for qi, cand in enumerate(cands):
        _assert_equal(got[qi], SM.mmr_columns(dense, queries[qi], cand, lambda_, limit), (qi, lambda_, limit) + tuple(what))


def _check_relevance_bits(st, dense, queries, cands):
    """unmapped segments: relevance(c) of the restatement has the bits of qmx_score_points"""
    ids = np.unique(np.concatenate([c["idx"] for c in cands] + [np.zeros(0, dtype=np.uint32)])).astype(np.uint32)
    if len(ids) == 0:
        return
    scorer = qa.new_raw_scorer(queries, st)
    scores = scorer.score_points(ids)
    scorer.close()
    for qi, q in enumerate(queries):
        assert np.array_equal(scores[qi].view(np.uint32), dense.scores(ids.astype(np.int64), q).view(np.uint32)), qi


def test_the_references_literal_case_and_the_map_case():
    g, points, query, cand = literal_case()
    rows = [points.get(i, ([], [])) for i in range(7)]      # ids 4, 5, 6 of a segment whose first four rows are empty
    got = qa.sparse_mmr(_storage(rows), [query], [cand], g["lambda"], g["limit"])[0]
    assert got["idx"].tolist() == g["derived_by_hand"]["order"] and got["score"].tolist() == [0.0, 0.0, 0.0]
    # under the non-monotone map the sums still run in ORIGINAL index order
    st = _storage(MAP_POINTS, dim_map=MAP)
    queries = [r[0] for r in MAP_REQUESTS]
    cands = [candidates(r[1]) for r in MAP_REQUESTS]
    got = qa.sparse_mmr(st, queries, cands, MAP_LAMBDA, 3)
    for (query, ids, limit, original, remapped), g_, cand in zip(MAP_REQUESTS, got, cands):
        assert g_["idx"].tolist() == original and g_["idx"].tolist() != remapped
        _assert_equal(g_, SM.mmr(MAP_POINTS, query, cand, MAP_LAMBDA, 3), ids)
    # ... and a map that keeps the order changes nothing
    same = qa.sparse_mmr(_storage(MAP_POINTS, dim_map={1: 10, 2: 20, 3: 30}), queries, cands, MAP_LAMBDA, 3)
    assert [s["idx"].tolist() for s in same] == [r[3] for r in MAP_REQUESTS]


@pytest.fixture(scope="module")
def shapes():
    rng = np.random.default_rng(600)
    n, n_dims = 600, 40
    rows = _rows(rng, n, n_dims, LENGTHS, integer=True)
    return rng, n, n_dims, rows, SM.Dense(rows, n_dims), _permutation_map(rng, n_dims)


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("nq", [1, 3, 33])
def test_shapes_counts_lambdas_limits(shapes, nq, mapped):
    _, n, n_dims, rows, dense, dim_map = shapes
    rng = np.random.default_rng(nq)
    st = _storage(rows, dim_map=dim_map if mapped else None)
    counts = [500] if nq == 1 else [129, 0, 65] if nq == 3 else [COUNTS[i % len(COUNTS)] for i in range(nq)]
    cands = _requests(rng, n, counts)
    assert any(len(set(c["idx"].tolist())) < len(c) for c in cands)      # duplicated ids inside a list
    queries = _rows(rng, nq, n_dims, [0, 3, 9, 40] if nq > 1 else [9], integer=True)
    if not mapped:
        _check_relevance_bits(st, dense, queries, cands)
    for lambda_ in (0.0, 0.5, 1.0):
        for limit in (1, 6, max(counts) + 3):
            _check(st, dense, queries, cands, lambda_, limit, (mapped,))


@pytest.mark.parametrize("mapped", [False, True])
def test_float_weights(shapes, mapped):
    _, n, n_dims, _, _, dim_map = shapes
    rng = np.random.default_rng(33)
    rows = _rows(rng, n, n_dims, LENGTHS, integer=False)
    dense = SM.Dense(rows, n_dims)
    st = _storage(rows, dim_map=dim_map if mapped else None)
    nq = 33
    cands = _requests(rng, n, [200] * nq, duplicates=False)
    queries = _rows(rng, nq, n_dims, [5, 12, 40], integer=False)
    if not mapped:
        _check_relevance_bits(st, dense, queries, cands)
    _check(st, dense, queries, cands, 0.5, 20, (mapped,))


@pytest.mark.parametrize("mapped", [False, True])
def test_a_row_and_a_query_longer_than_the_staging_capacity(mapped):
    """Point 0 has SPARSE_MMR_STAGE_CAP + 1 non-zeros and shares a heavy dimension with the first query: it is a candidate row, the first pick
    (so the row every other candidate is scored against) and the query's match.  The second request's QUERY is that long."""
    rng = np.random.default_rng(6145)
    long_n = F.SPARSE_MMR_STAGE_CAP + 1
    n, n_dims = 48, long_n + 40
    rows = _rows(rng, n, 48, [1, 7, 8, 9, 31], integer=True)      # the short rows live in the first 48 dimensions and overlap one another
    heavy = n_dims - 1
    long_ix = np.concatenate([np.arange(long_n - 1), [heavy]]).astype(np.uint32)
    long_vx = rng.choice([-2.0, -1.0, 1.0, 2.0], size=long_n).astype(np.float32)
    long_vx[-1] = 1000.0
    rows[0] = (long_ix, long_vx)
    dense = SM.Dense(rows, n_dims)
    st = _storage(rows, dim_map=_permutation_map(rng, n_dims) if mapped else None)
    q0 = (np.array([3, 5, 17, heavy], dtype=np.uint32), np.array([1.0, -2.0, 1.0, 1.0], dtype=np.float32))
    q1 = (np.arange(long_n, dtype=np.uint32), rng.choice([-1.0, 1.0, 2.0], size=long_n).astype(np.float32))
    cands = [candidates(np.arange(n)), candidates(rng.permutation(n)[:30])]
    queries = [q0, q1]
    if not mapped:
        _check_relevance_bits(st, dense, queries, cands)
    got = qa.sparse_mmr(st, queries, cands, 0.5, 6)
    assert got[0]["idx"][0] == 0
    for qi in range(2):
        _assert_equal(got[qi], SM.mmr_columns(dense, queries[qi], cands[qi], 0.5, 6), (qi, mapped))


def test_the_candidate_cap_itself_runs():
    rng = np.random.default_rng(4096)
    n, n_dims = 5000, 64
    rows = _rows(rng, n, n_dims, [8], integer=False)
    dense = SM.Dense(rows, n_dims)
    st = _storage(rows)
    cands = _requests(rng, n, [F.MMR_MAX_CANDIDATES], duplicates=False)
    _check(st, dense, _rows(rng, 1, n_dims, [20], integer=False), cands, 0.5, 6)


def test_index_weight_types_do_not_change_the_lists():
    rng = np.random.default_rng(16)
    n, n_dims, nq = 300, 40, 4
    rows = _rows(rng, n, n_dims, LENGTHS, integer=False)
    queries = _rows(rng, nq, n_dims, [6, 20], integer=False)
    cands = _requests(rng, n, [100] * nq, duplicates=False)
    want = qa.sparse_mmr(_storage(rows), queries, cands, 0.5, 15)
    for dt in (qa.VectorStorageDatatype.Float16, qa.VectorStorageDatatype.Uint8):
        got = qa.sparse_mmr(_storage(rows, index_datatype=dt), queries, cands, 0.5, 15)
        for g, w in zip(got, want):
            _assert_equal(g, w, dt)


def test_refusals_and_recovery():
    rng = np.random.default_rng(1)
    n, n_dims = 50, 40
    rows = _rows(rng, n, n_dims, LENGTHS, integer=True)
    st = _storage(rows)
    queries = _rows(rng, 1, n_dims, [9], integer=True)
    scorer = qa.new_raw_scorer(queries, st)
    cand = _requests(rng, n, [10], duplicates=False)
    bad = cand[0].copy()
    bad["idx"][4] = n      # past the segment's rows
    with pytest.raises(qa.QmxError) as e:
        qa.sparse_mmr(st, scorer, [bad], 0.5, 5)
    assert e.value.status == F.ERR_OUT_OF_BOUNDS
    again = qa.sparse_mmr(st, scorer, cand, 0.5, 5)      # the same batch is usable afterwards
    _assert_equal(again[0], SM.mmr(rows, queries[0], cand[0], 0.5, 5), "after the refusal")
    with pytest.raises(qa.QmxError) as e:
        qa.sparse_mmr(st, scorer, [np.zeros(F.MMR_MAX_CANDIDATES + 1, dtype=SPO)], 0.5, 5)
    assert e.value.status == F.ERR_NOT_SUPPORTED
    # a dense batch
    dense_st = qa.VectorStorage(rng.standard_normal((n, 8)).astype(np.float32), qa.Distance.Dot)
    dense_scorer = qa.new_raw_scorer(rng.standard_normal((1, 8)).astype(np.float32), dense_st)
    with pytest.raises(qa.QmxError) as e:
        qa.query._mmr(F.lib().qmx_sparse_mmr_select, dense_scorer, cand, 0.5, 5)
    assert e.value.status == F.ERR_BAD_ARG
    # a batch of stored rows: refused on a mapped segment (its rows have lost their original order), served on an unmapped one
    mapped = _storage(rows, dim_map=_permutation_map(rng, n_dims))
    with pytest.raises(qa.QmxError) as e:
        qa.sparse_mmr(mapped, qa.new_raw_scorer_internal([7], mapped), cand, 0.5, 5)
    assert e.value.status == F.ERR_NOT_SUPPORTED
    internal = qa.sparse_mmr(st, qa.new_raw_scorer_internal([7], st), cand, 0.5, 5)
    _assert_equal(internal[0], SM.mmr(rows, rows[7], cand[0], 0.5, 5), "internal batch")
    # the dense entry point keeps refusing sparse batches
    with pytest.raises(qa.QmxError) as e:
        qa.mmr(st, scorer, cand, 0.5, 5)
    assert e.value.status == F.ERR_NOT_SUPPORTED


def test_hybrid_search_with_mmr_over_the_sparse_vector():
    rng = np.random.default_rng(78)
    n, dim, n_dims, nq, top = 20000, 70, 300, 5, 30
    import oracle_ffi as O
    dense_rows = O.preprocess(O.COSINE, rng.standard_normal((n, dim)).astype(np.float32))
    st = qa.VectorStorage(dense_rows, qa.Distance.Cosine)
    rows = []
    for _ in range(n):
        k = int(rng.integers(1, 13))
        rows.append((rng.choice(n_dims, size=k, replace=False).astype(np.uint32), rng.lognormal(0.0, 1.0, k).astype(np.float32)))
    sparse = qa.SparseVectorStorage(rows)
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    sparse_queries = [(rng.choice(n_dims, size=8, replace=False).astype(np.uint32), rng.lognormal(0.0, 1.0, 8).astype(np.float32)) for _ in range(nq)]
    limits = (60, 100)
    f = qa.Rrf(k=2, weights=[1.0, 0.5])
    sources = [(qa.new_raw_scorer(queries, st), limits[0]), (qa.new_raw_scorer(sparse_queries, sparse), limits[1])]
    reranked = qa.hybrid_search(sources, f, top, mmr=qa.Mmr(qa.new_raw_scorer(sparse_queries, sparse), 0.5, 10))
    # by hand: the two searches, the restatement of the fusion, the sparse restatement of MMR over the fused list
    dense_lists = qa.BatchFilteredSearcher(queries, st, limits[0]).peek_top_all()
    sparse_lists = sparse.search(sparse_queries, limits[1])
    for qi in range(nq):
        fused = FR.rrf_scoring([dense_lists[qi], sparse_lists[qi]], 2, [1.0, 0.5], top)
        _assert_equal(reranked[qi], SM.mmr(rows, sparse_queries[qi], fused, 0.5, 10), qi)
