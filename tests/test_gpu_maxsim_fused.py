"""The fused MaxSim route (maxsim_fused.hip: dense f32 Dot / Cosine inner rows of 32, 64, .. 256 coordinates) through MultiDenseVectorStorage against
the oracle's MaxSim (oracle_ffi.multi_scores over an f32 DenseStorage), bit for bit; the shapes it does not take keep the two-step route."""
import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu
FUSED = "maxsim_fused_kernel"


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


def _dist(qa, d):
    return {O.COSINE: qa.Distance.Cosine, O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid}[d]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _kernel(qa, st):
    return qa._ffi.last_kernel(st.last_scorer._h)


def _world(qa, distance, dim, lens, tokens, seed):
    """points of `lens` inner rows, multi-queries of `tokens` tokens; the device storage, the queries and the oracle's score of every (query, point)"""
    rng = np.random.default_rng(seed)
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    stored = O.preprocess(distance, rng.standard_normal((int(offsets[-1]), dim)).astype(np.float32))
    queries = [rng.standard_normal((k, dim)).astype(np.float32) for k in tokens]
    first = np.concatenate([[0], np.cumsum(tokens)]).astype(np.uint32)
    full = O.multi_scores(O.DenseStorage(O.F32, distance, stored), np.concatenate(queries), first, offsets, np.arange(len(lens)))
    return rng, qa.MultiDenseVectorStorage(stored, offsets, _dist(qa, distance)), queries, full


@pytest.mark.parametrize("distance,dim", [(O.DOT, 32), (O.COSINE, 96), (O.DOT, 128), (O.COSINE, 256)])
def test_fused_scores_and_lists_bit_exact(qa, distance, dim):
    n_points = 300
    lens = np.random.default_rng(dim).integers(1, 41, n_points)
    lens[[5, 77, 200]] = 0, 150, 64          # an empty point, one that spans more than two 64-row tiles, one of exactly a tile
    # 120 tokens: two 64-token groups, the second one partial; the 70-token query (tokens 50 .. 119) straddles the two
    rng, st, queries, full = _world(qa, distance, dim, lens, (1, 17, 32, 70), seed=dim)
    ids = rng.permutation(n_points).astype(np.uint32)[:150]
    ids[10] = ids[3]                         # a candidate listed twice
    assert np.array_equal(_bits(st.score_points(queries, ids)), _bits(full[:, ids]))
    assert FUSED in _kernel(qa, st)
    for res, sc in zip(st.peek_top_all(queries, 10), full):
        assert np.array_equal(_bits(res["score"]), _bits(np.sort(sc)[::-1][:10]))
        assert np.array_equal(_bits(sc[res["idx"]]), _bits(res["score"]))
    assert FUSED in _kernel(qa, st)
    deleted = rng.random(n_points) < 0.3
    st.set_deleted(deleted)
    cand = np.unique(ids)
    for res, sc in zip(st.peek_top_all(queries, 7, ids=cand), full):
        live = cand[~deleted[cand]]
        assert not deleted[res["idx"]].any() and set(res["idx"].tolist()) <= set(cand.tolist())
        assert np.array_equal(_bits(res["score"]), _bits(np.sort(sc[live])[::-1][:7]))
    assert FUSED in _kernel(qa, st)


@pytest.mark.parametrize("distance,dim,off", [(O.EUCLID, 128, 0), (O.DOT, 33, 0), (O.DOT, 128, 1)])
def test_other_shapes_keep_the_two_step_route(qa, distance, dim, off):
    lens = np.random.default_rng(7).integers(0, 9, 60)
    rng, st, queries, full = _world(qa, distance, dim, lens, (3, 20), seed=dim + off)
    ids = rng.permutation(60).astype(np.uint32)
    qa.set_option("no_maxsim_fused", off)
    try:
        got = st.score_points(queries, ids)
        kernel = _kernel(qa, st)
    finally:
        qa.set_option("no_maxsim_fused", -1)
    assert np.array_equal(_bits(got), _bits(full[:, ids]))
    assert FUSED not in kernel


def test_multivector_custom_query_equals_the_two_step_route(qa):
    lens = np.random.default_rng(3).integers(1, 30, 120)
    rng, st, _, _ = _world(qa, O.DOT, 128, lens, (1,), seed=11)
    ex = [rng.standard_normal((k, 128)).astype(np.float32) for k in (6, 40, 9)]
    reco = [qa.CustomQuery.recommend_best_score(ex[:2], ex[2:])]
    ids = rng.permutation(120).astype(np.uint32)
    got = st.custom_score_points(reco, ids)
    assert FUSED in _kernel(qa, st)
    qa.set_option("no_maxsim_fused", 1)
    try:
        want = st.custom_score_points(reco, ids)
        assert FUSED not in _kernel(qa, st)
    finally:
        qa.set_option("no_maxsim_fused", -1)
    assert np.array_equal(_bits(got), _bits(want))


def test_candidate_past_the_points_is_an_error(qa):
    inner = np.random.default_rng(0).standard_normal((20, 64)).astype(np.float32)
    st = qa.MultiDenseVectorStorage(inner, [0, 5, 20], qa.Distance.Dot)
    with pytest.raises(qa.QmxError):
        st.score_points([inner[:2]], [1, 2])
