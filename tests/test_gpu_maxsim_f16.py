"""The fused f16 MaxSim route (maxsim_f16.hip: dense f16 Dot / Cosine inner rows of 32, 64, .. 256 halves in a segment created with SEG_F16_WIDE) through
MultiDenseVectorStorage against the oracle's MaxSim (oracle_ffi.multi_scores over an F16 DenseStorage), bit for bit; the shapes it does not take keep
the two-step route and its tolerance."""
import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu
F16K, F32K = "maxsim_f16_kernel", "maxsim_fused_kernel"
REL = 1e-5                # the exact f16 scans' tolerance (test_gpu_dense_f16_u8.py)


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _world(qa, distance, dim, lens, tokens, seed, flags=None, tweak=None):
    """points of `lens` inner f16 rows, multi-queries of `tokens` tokens (`tweak` edits the rows' bits and the queries in place); the device storage,
    the queries, the oracle's score of every (query, point) and the oracle's storage"""
    rng = np.random.default_rng(seed)
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    rows16 = O.to_f16(O.preprocess(distance, rng.standard_normal((int(offsets[-1]), dim)).astype(np.float32)))
    queries = [rng.standard_normal((k, dim)).astype(np.float32) for k in tokens]
    if tweak:
        tweak(rng, rows16, offsets, queries)
    first = np.concatenate([[0], np.cumsum(tokens)]).astype(np.uint32)
    ost = O.DenseStorage(O.F16, distance, rows16)
    full = O.multi_scores(ost, np.concatenate(queries), first, offsets, np.arange(len(lens)))
    dist = {O.COSINE: qa.Distance.Cosine, O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid}[distance]
    inner = qa.VectorStorage(rows16.view(np.float16), dist, qa.VectorStorageDatatype.Float16, flags=qa._ffi.SEG_F16_WIDE if flags is None else flags)
    st = qa.MultiDenseVectorStorage(None, offsets, dist, inner_storage=inner)
    return rng, st, queries, full, ost


@pytest.mark.parametrize("distance,dim", [(O.DOT, 32), (O.COSINE, 96), (O.DOT, 128), (O.COSINE, 256)])
def test_f16_scores_and_lists_bit_exact(qa, distance, dim):
    n_points = 300
    lens = np.random.default_rng(dim).integers(1, 41, n_points)
    lens[[5, 77, 200]] = 0, 150, 64          # an empty point, one that spans more than two 64-row tiles, one of exactly a tile
    # 120 tokens: two 64-token groups, the second one partial; the 70-token query (tokens 50 .. 119) straddles the two
    rng, st, queries, full, _ = _world(qa, distance, dim, lens, (1, 17, 32, 70), seed=dim)
    ids = rng.permutation(n_points).astype(np.uint32)[:150]
    ids[10] = ids[3]                         # a candidate listed twice
    assert np.array_equal(_bits(st.score_points(queries, ids)), _bits(full[:, ids]))
    assert F16K in qa._ffi.last_kernel(st.last_scorer._h)
    for res, sc in zip(st.peek_top_all(queries, 10), full):
        assert np.array_equal(_bits(res["score"]), _bits(np.sort(sc)[::-1][:10]))
        assert np.array_equal(_bits(sc[res["idx"]]), _bits(res["score"]))
    assert F16K in qa._ffi.last_kernel(st.last_scorer._h)
    deleted = rng.random(n_points) < 0.3
    st.set_deleted(deleted)
    cand = np.unique(ids)
    for res, sc in zip(st.peek_top_all(queries, 7, ids=cand), full):
        live = cand[~deleted[cand]]
        assert not deleted[res["idx"]].any() and set(res["idx"].tolist()) <= set(cand.tolist())
        assert np.array_equal(_bits(res["score"]), _bits(np.sort(sc[live])[::-1][:7]))
    assert F16K in qa._ffi.last_kernel(st.last_scorer._h)


def test_f16_flagged_pairs_take_the_whole_point(qa):
    """points 0 .. 9 are one row twice, points 10 .. 19 two rows that differ in the last bit of one small half: best and second best are inside the band
    for every token, the exact kernel walks the point.  Fifty row elements and five of one token are f16 subnormals, one token holds an Inf (its maxima
    are the oracle's +-inf)"""
    def tweak(rng, rows, offsets, queries):
        for p in range(20):
            s = int(offsets[p])
            rows[s, 7] = 0x1400              # 2^-10: a last-bit step of it is 2^-20
            rows[s + 1] = rows[s]
            rows[s + 1, 7] += p >= 10
        rows[rng.integers(0, len(rows), 50), rng.integers(0, 64, 50)] = rng.integers(1, 0x400, 50)
        queries[1][2, :5] = 3.0e-6
        queries[2][4, 9] = np.inf
    lens = np.random.default_rng(1).integers(2, 20, 60)
    lens[:20] = 2
    rng, st, queries, full, _ = _world(qa, O.DOT, 64, lens, (3, 9, 11), seed=64, tweak=tweak)
    assert np.isinf(full[2]).any() and np.isfinite(full[:2]).all()
    ids = rng.permutation(60).astype(np.uint32)
    assert np.array_equal(_bits(st.score_points(queries, ids)), _bits(full[:, ids]))
    assert F16K in qa._ffi.last_kernel(st.last_scorer._h)


@pytest.mark.parametrize("how", ["no_flag", "option_off", "euclid", "dim48", "inf_in_segment"])
def test_f16_other_shapes_keep_the_two_step_route(qa, how):
    """the exact f16 scans sum in their own order: every similarity is within REL of the oracle's, relative.  A MaxSim is a sum of per-token maxima, so
    the same relative bound holds for it where the maxima share a sign: points of 12 rows and more (Dot: the best of 12 normal dots is positive;
    Euclid: every score is negative), and one empty point (-inf on both sides)"""
    def tweak(rng, rows, offsets, queries):
        if how == "inf_in_segment":
            rows[3, 5] = 0x7C00
    distance, dim = (O.EUCLID if how == "euclid" else O.DOT), (48 if how == "dim48" else 64)
    lens = np.random.default_rng(7).integers(12, 24, 60)
    lens[4] = 0
    qa.set_option("no_maxsim_fused", 1 if how == "option_off" else 0)
    try:
        rng, st, queries, full, _ = _world(qa, distance, dim, lens, (3, 20), seed=dim, flags=0 if how == "no_flag" else None, tweak=tweak)
        ids = rng.permutation(60).astype(np.uint32)
        got = st.score_points(queries, ids)
        kernel = qa._ffi.last_kernel(st.last_scorer._h)
    finally:
        qa.set_option("no_maxsim_fused", -1)
    assert F16K not in kernel and F32K not in kernel
    assert np.allclose(got, full[:, ids], rtol=REL, atol=0)


def test_f16_multivector_custom_query_bit_exact(qa):
    """the oracle has the multi-vector custom scorer over f16 inner rows (qo_scorer kind 6 over kind 4 over an F16 DenseStorage): its bits"""
    lens = np.random.default_rng(3).integers(1, 30, 120)
    rng, st, _, _, ost = _world(qa, O.DOT, 128, lens, (1,), seed=11)
    ex = [rng.standard_normal((k, 128)).astype(np.float32) for k in (6, 40, 9)]
    reco = qa.CustomQuery.recommend_best_score(ex[:2], ex[2:])
    ids = rng.permutation(120).astype(np.uint32)
    got = st.custom_score_points([reco], ids)
    assert F16K in qa._ffi.last_kernel(st.last_scorer._h)
    s, keep = O.ScorerFactory("multi", O.MultiOracle(("dense", ost), st.offsets)).custom(ex, reco.kind, reco.n_a, reco.n_b, reco.coefs)
    assert np.array_equal(_bits(got[0]), _bits(O.scorer_score_points(s, ids)))
