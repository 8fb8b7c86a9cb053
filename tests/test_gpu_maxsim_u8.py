"""The fused u8 MaxSim route (maxsim_u8.hip: dense u8 Dot / Cosine / Euclid inner rows of 32, 64, .. 256 bytes) through MultiDenseVectorStorage against
the oracle's MaxSim (oracle_ffi.multi_scores over a U8 DenseStorage), bit for bit - as are the shapes that keep the two-step route, which is exact too.
The oracle casts f32 queries with `x as u8`: the queries are integers 0 .. 255 stored as f32, so both sides see the same bytes."""
import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu
U8K = "maxsim_u8_kernel"
TR = 128                  # rows per tile of maxsim_u8_kernel


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _world(qa, distance, dim, lens, tokens, seed, flags=0, tweak=None, isa=O.ISA_AUTO):
    """points of `lens` inner u8 rows, multi-queries of `tokens` tokens (`tweak` edits rows and queries in place); the device storage, the queries, the
    oracle's score of every (query, point) and the oracle's storage"""
    rng = np.random.default_rng(seed)
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    rows = rng.integers(0, 256, (int(offsets[-1]), dim), dtype=np.uint8)
    queries = [rng.integers(0, 256, (k, dim)).astype(np.float32) for k in tokens]
    if tweak:
        tweak(rows, offsets, queries)
    first = np.concatenate([[0], np.cumsum(tokens)]).astype(np.uint32)
    ost = O.DenseStorage(O.U8, distance, rows, u8_isa=isa)
    full = O.multi_scores(ost, np.concatenate(queries), first, offsets, np.arange(len(lens)))
    dist = {O.COSINE: qa.Distance.Cosine, O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid, O.MANHATTAN: qa.Distance.Manhattan}[distance]
    inner = qa.VectorStorage(rows, dist, qa.VectorStorageDatatype.Uint8, flags=flags)
    st = qa.MultiDenseVectorStorage(None, offsets, dist, inner_storage=inner)
    return rng, st, queries, full, ost


@pytest.mark.parametrize("distance,dim", [(O.DOT, 32), (O.COSINE, 96), (O.EUCLID, 128), (O.DOT, 160), (O.COSINE, 256), (O.EUCLID, 256)])
def test_u8_scores_and_lists_bit_exact(qa, distance, dim):
    n_points = 300
    lens = np.random.default_rng(dim).integers(1, 41, n_points)
    lens[[5, 77, 200]] = 0, 2 * TR + 44, TR          # an empty point, one that spans more than two tiles, one of exactly a tile
    # 120 tokens: two 64-token groups, the second one partial; the 70-token query (tokens 50 .. 119) straddles the two
    rng, st, queries, full, _ = _world(qa, distance, dim, lens, (1, 17, 32, 70), seed=dim)
    ids = rng.permutation(n_points).astype(np.uint32)[:150]
    ids[10] = ids[3]                                 # a candidate listed twice
    assert np.array_equal(_bits(st.score_points(queries, ids)), _bits(full[:, ids]))
    assert U8K in qa._ffi.last_kernel(st.last_scorer._h)
    for res, sc in zip(st.peek_top_all(queries, 10), full):
        assert np.array_equal(_bits(res["score"]), _bits(np.sort(sc)[::-1][:10]))
        assert np.array_equal(_bits(sc[res["idx"]]), _bits(res["score"]))
    assert U8K in qa._ffi.last_kernel(st.last_scorer._h)
    deleted = rng.random(n_points) < 0.3
    st.set_deleted(deleted)
    cand = np.unique(ids)
    for res, sc in zip(st.peek_top_all(queries, 7, ids=cand), full):
        live = cand[~deleted[cand]]
        assert not deleted[res["idx"]].any() and set(res["idx"].tolist()) <= set(cand.tolist())
        assert np.array_equal(_bits(res["score"]), _bits(np.sort(sc[live])[::-1][:7]))
    assert U8K in qa._ffi.last_kernel(st.last_scorer._h)


@pytest.mark.parametrize("distance,scalar_order", [(O.DOT, False), (O.COSINE, False), (O.EUCLID, False), (O.COSINE, True)])
def test_u8_extremes_that_decide_exactness(qa, distance, scalar_order):
    """a row and a token of all 255 (V = 256 * 255^2 = 16 646 400, one step from 2^24), a row and a token of all 0 (Cosine: 0.0 for those pairs), point 2
    = the zero row alone, points 3 and 4 = rows that tie exactly; in the scalar order (SEG_U8_SCALAR_ORDER / the oracle's scalar leaves) the same kernel
    gives the same bits"""
    def tweak(rows, offsets, queries):
        rows[int(offsets[0])] = 255
        rows[int(offsets[1])] = 0
        rows[int(offsets[2])] = 0
        for p in (3, 4):
            s = int(offsets[p])
            rows[s + 1:int(offsets[p + 1])] = rows[s]
        queries[0][0] = 255.0
        queries[0][1] = 0.0
        queries[1][3] = 0.0
    lens = np.random.default_rng(2).integers(2, 30, 40)
    lens[2], lens[3], lens[4] = 1, 2, 9
    rng, st, queries, full, _ = _world(qa, distance, 256, lens, (2, 9), seed=256, tweak=tweak,
                                       flags=qa._ffi.SEG_U8_SCALAR_ORDER if scalar_order else 0, isa=O.ISA_SCALAR if scalar_order else O.ISA_AUTO)
    ids = rng.permutation(40).astype(np.uint32)
    assert np.array_equal(_bits(st.score_points(queries, ids)), _bits(full[:, ids]))
    assert U8K in qa._ffi.last_kernel(st.last_scorer._h)


@pytest.mark.parametrize("how", ["option_off", "manhattan", "dim48"])
def test_u8_other_shapes_keep_the_two_step_route(qa, how):
    """the exact u8 scans + maxsim_kernel: the oracle's bits as well"""
    distance, dim = (O.MANHATTAN if how == "manhattan" else O.DOT), (48 if how == "dim48" else 64)
    lens = np.random.default_rng(7).integers(1, 24, 60)
    lens[4] = 0
    qa.set_option("no_maxsim_fused", 1 if how == "option_off" else 0)
    try:
        rng, st, queries, full, _ = _world(qa, distance, dim, lens, (3, 20), seed=dim)
        ids = rng.permutation(60).astype(np.uint32)
        got = st.score_points(queries, ids)
        kernel = qa._ffi.last_kernel(st.last_scorer._h)
    finally:
        qa.set_option("no_maxsim_fused", -1)
    assert U8K not in kernel
    assert np.array_equal(_bits(got), _bits(full[:, ids]))


def test_u8_multivector_custom_query_bit_exact(qa):
    """the oracle's multi-vector custom scorer over u8 inner rows (qo_scorer kind 6 over kind 4 over a U8 DenseStorage): its bits"""
    lens = np.random.default_rng(3).integers(1, 30, 120)
    rng, st, _, _, ost = _world(qa, O.DOT, 128, lens, (1,), seed=11)
    ex = [rng.integers(0, 256, (k, 128)).astype(np.float32) for k in (6, 40, 9)]
    reco = qa.CustomQuery.recommend_best_score(ex[:2], ex[2:])
    ids = rng.permutation(120).astype(np.uint32)
    got = st.custom_score_points([reco], ids)
    assert U8K in qa._ffi.last_kernel(st.last_scorer._h)
    s, keep = O.ScorerFactory("multi", O.MultiOracle(("dense", ost), st.offsets)).custom(ex, reco.kind, reco.n_a, reco.n_b, reco.coefs)
    assert np.array_equal(_bits(got[0]), _bits(O.scorer_score_points(s, ids)))
