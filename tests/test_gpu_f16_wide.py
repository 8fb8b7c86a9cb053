"""Dense f16 segments with QMX_SEG_F16_WIDE (qdrant_amd/csrc/scan_f16w.hip): 128 queries per pass of the f16 rows themselves on the f16 matrix cores, a band
for their summation order, and a re-scoring in the order of the reference's AVX leaf.  The pass's scores never leave the library: the lists must be the
oracle's ids and score bits."""
import functools

import numpy as np
import pytest

import oracle_ffi as O
from parity_asserts import assert_reference_lists

pytestmark = pytest.mark.gpu

N = (1 << 18) + 37        # the last 256-row tile is partial; just above the route's size gate
DISTS = [O.DOT, O.COSINE, O.EUCLID]
REL = 1e-5                # the exact f16 scans' tolerance (test_gpu_dense_f16_u8.py)


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


@pytest.fixture(scope="module", autouse=True)
def _every_batch_size_takes_the_pass(qa):
    qa.set_option("f16_wide_min_queries", 1)      # (the default is a measured crossover, not part of the contract)
    yield
    qa.set_option("f16_wide_min_queries", -1)


def _dist(qa, d):
    return {O.COSINE: qa.Distance.Cosine, O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid}[d]


@functools.lru_cache(maxsize=2)
def _rows(dim, dist=O.DOT):
    raw = np.random.default_rng(0xF16 + dim).standard_normal((N, dim), dtype=np.float32)
    return O.to_f16(O.preprocess(dist, raw) if dist == O.COSINE else raw)


def _queries(nq, dim):
    return np.random.default_rng(nq * 31 + dim).standard_normal((nq, dim)).astype(np.float32)


def _search(qa, rows16, dist, queries, top, flags=None):
    vs = qa.VectorStorage(rows16.view(np.float16), _dist(qa, dist), qa.VectorStorageDatatype.Float16, flags=qa._ffi.SEG_F16_WIDE if flags is None else flags)
    return vs, qa.BatchFilteredSearcher(queries, vs, top)


def _wide_lists(qa, s, nq, dim):
    got = s.peek_top_all()
    kernel = "scan_f16w_staged_kernel" if dim > 512 else "scan_f16w_kernel"
    assert kernel in qa._ffi.last_kernel(s.scorer._h), qa._ffi.last_kernel(s.scorer._h)
    assert s.counters.prefilter_queries == nq
    return got


@pytest.mark.parametrize("dim,nq,top", [(64, 17, 10), (96, 130, 64), (512, 40, 10), (544, 17, 10), (1024, 40, 10)])
@pytest.mark.parametrize("dist", DISTS)
def test_f16_wide_pass_returns_the_oracle_lists(qa, dist, dim, nq, top):
    """dim 64: one stage; 96: three chunks - a partial load group - and a nearly empty second query tile; 512: the resident LDS limit; 544: the first staged
    length, its last stage of one chunk; 1024: the route's limit.  Rows iid normal: nothing overflows"""
    rows, queries = _rows(dim, dist), _queries(nq, dim)
    vs, s = _search(qa, rows, dist, queries, top)
    assert_reference_lists(_wide_lists(qa, s, nq, dim), O.DenseStorage(O.F16, dist, rows), queries, top, threads=16)
    assert s.counters.fallback_queries == 0
    if dim == 64:
        info = vs.info()
        assert info["derived_copy"] == "f16_wide" and info["derived_copy_bytes"] == ((N + 255) // 256 * 256 * 4 if dist == O.EUCLID else 0)


def test_f16_wide_winners_in_the_last_rows_of_the_partial_tile(qa):
    """the last three rows as queries: they lead their lists (a column entry or a row index from the wrong slot loses them), and are absent once deleted"""
    dim, nq, top, dist = 96, 17, 10, O.EUCLID
    rows = _rows(dim)
    queries = _queries(nq, dim)
    queries[:3] = O.f16_to_f32(rows[N - 3:])
    vs, s = _search(qa, rows, dist, queries, top)
    got = _wide_lists(qa, s, nq, dim)
    assert [int(got[i]["idx"][0]) for i in range(3)] == [N - 3, N - 2, N - 1]
    assert_reference_lists(got, O.DenseStorage(O.F16, dist, rows), queries, top, threads=16)
    deleted = np.zeros(N, dtype=bool)
    deleted[N - 3:] = True
    vs.set_deleted(deleted, None)
    s = qa.BatchFilteredSearcher(queries, vs, top)
    got = _wide_lists(qa, s, nq, dim)
    assert not any(np.isin(got[i]["idx"], [N - 3, N - 2, N - 1]).any() for i in range(nq))
    assert_reference_lists(got, O.DenseStorage(O.F16, dist, rows, point_deleted=deleted), queries, top, live=~deleted, threads=16)


def test_f16_wide_subnormal_operands(qa):
    """half of the columns hold f16 subnormals in the rows (values x 2^-17) under queries about 2^13 times larger there: a pass that flushed them would
    rank by the other columns alone - and the oracle's top 10 is not that ranking"""
    dim, nq, top = 64, 17, 10
    raw = np.random.default_rng(77).standard_normal((N, dim), dtype=np.float32)
    raw[:, dim // 2:] *= 2.0 ** -17
    rows = O.to_f16(raw)
    assert ((rows[:, dim // 2:] & 0x7C00) == 0).mean() > 0.99
    queries = _queries(nq, dim)
    queries[:, dim // 2:] *= 2.0 ** 13
    want = O.DenseStorage(O.F16, O.DOT, rows).peek_top(queries, top)
    flushed = rows.copy()
    flushed[:, dim // 2:] = 0
    other = O.DenseStorage(O.F16, O.DOT, flushed).peek_top(queries, top)
    assert any(w["idx"].tolist() != o["idx"].tolist() for w, o in zip(want, other))
    _, s = _search(qa, rows, O.DOT, queries, top)
    assert_reference_lists(_wide_lists(qa, s, nq, dim), O.DenseStorage(O.F16, O.DOT, rows), queries, top, threads=16)


def test_f16_wide_falls_back_when_scores_crowd(qa):
    """nine rows 30 000 times each: the tied rows want more room than the lists have, such queries take the conditional AVX-order exact pass"""
    dim, nq, top, rep = 64, 20, 10, 30_000
    rows = np.tile(_rows(dim)[:-(-N // rep)], (rep, 1))[:N]
    queries = _queries(nq, dim)
    _, s = _search(qa, rows, O.DOT, queries, top)
    got = _wide_lists(qa, s, nq, dim)
    assert 0 < s.counters.fallback_queries <= nq
    assert_reference_lists(got, O.DenseStorage(O.F16, O.DOT, rows), queries, top, threads=16)


def test_f16_wide_with_deleted_rows_and_per_request_filters(qa):
    dim, nq, top = 64, 30, 10
    rng = np.random.default_rng(5)
    rows, queries = _rows(dim), _queries(nq, dim)
    deleted, vdel = rng.random(N) < 0.4, rng.random(N) < 0.05
    masks = rng.random((2, N)) < 0.3
    vs, s = _search(qa, rows, O.EUCLID, queries, top)
    vs.set_deleted(deleted, vdel)
    s.scorer.set_filters(masks, [(0, 1, None)[i % 3] for i in range(nq)])
    got = _wide_lists(qa, s, nq, dim)
    for f, mask in enumerate((masks[0], masks[1], np.ones(N, dtype=bool))):      # the lists of each request alone
        sel = np.arange(f, nq, 3)
        dead = deleted | ~mask
        assert_reference_lists([got[i] for i in sel], O.DenseStorage(O.F16, O.EUCLID, rows, point_deleted=dead, vec_deleted=vdel), queries[sel], top,
                               live=~(dead | vdel), threads=16)


@pytest.mark.parametrize("how", ["no_flag", "no_f16_wide", "dim80"])
def test_f16_wide_route_is_not_taken(qa, how):
    """the exact f16 scans sum in their own order: their lists meet test_f16_peek_top's tolerance checks against the oracle, not bit equality"""
    dim, nq, top = (80 if how == "dim80" else 64), 20, 10
    rows, queries = _rows(dim), _queries(nq, dim)
    qa.set_option("no_f16_wide", 1 if how == "no_f16_wide" else 0)
    try:
        vs, s = _search(qa, rows, O.DOT, queries, top, flags=0 if how == "no_flag" else None)
        got = s.peek_top_all()
    finally:
        qa.set_option("no_f16_wide", -1)
    assert vs.info()["derived_copy"] == (None if how != "no_f16_wide" else "f16_wide")
    assert "scan_f16w" not in qa._ffi.last_kernel(s.scorer._h) and s.counters.prefilter_queries == 0
    ost = O.DenseStorage(O.F16, O.DOT, rows)
    want = ost.peek_top(queries, top)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == top
        assert np.allclose(g["score"], w["score"], rtol=REL, atol=0)
        exact = ost.score_points(queries[i:i + 1], g["idx"].astype(np.uint32))[0]
        kth = w["score"][-1]
        assert np.all(exact >= kth - REL * abs(kth)) and np.allclose(exact, g["score"], rtol=REL, atol=0)
