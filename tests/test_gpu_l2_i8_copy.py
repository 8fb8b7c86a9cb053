"""The centred int8 copy of an f32 Euclid block (QMX_SEG_L2_I8_COPY; qdrant_amd/csrc/scan_l2i8.hip): 128 queries per pass of the codes of x - mu on the
int8 matrix cores, |q - x|^2 = |q - mu|^2 + |x - mu|^2 - 2 (q - mu).(x - mu), the rows within a worst-case band of a sample's k-th best score re-scored
exactly.  The approximate scores never leave the library: the lists must be the oracle's ids and score bits, ties included."""
import functools

import numpy as np
import pytest

import oracle_ffi as O
from parity_asserts import assert_reference_lists

pytestmark = pytest.mark.gpu

N = (1 << 18) + 37        # the last 256-row tile is partial; one row tile above the route's size gate
KERNEL = "scan_l2i8_kernel"


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


@functools.lru_cache(maxsize=2)
def _rows(dim, kind="plain"):
    rows = O.synth(0x5EED0900 + dim, 0, N, dim)
    if kind == "shifted":
        rows = rows + np.float32(50.0)
    elif kind == "outlier_columns":
        rows[:, :3] *= 40.0
    elif kind == "scaled_rows":
        rows = rows * np.exp(np.random.default_rng(11).standard_normal((N, 1))).astype(np.float32)
    return np.ascontiguousarray(rows, dtype=np.float32)


def _queries(rows, nq, dim):
    """Queries distributed like the rows (a Euclid collection's queries live where its points do): stored rows, jittered."""
    pick = np.random.default_rng(nq).choice(rows.shape[0], nq, replace=False)
    return np.ascontiguousarray(rows[pick] + 0.1 * O.synth(0x5EED0901 + nq, 0, nq, dim), dtype=np.float32)


def _search(qa, rows, queries, top, flags=None):
    vs = qa.VectorStorage(rows, qa.Distance.Euclid, flags=qa._ffi.SEG_L2_I8_COPY if flags is None else flags)
    return vs, qa.BatchFilteredSearcher(queries, vs, top)


@pytest.mark.parametrize("dim,nq,top", [(128, 1, 10), (128, 130, 1), (256, 65, 64), (768, 200, 10)])
def test_l2_int8_copy_returns_the_exact_scan(qa, dim, nq, top):
    rows = _rows(dim)
    queries = _queries(rows, nq, dim)
    vs, s = _search(qa, rows, queries, top)
    got = s.peek_top_all()
    assert KERNEL in qa._ffi.last_kernel(s.scorer._h), qa._ffi.last_kernel(s.scorer._h)
    assert_reference_lists(got, O.DenseStorage(O.F32, O.EUCLID, rows), queries, top)
    assert s.counters.prefilter_queries == nq
    if dim == 128:
        info = vs.info()
        assert info["derived_copy"] == "l2_i8" and info["derived_copy_bytes"] == (N + 255) // 256 * 256 * (dim + 4)


@pytest.mark.parametrize("kind", ["shifted", "outlier_columns", "scaled_rows"])
def test_l2_int8_copy_on_rows_that_stretch_the_band(qa, kind):
    """A constant 50.0 in every coordinate (centring must leave the band where the plain rows have it: nobody overflows), columns forty times the others,
    rows of very different lengths: more rows are verified or a query takes the exact scan - the lists stay the exact scan's."""
    dim, nq, top = 128, 96, 10
    rows = _rows(dim, kind)
    queries = _queries(rows, nq, dim)
    _, s = _search(qa, rows, queries, top)
    got = s.peek_top_all()
    assert_reference_lists(got, O.DenseStorage(O.F32, O.EUCLID, rows), queries, top)
    assert s.counters.prefilter_queries == nq
    if kind == "shifted":
        assert KERNEL in qa._ffi.last_kernel(s.scorer._h) and s.counters.fallback_queries == 0


@pytest.mark.parametrize("how", ["deleted", "filter", "filters"])
def test_l2_int8_copy_with_deleted_rows_and_filters(qa, how):
    dim, nq, top = 128, 100, 10
    rng = np.random.default_rng(3)
    rows = _rows(dim)
    queries = _queries(rows, nq, dim)
    deleted, vdel = rng.random(N) < 0.4, rng.random(N) < 0.05
    vs, s = _search(qa, rows, queries, top)
    vs.set_deleted(deleted, vdel)
    masks = rng.random((2, N)) < 0.3
    if how == "filter":
        s.scorer.set_filter(masks[0])
    elif how == "filters":
        s.scorer.set_filters(masks, [i % 2 for i in range(nq)])
    got = s.peek_top_all()
    assert KERNEL in qa._ffi.last_kernel(s.scorer._h) and s.counters.prefilter_queries == nq
    for f in range(2):      # the queries held to mask f (no filter: all of them once)
        sel = np.arange(nq) if how != "filters" else np.arange(f, nq, 2)
        dead = deleted if how == "deleted" else deleted | ~masks[f]
        if how == "filters" or f == 0:
            assert_reference_lists([got[i] for i in sel], O.DenseStorage(O.F32, O.EUCLID, rows, point_deleted=dead, vec_deleted=vdel), queries[sel], top,
                                   live=~(dead | vdel))


def test_l2_int8_copy_falls_back_when_scores_tie_in_masses(qa):
    """Every row exists 30 000 times: the tied rows at the top want more room than the verification pool has, the queries that come too late take the
    conditional exact Euclid pass (scan_l2_exact_groups_kernel) - the lists stay exact, the lowest offsets of every tied group."""
    dim, nq, top, rep = 128, 70, 10, 30_000
    rows = np.tile(O.synth(0x5EED0930, 0, -(-N // rep), dim), (rep, 1))      # 9 x 30 000 rows: above the route's size gate
    queries = O.synth(0x5EED0931, 0, nq, dim)
    _, s = _search(qa, rows, queries, top)
    got = s.peek_top_all()
    assert KERNEL in qa._ffi.last_kernel(s.scorer._h)
    assert s.counters.prefilter_queries == nq and 0 < s.counters.fallback_queries <= nq
    assert assert_reference_lists(got, O.DenseStorage(O.F32, O.EUCLID, rows), queries, top) == nq


@pytest.mark.parametrize("how", ["top65", "ids", "dot_segment"])
def test_l2_int8_route_is_not_taken(qa, how):
    """top above the fast list, an id list: today's exact route, exact lists.  A dot segment with the flag holds no copy."""
    dim, nq = 128, 20
    rows = _rows(dim)
    queries = _queries(rows, nq, dim)
    if how == "dot_segment":
        vs = qa.VectorStorage(rows, qa.Distance.Dot, flags=qa._ffi.SEG_L2_I8_COPY)
        assert vs.info()["derived_copy"] is None and vs.info()["derived_copy_bytes"] == 0
        return
    top = 65 if how == "top65" else 10
    _, s = _search(qa, rows, queries, top)
    ids = None if how == "top65" else np.arange(0, N, 3, dtype=np.uint32)
    got = s.peek_top_all() if ids is None else s.peek_top_iter(ids)
    assert KERNEL not in qa._ffi.last_kernel(s.scorer._h) and s.counters.prefilter_queries == 0
    dead = None if ids is None else ~np.isin(np.arange(N), ids)
    assert_reference_lists(got, O.DenseStorage(O.F32, O.EUCLID, rows, point_deleted=dead), queries, top, live=None if dead is None else ~dead)
