"""The int8 prefilter's first launch (the strided sixteenth of the 256-row tiles, admitted on the sample's bound: tens of candidates per wave and tile)
has an epilogue of its own since option `i8_dense_epilogue` (default 1; qdrant_amd/csrc/scan_i8copy.hip, scan_i8copy_kernel_res_dense): a hit mask per
lane and query tile and dense slots per wave instead of a ballot per row.  0 gives the one epilogue for both launches.  Every case runs with both
values: the lists are the oracle's (ids and score bits) either way, and the candidate, verified-row and fallback counters are equal - the set of
candidates a launch lists does not depend on which epilogue listed it.

Where the special rows go: the first launch takes the tiles whose index is a multiple of 16, rows [4096 m, 4096 m + 256).  Lane (kq, m_r) of wave w
holds rows 4096 m + 32 w + 4 kq + {0 .. 3} and the same + 16, for query 16 nt + m_r."""
import numpy as np
import pytest

import oracle_ffi as O
from parity_asserts import assert_reference_lists

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


class _Once:
    """The oracle's answers, computed once and shared by the two runs of a case."""

    def __init__(self, storage):
        self._st, self.rows, self._memo = storage, storage.rows, {}

    def peek_top(self, queries, top, threads=0):
        key = ("peek", queries.tobytes(), top)
        if key not in self._memo:
            self._memo[key] = self._st.peek_top(queries, top, threads=threads)
        return self._memo[key]

    def score_points(self, queries, ids):
        key = ("score", queries.tobytes(), len(ids))
        if key not in self._memo:
            self._memo[key] = self._st.score_points(queries, ids)
        return self._memo[key]


def _search(qa, option, queries, vs, top, allowed=None):
    qa.set_option("i8_dense_epilogue", option)
    try:
        s = qa.BatchFilteredSearcher(queries, vs, top)
        if allowed is not None:
            s.scorer.set_filter(allowed)
        got = s.peek_top_all()
        kernel = qa._ffi.last_kernel(s.scorer._h)
    finally:
        qa.set_option("i8_dense_epilogue", -1)
    assert "scan_i8copy_kernel_res" in kernel, kernel
    c = s.counters
    assert c.prefilter_queries == len(queries)
    return got, (c.prefilter_candidates, c.verified_rows, c.fallback_queries)


def _both(qa, storage, queries, vs, top, live=None, allowed=None):
    """Both option values against the oracle; returns the (equal) counters."""
    once = _Once(storage)
    counters = []
    for option in (0, 1):
        got, cnt = _search(qa, option, queries, vs, top, allowed)
        assert_reference_lists(got, once, queries, top, live=live)
        print("i8_dense_epilogue=%d: prefilter_candidates %d, verified_rows %d, fallback_queries %d" % ((option,) + cnt))
        counters.append(cnt)
    assert counters[0] == counters[1], counters
    return counters[1]


def _lane_rows(m, w, kq):
    """the eight rows of lane (kq, *) of wave w in first-launch tile 16 m"""
    base = 4096 * m + 32 * w + 4 * kq
    return [base + j for j in range(4)] + [base + 16 + j for j in range(4)]


def _plant_eight_in_one_lane(raw, queries, dim):
    """For four queries: the query itself and seven small perturbations of it on the eight rows of ONE lane (eight hits in one lane and query tile), in
    three different waves and kq groups.  Returns the planted rows per query."""
    noise = O.synth(0x5EED0E10, 0, 8, dim)
    planted = {}
    for qi, (m, w, kq) in ((5, (1, 0, 0)), (37, (2, 3, 2)), (127, (3, 7, 3)), (16, (3, 7, 1))):
        rows = _lane_rows(m, w, kq)
        for j, r in enumerate(rows):
            raw[r] = queries[qi] + (0.002 * j) * noise[j]
        planted[qi] = rows
    return planted


@pytest.mark.parametrize("n", [300_000, 270_001])
@pytest.mark.parametrize("dim,nq,top", [(128, 128, 10), (768, 130, 10), (1024, 7, 64), (128, 1, 10)])
def test_plain_blocks_with_either_epilogue(qa, n, dim, nq, top):
    """One, six and eight 128-coordinate stages per tile, a second query tile with two live queries, query slots past nq, a ragged last tile."""
    rows = O.preprocess(O.COSINE, O.synth(0x5EED0E00 + dim, 0, n, dim))
    queries = O.synth(0x5EED0E01 + nq, 0, nq, dim)
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    cnt = _both(qa, O.DenseStorage(O.F32, O.COSINE, rows), queries, vs, top)
    assert cnt[0] > 0 and cnt[2] == 0


def test_eight_hits_in_one_lane(qa):
    n, dim, nq, top = 300_000, 128, 128, 10
    raw = O.synth(0x5EED0E20, 0, n, dim)
    queries = O.synth(0x5EED0E21, 0, nq, dim)
    planted = _plant_eight_in_one_lane(raw, queries, dim)
    rows = O.preprocess(O.COSINE, raw)
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    _both(qa, O.DenseStorage(O.F32, O.COSINE, rows), queries, vs, top)
    got, _ = _search(qa, 1, queries, vs, top)
    for qi, want_rows in planted.items():
        assert sorted(got[qi]["idx"][:8].tolist()) == want_rows, qi          # the eight rows of the one lane are the query's eight best


def test_a_wave_whose_32_rows_are_near_copies_of_20_queries(qa):
    n, dim, nq, top = 300_000, 128, 128, 10
    raw = O.synth(0x5EED0E30, 0, n, dim)
    queries = O.synth(0x5EED0E31, 0, nq, dim)
    noise = O.synth(0x5EED0E32, 0, 32, dim)
    near = 3 + 6 * np.arange(20)                                             # queries 3, 9, .., 117: eight of the lane columns, all eight query tiles
    for m, w in ((1, 2), (4, 5)):
        for i in range(32):
            raw[4096 * m + 32 * w + i] = queries[near[i % 20]] + 0.01 * noise[i]
    rows = O.preprocess(O.COSINE, raw)
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    _both(qa, O.DenseStorage(O.F32, O.COSINE, rows), queries, vs, top)


def test_planted_hits_with_deleted_rows_and_a_filter(qa):
    n, dim, nq, top = 300_000, 128, 128, 10
    rng = np.random.default_rng(17)
    raw = O.synth(0x5EED0E40, 0, n, dim)
    queries = O.synth(0x5EED0E41, 0, nq, dim)
    planted = _plant_eight_in_one_lane(raw, queries, dim)
    rows = O.preprocess(O.COSINE, raw)
    deleted = rng.random(n) < 0.1
    vdel = rng.random(n) < 0.02
    for lane_rows in planted.values():                                       # half of every lane's hits: two point-deleted, two vector-deleted
        deleted[lane_rows] = False
        vdel[lane_rows] = False
        deleted[[lane_rows[0], lane_rows[5]]] = True
        vdel[[lane_rows[2], lane_rows[7]]] = True
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    vs.set_deleted(deleted, vdel)
    st = O.DenseStorage(O.F32, O.COSINE, rows, point_deleted=deleted, vec_deleted=vdel)
    _both(qa, st, queries, vs, top, live=~(deleted | vdel))
    allowed = rng.random(n) < 0.5
    for lane_rows in planted.values():                                       # ... and the bitmap takes two more of them
        allowed[lane_rows] = True
        allowed[[lane_rows[1], lane_rows[6]]] = False
    st_f = O.DenseStorage(O.F32, O.COSINE, rows, point_deleted=deleted | ~allowed, vec_deleted=vdel)
    _both(qa, st_f, queries, vs, top, live=~(deleted | ~allowed | vdel), allowed=allowed)
    got, _ = _search(qa, 1, queries, vs, top, allowed)
    for qi, lane_rows in planted.items():
        left = [lane_rows[j] for j in (3, 4)]
        assert sorted(got[qi]["idx"][:2].tolist()) == left, qi


def test_a_wave_list_is_clamped_at_its_capacity(qa):
    """2 200 000 equal unit rows: the smallest block in which a thread block of the first launch owns three tiles (more than 2 097 152 rows), so that a
    wave meets 96 rows x 128 queries = 12 288 hits for a list of 8 192: the count goes on past the capacity, the stores stop at it, the regroup
    reports the overflow and every query takes the exact scan - with either epilogue.  Every score is a 2 200 000-fold tie: the lowest offsets."""
    n, dim, nq, top = 2_200_000, 128, 128, 10
    unit = O.preprocess(O.COSINE, O.synth(0x5EED0E50, 0, 1, dim))
    rows = np.tile(unit, (n, 1))
    queries = O.synth(0x5EED0E51, 0, nq, dim)
    st = O.DenseStorage(O.F32, O.COSINE, rows)
    want = st.peek_top(queries, top, threads=8)
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    counters = []
    for option in (0, 1):
        got, cnt = _search(qa, option, queries, vs, top)
        print("i8_dense_epilogue=%d: prefilter_candidates %d, verified_rows %d, fallback_queries %d" % ((option,) + cnt))
        for qi, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32)), qi
            assert g["idx"].tolist() == list(range(top)) and sorted(w["idx"].tolist()) == list(range(top)), qi
        # (parity_asserts scores every row for each query of a mass tie: two of them say what all 128 would)
        assert assert_reference_lists(got[:2], st, queries[:2], top) == 2
        counters.append(cnt)
    assert counters[0] == counters[1] and counters[1][2] > 0, counters
