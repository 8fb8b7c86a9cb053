"""Results in the LAST rows of a block on the prefilter routes other than SQ wide (tests/test_gpu_sq_wide.py plants them there): the int8 copy, the f16
half copy, the f32 split over the rows themselves, TurboQuant wide and the PQ prefilter.  A block of 2^18 + 87 rows - n % 4 = 3, a last tile of 87 rows -
and queries that are near-copies of rows n - 1 ... n - 7 and of the first row of that last, partial 256-row tile: a scan that mistreats the rows behind
its last whole tile, quad or load loses exactly these.  Every route at its minimum batch, or the eight planted queries where that is more (70 for the
split over f32 rows: its tiles start at 65).  The dense routes return the oracle's lists (parity_asserts.assert_reference_lists); the quantized ones
their own 32-query / option-off scans', as tests/test_gpu_tq_wide.py and tests/test_gpu_pq_prefilter.py compare them."""
import numpy as np
import pytest

import oracle_ffi as O
from parity_asserts import assert_reference_lists

pytestmark = pytest.mark.gpu

N, DIM, DIM_TQ, TOP = (1 << 18) + 87, 128, 256, 10
PLANTED = [N - 1 - i for i in range(N % 4 + 4)] + [N - N % 256]
ROUTES = ["i8_copy", "half_copy", "f32_split", "tq_wide", "pq_prefilter"]


def _queries(rows, seed, nq):
    """near-copies of the planted rows first, then rows from anywhere with more noise"""
    rng = np.random.default_rng(seed)
    dim = rows.shape[1]
    sd = float(rows.std())
    nq = max(nq, len(PLANTED))
    queries = (rows[rng.integers(0, N, nq)] + 0.3 * sd * rng.standard_normal((nq, dim))).astype(np.float32)
    queries[:len(PLANTED)] = rows[PLANTED] + 0.05 * sd * rng.standard_normal((len(PLANTED), dim))
    return queries


@pytest.fixture(scope="module")
def world():
    """every segment once: route -> (storage, queries, kernel the route reports, the scan to compare with: None = the dense oracle, else (option, value))"""
    import qdrant_amd as qa
    assert qa.device_count() >= 1
    F = qa._ffi
    assert N % 4 == 3 and N % 256 == 87 and len(PLANTED) == 8 and all(0 < N - x <= 87 for x in PLANTED)
    cos = qa.Distance.Cosine
    rows = O.preprocess(O.COSINE, O.synth(0x7A110001, 0, N, DIM))
    rows_tq = O.preprocess(O.COSINE, O.synth(0x7A110002, 0, N, DIM_TQ))
    tq = qa.TurboQuantizer(DIM_TQ, cos, O.TQ_BITS4)
    centroids = O.PqOracle.train(rows[:3000], DIM, 8, 256, iters=3)
    pq = qa.ProductQuantizer(DIM, cos, 8, centroids)
    nq_tq, nq_pq = int(qa.get_option("tq_wide_min_queries")), int(qa.get_option("pq_prefilter_min_queries"))
    assert nq_tq == 33 and nq_pq == 4      # the defaults these cases are sized for
    cases = {
        "i8_copy": (qa.VectorStorage(rows, cos, flags=F.SEG_I8_COPY), _queries(rows, 1, 5), "scan_i8copy_kernel", None),
        "half_copy": (qa.VectorStorage(rows, cos, flags=F.SEG_HALF_COPY), _queries(rows, 2, 5), "scan_f16pair_kernel<true>", None),
        "f32_split": (qa.VectorStorage(rows, cos), _queries(rows, 3, 70), "scan_f32_split_kernel", None),
        "tq_wide": (qa.EncodedVectorsTQ(tq.encode(rows_tq), tq), _queries(rows_tq, 4, nq_tq), "scan_tq4w_kernel", ("tq_wide_min_queries", 0)),
        "pq_prefilter": (qa.EncodedVectorsPQ(pq.encode(rows), pq), _queries(rows, 5, nq_pq), "pq_prefilter_kernel", ("no_pq_prefilter", 1)),
    }
    return {"qa": qa, "F": F, "cases": cases, "dense": O.DenseStorage(O.F32, O.COSINE, rows)}


@pytest.mark.parametrize("route", ROUTES)
def test_results_in_the_last_rows(world, route):
    qa, F = world["qa"], world["F"]
    st, queries, kernel, other = world["cases"][route]
    s = qa.BatchFilteredSearcher(queries, st, TOP)
    got = s.peek_top_all()
    assert kernel in F.last_kernel(s.scorer._h), F.last_kernel(s.scorer._h)
    assert s.counters.prefilter_queries == len(queries)
    assert all(len(g) == TOP for g in got)
    if other is None:
        assert_reference_lists(got, world["dense"], queries, TOP)
        want = got
    else:
        option, value = other
        qa.set_option(option, value)
        try:
            s2 = qa.BatchFilteredSearcher(queries, st, TOP)
            want = s2.peek_top_all()
            assert kernel not in F.last_kernel(s2.scorer._h)
        finally:
            qa.set_option(option, -1)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g["idx"].tolist() == w["idx"].tolist()
            assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32))
    # the input does what it is for: each planted row is its query's best match in the lists compared with (behind a quantizer: one of the ten)
    for w, row in zip(want, PLANTED):
        assert int(w["idx"][0]) == row if other is None else row in w["idx"].tolist()
