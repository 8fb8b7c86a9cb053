"""The brute-force search driver (qdrant_amd/csrc/api_search.hip: search_plan picks the route, one function per route) at the smallest shapes that reach
every route - blocks of 2^18 rows, the gate of the prefilters - for what the route suites do not pin: a search cancelled before its first launch on
every route (and the batch object still good afterwards), the counters of the asynchronous call against the synchronous one's, and empty results
(an empty id list, a sparse search with top 0) for host and device counts.

Routes: the int8 copy, the f16 half copy, the f32 split over the rows themselves with 130 queries (a split tile of 128, then a remainder tile of 2 on
the exact route), SQ wide with 33 queries, TurboQuant wide and the PQ prefilter at their options' minimum batches (rows of 256 coordinates for
TurboQuant: its wide pass takes multiples of 256), and exact tiles with top 65 (two passes of the lists)."""
import ctypes as C

import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

N, DIM, TOP = 1 << 18, 128, 10
PREFILTER_ROUTES = ["i8_copy", "half_copy", "f32_split", "sq_wide", "tq_wide", "pq_prefilter"]
ROUTES = PREFILTER_ROUTES + ["exact_top65"]
COMPARED = ["prefilter_queries", "prefilter_candidates", "verified_rows", "fallback_queries", "vectors_scored", "bytes_read"]


@pytest.fixture(scope="module")
def world():
    """every segment once: route -> (storage, queries, top, kernel the route reports or None, queries the prefilter serves)"""
    import qdrant_amd as qa
    assert qa.device_count() >= 1
    F = qa._ffi
    rows = O.preprocess(O.COSINE, O.synth(0x50C70001, 0, N, DIM))
    queries = O.synth(0x50C70002, 0, 130, DIM)
    cos = qa.Distance.Cosine
    plain = qa.VectorStorage(rows, cos)
    sq = qa.ScalarQuantizer.from_min_max(rows[:20000], DIM, cos)
    rows_tq = O.preprocess(O.COSINE, O.synth(0x50C70003, 0, N, 256))
    tq = qa.TurboQuantizer(256, cos, O.TQ_BITS4)
    centroids = O.PqOracle.train(rows[:3000], DIM, 8, 256, iters=3)
    pq = qa.ProductQuantizer(DIM, cos, 8, centroids)
    nq_tq, nq_pq = int(qa.get_option("tq_wide_min_queries")), int(qa.get_option("pq_prefilter_min_queries"))
    assert nq_tq == 33 and nq_pq == 4 and int(qa.get_option("sq_wide_min_queries")) == 33      # the defaults these cases are sized for
    cases = {
        "i8_copy": (qa.VectorStorage(rows, cos, flags=F.SEG_I8_COPY), queries[:5], TOP, "scan_i8copy_kernel", 5),
        "half_copy": (qa.VectorStorage(rows, cos, flags=F.SEG_HALF_COPY), queries[:5], TOP, "scan_f16pair_kernel<true>", 5),
        "f32_split": (plain, queries, TOP, None, 128),      # (the remainder tile's exact kernel is the last one launched)
        "sq_wide": (qa.EncodedVectorsU8(sq.encode(rows), sq), queries[:33], TOP, "scan_sqw_kernel", 33),
        "tq_wide": (qa.EncodedVectorsTQ(tq.encode(rows_tq), tq), O.synth(0x50C70004, 0, nq_tq, 256), TOP, "scan_tq4w_kernel", nq_tq),
        "pq_prefilter": (qa.EncodedVectorsPQ(pq.encode(rows), pq), queries[:nq_pq], TOP, "pq_prefilter_kernel", nq_pq),
        "exact_top65": (plain, queries[:3], 65, None, 0),
    }
    return {"qa": qa, "F": F, "cases": cases, "fresh": {}}


def _fresh(world, route):
    """the lists, counters and kernel of an ordinary search on a new batch object: computed once per route, left unchanged"""
    if route not in world["fresh"]:
        qa = world["qa"]
        st, queries, top, kernel, served = world["cases"][route]
        s = qa.BatchFilteredSearcher(queries, st, top)
        lists = s.peek_top_all()
        name = world["F"].last_kernel(s.scorer._h)
        assert kernel is None or kernel in name, name
        assert s.counters.prefilter_queries == served
        assert all(len(r) == top for r in lists)
        world["fresh"][route] = (lists, s.counters, name)
    return world["fresh"][route]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["idx"].tolist() == w["idx"].tolist()
        assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32))


def test_split_tiles_then_an_exact_remainder_tile(world):
    """130 queries over a block without a copy: queries 0 .. 127 are the split route's (its kernel is what a 128-query batch reports), queries 128 and 129
    the exact route's (the last kernel launched, and what the 130-query batch reports); each part returns what it returns alone"""
    qa, F = world["qa"], world["F"]
    st, queries, top, _, _ = world["cases"]["f32_split"]
    lists, _, name = _fresh(world, "f32_split")
    head = qa.BatchFilteredSearcher(queries[:128], st, top)
    _same(lists[:128], head.peek_top_all())
    assert "scan_f32_split_kernel" in F.last_kernel(head.scorer._h) and head.counters.prefilter_queries == 128
    tail = qa.BatchFilteredSearcher(queries[128:], st, top)
    _same(lists[128:], tail.peek_top_all())
    assert tail.counters.prefilter_queries == 0 and "scan_f32_split_kernel" not in name and name == F.last_kernel(tail.scorer._h)


@pytest.mark.parametrize("route", ROUTES)
def test_cancelled_before_the_first_launch_and_the_batch_stays_good(world, route):
    qa, F = world["qa"], world["F"]
    st, queries, top, _, served = world["cases"][route]
    want, want_counters, want_kernel = _fresh(world, route)
    s = qa.BatchFilteredSearcher(queries, st, top)
    with pytest.raises(F.QmxError) as e:
        s.peek_top_all(is_stopped=True)
    assert e.value.status == F.ERR_CANCELLED and "search cancelled" in str(e.value)
    _same(s.peek_top_all(), want)
    assert F.last_kernel(s.scorer._h) == want_kernel
    for field, _ in F.Counters._fields_:
        if field != "kernel_ms":
            assert getattr(s.counters, field) == getattr(want_counters, field), field


@pytest.mark.parametrize("route", PREFILTER_ROUTES)
def test_async_counters_equal_the_synchronous_call(world, route):
    import torch
    qa, F = world["qa"], world["F"]
    lib = F.lib()
    st, queries, top, _, served = world["cases"][route]
    want, sync, _ = _fresh(world, route)
    s = qa.BatchFilteredSearcher(queries, st, top)
    nq = len(queries)
    out = torch.zeros((nq, top, 2), dtype=torch.int32, device="cuda")
    counts = torch.zeros(nq, dtype=torch.int32, device="cuda")
    F.check(lib.qmx_search_topk_async(s.scorer._h, top, None, 0, F.ptr(out), F.ptr(counts)))
    got = s.scorer.last_counters()      # (synchronises)
    for field in COMPARED:
        assert getattr(got, field) == getattr(sync, field), (field, getattr(got, field), getattr(sync, field))
    assert got.prefilter_queries == served and got.verified_rows >= top * (served - got.fallback_queries)
    o = out.cpu().numpy()
    assert counts.cpu().numpy().tolist() == [top] * nq
    for i in range(nq):
        assert o[i, :, 0].view(np.uint32).tolist() == want[i]["idx"].tolist()
        assert np.array_equal(o[i, :, 1].view(np.uint32), want[i]["score"].view(np.uint32))


@pytest.mark.parametrize("device_counts", [False, True])
def test_empty_results_zero_the_counts(world, device_counts):
    import torch
    qa, F = world["qa"], world["F"]
    lib = F.lib()

    def run(handle, nq, top, ids, n_ids):
        out = np.zeros((nq, max(top, 1)), dtype=O.ScoredPointOffset)
        counts = torch.full((nq,), 7, dtype=torch.int32, device="cuda") if device_counts else np.full(nq, 7, dtype=np.uint32)
        c = F.Counters()
        F.check(lib.qmx_search_topk(handle, top, F.ptr(ids), n_ids, F.ptr(out), F.ptr(counts), None, C.byref(c)))
        assert (counts.cpu().numpy() if device_counts else counts).tolist() == [0] * nq

    # an id list that is given and empty: every queue stays empty, on a prefilter segment and on a plain one
    ids = np.zeros(1, dtype=np.uint32)
    for route in ("i8_copy", "exact_top65"):
        st, queries, top, _, _ = world["cases"][route]
        s = qa.BatchFilteredSearcher(queries, st, top)
        run(s.scorer._h, len(queries), top, ids, 0)
        _same(s.peek_top_all(), _fresh(world, route)[0])
    # a sparse batch with top 0
    rng = np.random.default_rng(5)
    rows = [(np.sort(rng.choice(50, 6, replace=False)).astype(np.uint32), rng.standard_normal(6).astype(np.float32)) for _ in range(200)]
    sparse = qa.SparseVectorStorage(rows)
    scorer = qa.new_raw_scorer(rows[:3], sparse)
    run(scorer._h, 3, 0, None, 0)
