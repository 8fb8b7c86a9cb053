"""Fusion of prefetch lists on the device (qmx_fuse_topk, qmx_fuse_topk_async; fusion.hip) against the numpy restatement of rrf_scoring /
score_fusion in tests/fusion_reference.py.  Every comparison is on the uint32 view of the scores and id for id (score descending, lower offset
first): no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import qdrant_amd as qa
from qdrant_amd import _ffi as F
import fusion_reference as FR

pytestmark = pytest.mark.gpu
SPO = FR.ScoredPointOffset


def _one_list(rng, count, pool, duplicates=False, scale=1.0):
    """A list as a search returns it: ids of `pool`, scores descending."""
    ids = rng.choice(pool, size=count, replace=duplicates) if count else np.zeros(0, dtype=np.int64)
    scores = np.sort((rng.standard_normal(count) * scale).astype(np.float32))[::-1]
    out = np.zeros(count, dtype=SPO)
    out["idx"], out["score"] = ids, scores
    return out


def _lists(seed, n_sources, nq, stride, pools, duplicates=False):
    """Ragged lists: every count in 0..stride, an empty list, a one-entry list and a full list planted."""
    rng = np.random.default_rng(seed)
    lists = []
    for s in range(n_sources):
        src = []
        for qi in range(nq):
            pool = pools[s % len(pools)]
            count = int(rng.integers(0, min(stride, len(pool)) + 1))
            if (qi + s) % 7 == 3:
                count = 0
            elif (qi + s) % 7 == 1:
                count = 1
            elif (qi + s) % 7 == 2:
                count = min(stride, len(pool))
            src.append(_one_list(rng, count, pool, duplicates, scale=10.0 ** (s - 1)))
        lists.append(src)
    return lists


def _check(got, lists, kind, top, k=2, weights=None):
    nq = len(lists[0])
    assert len(got) == nq
    for qi in range(nq):
        responses = [src[qi] for src in lists]
        want = FR.rrf_scoring(responses, k, weights, top) if kind == "rrf" else FR.score_fusion(responses, weights or (), top)
        g = got[qi]
        assert g["idx"].tolist() == want["idx"].tolist(), (kind, qi)
        assert np.array_equal(g["score"].view(np.uint32), want["score"].view(np.uint32)), (kind, qi)


def _fuse(lists, kind, top, k=2, weights=None):
    return qa.rrf(lists, top, k, weights) if kind == "rrf" else qa.dbsf(lists, top, weights)


@pytest.mark.parametrize("kind", ["rrf", "dbsf"])
@pytest.mark.parametrize("n_sources,nq", [(1, 1), (2, 33), (3, 128), (5, 33)])
def test_sources_ragged_counts_heavy_overlap(kind, n_sources, nq):
    pool = np.arange(1000, 1090)      # 90 ids for up to 5 x 60 entries: nearly every id in several lists
    lists = _lists(n_sources * 131 + nq, n_sources, nq, 60, [pool])
    assert any(len(l) == 0 for src in lists for l in src) or nq == 1
    for top in (10, 400):      # below and above the number of distinct ids
        _check(_fuse(lists, kind, top), lists, kind, top)


@pytest.mark.parametrize("kind", ["rrf", "dbsf"])
def test_no_overlap_and_duplicates_inside_a_list(kind):
    pools = [np.arange(s * 10000, s * 10000 + 500) for s in range(3)]      # disjoint id ranges
    lists = _lists(7, 3, 33, 80, pools)
    _check(_fuse(lists, kind, 64), lists, kind, 64)
    _check(_fuse(lists, kind, 300), lists, kind, 300)
    dup = _lists(8, 3, 33, 50, [np.arange(40)], duplicates=True)            # 50 draws of 40 ids: ids repeat inside a list
    assert any(len(set(l["idx"].tolist())) < len(l) for l in dup[0])
    _check(_fuse(dup, kind, 30), dup, kind, 30)


@pytest.mark.parametrize("k", [1, 2, 60])
def test_rrf_k_and_weights(k):
    lists = _lists(90 + k, 3, 33, 40, [np.arange(70)])
    _check(_fuse(lists, "rrf", 50, k), lists, "rrf", 50, k)
    w = [1.5, 0.0, -2.0]      # a zero and a negative weight: position_score is 0.0 for both
    _check(_fuse(lists, "rrf", 50, k, w), lists, "rrf", 50, k, w)
    _check(_fuse(lists, "rrf", 50, k, [3.0, 1.0, 0.25]), lists, "rrf", 50, k, [3.0, 1.0, 0.25])


def test_dbsf_weights_missing_zero_negative_and_constant_list():
    lists = _lists(5, 3, 33, 40, [np.arange(70)])
    for w in ([0.5], [1.0, 0.0, -2.0], [2.0, -0.5]):      # missing weights are 1.0
        _check(_fuse(lists, "dbsf", 50, weights=w), lists, "dbsf", 50, weights=w)
    const = [[np.array([(i, 0.25) for i in range(5, 25)], dtype=SPO)], [_one_list(np.random.default_rng(1), 30, np.arange(40))]]
    got = _fuse(const, "dbsf", 64)      # a constant-score list: variance 0, min == max, 0.5 for every entry
    _check(got, const, "dbsf", 64)
    only = _fuse([const[0]], "dbsf", 64)
    assert np.all(only[0]["score"] == np.float32(0.5)) and only[0]["idx"].tolist() == list(range(5, 25))


def test_dbsf_negative_zero_ties_with_zero_and_keeps_its_bits():
    """An entry more than three deviations below its list's mean normalises below 0; under a zero weight it becomes -0.0, which OrderedFloat
    holds equal to the 0.0 of the list's other entries: the offset decides, and the result carries the sum's own sign bit."""
    outlier = np.array([(i, 10.0) for i in range(20, 31)] + [(3, -1000.0)], dtype=SPO)      # id 3, the lowest, is the outlier
    other = np.array([(100, 2.0), (101, 1.0), (102, 0.5)], dtype=SPO)
    lists = [[outlier], [other]]
    got = _fuse(lists, "dbsf", 64, weights=[0.0, 1.0])[0]
    _check([got], lists, "dbsf", 64, weights=[0.0, 1.0])
    zeros = got[got["score"] == 0]
    assert zeros["idx"].tolist() == [3] + list(range(20, 31))
    assert zeros["score"].view(np.uint32).tolist() == [0x80000000] + [0] * 11


def test_reference_literals_on_device():
    import json
    import os
    lit = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "fusion_literals.json")))
    for case in lit["rrf"]:
        if "expected" not in case:
            continue
        lists = [[np.array([tuple(e) for e in r], dtype=SPO)] for r in case["responses"]]
        got = qa.rrf(lists, 10, case["k"], case["weights"])[0]
        assert got["idx"].tolist() == [e[0] for e in case["expected"]]
        assert np.array_equal(got["score"].view(np.uint32), np.array([e[1] for e in case["expected"]], dtype=np.float32).view(np.uint32))
    for case in lit["rrf_errors"]:
        lists = [[np.array([tuple(e) for e in r], dtype=SPO)] for r in case["responses"]]
        with pytest.raises(qa.QmxError) as e:
            qa.rrf(lists, 10, case["k"], case["weights"])
        assert e.value.status == F.ERR_BAD_ARG


def test_caps_are_refused():
    one = np.array([(1, 1.0)], dtype=SPO)
    with pytest.raises(qa.QmxError) as e:
        qa.rrf([[one]] * (F.FUSE_MAX_SOURCES + 1), 10)
    assert e.value.status == F.ERR_NOT_SUPPORTED
    big = np.zeros(F.FUSE_MAX_ENTRIES // 2 + 1, dtype=SPO)
    big["idx"] = np.arange(len(big))
    with pytest.raises(qa.QmxError) as e:
        qa.rrf([[big], [big]], 10)
    assert e.value.status == F.ERR_NOT_SUPPORTED
    full = big[:F.FUSE_MAX_ENTRIES // 2]      # exactly the cap: 2 x 4096 entries
    full["score"] = -np.arange(len(full), dtype=np.float32)
    lists = [[full], [full[::-1].copy()]]
    _check(_fuse(lists, "rrf", 100), lists, "rrf", 100)
    _check(_fuse(lists, "dbsf", 5000), lists, "dbsf", 5000)


def _sparse_rows(rng, n, n_dims, nnz):
    p = 1.0 / np.arange(1, n_dims + 1) ** 1.1
    p /= p.sum()
    rows = []
    for _ in range(n):
        k = int(rng.integers(1, nnz + 1))
        ix = rng.choice(n_dims, size=k, replace=False, p=p).astype(np.uint32)
        rows.append((ix, rng.lognormal(0.0, 1.0, k).astype(np.float32)))
    return rows


def test_lists_of_a_real_dense_and_sparse_search_async_on_a_user_stream():
    """50 k points with a dense and a sparse vector each: both searches and the fusion enqueued on one user stream with device buffers
    (qmx_search_topk_async x 2, qmx_fuse_topk_async), one synchronisation; against the restatement over the same lists read back."""
    import torch
    import oracle_ffi as O
    rng = np.random.default_rng(50)
    n, dim, nq, prefetch, top = 50000, 64, 8, 200, 10
    dense = qa.VectorStorage(O.preprocess(O.COSINE, O.synth(0x51, 0, n, dim)), qa.Distance.Cosine)
    sparse = qa.SparseVectorStorage(_sparse_rows(rng, n, 2000, 24))
    dq = qa.new_raw_scorer(O.synth(0x52, 0, nq, dim), dense)
    sq = qa.new_raw_scorer(_sparse_rows(rng, nq, 2000, 12), sparse)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    lib = F.lib()
    for kind, fkind in (("rrf", F.FUSION_RRF), ("dbsf", F.FUSION_DBSF)):
        with torch.cuda.stream(stream):
            lists = torch.zeros((2, nq, prefetch), dtype=torch.int64, device=dev)
            counts = torch.zeros((2, nq), dtype=torch.int32, device=dev)
            out = torch.zeros((nq, top), dtype=torch.int64, device=dev)
            oc = torch.zeros(nq, dtype=torch.int32, device=dev)
            params = F.FusionParams()
            params.kind, params.rrf_k, params.top = fkind, 2, top
            for i, s in enumerate((dq, sq)):
                F.check(lib.qmx_query_set_stream(s._h, C.c_void_p(stream.cuda_stream)))
                F.check(lib.qmx_search_topk_async(s._h, prefetch, None, 0, F.ptr(lists[i]), F.ptr(counts[i])))
            F.check(lib.qmx_fuse_topk_async(0, C.c_void_p(stream.cuda_stream), F.ptr(lists), F.ptr(counts), 2, nq, prefetch, C.byref(params),
                                            F.ptr(out), F.ptr(oc)))
        stream.synchronize()
        for s in (dq, sq):
            F.check(lib.qmx_query_set_stream(s._h, None))
        h_lists = lists.cpu().numpy().view(SPO).reshape(2, nq, prefetch)
        h_counts = counts.cpu().numpy()
        assert h_counts[0].tolist() == [prefetch] * nq and h_counts[1].min() > 0
        src = [[h_lists[s, qi, :h_counts[s, qi]] for qi in range(nq)] for s in range(2)]
        h_out, h_oc = out.cpu().numpy().view(SPO).reshape(nq, top), oc.cpu().numpy()
        _check([h_out[qi, :h_oc[qi]] for qi in range(nq)], src, kind, top)
        # the lists the two searches return on their own are the ones that were fused
        want_dense = qa.BatchFilteredSearcher(O.synth(0x52, 0, nq, dim), dense, prefetch).peek_top_all()
        for a, b in zip(src[0], want_dense):
            assert a["idx"].tolist() == b["idx"].tolist() and np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32))
