"""Host or device memory, in and out: the one-shot entry points stage host arguments through device buffers they own (csrc/dev_mem.hpp, Staging) and
use device arguments where they lie.  For every entry point below the four placements {host, device} input x {host, device} output must give the
same bytes, and the host-to-host bytes must be what the entry point's oracle comparison expects.  37 rows of 40 floats: 40 is no multiple of 16
(an SQ row pads to actual_dim 48), 37 no multiple of anything a kernel unrolls by.  The last test runs ten create / use / destroy rounds of every
handle kind on a fresh thread (qmx_last_error is per thread) and expects no error text behind them."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_ffi as O
import fusion_reference as FR

pytestmark = pytest.mark.gpu

N, DIM = 37, 40
PLACEMENTS = [(False, False), (True, False), (False, True), (True, True)]      # (inputs on the device, outputs on the device)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(3740)
    return (rng.standard_normal((N, DIM)) * 1.5 + rng.standard_normal(DIM) * 0.25).astype(np.float32)


def _on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _placed(call, inputs, out_bytes, placements=PLACEMENTS):
    """call(ins, outs) under every placement; the outputs' bytes must not depend on it.  Returns the host-to-host outputs as uint8 arrays."""
    import torch
    from qdrant_amd import _ffi as F
    got = {}
    for in_dev, out_dev in placements:
        ins = [None if a is None else _on_device(a) if in_dev else np.ascontiguousarray(a) for a in inputs]
        outs = [torch.full((nb,), SENTINEL, dtype=torch.uint8, device="cuda") if out_dev else np.full(nb, SENTINEL, dtype=np.uint8) for nb in out_bytes]
        F.check(call(ins, outs))
        got[(in_dev, out_dev)] = [o.cpu().numpy().copy() if out_dev else o for o in outs]
    base = got[placements[0]]
    for place, outs in got.items():
        for k, (o, b) in enumerate(zip(outs, base)):
            assert np.array_equal(o, b), "output %d differs with inputs on %s, outputs on %s" % (
                k, "device" if place[0] else "host", "device" if place[1] else "host")
    return base


def test_preprocess_cosine(qa, rows):
    from qdrant_amd import _ffi as F
    out, = _placed(lambda i, o: F.lib().qmx_preprocess_f32(0, int(qa.Distance.Cosine), F.ptr(i[0]), N, DIM, F.ptr(o[0])), [rows], [N * DIM * 4])
    assert np.array_equal(out.view(np.uint32), O.preprocess(O.COSINE, rows).reshape(-1).view(np.uint32))


@pytest.mark.parametrize("name", ["f16", "u8"])
def test_cast(qa, rows, name):
    from qdrant_amd import _ffi as F
    dtype, width, oracle = {"f16": (F.DTYPE_F16, 2, O.to_f16), "u8": (F.DTYPE_U8, 1, O.to_u8)}[name]
    x = rows if name == "f16" else (rows * 90.0 + 100.0).astype(np.float32)      # u8: values below 0, above 255 and with fractions
    if name == "u8":
        assert x.min() < 0 and x.max() > 255
    out, = _placed(lambda i, o: F.lib().qmx_cast_f32(0, dtype, F.ptr(i[0]), N * DIM, F.ptr(o[0])), [x], [N * DIM * width])
    assert np.array_equal(out, oracle(x).reshape(-1).view(np.uint8))


def test_sq_encode(qa, rows):
    import torch
    from qdrant_amd import _ffi as F
    quant = qa.ScalarQuantizer.from_min_max(rows, DIM, qa.Distance.Dot)
    assert quant.actual_dim == 48
    p = quant.params()
    out, = _placed(lambda i, o: F.lib().qmx_sq_encode(0, int(qa.Distance.Dot), C.byref(p), F.ptr(i[0]), N, DIM, F.ptr(o[0])), [rows], [N * 52])
    want = O.SqOracle(O.DOT, DIM, quant.alpha, quant.offset).encode_rows(rows)
    assert np.array_equal(out.reshape(N, 52), want)
    # the fit on the device reads the same rows from either memory
    for f in [qa.ScalarQuantizer.fit(r, DIM, qa.Distance.Dot) for r in (rows, _on_device(rows).view(torch.float32).reshape(N, DIM))]:
        assert (np.float32(f.alpha), np.float32(f.offset)) == (np.float32(quant.alpha), np.float32(quant.offset))


@pytest.mark.parametrize("stats_on_device", [False, True])
def test_bq_encode_two_bits(qa, rows, stats_on_device):
    from qdrant_amd import _ffi as F
    mean, stddev = O.vector_stats(rows)[2:]
    keep = [_on_device(mean), _on_device(stddev)] if stats_on_device else [mean, stddev]
    p = F.BqParams()
    p.encoding, p.query_encoding = F.BQ_TWO_BITS, F.BQ_QUERY_SAME_AS_STORAGE
    p.mean, p.stddev = F.ptr(keep[0]).value, F.ptr(keep[1]).value
    row_bytes = int(F.lib().qmx_bq_row_bytes(DIM, F.BQ_TWO_BITS))
    out, = _placed(lambda i, o: F.lib().qmx_bq_encode_ex(0, C.byref(p), F.ptr(i[0]), N, DIM, F.ptr(o[0])), [rows], [N * row_bytes])
    want = O.BqOracle(O.DOT, DIM, encoding=F.BQ_TWO_BITS, mean=mean, stddev=stddev).encode_rows(rows)
    assert np.array_equal(out.reshape(N, row_bytes), want)


def _pq(qa, rows):
    chunk, ncent = 8, 16
    cen = O.PqOracle.train(rows, DIM, chunk, ncent, iters=3)
    return chunk, ncent, np.ascontiguousarray(cen, dtype=np.float32), O.PqOracle(O.DOT, DIM, chunk, cen)


@pytest.mark.parametrize("centroids_on_device", [False, True])
def test_pq_encode(qa, rows, centroids_on_device):
    from qdrant_amd import _ffi as F
    chunk, ncent, cen, opq = _pq(qa, rows)
    keep = _on_device(cen) if centroids_on_device else cen
    p = F.PqParams()
    p.chunk_size, p.n_centroids, p.centroids = chunk, ncent, F.ptr(keep).value
    out, = _placed(lambda i, o: F.lib().qmx_pq_encode(0, C.byref(p), F.ptr(i[0]), N, DIM, F.ptr(o[0])), [rows], [N * opq.m])
    assert np.array_equal(out.reshape(N, opq.m), opq.encode(rows))


def test_score_internal_on_a_pq_segment(qa, rows):
    from qdrant_amd import _ffi as F
    chunk, ncent, cen, opq = _pq(qa, rows)
    codes = opq.encode(rows)
    st = qa.EncodedVectorsPQ(codes, qa.ProductQuantizer(DIM, qa.Distance.Dot, chunk, cen))
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, N, 64).astype(np.uint32), rng.integers(0, N, 64).astype(np.uint32)
    out, = _placed(lambda i, o: F.lib().qmx_score_internal(st._h, F.ptr(i[0]), F.ptr(i[1]), 64, F.ptr(o[0])), [a, b], [64 * 4])
    assert np.array_equal(out.view(np.uint32), opq.score_internal(a, b).view(np.uint32))
    st.close()


def test_vector_stats(qa, rows):
    from qdrant_amd import _ffi as F
    outs = _placed(lambda i, o: F.lib().qmx_vector_stats(0, F.ptr(i[0]), N, DIM, *[F.ptr(x) for x in o]), [rows], [DIM * 4] * 4)
    for got, want in zip(outs, O.vector_stats(rows)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _search_lists(rng, n_lists, nq, k, pool):
    lists = np.zeros((n_lists, nq, k), dtype=O.ScoredPointOffset)
    for l in range(n_lists):
        for q in range(nq):
            lists[l, q]["score"] = np.sort(rng.standard_normal(k).astype(np.float32))[::-1]
            lists[l, q]["idx"] = rng.permutation(pool)[:k]
    counts = rng.integers(0, k + 1, size=(n_lists, nq)).astype(np.uint32)
    counts[0, 0], counts[-1, -1] = 0, k      # an empty and a full list
    return lists, counts


def _counted(out, oc, nq, top):
    """The lists behind (out, counts): entries past a list's count are not part of the result."""
    oc = oc.view(np.uint32)
    pts = out.view(O.ScoredPointOffset).reshape(nq, top)
    return [pts[q, :oc[q]] for q in range(nq)]


def test_merge_topk(qa):
    from qdrant_amd import _ffi as F
    n_lists, nq, k = 3, 5, 7
    lists, counts = _search_lists(np.random.default_rng(71), n_lists, nq, k, 1000)
    got = {}
    for place in PLACEMENTS:      # (entries past a list's count are unspecified: compare list by list, placement by placement)
        out, oc = _placed(lambda i, o: F.lib().qmx_merge_topk(0, F.ptr(i[0]), F.ptr(i[1]), n_lists, nq, k, F.ptr(o[0]), F.ptr(o[1])), [lists, counts],
                          [nq * k * 8, nq * 4], placements=[place])
        got[place] = _counted(out, oc, nq, k)
    want = O.merge_topk(lists, counts, k)
    for place, res in got.items():
        for q in range(nq):
            assert res[q].tobytes() == want[q].tobytes(), (place, q)


def test_fuse_topk(qa):
    from qdrant_amd import _ffi as F
    n_sources, nq, stride, top = 3, 5, 9, 12
    lists, counts = _search_lists(np.random.default_rng(72), n_sources, nq, stride, 30)      # 30 ids for 27 entries: heavy overlap
    p = F.FusionParams()
    p.kind, p.rrf_k, p.top, p.weights, p.n_weights = F.FUSION_RRF, 2, top, None, 0
    got = {}
    for place in PLACEMENTS:
        out, oc = _placed(lambda i, o: F.lib().qmx_fuse_topk(0, F.ptr(i[0]), F.ptr(i[1]), n_sources, nq, stride, C.byref(p), F.ptr(o[0]), F.ptr(o[1])),
                          [lists, counts], [nq * top * 8, nq * 4], placements=[place])
        got[place] = _counted(out, oc, nq, top)
    for q in range(nq):
        want = FR.rrf_scoring([lists[s, q, :counts[s, q]] for s in range(n_sources)], 2, None, top)
        for place, res in got.items():
            assert res[q]["idx"].tolist() == want["idx"].tolist(), (place, q)
            assert np.array_equal(res[q]["score"].view(np.uint32), want["score"].view(np.uint32)), (place, q)


def test_ten_rounds_of_every_handle_leave_no_error(qa, rows):
    from qdrant_amd import _ffi as F
    chunk, ncent, cen, opq = _pq(qa, rows)
    codes = opq.encode(rows)
    queries = rows[:3] + np.float32(0.125)
    sparse = [(np.array([1, 5, 9 + i % 3], dtype=np.uint32), np.array([0.5, 1.5, 2.0], dtype=np.float32)) for i in range(N)]
    result = {}

    def rounds():
        try:
            for _ in range(10):
                st = qa.VectorStorage(rows, qa.Distance.Dot)                       # segment + query batch
                s = qa.BatchFilteredSearcher(queries, st, 5)
                assert all(len(l) == 5 for l in s.peek_top_all())
                graph = qa.GraphLayers.build(st, m=4, ef_construct=16)             # graph
                walk = qa.new_raw_scorer(queries, st)
                assert len(graph.search(5, 16, walk)) == 3
                keys = qa.GroupKeys(N, np.arange(N, dtype=np.uint32) % 4)          # group keys
                assert len(qa.search_groups(st, queries, keys, 2, 2)) == 3
                cols = qa.PayloadColumns(N, numbers={"x": np.arange(N, dtype=np.float64)})      # payload columns + formula
                f = qa.CompiledFormula(qa.sum_(qa.payload("x"), qa.const(1.0)), cols)
                precise, _, status = qa.formula_eval(f, cols, np.arange(N, dtype=np.uint32))
                assert not status.any() and precise[N - 1] == N
                pq = qa.EncodedVectorsPQ(codes, qa.ProductQuantizer(DIM, qa.Distance.Dot, chunk, cen))      # quantized segment
                sp = qa.SparseVectorStorage(sparse)                                 # sparse segment + sparse query batch
                sq = qa.new_raw_scorer([sparse[0]], sp)
                assert sq.score_points(np.arange(N, dtype=np.uint32)).shape == (1, N)
                for h in (sq, sp, pq, f, cols, keys, walk, graph, s.scorer, st):
                    h.close()
            result["error"] = F.last_error()
        except BaseException as e:      # noqa: BLE001 - reported by the asserting thread
            result["raised"] = e

    t = threading.Thread(target=rounds)
    t.start()
    t.join()
    assert "raised" not in result, repr(result.get("raised"))
    assert result["error"] == ""
