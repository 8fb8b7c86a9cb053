"""The exact tiled top-k scans (api_search.hip exact_tile - "the narrow scan" every prefilter route is checked against) on blocks that are larger than
one pass of their grid, with the prefix pre-scan on, and with the ids among tied scores asserted.

Row counts (tests/exact_scan_expectations.py derives them, tests/test_exact_scan_expectations.py checks the arithmetic).  Every scan kernel is
persistent: the grid is capped at num_cus * per_cu (or num_cus * 8) blocks and each wave loops `tile += tw`.  On 256 CUs

  N_MFMA   = 2^18 + 87          scan_sq_mfma_kernel: 16 rows per wave, 8 waves per block -> one grid pass covers 32 768 rows at one block per CU and at
                                most 2^18 at eight: every wave takes at least two tiles under any occupancy (the cross-tile double buffer, the
                                `ones` accumulator that restarts per tile), the pre-scan is on (n >= 2^18), n % 16 = 7 (a partial last tile)
  N_VALU   = 3 * 2^17 + 87      the generic scan_kernel, launch_scan_sq, launch_scan_tq: R = 4 groups of 8 rows per wave, four blocks per CU ->
                                262 144 rows per pass
  N_BQROWS = 2^19 + 2^17 + 87   bq_rows_kernel: 2 048 blocks of 256 rows -> 524 288 rows per pass
  N_L1     = 65 536 + 37, 2 * 65 536 + 5      tq_l1_scores_device works in batches of 65 536 rows

From 2^18 candidates on, pass 0 scores a prefix of max(n >> 10, 8192) & ~15 rows first and starts from its k-th best key: scan_sq_mfma_kernel keeps
the score half ("equal scores pass"), bq_rows_kernel the whole key.  The bound is sound while the score-mode and the top-k kernels give a pair the
same bits and while what ties with the bound survives.

Expectation: the rule of tests/parity_asserts.py over the oracle's scores - descending score, ascending offset, the lowest offsets fill a tied
boundary (exact_scan_expectations.expected_list) - ids and score bits, element for element.  Every block is built so that each checked query's boundary
IS a tie group that does not fit, and carries the query's best row at offsets 0, pre_n - 1, pre_n, 32 768, n - 16 and n - 1: a lost tile, a lost last
partial tile or an off-by-one at the prefix edge changes the head of the list.  At most 4 queries of a batch are checked against the oracle; the batch
repeats them, and every other list must equal the device's own list of the query it repeats.
f16 on the matrix cores sums in another order than the oracle: there (a) the lists must be that rule over the device's OWN score_points of every row,
bit for bit - what makes the pre-scan's bound sound -, and (b) those scores are within the bar of tests/test_gpu_dense_f16_u8.py (1e-5 of the sum of
absolute terms) of the oracle's.

Repeated ids in a candidate list (legal input): the device returns an id once per occurrence, as far as the entries fit - the top-k of the MULTISET of
(score, id) entries, which is also what the oracle's queue holds after pushing every occurrence (FixedLengthPriorityQueue has no notion of identity)."""
import numpy as np
import pytest

import exact_scan_expectations as X
import oracle_ffi as O

pytestmark = pytest.mark.gpu
REL = 1e-5          # the f16 bar of tests/test_gpu_dense_f16_u8.py


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


def _dist(qa, d):
    return {O.COSINE: qa.Distance.Cosine, O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid, O.MANHATTAN: qa.Distance.Manhattan}[d]


_DEVICE = {}


def _storage(qa, w):
    """the world's rows on the device (one storage at a time is kept)"""
    if _DEVICE.get("world") is w:
        return _DEVICE["st"]
    _DEVICE.clear()
    spec, dist = w.spec, _dist(qa, w.spec.dist)
    if spec.kind == "bq":
        quant = qa.BinaryQuantizer(spec.dim, dist, query_encoding={1: 0, 4: 1, 8: 2}[spec.bits])
        st = qa.EncodedVectorsBin(w.rows, quant)
    elif spec.kind == "tq":
        plus = w.base.tq_plus
        quant = qa.TurboQuantizer(spec.dim, dist, spec.bits, shift=None if plus is None else plus[0], scale=None if plus is None else plus[1])
        assert quant.quantized_vector_size() == w.rows.shape[1] == w.oracle.row_bytes
        st = qa.EncodedVectorsTQ(w.rows, quant)
    elif spec.kind == "sq":
        quant = qa.ScalarQuantizer(spec.dim, dist, *w.base.sq_params)
        assert np.float32(w.oracle.sq.multiplier) == quant.multiplier and quant.quantized_vector_size() == w.rows.shape[1]
        st = qa.EncodedVectorsU8(w.rows, quant)
    elif spec.kind == "u8":
        st = qa.VectorStorage(w.rows, dist, qa.VectorStorageDatatype.Uint8)
    else:
        st = qa.VectorStorage(w.rows.view(np.float16), dist, qa.VectorStorageDatatype.Float16)
    _DEVICE.update(world=w, st=st)
    return st


def _search(qa, w, nq, top, cand=None, live=None, options=()):
    """the batch = the checked queries repeated; returns (lists, kernel, searcher)"""
    st = _storage(qa, w)
    k = min(nq, X.N_CHECKED)
    queries = np.ascontiguousarray(w.queries[np.arange(nq) % k])
    if live is not None:
        st.set_deleted(~live)
    for name, value in options:
        qa.set_option(name, value)
    try:
        s = qa.BatchFilteredSearcher(queries, st, top)
        got = s.peek_top_all() if cand is None else s.peek_top_iter(np.ascontiguousarray(cand, dtype=np.uint32))
        kernel = qa._ffi.last_kernel(s.scorer._h)
    finally:
        for name, _ in options:
            qa.set_option(name, -1)
        if live is not None:
            st.set_deleted(None)
    return got, kernel, s


def _f16_scale(w, k):
    """sum of absolute terms per (checked query, block row), gathered from the base like the scores"""
    q = O.f16_to_f32(w.oracle.encode_queries(w.queries[:k])).astype(np.float64)
    v = O.f16_to_f32(w.base.rows).astype(np.float64)
    if w.spec.dist == O.EUCLID:
        base = ((q[:, None, :] - v[None, :, :]) ** 2).sum(-1)
    else:
        base = np.abs(q[:, None, :] * v[None, :, :]).sum(-1)
    return base[:, w.draw]


def _scores(w, s, k):
    """what the lists are held to: the oracle's scores - for f16 the device's own score_points of every row by the batch that searched (a), which
    must be within the f16 bar of the oracle's (b)"""
    if w.spec.kind != "f16":
        return w.scores
    dev = s.scorer.score_points(np.arange(w.n, dtype=np.uint32))
    for i in range(k, dev.shape[0]):                                     # the repeated queries score like the ones they repeat
        assert np.array_equal(dev[i].view(np.uint32), dev[i % k].view(np.uint32)), i
    err = np.abs(dev[:k].astype(np.float64) - w.scores[:k])
    assert np.all(err <= REL * _f16_scale(w, k) + 1e-30), float((err / _f16_scale(w, k)).max())
    return dev[:k]


def _check(w, got, scores, nq, top, cand=None, live=None):
    k = min(nq, X.N_CHECKED)
    assert len(got) == nq
    for c in range(k):
        ids, sc = X.expected_list(scores[c], top, cand, live)
        g = got[c]
        assert g["idx"].tolist() == ids.tolist(), (c, g["idx"].tolist(), ids.tolist(), g["score"].tolist(), sc.tolist())
        assert np.array_equal(g["score"].view(np.uint32), sc.view(np.uint32)), (c, g["score"].tolist(), sc.tolist())
    for i in range(k, nq):
        assert got[i]["idx"].tolist() == got[i % k]["idx"].tolist(), (i, got[i]["idx"].tolist(), got[i % k]["idx"].tolist())
        assert np.array_equal(got[i]["score"].view(np.uint32), got[i % k]["score"].view(np.uint32)), i


def _sorted(cases):
    return sorted(cases, key=lambda c: (repr(c.spec), c.n, c.nq, c.top))


@pytest.mark.parametrize("case", _sorted(X.CASES), ids=repr)
def test_exact_scan_of_a_block_larger_than_a_grid_pass(qa, case):
    w = X.world_of(case.spec, case.n)
    k = min(case.nq, X.N_CHECKED)
    X.check_preconditions(w.scores[:k], case.top, w.planted[:k])
    got, kernel, s = _search(qa, w, case.nq, case.top, options=case.options)
    assert case.kernel in kernel, kernel
    _check(w, got, _scores(w, s, k), case.nq, case.top)


@pytest.mark.parametrize("edge", X.EDGES)
@pytest.mark.parametrize("case", X.EDGE_CASES, ids=repr)
def test_prescan_edges(qa, case, edge):
    """exact_scan_expectations.edge_setup says what each edge is; the same search without the pre-scan (option no_prescan) returns identical lists"""
    w, live, cand = X.edge_setup(case, edge)
    k = min(case.nq, X.N_CHECKED)
    X.check_preconditions(w.scores[:k], X.TOP, w.planted[:k], cand=cand, live=live)
    got, kernel, s = _search(qa, w, case.nq, X.TOP, cand=cand, live=live)
    assert case.kernel in kernel, kernel
    plain, kernel2, _ = _search(qa, w, case.nq, X.TOP, cand=cand, live=live, options=(("no_prescan", 1),))
    assert case.kernel in kernel2, kernel2
    scores = _scores(w, s, k)
    _check(w, plain, scores, case.nq, X.TOP, cand=cand, live=live)
    _check(w, got, scores, case.nq, X.TOP, cand=cand, live=live)
    for a, b in zip(got, plain):
        assert a["idx"].tolist() == b["idx"].tolist() and np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32))


@pytest.mark.parametrize("case", X.ID_LIST_CASES, ids=repr)
def test_id_lists_with_repeated_ids(qa, case):
    """peek_top_iter over n ids drawn with repeats, shuffled.  The device returns an id once per occurrence (the module's docstring): the first and the
    last planted row of a query occur twice in the list and twice at the head of the result.  The oracle's queue does the same with the ids it is pushed."""
    w, cand = X.id_list_of(case)
    k = min(case.nq, X.N_CHECKED)
    X.check_preconditions(w.scores[:k], X.TOP, w.planted[:k], cand=cand)
    got, kernel, s = _search(qa, w, case.nq, X.TOP, cand=cand)
    assert case.kernel in kernel, kernel
    _check(w, got, _scores(w, s, k), case.nq, X.TOP, cand=cand)
    for c in range(k):
        ids = got[c]["idx"].tolist()
        assert ids.count(w.planted[c][0]) == 2 and ids.count(w.planted[c][-1]) == 2 and len(set(ids)) < len(ids)
    if case.spec.kind == "u8":              # the oracle's own bounded queue over the same list (qo_peek_top_iter): the same scores, every repeated id as often
        want = O.DenseStorage(O.U8, case.spec.dist, w.rows).peek_top(w.queries[:k], X.TOP, ids=cand)
        for g, o in zip(got[:k], want):
            assert np.array_equal(g["score"].view(np.uint32), o["score"].view(np.uint32))
            above = o["score"] > o["score"][-1]
            assert sorted(g["idx"][above].tolist()) == sorted(o["idx"][above].tolist())


@pytest.mark.parametrize("n", X.N_L1)
def test_tq_l1_batches_of_65536_rows(qa, n):
    """TurboQuant over Manhattan (4 bits, dim 64): tq_l1_scores_device dequantises, rotates back and sums |q - v| in batches of 65 536 rows.  The
    scores of every row of a block of one batch + 37 rows / two batches + 5 rows are the oracle's bits; the top-10 with 20 % of the rows deleted
    finds the best rows at the batch edges (65 535, 65 536, 131 071, 131 072) and at n - 1.  (This route selects with the custom top-k kernel over the
    score matrix and reports no scan kernel.)"""
    w, live = X.l1_setup(n)
    nq = X.L1_QUERIES
    X.check_preconditions(w.scores[:nq], X.TOP, w.planted[:nq], live=live)
    st = _storage(qa, w)
    scorer = qa.new_raw_scorer(np.ascontiguousarray(w.queries[:nq]), st)
    got = scorer.score_points(np.arange(n, dtype=np.uint32))
    bad = np.flatnonzero((got.view(np.uint32) != np.ascontiguousarray(w.scores[:nq]).view(np.uint32)).any(axis=0))
    assert len(bad) == 0, (len(bad), bad[:8].tolist())
    res, _, _ = _search(qa, w, nq, X.TOP, live=live)
    _check(w, res, w.scores, nq, X.TOP, live=live)
    for c in range(nq):
        assert set(w.planted[c]) <= set(res[c]["idx"].tolist())
