"""Option `prescan_beside_scan` (default 1): the exact scores of a prefilter's sample and the top-k behind them run as 256-thread blocks that fit on a CU
beside a block of the resident int8 scan - 16-query tiles on 4 waves (qdrant_amd/csrc/scan_mfma.hip, launch_scan_f32_mfma_beside) and
custom_topk_beside_kernel (qdrant_amd/csrc/custom_query.hip).  0 gives the former shapes: the 32-query tile on 8 waves, the 1024-thread top-k.  Neither
changes a bit of any score, list, count or bound; every case here runs both values and compares.

How the tests reach the two kernels:
* the score matrix through qmx_score_points: an id list of at most 16 384 rows takes the same route as a sample;
* the top-k through the custom queries' peek_top with option value 2 (every top-k of a short score row takes the 256-thread kernel), which lets a test
  choose the scores: equal ones, NaN, +inf.  That route asks for no bound word.  The bound is checked where it acts, in whole searches over the int8
  copy: the thresholds of both scan launches come from it, so the candidate, verified-row and fallback counters move when it moves.  The searches
  cover the top-k kernel's three ways to a bound - the ranked survivors (plain blocks, filters), more survivors than its list holds (a sample whose
  8 192 scores tie, a block of equal rows: the insertion walk) and no bound (a sample that is all deleted, one with fewer live rows than top)."""
import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

OPTION = "prescan_beside_scan"


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


def _with_option(qa, value, fn):
    qa.set_option(OPTION, value)
    try:
        return fn()
    finally:
        qa.set_option(OPTION, -1)


def _same_lists(a, b, what):
    assert len(a) == len(b)
    for qi, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y), (what, qi, len(x), len(y))                                   # the counts
        assert x["idx"].tolist() == y["idx"].tolist(), (what, qi)
        assert np.array_equal(x["score"].view(np.uint32), y["score"].view(np.uint32)), (what, qi)


# ---- the score matrix ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [128, 768, 1024])       # 4, 24 and 32 steps of 32 floats: 768 takes the guard-free main loop (steps % 12 == 0), the others the guarded one
def test_score_matrix_bits_do_not_depend_on_the_tile_shape(qa, dim):
    """Strided id lists of 8 192 rows (whole 8-row tiles, a multiple of 8 x 4), 8 191 (a ragged last tile), 8 200 (a row count that is no multiple of
    8 rows x 4 waves) and 33, against 1 .. 130 queries: a lone query, ragged and whole 16-query tiles, a second 32-query tile with two queries."""
    stride = 2
    n_rows = 8200 * stride
    rows = O.preprocess(O.COSINE, O.synth(0x5EED0F00 + dim, 0, n_rows, dim))
    vs = qa.VectorStorage(rows, qa.Distance.Cosine)
    all_queries = O.synth(0x5EED0F01 + dim, 0, 130, dim)
    checked_against_oracle = False
    for nq in (1, 15, 16, 17, 33, 128, 130):
        scorer = qa.new_raw_scorer(all_queries[:nq], vs)
        for n in (8192, 8191, 8200, 33):
            ids = (np.arange(n, dtype=np.uint32) * stride + (n & 1)).astype(np.uint32)
            new, new_kernel = _with_option(qa, 1, lambda: (scorer.score_points(ids), qa._ffi.last_kernel(scorer._h)))
            old, old_kernel = _with_option(qa, 0, lambda: (scorer.score_points(ids), qa._ffi.last_kernel(scorer._h)))
            if nq > 8:         # (9 .. 16 queries make a 16-query tile) the two values did run two kernels: 4 waves against 8
                assert "scan_f32_mfma_kernel<16, 1, 6, true, 4, " in new_kernel, new_kernel
                assert "scan_f32_mfma_kernel<16, " in old_kernel and ", 8, " in old_kernel, old_kernel
            else:
                assert new_kernel == old_kernel, (new_kernel, old_kernel)
            assert new.shape == (nq, n)
            assert np.array_equal(new.view(np.uint32), old.view(np.uint32)), (dim, nq, n)
            if nq == 17 and n == 33 and not checked_against_oracle:      # ... and they are the reference's bits
                want = O.DenseStorage(O.F32, O.COSINE, rows).score_points(all_queries[:nq], ids)
                assert np.array_equal(new.view(np.uint32), np.asarray(want, dtype=np.float32).view(np.uint32))
                checked_against_oracle = True
    assert checked_against_oracle


# ---- the top-k of a short score row ------------------------------------------------------------------------------------------------------------------

def _topk_case(n, case, rng):
    """rows (dot distance, 16 coordinates), deleted flags and whether numpy's ordering applies"""
    dim = 16
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    deleted = np.zeros(n, dtype=bool)
    plain = True
    if case == "duplicates":                            # equal scores across ids: a quarter of the rows are copies of eight rows
        src = rng.integers(0, min(n, 8), size=n)
        dup = rng.random(n) < 0.25
        rows[dup] = rows[src[dup]]
    elif case == "deleted_1pct":
        deleted = rng.random(n) < 0.01
        deleted[n // 2] = True
    elif case == "deleted_all":
        deleted[:] = True
    elif case == "non_finite":                          # one NaN and one +inf (or -inf, by the query's sign) score per query
        rows[n // 3, 0] = np.nan
        rows[(2 * n) // 3, 1] = np.inf
        plain = False
    elif case == "all_equal":                           # every score of a query the same bits: an n-fold tie, the lowest ids win
        rows[:] = rows[0]
    return rows, deleted, plain


@pytest.mark.parametrize("n", [8192, 8191, 8200, 33, 7])
def test_bound_topk_lists_do_not_depend_on_the_kernel(qa, n):
    """Every case with top 1, 10 and 64 (7 and 33 rows: fewer than top live rows - short lists, no bound), by the 256-thread kernel (option value 2) and
    by the 1024-thread one (0): the same lists and counts; the cases without NaN also against numpy's (score descending, lower id first) ordering."""
    rng = np.random.default_rng(1000 + n)
    ids = np.arange(n)
    for case in ("duplicates", "deleted_1pct", "deleted_all", "non_finite", "all_equal"):
        rows, deleted, plain = _topk_case(n, case, rng)
        vs = qa.VectorStorage(rows, qa.Distance.Dot)
        vs.set_deleted(deleted, None)
        queries = [qa.CustomQuery.recommend_sum_scores([rng.standard_normal(rows.shape[1]).astype(np.float32)], []) for _ in range(3)]
        scorer = qa.CustomRawScorer(queries, vs)
        sc = scorer.score_points(ids.astype(np.uint32))
        live = ~deleted
        for top in (1, 10, 64):
            new, new_kernel = _with_option(qa, 2, lambda: (scorer.peek_top(top), qa._ffi.last_kernel(scorer.examples._h)))
            old, old_kernel = _with_option(qa, 0, lambda: (scorer.peek_top(top), qa._ffi.last_kernel(scorer.examples._h)))
            assert "custom_topk_beside_kernel" in new_kernel and "custom_topk_small_kernel" in old_kernel, (new_kernel, old_kernel)
            _same_lists(new, old, (n, case, top))
            for qi in range(len(queries)):
                assert len(new[qi]) == min(top, int(live.sum())), (n, case, top, qi)
                if plain:
                    order = np.lexsort((ids[live], -sc[qi][live].astype(np.float64)))[:top]
                    assert new[qi]["idx"].tolist() == ids[live][order].tolist(), (n, case, top, qi)
                    assert np.array_equal(new[qi]["score"].view(np.uint32), sc[qi][live][order].view(np.uint32)), (n, case, top, qi)
        if case == "non_finite":                        # NaN is the greatest score (OrderedFloat), +inf next
            best = _with_option(qa, 2, lambda: scorer.peek_top(1))
            assert all(int(b["idx"][0]) == n // 3 and np.isnan(b["score"][0]) for b in best)
        # a candidate list with a payload filter on top (DeletedView::allowed)
        if case == "deleted_1pct":
            allowed = rng.random(n) < 0.5
            scorer.examples.set_filter(allowed)
            sub = rng.permutation(n)[: max(n // 2, 1)].astype(np.uint32)
            new = _with_option(qa, 2, lambda: scorer.peek_top(10, points=sub))
            old = _with_option(qa, 0, lambda: scorer.peek_top(10, points=sub))
            _same_lists(new, old, (n, case, "filtered"))
            assert all(allowed[r["idx"]].all() and not deleted[r["idx"]].any() for r in new)
            scorer.examples.set_filter(None)


# ---- the whole search over the int8 copy ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def block(qa):
    n, dim = 1 << 18, 768
    rows = O.preprocess(O.COSINE, O.synth(0x5EED0F10, 0, n, dim))
    queries = O.synth(0x5EED0F11, 0, 130, dim)
    return n, rows, queries


def _search(qa, value, queries, vs, top, filters=None, exact=False):
    def run():
        if exact:
            qa.set_option("no_split_scan", 1)
        try:
            s = qa.BatchFilteredSearcher(queries, vs, top)
            if filters is not None:
                s.scorer.set_filters(*filters)
            got = s.peek_top_all()
            return got, s.counters, qa._ffi.last_kernel(s.scorer._h)
        finally:
            if exact:
                qa.set_option("no_split_scan", -1)
    return _with_option(qa, value, run)


def _both_against_exact(qa, queries, vs, top, filters=None):
    want, _, kernel = _search(qa, 0, queries, vs, top, filters, exact=True)
    assert "scan_i8copy" not in kernel, kernel
    counters = []
    for value in (1, 0):
        got, c, kernel = _search(qa, value, queries, vs, top, filters)
        assert "scan_i8copy_kernel_res" in kernel, kernel
        _same_lists(got, want, ("search", value, len(queries)))
        cnt = (c.prefilter_queries, c.prefilter_candidates, c.verified_rows, c.fallback_queries)
        print("%s=%d, %d queries: prefilter_queries %d, prefilter_candidates %d, verified_rows %d, fallback_queries %d" % ((OPTION, value, len(queries)) + cnt))
        counters.append(cnt)
    assert counters[0] == counters[1], counters          # the sample's bound, hence every threshold behind it, did not move
    return counters[0]


@pytest.mark.parametrize("nq", [1, 16, 128, 130])
def test_search_over_the_int8_copy(qa, block, nq):
    n, rows, queries = block
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    cnt = _both_against_exact(qa, queries[:nq], vs, 10)
    assert cnt[0] == nq and cnt[3] == 0


def test_search_with_per_request_filters(qa, block):
    n, rows, queries = block
    nq = 130
    rng = np.random.default_rng(5)
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.05, np.arange(n) % 3 == 0])
    filter_of = [(qi % 4) if qi % 4 < 3 else None for qi in range(nq)]      # three bitmaps and "no filter", interleaved
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    _both_against_exact(qa, queries[:nq], vs, 10, filters=(masks, filter_of))


def test_search_with_a_sample_that_is_all_deleted(qa, block):
    """The sample of a 2^18-row block is every 32nd row; with all of them deleted the sample has no bound (count 0, bound word 0) for any query."""
    n, rows, queries = block
    deleted = np.arange(n) % 32 == 0
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    vs.set_deleted(deleted, None)
    want, _, _ = _search(qa, 0, queries[:128], vs, 10, exact=True)
    assert not any(deleted[w["idx"]].any() for w in want)
    _both_against_exact(qa, queries[:128], vs, 10)


def test_search_with_a_sample_whose_scores_all_tie(qa, block):
    """Every sample row (every 32nd) is a copy of one row: each query's 8 192 sample scores are the same bits, more survivors than the top-k kernel's list
    of 2 048 holds, so the bound comes from its insertion walk: the tied score with the 10th lowest sample id.  Rows between them are the block's own,
    so the bound decides how many of them each query admits."""
    n, rows, queries = block
    rows = rows.copy()
    rows[::32] = rows[5]
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    cnt = _both_against_exact(qa, queries[:128], vs, 10)
    assert cnt[1] > 0                                    # the bound admitted candidates: it was there


def test_search_over_a_block_of_equal_rows(qa):
    """2^18 copies of one row: the sample ties and so does everything else - every list is the ten lowest ids, by either value and by the exact scan."""
    n, dim = 1 << 18, 128
    rows = np.tile(O.preprocess(O.COSINE, O.synth(0x5EED0F20, 0, 1, dim)), (n, 1))
    queries = O.synth(0x5EED0F21, 0, 128, dim)
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    _both_against_exact(qa, queries, vs, 10)
    got, _, _ = _search(qa, 1, queries, vs, 10)
    assert all(g["idx"].tolist() == list(range(10)) for g in got)


def test_search_with_fewer_live_sample_rows_than_top(qa, block):
    """All sample rows deleted but five: the sample's list has five entries and no bound word, for every query."""
    n, rows, queries = block
    deleted = np.arange(n) % 32 == 0
    deleted[[0, 32 * 100, 32 * 4000, 32 * 8000, 32 * 8191]] = False
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    vs.set_deleted(deleted, None)
    _both_against_exact(qa, queries[:128], vs, 10)
