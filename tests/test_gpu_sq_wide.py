"""The 128-query pass over scalar-int8 blocks (qdrant_amd/csrc/scan_sqw.hip): brute-force top-k of 33 and more queries over a block of 2^18 rows and more
streams the codes once per 128 queries - a wave's lanes fetch exactly their matrix-core operand pieces, the integer dots are exact, the f32 expression of
postprocess_score (encoded_vectors_u8.rs:100-103) finishes them - so the lists must be the 32-query scan's and the oracle's (ids, score bits, tie order).
A query whose candidate lists overflow (masses of equal scores) takes the 32-query scan alone (qmx_counters.fallback_queries).
Further down: results planted in the block's last n % 4 rows, behind rows whose column entries would reject them (the pass's integer test reads a row's
entry from a 16-byte piece that straddles the end of the block there), and un-centred blocks, whose entries leave what the integer test can hold."""
import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

N = 262_144 + 1_111      # >= 2^18 rows: the wide pass applies; not a multiple of the 256-row tile


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


def _dist(qa, d):
    return {O.COSINE: qa.Distance.Cosine, O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid, O.MANHATTAN: qa.Distance.Manhattan}[d]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["idx"].tolist() == w["idx"].tolist()
        assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32))


def _kernel(qa, searcher):
    return qa._ffi.last_kernel(searcher.scorer._h)


def _narrow(qa, queries, st, top):
    qa.set_option("sq_wide_min_queries", 0)
    try:
        s = qa.BatchFilteredSearcher(queries, st, top)
        res = s.peek_top_all()
        assert "scan_sqw_kernel" not in _kernel(qa, s)
        return res
    finally:
        qa.set_option("sq_wide_min_queries", -1)


_CACHE = {}


def _segment(qa, dist, dim, n, seed, ties=0, vecs=None):
    """vecs: prepared rows, taken as the block's (already preprocessed) rows and not cached - the cases that plant rows each bring their own block"""
    key = (dist, dim, n, seed, ties)
    if vecs is None and key in _CACHE:
        return _CACHE[key]
    _CACHE.clear()
    if vecs is None:
        rng = np.random.default_rng(seed)
        if ties:
            base = rng.standard_normal((ties, dim)).astype(np.float32)
            vecs = base[rng.integers(0, ties, n)]
        else:
            centres = rng.standard_normal((64, dim)).astype(np.float32)
            vecs = (centres[rng.integers(0, 64, n)] * rng.uniform(0.5, 2.0, (n, 1)) + 0.5 * rng.standard_normal((n, dim))).astype(np.float32)
        vecs = O.preprocess(dist, vecs)
        prepared = False
    else:
        assert vecs.shape == (n, dim) and vecs.dtype == np.float32
        prepared = True
    quant = qa.ScalarQuantizer.from_min_max(vecs[:20000], dim, _dist(qa, dist))
    osq = O.SqOracle(dist, dim, quant.alpha, quant.offset)
    rows = quant.encode(vecs)                                 # (byte-exact against the oracle's encoder: tests/test_gpu_sq.py)
    assert np.array_equal(rows[:64], osq.encode_rows(vecs[:64]))
    st = qa.EncodedVectorsU8(rows, quant)
    if prepared:
        return vecs, osq, rows, st
    _CACHE[key] = (vecs, osq, rows, st)
    return _CACHE[key]


def _oracle_scores(osq, rows, qpre, n):
    osq.rows = rows
    return osq.score_points(qpre, np.arange(n, dtype=np.uint32))


def _oracle_top(osq, rows, qpre, n, top, dead=None, sc=None):
    """sc: the oracle's scores of every row (_oracle_scores), where the caller has them already"""
    if sc is None:
        sc = _oracle_scores(osq, rows, qpre, n)
    out = []
    for i in range(len(qpre)):
        s = sc[i].copy()
        if dead is not None:
            s[dead] = -np.inf
        order = np.lexsort((np.arange(n), -s.astype(np.float64)))[:top]      # descending score, ties -> lower id
        out.append((order, s[order]))
    return out


@pytest.mark.parametrize("nq,top", [(33, 10), (128, 10), (150, 1), (300, 64)])
@pytest.mark.parametrize("dist,dim", [(O.DOT, 128), (O.COSINE, 768), (O.EUCLID, 768), (O.DOT, 1024)])
def test_sq_wide_pass_returns_the_narrow_scan_and_the_oracle(qa, dist, dim, nq, top):
    n = N
    vecs, osq, rows, st = _segment(qa, dist, dim, n, seed=dim * 3 + dist)
    rng = np.random.default_rng(nq * 7 + top)
    queries = (vecs[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, dim))).astype(np.float32)
    queries[nq // 2] = 0.0
    s = qa.BatchFilteredSearcher(queries, st, top)
    got = s.peek_top_all()
    assert "scan_sqw_kernel" in _kernel(qa, s), _kernel(qa, s)
    c = s.counters
    assert c.prefilter_queries == nq and c.prefilter_candidates >= c.verified_rows >= top * (nq - c.fallback_queries)
    _same(got, _narrow(qa, queries, st, top))
    k = 2
    want = _oracle_top(osq, rows, O.preprocess(dist, queries[:k]), n, top)
    for g, (ids, sc) in zip(got[:k], want):
        assert g["idx"].tolist() == ids.tolist()
        assert np.array_equal(g["score"].view(np.uint32), sc.view(np.uint32))


@pytest.mark.parametrize("dist", [O.DOT, O.EUCLID])
def test_sq_wide_pass_with_deleted_rows(qa, dist):
    n, dim, nq, top = N, 128, 140, 10
    vecs, osq, rows, st = _segment(qa, dist, dim, n, seed=dim * 3 + dist)
    rng = np.random.default_rng(5)
    queries = (vecs[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, dim))).astype(np.float32)
    deleted = rng.random(n) < 0.3
    deleted[n - 300:] = True                                   # the last tile: all deleted
    st.set_deleted(deleted)
    try:
        s = qa.BatchFilteredSearcher(queries, st, top)
        got = s.peek_top_all()
        assert "scan_sqw_kernel" in _kernel(qa, s)
        _same(got, _narrow(qa, queries, st, top))
        want = _oracle_top(osq, rows, O.preprocess(dist, queries[:2]), n, top, dead=deleted)
        for g, (ids, sc) in zip(got[:2], want):
            assert g["idx"].tolist() == ids.tolist() and not deleted[g["idx"]].any()
            assert np.array_equal(g["score"].view(np.uint32), sc.view(np.uint32))
    finally:
        st.set_deleted(np.zeros(n, dtype=bool))


def test_sq_wide_pass_masses_of_equal_scores_take_the_narrow_scan(qa):
    """one row repeated 263 k times: every score of a query is the same number, every candidate list overflows, every query takes the conditional
    32-query scan; the lists are the linear scan's (the lowest ids)"""
    n, dim, nq, top = N, 128, 70, 10
    vecs, osq, rows, st = _segment(qa, O.DOT, dim, n, seed=11, ties=1)
    rng = np.random.default_rng(6)
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    s = qa.BatchFilteredSearcher(queries, st, top)
    got = s.peek_top_all()
    assert "scan_sqw_kernel" in _kernel(qa, s)
    assert s.counters.fallback_queries == nq
    _same(got, _narrow(qa, queries, st, top))
    for g in got[:3]:
        assert g["idx"].tolist() == list(range(top))


def test_sq_wide_pass_few_distinct_rows_and_manhattan_keeps_the_narrow_kernel(qa):
    n, dim, nq, top = N, 128, 40, 10
    vecs, osq, rows, st = _segment(qa, O.DOT, dim, n, seed=12, ties=5)
    rng = np.random.default_rng(7)
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    s = qa.BatchFilteredSearcher(queries, st, top)
    got = s.peek_top_all()
    assert "scan_sqw_kernel" in _kernel(qa, s)
    _same(got, _narrow(qa, queries, st, top))
    # Manhattan (sad, not a dot) and rows that are not a multiple of 128 codes: the 32-query / VALU kernels serve
    for dist, d2 in ((O.MANHATTAN, 128), (O.DOT, 96)):
        vecs, osq, rows, st = _segment(qa, dist, d2, n, seed=13)
        q2 = rng.standard_normal((nq, d2)).astype(np.float32)
        s = qa.BatchFilteredSearcher(q2, st, top)
        s.peek_top_all()
        assert "scan_sqw_kernel" not in _kernel(qa, s)


# ---- the block's last rows.  A lane of the pass loads the column entries B[row] of its four rows as one 16-byte piece; in the block's last, partial tile the
# quad that holds the last row runs past the end when n % 4 != 0.  Whatever the load does there, entry j has to be row (quad + j)'s: a load shifted back to
# end inside the column hands the last n % 4 rows the entries of the rows 4 - n % 4 places in front of them, and where such an entry is smaller than the
# row's own by more than the row's lead over the threshold the pass drops a member of the top k.  So: a query for each of the last n % 4 rows (a near-copy of
# it), and in front of each of them, 4 - n % 4 places earlier, a row whose entry is FAR smaller: a loud row (every coordinate at the block's maximum: all
# codes 127 - the smallest vector_offset a row can have when the offset is negative or the distance inverted).  With n % 4 = 3 the rows in front of the last
# two are themselves planted, so the three descend in steps (fractions of the block's maximum, small noise; None: an ordinary row) wide enough that each
# one's entry is as far below the next one's as the condition wants - found on the host with the oracle, per distance, and asserted below for every case. ----
TAIL_R = [5, 6, 7, 87, 255, 1, 2, 3]      # n % 256; below 4 the last quad is the tile's first: nothing to shift, the load just runs past the end
TAIL_LEVELS = {O.DOT: (0.35, 0.20, None), O.COSINE: (0.50, 0.25, None), O.EUCLID: (0.60, 0.45, 0.10)}


def _tail_block(dist, r, dim=64):
    """-> rows (as stored), the planted rows, the loud rows, the distance between a planted row and the row whose entry a shifted load would give it, queries
    (the first len(planted) of them near-copies of the planted rows)"""
    n = (1 << 18) + r
    k = n % 4
    assert k != 0
    shift = 4 - k
    rng = np.random.default_rng(1000 * dist + r)
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    if dist == O.COSINE:
        vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
    hi, sd = vecs.max(), vecs.std()
    planted = list(range(n - k, n))
    loud = [w - shift for w in planted if w - shift not in planted]
    if k == 3:
        for w, level in zip(planted, TAIL_LEVELS[dist]):
            if level is not None:
                vecs[w] = level * hi + 0.1 * sd * rng.standard_normal(dim)
    vecs[loud] = hi
    nq = 33 + r % 8
    queries = (vecs[rng.integers(0, 1 << 18, nq)] + 0.3 * sd * rng.standard_normal((nq, dim))).astype(np.float32)
    queries[:k] = vecs[planted] + 0.05 * sd * rng.standard_normal((k, dim))
    return vecs, planted, loud, shift, queries


def _tail_precondition(osq, vecs, rows, planted, loud, shift, sc, want):
    """The input discriminates - from the oracle's encoder and scores alone: the entry a shifted load would test row w with, B[w - shift], is below the
    row's own by more than the row's score leads the LOWEST score of any row for its query (in code units: / multiplier) - a bound of the lead over any
    threshold a sample can give.  With such an entry the pass's integer test rejects w, a member of the oracle's list."""
    mult = float(osq.sq.multiplier)
    lo = min(loud + planted)
    enc = osq.encode_rows(vecs[lo:])
    assert np.array_equal(enc, rows[lo:])
    assert all((enc[x - lo, 4:4 + vecs.shape[1]] == 127).all() for x in loud)
    b = np.ceil(enc[:, :4].copy().view(np.float32)[:, 0].astype(np.float64) / mult) + 1.0
    for i, w in enumerate(planted):
        gap = b[w - lo] - b[w - shift - lo]
        lead = (float(sc[i, w]) - float(sc[i].min())) / mult
        print("row n - %d: B[w] - B[w - %d] = %.4g, lead = %.4g" % (len(vecs) - w, shift, gap, lead))
        assert gap > lead
        assert w in want[i][0].tolist()


def _tail_case(qa, dist, r, with_deleted):
    top = 10
    block, planted, loud, shift, queries = _tail_block(dist, r)
    n, dim = block.shape
    # (row 2^18 is among the last four rows when n % 256 < 4; everywhere else neither a planted nor a loud row is one of the 256-th rows a sample may hold)
    assert r < 4 or all(x % 256 for x in planted + loud)
    vecs, osq, rows, st = _segment(qa, dist, dim, n, seed=0, vecs=block)
    k = len(planted)
    dead = None
    if with_deleted:      # the loud rows point-deleted, and the rest of the last tile except the planted rows
        dead = np.zeros(n, dtype=bool)
        dead[n - n % 256:] = True
        dead[loud] = True
        dead[planted] = False
        st.set_deleted(dead)
    qpre = O.preprocess(dist, queries[:k + 2])
    sc = _oracle_scores(osq, rows, qpre, n)
    want = _oracle_top(osq, rows, qpre, n, top, dead=dead, sc=sc)
    _tail_precondition(osq, vecs, rows, planted, loud, shift, sc, want)
    s = qa.BatchFilteredSearcher(queries, st, top)
    got = s.peek_top_all()
    assert "scan_sqw_kernel" in _kernel(qa, s), _kernel(qa, s)
    assert s.counters.fallback_queries == 0      # (the 32-query scan would put a dropped row back)
    assert all(len(g) == top for g in got)
    for g, (ids, scores) in zip(got[:k + 2], want):
        assert g["idx"].tolist() == ids.tolist()
        assert np.array_equal(g["score"].view(np.uint32), scores.view(np.uint32))
        assert dead is None or not dead[g["idx"]].any()
    _same(got, _narrow(qa, queries, st, top))


@pytest.mark.parametrize("r", TAIL_R)
@pytest.mark.parametrize("dist", [O.DOT, O.COSINE, O.EUCLID])
def test_sq_wide_pass_a_result_in_each_of_the_last_rows(qa, dist, r):
    _tail_case(qa, dist, r, with_deleted=False)


def test_sq_wide_pass_a_result_in_each_of_the_last_rows_beside_deleted_ones(qa):
    _tail_case(qa, O.DOT, 87, with_deleted=True)


# ---- un-centred blocks.  Dot / cosine: vector_offset / multiplier ~ dim (offset / alpha)^2, which values in a narrow range far from zero drive past what
# the pass's int32 column and bound hold (2^30: the column's clamp; 2^31: the bound itself).  Such a block has to be served all the same - by whichever
# route - with the full, exact lists.  One code step is far below an ulp of the f32 score here, so scores tie in masses: score, then lower id. ----
@pytest.mark.parametrize("regime,low", [("inside", 0.9), ("clamped", 0.955), ("saturated", 0.97)])
@pytest.mark.parametrize("dist", [O.DOT, O.COSINE])
def test_sq_wide_pass_uncentred_blocks(qa, dist, regime, low):
    n, dim, nq, top = (1 << 18) + 87, 256, 36, 10
    rng = np.random.default_rng(100 * dist + int(1000 * low))
    block = rng.uniform(low, 1.0, (n, dim)).astype(np.float32)
    queries = rng.uniform(low, 1.0, (nq, dim)).astype(np.float32)
    if dist == O.COSINE:
        block /= np.linalg.norm(block, axis=1, keepdims=True)
    vecs, osq, rows, st = _segment(qa, dist, dim, n, seed=0, vecs=block)
    # the regime, from the oracle's encoder: with a positive offset vector_offset grows with the sum of the codes, so every row's vector_offset / multiplier
    # lies between those of a row of codes 0 and a row of codes 127
    assert float(osq.sq.offset) > 0.0
    ends = osq.encode_rows(np.stack([np.full(dim, vecs.min(), dtype=np.float32), np.full(dim, vecs.max(), dtype=np.float32)]))
    assert (ends[0, 4:] == 0).all() and (ends[1, 4:] == 127).all()
    b_low, b_high = (ends[:, :4].copy().view(np.float32)[:, 0].astype(np.float64) / float(osq.sq.multiplier)).tolist()
    b_rows = rows[::997, :4].copy().view(np.float32)[:, 0].astype(np.float64) / float(osq.sq.multiplier)
    assert 0.0 < b_low <= b_rows.min() and b_rows.max() <= b_high
    print("vector_offset / multiplier in [%.4g, %.4g]" % (b_low, b_high))
    if regime == "inside":
        assert b_high < 2.0 ** 29
    elif regime == "clamped":
        assert 2.0 ** 30 < b_low and b_high < 2.0 ** 31
    else:
        assert b_low > 2.0 ** 31
    s = qa.BatchFilteredSearcher(queries, st, top)
    got = s.peek_top_all()
    name, c = _kernel(qa, s), s.counters
    if regime == "inside":
        assert "scan_sqw_kernel" in name, name
    # every query is served: by the prefilter (the pass, with or without the 32-query scan behind it), or the whole batch outside it
    assert c.prefilter_queries + (0 if "scan_sqw_kernel" in name else nq) == nq and c.fallback_queries <= c.prefilter_queries
    assert all(len(g) == top for g in got)
    _same(got, _narrow(qa, queries, st, top))
    want = _oracle_top(osq, rows, O.preprocess(dist, queries[:2]), n, top)
    for g, (ids, scores) in zip(got[:2], want):
        assert g["idx"].tolist() == ids.tolist()
        assert np.array_equal(g["score"].view(np.uint32), scores.view(np.uint32))
