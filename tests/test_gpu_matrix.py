"""The distance matrix API on the device (qmx_sample_points, qmx_search_matrix; matrix.hip, api_matrix.hip).  The sampler is checked against
`sample_reference`, the nearest lists against `matrix_reference` over the ORACLE's score matrix - `DenseStorage.score_points(rows[sample], sample,
encoded=True)` - with scores compared bit for bit and ids and columns exactly (tests/matrix_reference.py has the contract in a few lines).

f16: the project's other f16 kernels sum in another order than the oracle's AVX leaf (1e-5), so the matrix call scans its f16
block of 32 and more elements per row with a policy of its own that keeps that leaf's 32 running sums apart (matrix_f16.hip): the f16 lists are held to
the oracle's bits like the f32 and u8 ones.  Each comparison prints its worst relative difference before it asserts."""
import numpy as np
import pytest

import qdrant_amd as qa
from qdrant_amd import _ffi as F
import matrix_reference as R
import oracle_ffi as O

pytestmark = pytest.mark.gpu
DIST = {O.COSINE: qa.Distance.Cosine, O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid, O.MANHATTAN: qa.Distance.Manhattan}
DT = {O.F32: qa.VectorStorageDatatype.Float32, O.F16: qa.VectorStorageDatatype.Float16, O.U8: qa.VectorStorageDatatype.Uint8}
N = 2000
SAMPLE_SIZES = (2, 3, 17, 65, 129, 130)


def _stored(dtype, dist, raw):
    """f32 values -> the rows as stored: preprocessed and cast as at insert."""
    if dtype == O.U8:
        return O.to_u8(raw * 36.0 + 128.0)
    pre = O.preprocess(dist, raw)
    return O.to_f16(pre) if dtype == O.F16 else pre


def _pair(dtype, dist, stored, point_deleted=None, vec_deleted=None):
    """(device storage with the flags, oracle storage without: a deleted point keeps its row, and the oracle only scores) over the same stored rows."""
    st = qa.VectorStorage(stored.view(np.float16) if dtype == O.F16 else stored, DIST[dist], DT[dtype])
    if point_deleted is not None or vec_deleted is not None:
        st.set_deleted(point_deleted, vec_deleted)
    return st, O.DenseStorage(dtype, dist, stored)


def _sample_ids(seed, n, s):
    return np.sort(np.random.default_rng(seed).choice(n, size=s, replace=False)).astype(np.uint32)


def _live(n, point_deleted, vec_deleted):
    live = np.ones(n, dtype=bool)
    if point_deleted is not None:
        live &= ~np.asarray(point_deleted, dtype=bool)
    if vec_deleted is not None:
        live &= ~np.asarray(vec_deleted, dtype=bool)
    return live


def _check(st, ost, sample, limit, live=None, scores=None, label=""):
    """search_matrix against matrix_reference over the oracle's scores of the sample (`scores`: that matrix, or a larger one whose leading block it is)."""
    sample = np.ascontiguousarray(sample, dtype=np.uint32)
    s = len(sample)
    if scores is None:
        scores = ost.score_points(ost.rows[sample], sample, encoded=True)
    live_s = np.ones(s, dtype=bool) if live is None else np.asarray(live, dtype=bool)[sample]
    want = R.matrix_reference(scores[:s, :s], live_s, limit)
    got = qa.search_matrix(st, sample, limit)
    assert got.ids.tolist() == sample.tolist() and len(got.nearests) == s
    worst = 0.0
    for i in range(s):
        cols, sc = want[i]
        if len(sc) == len(got.nearests[i]) and len(sc):
            worst = max(worst, float(np.max(np.abs(got.nearests[i]["score"].astype(np.float64) - sc) / np.maximum(np.abs(sc.astype(np.float64)), 1e-30))))
    print("%s S=%d limit=%d worst relative score difference %.3g" % (label, s, limit, worst))
    for i in range(s):
        cols, sc = want[i]
        assert got.cols[i].tolist() == cols.tolist(), (label, s, limit, i)
        assert got.nearests[i]["idx"].tolist() == sample[cols].tolist(), (label, s, limit, i)
        assert np.array_equal(got.nearests[i]["score"].view(np.uint32), sc.view(np.uint32)), (label, s, limit, i)
    return got


# ---- the sampler --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flagged():
    n = 3000
    rng = np.random.default_rng(11)
    pdel = rng.random(n) < 0.30
    vdel = rng.random(n) < 0.05
    mask = np.arange(n) % 3 == 0
    st = qa.VectorStorage(np.zeros((n, 4), dtype=np.uint8), qa.Distance.Dot, qa.VectorStorageDatatype.Uint8)
    st.set_deleted(pdel, vdel)
    yield st, ~pdel & ~vdel, mask
    st.close()


def test_sampler_matches_the_reference(flagged):
    st, live, mask = flagged
    cand = int((live & mask).sum())
    assert 400 < cand < 800
    for seed in (0, 0x5EED0001FFFF):
        for n in (1, 2, 10, 64, 65, 1000, cand, cand + 5, 65536):
            got = qa.sample_points(st, n, mask=mask, seed=seed)
            assert got.tolist() == R.sample_reference(live & mask, n, seed).tolist(), (seed, n)
    # without a mask: the live offsets; n past them returns all of them in ascending order
    assert qa.sample_points(st, 65536, seed=3).tolist() == np.flatnonzero(live).tolist()
    assert qa.sample_points(st, 100, seed=3).tolist() == R.sample_reference(live, 100, 3).tolist()
    assert qa.sample_points(st, 0, seed=3).tolist() == []


def test_sampler_allow_bits_shorter_than_the_rows_and_no_candidates(flagged):
    st, live, mask = flagged
    for bits in (1, 63, 64, 65, 1000):
        want_live = live.copy()
        want_live[bits:] = False
        got = qa.sample_points(st, 20, mask=np.ones(bits, dtype=bool), seed=9)
        assert got.tolist() == R.sample_reference(want_live, 20, 9).tolist(), bits
    assert qa.sample_points(st, 5, mask=np.zeros(3000, dtype=bool), seed=1).tolist() == []
    assert qa.sample_points(st, 5, mask=np.zeros(0, dtype=bool), seed=1).tolist() == []
    # flags shorter than the rows: past the point flags a row is deleted, past the vector flags it is not (DeletedView)
    st2 = qa.VectorStorage(np.zeros((300, 4), dtype=np.uint8), qa.Distance.Dot, qa.VectorStorageDatatype.Uint8)
    st2.set_deleted(np.zeros(130, dtype=bool), np.ones(70, dtype=bool))
    assert qa.sample_points(st2, 65536, seed=2).tolist() == list(range(70, 130))
    st2.close()


def test_sampler_crowded_boundary_bin():
    """Every candidate shares the top 12 bits of its key: the first level's boundary bin holds them all and the later levels decide."""
    n, seed = 200000, 77
    keys = R.sample_keys_np(seed, np.arange(n))
    top = keys >> np.uint64(52)
    mask = top == top[12345]
    cand = int(mask.sum())
    assert cand >= 20
    st = qa.VectorStorage(np.zeros((n, 4), dtype=np.uint8), qa.Distance.Dot, qa.VectorStorageDatatype.Uint8)
    for k in (1, 2, cand // 2, cand - 1, cand, cand + 1):
        assert qa.sample_points(st, k, mask=mask, seed=seed).tolist() == R.sample_reference(mask, k, seed).tolist(), k
    # ... and a plain sample of the same rows, where the boundary bin of the first level holds a few dozen
    for k in (10, 1000, 65536):
        assert qa.sample_points(st, k, seed=seed).tolist() == R.sample_reference(np.ones(n, dtype=bool), k, seed).tolist(), k
    st.close()


def test_sampler_refusals(flagged):
    st, _, _ = flagged
    with pytest.raises(qa.QmxError) as e:
        qa.sample_points(st, 65537)
    assert e.value.status == F.ERR_NOT_SUPPORTED
    sp = qa.SparseVectorStorage([(np.array([1, 5], dtype=np.uint32), np.array([1.0, 2.0], dtype=np.float32))] * 4)
    with pytest.raises(qa.QmxError) as e:
        qa.sample_points(sp, 2)
    assert e.value.status == F.ERR_NOT_SUPPORTED
    with pytest.raises(qa.QmxError) as e:
        qa.search_matrix(sp, [0, 1], 1)
    assert e.value.status == F.ERR_NOT_SUPPORTED
    sp.close()


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", [O.DOT, O.COSINE, O.EUCLID, O.MANHATTAN])
@pytest.mark.parametrize("dtype", [O.F32, O.F16, O.U8])
def test_matrix_shapes(dtype, dist):
    """dim: below 32 the small leaf, then a scalar tail, then the workload's width; S and limit: the tile remainders of the 64- and 128-query shapes, the clipped counts."""
    for dim in (4, 31, 33, 768):
        stored = _stored(dtype, dist, O.synth(0x3A7 + dim, 0, N, dim))
        st, ost = _pair(dtype, dist, stored)
        big = _sample_ids(dim, N, max(SAMPLE_SIZES))
        for s in SAMPLE_SIZES:
            sample = np.sort(big[:s])
            scores = ost.score_points(ost.rows[sample], sample, encoded=True)
            for limit in sorted({1, 3, s - 1, s + 4}):
                got = _check(st, ost, sample, limit, scores=scores, label="dtype %d dist %d dim %d" % (dtype, dist, dim))
                assert all(len(r) == min(limit, s - 1) for r in got.nearests)
        st.close()


@pytest.mark.parametrize("dist", [O.DOT, O.COSINE, O.EUCLID, O.MANHATTAN])
def test_matrix_f16_block_layout(dist):
    """f16 rows of 32 and more elements are gathered into whole two-iteration segments (matrix_f16.hip): one iteration padded with zeros, two, an odd
    count, each with and without a scalar tail; 17 queries = one full 16-query tile and a tile of one."""
    for dim in (32, 63, 64, 96, 100, 130):
        stored = _stored(O.F16, dist, O.synth(0xF16 + dim, 0, 300, dim))
        st, ost = _pair(O.F16, dist, stored)
        sample = _sample_ids(dim, 300, 17)
        scores = ost.score_points(ost.rows[sample], sample, encoded=True)
        for limit in (3, 16):
            _check(st, ost, sample, limit, scores=scores, label="f16 dist %d dim %d" % (dist, dim))
        st.close()


@pytest.fixture(scope="module")
def rows33():
    return O.synth(0xABCD, 0, N, 33)


def test_matrix_self_below_the_list_pops_the_last(rows33):
    """Dot over rows of very different norms: for the short rows self ranks below limit + 1, and the full list loses its last entry."""
    raw = rows33 * np.geomspace(0.01, 100.0, N, dtype=np.float32)[:, None]
    st, ost = _pair(O.F32, O.DOT, raw)
    sample = _sample_ids(1, N, 97)
    scores = ost.score_points(ost.rows[sample], sample, encoded=True)
    self_rank = [int((scores[i] > scores[i, i]).sum()) for i in range(len(sample))]
    assert sum(r > 4 for r in self_rank) > 10 and sum(r <= 3 for r in self_rank) > 3      # both branches run at limit 3
    _check(st, ost, sample, 3, scores=scores, label="norms")
    st.close()


def test_matrix_duplicates_and_all_equal_rows(rows33):
    # every sample row stored twice: self and its twin tie, self goes by position, the twin stays
    half = O.preprocess(O.COSINE, rows33[:N // 2])
    stored = np.concatenate([half, half])
    st, ost = _pair(O.F32, O.COSINE, stored)
    base = _sample_ids(2, N // 2, 40)
    sample = np.sort(np.concatenate([base, base + N // 2])).astype(np.uint32)
    got = _check(st, ost, sample, 3, label="twins")
    where = {int(x): i for i, x in enumerate(sample)}
    for i, x in enumerate(sample):
        twin = int(x) + N // 2 if x < N // 2 else int(x) - N // 2
        assert where[twin] in got.cols[i].tolist(), i
    st.close()
    # all rows equal: pure tie order - the lowest positions that are not the row's own
    same = np.tile(rows33[:1], (200, 1))
    st, ost = _pair(O.F32, O.DOT, same)
    sample = _sample_ids(3, 200, 70)
    got = _check(st, ost, sample, 5, label="equal")
    assert got.cols[0].tolist() == [1, 2, 3, 4, 5] and got.cols[3].tolist() == [0, 1, 2, 4, 5] and got.cols[69].tolist() == [0, 1, 2, 3, 4]
    st.close()


def test_matrix_deleted_sample_points(rows33):
    rng = np.random.default_rng(5)
    sample = _sample_ids(4, N, 66)
    pdel, vdel = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    gone = rng.choice(sample, size=22, replace=False)
    pdel[gone[:11]] = True
    vdel[gone[11:]] = True
    st, ost = _pair(O.F32, O.EUCLID, rows33, pdel, vdel)
    scores = ost.score_points(ost.rows[sample], sample, encoded=True)
    for limit in (1, 3, 43, 44, 65, 70):
        got = _check(st, ost, sample, limit, live=_live(N, pdel, vdel), scores=scores, label="deleted")
        assert all(len(r) == min(limit, 44 if (pdel | vdel)[sample[i]] else 43) for i, r in enumerate(got.nearests))
        assert not set(np.concatenate([r["idx"] for r in got.nearests]).tolist()) & set(gone.tolist())
    st.close()
    # every sample point but one deleted: the live one has no neighbour, the others have it alone
    pdel = np.zeros(N, dtype=bool)
    pdel[sample[1:]] = True
    st, ost = _pair(O.F32, O.EUCLID, rows33, pdel)
    got = _check(st, ost, sample, 3, live=~pdel, scores=scores, label="one live")
    assert [len(r) for r in got.nearests] == [0] + [1] * 65
    st.close()


@pytest.mark.parametrize("s", [4099, 8200])
def test_matrix_crosses_the_chunks(s):
    """More sample points than one chunk of 4 096 queries holds; limit 2."""
    stored = O.synth(0xC0FFEE, 0, 9000, 8)
    st, ost = _pair(O.F32, O.DOT, stored)
    _check(st, ost, _sample_ids(s, 9000, s), 2, label="chunks")
    st.close()


@pytest.mark.parametrize("dtype,dist,dim,s,limit", [(O.F32, O.COSINE, 768, 130, 3), (O.U8, O.EUCLID, 33, 65, 64), (O.F32, O.MANHATTAN, 31, 17, 5)])
def test_matrix_equals_the_hand_made_path(dtype, dist, dim, s, limit):
    """new_raw_scorer_internal(sample) + the top limit + 1 among the sample, the row's own entry dropped on the host."""
    stored = _stored(dtype, dist, O.synth(0xE0 + dim, 0, N, dim))
    st, _ = _pair(dtype, dist, stored)
    sample = _sample_ids(dim, N, s)
    scorer = qa.new_raw_scorer_internal(sample, st)
    top = min(limit + 1, s)
    out = np.zeros((s, top), dtype=qa.ScoredPointOffset)
    counts = np.zeros(s, dtype=np.uint32)
    F.check(F.lib().qmx_search_topk(scorer._h, top, F.ptr(sample), s, F.ptr(out), F.ptr(counts), None, None))
    got = qa.search_matrix(st, sample, limit)
    for i in range(s):
        row = out[i, :counts[i]]
        row = row[row["idx"] != sample[i]][:limit]
        assert got.nearests[i]["idx"].tolist() == row["idx"].tolist(), i
        assert np.array_equal(got.nearests[i]["score"].view(np.uint32), row["score"].view(np.uint32)), i
    scorer.close()
    st.close()


# ---- Python -------------------------------------------------------------------------------------------------------------------------------------
def test_python_responses_and_the_sampled_calls(rows33):
    pdel = np.random.default_rng(8).random(N) < 0.2
    st, ost = _pair(O.F32, O.DOT, rows33, pdel)
    sample = _sample_ids(6, N, 33)
    m = qa.search_matrix(st, sample, 4)
    for i, (row, cols) in enumerate(zip(m.nearests, m.cols)):
        assert sample[cols].tolist() == row["idx"].tolist()      # out_cols maps back
    nearests = [[(int(p["idx"]), p["score"]) for p in row] for row in m.nearests]
    assert np.array_equal(m.pairs(), R.pairs_reference(sample, nearests))
    for got, want in zip(m.offsets(), R.offsets_reference(sample, nearests)):
        assert np.array_equal(got, want)
    # sample + search in one call == the two calls made separately
    mask = np.arange(N) % 2 == 1
    ids = qa.sample_points(st, 10, mask=mask, seed=21)
    assert len(ids) == 10 and ids.tolist() == R.sample_reference(mask & ~pdel, 10, 21).tolist()
    two = qa.search_matrix(st, ids, 3)
    assert np.array_equal(qa.search_matrix_pairs(st, sample=10, limit=3, mask=mask, seed=21), two.pairs())
    for got, want in zip(qa.search_matrix_offsets(st, sample=10, limit=3, mask=mask, seed=21), two.offsets()):
        assert np.array_equal(got, want)
    _check(st, ost, ids, 3, live=~pdel, label="sampled")
    st.close()


# ---- errors and empty answers -----------------------------------------------------------------------------------------------------------------------
def test_matrix_errors_and_empty_answers(rows33):
    st, _ = _pair(O.F32, O.DOT, rows33)
    for bad, status in (([5, 3, 9], F.ERR_BAD_ARG), ([3, 5, 5], F.ERR_BAD_ARG), ([3, 5, N], F.ERR_OUT_OF_BOUNDS)):
        with pytest.raises(qa.QmxError) as e:
            qa.search_matrix(st, bad, 2)
        assert e.value.status == status, bad
    with pytest.raises(qa.QmxError) as e:      # (validated in the order the header lists: the size first)
        F.check(F.lib().qmx_search_matrix(st._h, F.ptr(np.zeros(65537, dtype=np.uint32)), 65537, 1, None, None, F.ptr(np.zeros(65537, dtype=np.uint32)), None))
    assert e.value.status == F.ERR_NOT_SUPPORTED
    assert [len(r) for r in qa.search_matrix(st, [3, 5, 9], 0).nearests] == [0, 0, 0]      # limit 0
    assert [len(r) for r in qa.search_matrix(st, [7], 3).nearests] == [0]                  # one point has no others
    assert qa.search_matrix(st, [], 3).nearests == []
    st.close()
    quant = qa.ScalarQuantizer.from_min_max(rows33, 33, qa.Distance.Dot)
    sq = qa.EncodedVectorsU8(quant.encode(rows33), quant)
    with pytest.raises(qa.QmxError) as e:
        qa.search_matrix(sq, [1, 2, 3], 2)
    assert e.value.status == F.ERR_NOT_SUPPORTED
    assert len(qa.sample_points(sq, 5, seed=1)) == 5      # (the sampler serves every non-sparse dtype)
    sq.close()
