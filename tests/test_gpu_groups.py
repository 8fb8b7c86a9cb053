"""Grouped search on the device (qmx_group_search; groups.hip, api_groups.hip).  The expected value of every case is `grouped_exact`
(tests/group_reference.py: the contract, a dozen lines) applied to the device's OWN full ranked list - qmx_search_topk with top = n over the same
candidates - and the key column, so scores are compared bit for bit.  The counters prove which path ran: stage 0 alone, or the score-matrix
fallback with its selection pages."""
import ctypes as C

import numpy as np
import pytest

import qdrant_amd as qa
from qdrant_amd import _ffi as F
import group_reference as G

pytestmark = pytest.mark.gpu
NONE = F.GROUP_NONE
N, DIM, NQ = 4096, 32, 4


def _rows(seed, n=N, dim=DIM, dominant=0):
    """Gaussian rows; the first `dominant` rows lie along the direction every query shares, far above the rest."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(dim).astype(np.float32)
    v /= np.linalg.norm(v)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    if dominant:
        rows[:dominant] = 12.0 * v + 0.1 * rows[:dominant]
    queries = (v + 0.05 * rng.standard_normal((NQ, dim))).astype(np.float32)
    return rows, queries


def _ranked(scorer, top, ids=None):
    out = np.zeros((scorer.nq, top), dtype=qa.ScoredPointOffset)
    counts = np.zeros(scorer.nq, dtype=np.uint32)
    F.check(F.lib().qmx_search_topk(scorer._h, top, F.ptr(ids), 0 if ids is None else len(ids), F.ptr(out), F.ptr(counts), None, None))
    return [out[q, :counts[q]] for q in range(scorer.nq)]


def _keys_of(keys, offsets=None):
    if offsets is None:
        return lambda i: [] if keys[i] == NONE else [int(keys[i])]
    return lambda i: [int(k) for k in keys[int(offsets[i]):int(offsets[i + 1])]]


def _check(scorer, gk, keys_of, limit, group_size, ids=None, thr=None, top=None, ranked=None):
    """search_groups against grouped_exact over the device's ranked lists; returns (counters, the groups)."""
    cnt = F.GroupCounters()
    got = qa.search_groups(scorer, None, gk, limit, group_size, ids=ids, score_threshold=thr, counters=cnt)
    ranked = ranked if ranked is not None else _ranked(scorer, top or (len(ids) if ids is not None else scorer.storage.total_vector_count()), ids)
    assert len(got) == scorer.nq
    for q in range(scorer.nq):
        want = G.grouped_exact([(int(p["idx"]), p["score"]) for p in ranked[q]], keys_of, limit, group_size, thr)
        assert [k for k, _ in got[q]] == [k for k, _ in want], q
        for (k, hits), (_, whits) in zip(got[q], want):
            assert hits["idx"].tolist() == [i for i, _ in whits], (q, k)
            assert np.array_equal(hits["score"].view(np.uint32), np.array([s for _, s in whits], dtype=np.float32).view(np.uint32)), (q, k)
    return cnt, got


@pytest.fixture(scope="module")
def plain():
    rows, queries = _rows(1)
    st = qa.VectorStorage(rows, qa.Distance.Dot)
    scorer = qa.new_raw_scorer(queries, st)
    ranked = _ranked(scorer, N)
    yield st, scorer, ranked
    scorer.close()
    st.close()


@pytest.fixture(scope="module")
def dominated():
    rows, queries = _rows(2, dominant=200)
    st = qa.VectorStorage(rows, qa.Distance.Dot)
    scorer = qa.new_raw_scorer(queries, st)
    ranked = _ranked(scorer, N)
    assert all(set(r["idx"][:200].tolist()) == set(range(200)) for r in ranked)
    yield st, scorer, ranked
    scorer.close()
    st.close()


def test_a_singleton_groups_finish_in_stage_0(plain):
    _, scorer, ranked = plain
    keys = np.arange(N, dtype=np.uint32)
    gk = qa.GroupKeys(N, keys)
    cnt, got = _check(scorer, gk, _keys_of(keys), 10, 1, ranked=ranked)
    assert cnt.fallback_queries == 0 and cnt.score_passes == 0 and cnt.pages == NQ
    assert all(len(g) == 10 for g in got)
    # 64 singleton groups are exactly one page; 65 need a second
    cnt, _ = _check(scorer, gk, _keys_of(keys), 64, 1, ranked=ranked)
    assert cnt.fallback_queries == 0
    cnt, _ = _check(scorer, gk, _keys_of(keys), 65, 1, ranked=ranked)
    assert cnt.fallback_queries == NQ and cnt.pages == 2 * NQ


def test_b_one_group_holds_the_200_best_hits(dominated):
    _, scorer, ranked = dominated
    keys = (1 + np.arange(N) % 20).astype(np.uint32)
    keys[:200] = 0
    gk = qa.GroupKeys(N, keys)
    cnt, got = _check(scorer, gk, _keys_of(keys), 3, 2, ranked=ranked)
    assert cnt.fallback_queries == NQ and cnt.score_passes >= 1
    assert all(g[0][0] == 0 and len(g) == 3 for g in got)
    # the bound is limit * group_size + 1 = 7 fallback pages per query: two groups are left after stage 0, a page of 64 rows outside the full group fills them
    assert NQ < cnt.pages <= 3 * NQ
    assert "group_select_kernel" in F.last_kernel(scorer._h)


def test_c_small_groups_and_fewer_groups_than_limit(plain):
    _, scorer, ranked = plain
    keys = np.full(N, NONE, dtype=np.uint32)
    carry = np.random.default_rng(3).choice(N, 12, replace=False)
    keys[carry] = np.arange(12) % 5
    gk = qa.GroupKeys(N, keys)
    cnt, got = _check(scorer, gk, _keys_of(keys), 10, 4, ranked=ranked)
    assert all(len(g) == 5 and sum(len(h) for _, h in g) == 12 for g in got)      # every group short of group_size: the stream was exhausted
    assert cnt.fallback_queries == NQ
    # every point one of 3 groups, group_size beyond a page: filled from many pages, limit never reached
    keys3 = (np.arange(N) % 3).astype(np.uint32)
    gk3 = qa.GroupKeys(N, keys3)
    _check(scorer, gk3, _keys_of(keys3), 7, 70, ranked=ranked)


@pytest.mark.parametrize("limit,group_size,modulus", [(40, 4, 60), (2, 100, 3)])
def test_d_more_hits_than_a_page(plain, limit, group_size, modulus):
    _, scorer, ranked = plain
    keys = ((np.arange(N) * 7919) % modulus).astype(np.uint32)
    gk = qa.GroupKeys(N, keys)
    cnt, got = _check(scorer, gk, _keys_of(keys), limit, group_size, ranked=ranked)
    assert all(len(g) == limit and all(len(h) == group_size for _, h in g) for g in got)
    assert cnt.fallback_queries == NQ and cnt.pages <= NQ * (limit * group_size + 2)


@pytest.mark.parametrize("within", [True, False])
def test_e_duplicated_rows_tie_within_and_across_groups(within):
    rows, queries = _rows(5)
    rows[N // 2:] = rows[:N // 2]                       # row i and row i + 2048 score the same
    rows[100:140] = rows[100]                           # and a run of 40 equal rows
    st = qa.VectorStorage(rows, qa.Distance.Dot)
    scorer = qa.new_raw_scorer(queries, st)
    half = np.arange(N) % (N // 2)
    keys = (half % 50 if within else (half % 50) + 50 * (np.arange(N) // (N // 2))).astype(np.uint32)
    gk = qa.GroupKeys(N, keys)
    ranked = _ranked(scorer, N)
    assert all(len(np.unique(r["score"])) < N // 2 + 1 for r in ranked)
    _check(scorer, gk, _keys_of(keys), 12, 3, ranked=ranked)
    _check(scorer, gk, _keys_of(keys), 100, 2, ranked=ranked)
    scorer.close()
    st.close()


def test_f_none_keys_deleted_flags_filter_and_ids_together():
    rows, queries = _rows(6, dominant=200)
    rng = np.random.default_rng(60)
    st = qa.VectorStorage(rows, qa.Distance.Dot)
    deleted = rng.random(N) < 0.2
    st.set_deleted(point_deleted=deleted)
    scorer = qa.new_raw_scorer(queries, st)
    allowed = rng.random(N) < 0.7
    scorer.set_filter(allowed)
    ids = rng.permutation(N)[:3000].astype(np.uint32)
    keys = (np.arange(N) % 37).astype(np.uint32)
    keys[:200] = 36
    keys[rng.random(N) < 0.3] = NONE
    gk = qa.GroupKeys(N, keys, n_distinct=37)
    ranked = _ranked(scorer, len(ids), ids)
    live = set(np.flatnonzero(~deleted & allowed).tolist()) & set(ids.tolist())
    assert all(set(r["idx"].tolist()) == live for r in ranked)
    cnt, got = _check(scorer, gk, _keys_of(keys), 8, 5, ids=ids, ranked=ranked)
    assert cnt.fallback_queries == NQ
    assert all(int(h["idx"][j]) in live and keys[h["idx"][j]] == k for g in got for k, h in g for j in range(len(h)))
    # without the list: the rows themselves are the candidates (the selection's 16-byte loads)
    _check(scorer, gk, _keys_of(keys), 8, 5, ranked=_ranked(scorer, N))
    scorer.close()
    st.close()


def test_g_multi_valued_keys_csr(dominated):
    _, scorer, ranked = dominated
    rng = np.random.default_rng(7)
    per = [sorted(set(int(k) for k in rng.integers(0, 30, int(rng.integers(0, 4))))) for _ in range(N)]
    for i in range(200):
        per[i] = [40] if i % 2 else [40, 41]
    best = [int(r["idx"][0]) for r in ranked]
    for b in best:
        per[b] = [3, 7, 41]                                          # a best hit shared by three groups: ordered by key index
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.uint64)
    keys = np.array([k for p in per for k in p], dtype=np.uint32)
    gk = qa.GroupKeys(N, keys, offsets)
    for limit, group_size in ((2, 3), (6, 2), (5, 70)):              # (2, 3): slots run out between the best hit's keys
        cnt, got = _check(scorer, gk, _keys_of(keys, offsets), limit, group_size, ranked=ranked)
        assert all([k for k, _ in g][:2] == [3, 7] for g in got)
    assert cnt.fallback_queries == NQ


def test_g_the_reference_literal_with_multiple_payload_values():
    """aggregator.rs test_group_with_multiple_payload_values: ["a", "a"], ["a", "b"], "b" with 3 groups of 2 -> a: [1, 2], b: [2, 3]."""
    rows = np.zeros((3, DIM), dtype=np.float32)
    rows[:, 0] = [0.99, 0.85, 0.75]
    query = np.zeros((1, DIM), dtype=np.float32)
    query[0, 0] = 1.0
    st = qa.VectorStorage(rows, qa.Distance.Dot)
    gk = qa.GroupKeys(3, [0, 0, 0, 1, 1], offsets=[0, 2, 4, 5])
    got = qa.search_groups(st, query, gk, 3, 2)[0]
    assert [(k, h["idx"].tolist()) for k, h in got] == [(0, [0, 1]), (1, [1, 2])]
    assert got[0][1]["score"].tolist() == [np.float32(0.99), np.float32(0.85)]
    st.close()


def test_h_score_threshold(dominated):
    _, scorer, ranked = dominated
    keys = (1 + np.arange(N) % 20).astype(np.uint32)
    keys[:200] = 0
    gk = qa.GroupKeys(N, keys)
    for rank in (0, 1, 3, 199, 201, 230, 1000):      # inside the first group; before 5 groups exist; inside later groups; far down
        thr = float(ranked[0]["score"][rank])        # a score of the list itself: `>=` keeps it
        cnt, got = _check(scorer, gk, _keys_of(keys), 5, 3, thr=thr, ranked=ranked)
        assert all(float(h["score"].min()) >= np.float32(thr) for g in got for _, h in g)
    cnt, got = _check(scorer, gk, _keys_of(keys), 5, 3, thr=float(ranked[0]["score"][1]), ranked=ranked)
    assert len(got[0]) == 1 and len(got[0][0][1]) == 2
    cnt, got = _check(scorer, gk, _keys_of(keys), 5, 3, thr=1e30, ranked=ranked)
    assert all(g == [] for g in got)


def test_i_score_matrix_budget_tiles_the_unfinished_queries():
    rows, queries = _rows(9, dominant=200)
    queries = np.concatenate([queries, queries[:1] * 1.5])      # 5 queries, all unfinished after stage 0
    st = qa.VectorStorage(rows, qa.Distance.Dot)
    scorer = qa.new_raw_scorer(queries, st)
    keys = (1 + np.arange(N) % 20).astype(np.uint32)
    keys[:200] = 0
    gk = qa.GroupKeys(N, keys)
    ranked = _ranked(scorer, N)
    whole, got_whole = _check(scorer, gk, _keys_of(keys), 4, 3, ranked=ranked)
    assert whole.fallback_queries == 5
    qa.set_option("group_matrix_bytes", 2 * N * 4)      # two score rows: tiles of 2, 2 and 1 queries
    try:
        tiled, got_tiled = _check(scorer, gk, _keys_of(keys), 4, 3, ranked=ranked)
    finally:
        qa.set_option("group_matrix_bytes", -1)
    assert tiled.fallback_queries == 5 and tiled.score_passes == 3 * whole.score_passes and tiled.pages == whole.pages
    assert tiled.kernel_launches > whole.kernel_launches
    scorer.close()
    st.close()


@pytest.mark.parametrize("kind", ["f16", "u8", "sq"])
def test_j_other_segment_types(kind):
    rows, queries = _rows(10, dominant=200)
    if kind == "f16":
        st = qa.VectorStorage(rows, qa.Distance.Cosine, qa.VectorStorageDatatype.Float16)
    elif kind == "u8":
        rows = np.clip(np.round(rows * 20 + 128), 0, 255).astype(np.float32)
        rows[:200] = np.clip(250 + np.round(rows[:200] / 64), 0, 255)      # (all-positive queries: the brightest rows score highest)
        queries = np.clip(np.round(queries * 100 + 128), 0, 255).astype(np.float32)
        st = qa.VectorStorage(rows, qa.Distance.Dot, qa.VectorStorageDatatype.Uint8)
    else:
        quant = qa.ScalarQuantizer.from_min_max(rows, DIM, qa.Distance.Dot)
        st = qa.EncodedVectorsU8(quant.encode(rows), quant)
    scorer = qa.new_raw_scorer(queries, st)
    keys = ((np.arange(N) * 31) % 23).astype(np.uint32)
    keys[:200] = 22
    gk = qa.GroupKeys(N, keys)
    ranked = _ranked(scorer, N)
    cnt, _ = _check(scorer, gk, _keys_of(keys), 6, 4, ranked=ranked)
    assert cnt.fallback_queries > 0
    _check(scorer, gk, _keys_of(keys), 3, 1, ranked=ranked)
    scorer.close()
    st.close()


def test_k_large_block_65_queries():
    n, dim, nq, chunk, dom = 1 << 18, 128, 65, 8, 512
    rng = np.random.default_rng(11)
    v = rng.standard_normal(dim).astype(np.float32)
    centers = rng.standard_normal((n // chunk, dim)).astype(np.float32)
    rows = np.repeat(centers, chunk, axis=0)
    rows += np.float32(0.05) * rng.standard_normal((n, dim)).astype(np.float32)
    rows[:dom] = v + np.float32(0.05) * rng.standard_normal((dom, dim)).astype(np.float32)      # one document near every query
    queries = (v + 0.2 * rng.standard_normal((nq, dim))).astype(np.float32)
    keys = (np.arange(n) // chunk).astype(np.uint32)
    keys[:dom] = 0
    st = qa.VectorStorage(rows, qa.Distance.Dot)
    scorer = qa.new_raw_scorer(queries, st)
    gk = qa.GroupKeys(n, keys)
    top, limit, group_size = 4096, 10, 3
    ranked = _ranked(scorer, top)
    keys_of = _keys_of(keys)
    for r in ranked:      # 4 096 ranks suffice: the contract's walk fills `limit` groups inside the list
        want = G.grouped_exact([(int(p["idx"]), p["score"]) for p in r], keys_of, limit, group_size)
        assert len(want) == limit and all(len(h) == group_size for _, h in want)
        assert set(r["idx"][:64].tolist()) <= set(range(dom))
    cnt, _ = _check(scorer, gk, keys_of, limit, group_size, ranked=ranked)
    assert cnt.fallback_queries == nq and cnt.pages <= 4 * nq
    scorer.close()
    st.close()


def test_l_argument_errors(plain):
    st, scorer, _ = plain
    keys = (np.arange(N) % 9).astype(np.uint32)
    with pytest.raises(qa.QmxError) as e:
        qa.GroupKeys(N, keys, n_distinct=8)                      # key 8 >= n_distinct: found on the device at create
    assert e.value.status == F.ERR_OUT_OF_BOUNDS
    h = C.c_void_p()
    off = np.array([0, 2, 1, 3], dtype=np.uint64)
    assert F.lib().qmx_group_keys_create(0, 3, F.ptr(np.zeros(3, dtype=np.uint32)), F.ptr(off), 1, C.byref(h)) == F.ERR_BAD_ARG
    gk = qa.GroupKeys(N, keys)
    for limit, group_size in ((F.GROUP_MAX_LIMIT + 1, 1), (1024, 65), (2, 32769)):
        with pytest.raises(qa.QmxError) as e:
            qa.search_groups(scorer, None, gk, limit, group_size)
        assert e.value.status == F.ERR_NOT_SUPPORTED
    assert qa.search_groups(scorer, None, gk, 0, 3) == [[]] * NQ and qa.search_groups(scorer, None, gk, 3, 0) == [[]] * NQ
    assert qa.search_groups(scorer, None, gk, 3, 2, ids=np.zeros(0, dtype=np.uint32)) == [[]] * NQ
    short = qa.GroupKeys(N - 1, keys[:-1])
    with pytest.raises(qa.QmxError) as e:
        qa.search_groups(scorer, None, short, 3, 2)              # the column does not cover the segment
    assert e.value.status == F.ERR_BAD_ARG
    with pytest.raises(qa.QmxError) as e:
        qa.search_groups(scorer, None, gk, 3, 2, ids=np.array([1, N + 5], dtype=np.uint32))
    assert e.value.status == F.ERR_OUT_OF_BOUNDS
    assert len(qa.search_groups(scorer, None, gk, 1024, 64)[0]) == 9      # the largest request: limit * group_size = 65536
