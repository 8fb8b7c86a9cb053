"""Option `fallback_beside_scan` (default 1): the conditional exact pass at the end of an int8-copy prefilter search - the queries whose candidate lists
overflowed - is ONE launch of 16-query block rows (scan_mfma16.hip launch_scan_f32_mfma16_groups: block row g serves packed queries 16 g .. 16 g + 15)
and one merge, where a block of it fits beside a block of the int8 scan (128 and 768 coordinates here; not 1 024).  0: a 16-query pass and passes of 64.

Every case runs the same search under option 1, option 0 and the exact scan (`no_split_scan` = 1) and compares ids and score bits; the counters
`prefilter_queries`, `prefilter_candidates`, `verified_rows` and `fallback_queries` must be equal between the two option values, and
`fallback_queries` is what the case constructed - no case passes without running the pass.  `bytes_read` pins which form ran: f overflowed queries stream
the block ceil(f / 16) times in the one-launch form, once (f <= 16) or ceil(f / 64) times (ceil(f / 32) at 1 024 coordinates) in the other.

What depends on the group offsets: a block row that read the queries, bounds, filter indices or `nq` of another group, or wrote its partial lists into
another group's, gives any query past the first sixteen overflowed ones the list of a different query - every case with f > 16 compares those lists with
the exact scan's; the merge's write-back through the packed list is what the scattered cases compare.

How a query is made to overflow: 3 000 rows of the block are copies of one vector v and option `verify_max_per_query` is 2 048 - a query near v has
3 000 equal scores at the top, more than its verification list may take, so it alone is scanned exactly ("hot" queries, as tests/test_gpu_split_scan.py;
the k-th place lies inside that mass of equal scores: the lower id comes first, as the exact scan orders it).  The per-request filter case takes the
other way, a bitmap that allows no row of the sample (tests/test_gpu_i8_sample_scan.py).  The inputs were checked by running them: the asserted
`fallback_queries` are what they give.

Blocks of 2^18 rows, the smallest the prefilters take."""
import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

N = 1 << 18
N_DUP = 3000
OPTION = "fallback_beside_scan"
COUNTERS = ("prefilter_queries", "prefilter_candidates", "verified_rows", "fallback_queries")


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    assert qdrant_amd.get_option(OPTION) == 1 and qdrant_amd.get_option("i8_sample_scan") == 1 and qdrant_amd.get_option("i8_resident") == 1
    return qdrant_amd


@pytest.fixture(scope="module")
def blocks(qa):
    """per row length, made once and left unchanged: (storage with an int8 copy, v, the rows that are copies of v, 128 queries far from v)"""
    memo = {}

    def get(dim):
        if dim not in memo:
            rng = np.random.default_rng(1700 + dim)
            raw = O.synth(0x5EED1700 + dim, 0, N, dim)
            v = O.synth(0x5EED1701 + dim, 0, 1, dim)[0]
            dup_at = np.sort(rng.choice(N, N_DUP, replace=False))
            raw[dup_at] = v
            vs = qa.VectorStorage(O.preprocess(O.COSINE, raw), qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
            memo[dim] = (vs, v, dup_at, O.synth(0x5EED1702 + dim, 0, 128, dim))
        return memo[dim]
    return get


def _queries(block, nq, hot):
    """the first nq cold queries with those at the places `hot` moved next to v"""
    _, v, _, cold = block
    queries = cold[:nq].copy()
    hot = np.asarray(hot, dtype=np.int64)
    if len(hot):
        queries[hot] = v + 0.05 * O.synth(0x5EED1703, 0, len(hot), len(v))
    return queries


def _passes(f, option, dim):
    """how often the conditional pass streams the block for f overflowed queries"""
    if f == 0:
        return 0
    if option == 1 and dim <= 768:
        return (f + 15) // 16
    fqt = 64 if dim <= 768 else 32
    return 1 if f <= 16 else (f + fqt - 1) // fqt


def _run(qa, searcher, settings):
    for name, value in settings.items():
        qa.set_option(name, value)
    try:
        got = searcher.peek_top_all()
        kernel = qa._ffi.last_kernel(searcher.scorer._h)
    finally:
        for name in settings:
            qa.set_option(name, -1)
    return got, searcher.counters, kernel


def _same(got, want, what=""):
    assert len(got) == len(want)
    for qi, (g, w) in enumerate(zip(got, want)):
        assert g["idx"].tolist() == w["idx"].tolist(), (what, qi)
        assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32)), (what, qi)


def _three(qa, vs, queries, top, f, dim, filters=None, verify_max=2048):
    """option 1, option 0 and the exact scan: the same lists, the same counters, f queries through the conditional pass; returns the exact scan's lists"""
    def searcher():
        s = qa.BatchFilteredSearcher(queries, vs, top)
        if filters is not None:
            s.scorer.set_filters(*filters)
        return s
    want, _, _ = _run(qa, searcher(), {"no_split_scan": 1})
    seen = []
    for option in (1, 0):
        got, c, kernel = _run(qa, searcher(), {OPTION: option, "verify_max_per_query": verify_max})
        assert "scan_i8copy_kernel" in kernel, kernel      # (what the search reports stays the prefilter's scan)
        _same(got, want, "%s=%d" % (OPTION, option))
        print("%s=%d, dim %d, %d queries, top %d: %s, bytes_read %d" % (OPTION, option, dim, len(queries), top,
                                                                         ", ".join("%s %d" % (k, getattr(c, k)) for k in COUNTERS), c.bytes_read))
        assert c.prefilter_queries == len(queries) and c.fallback_queries == f, (option, c.fallback_queries, f)
        seen.append({k: getattr(c, k) for k in COUNTERS + ("bytes_read",)})
    for k in COUNTERS:
        assert seen[0][k] == seen[1][k], (k, seen)
    block_bytes = N * dim * 4
    assert seen[0]["bytes_read"] - seen[1]["bytes_read"] == (_passes(f, 1, dim) - _passes(f, 0, dim)) * block_bytes, (seen, f)
    return want


@pytest.mark.parametrize("dim", [128, 768])
@pytest.mark.parametrize("f", [0, 1, 16, 17, 32, 33, 128])
def test_exactly_f_queries_overflow(qa, blocks, dim, f):
    block = blocks(dim)
    want = _three(qa, block[0], _queries(block, 128, range(f)), 10, f, dim)
    for w in want[:f]:      # the ten lowest ids among the copies of v: a mass of equal scores across the k-th place
        assert w["idx"].tolist() == block[2][:10].tolist()


@pytest.mark.parametrize("dim", [128, 768])
def test_a_small_batch_in_which_every_query_overflows(qa, blocks, dim):
    block = blocks(dim)
    _three(qa, block[0], _queries(block, 5, range(5)), 10, 5, dim)


@pytest.mark.parametrize("dim,nq,hot", [(128, 128, (0, 15, 16, 17, 31, 32, 63, 64, 65, 90, 111, 112, 126, 127, 5, 40, 41, 77, 100)),
                                        (768, 100, (99, 3, 50, 51, 52, 16, 80, 81, 7, 8, 9, 33, 34, 35, 36, 64, 65, 66, 67, 68, 97)),
                                        (128, 37, (36, 1))])
def test_overflowed_queries_scattered_over_the_batch(qa, blocks, dim, nq, hot):
    """packing, and the write-back through the packed list across group boundaries: 19 and 21 overflowed queries fill a group and start the next"""
    block = blocks(dim)
    want = _three(qa, block[0], _queries(block, nq, hot), 10, len(hot), dim)
    for qi in hot:
        assert want[qi]["idx"].tolist() == block[2][:10].tolist()
    cold = [qi for qi in range(nq) if qi not in hot]
    assert all(not np.isin(want[qi]["idx"], block[2]).all() for qi in cold)


@pytest.mark.parametrize("top", [1, 10, 64])
def test_top_1_10_64(qa, blocks, top):
    block = blocks(128)
    hot = (2, 3, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 60, 61, 62, 100, 127)
    want = _three(qa, block[0], _queries(block, 128, hot), top, len(hot), 128)
    for qi in hot:
        assert want[qi]["idx"].tolist() == block[2][:top].tolist()


def test_deleted_rows(qa, blocks):
    """a fifth of the rows deleted (points and vectors), the lowest copies of v among them: ~2 400 copies stay, still more than the verification list takes"""
    vs, _, dup_at, _ = block = blocks(128)
    rng = np.random.default_rng(171)
    deleted, vdel = rng.random(N) < 0.15, rng.random(N) < 0.05
    deleted[dup_at[:3]] = True
    vdel[dup_at[3:5]] = True
    live_dups = dup_at[~(deleted | vdel)[dup_at]]
    assert len(live_dups) > 2200
    hot = tuple(range(10, 40)) + (70, 127)
    vs.set_deleted(deleted, vdel)
    try:
        want = _three(qa, vs, _queries(block, 128, hot), 10, len(hot), 128)
    finally:
        vs.set_deleted(np.zeros(N, dtype=bool), np.zeros(N, dtype=bool))
    for qi in hot:
        assert want[qi]["idx"].tolist() == live_dups[:10].tolist()
    assert not (deleted | vdel)[np.concatenate([w["idx"] for w in want])].any()


def _sample_rows(n):
    """the sample of option i8_sample_scan (include/qdrant_amd.h): S = max(n >> 11, 8 192) rounded down to 16, T = S / 16 tiles, tile i = row tile i * ((n / 16) / T)"""
    S = min(n, max(n >> 11, 8192)) // 16 * 16
    T = S // 16
    step = (n // 16) // T
    return (16 * step * np.arange(T)[:, None] + np.arange(16)[None, :]).reshape(-1)


@pytest.mark.parametrize("dim", [128, 768])
def test_per_request_filters(qa, blocks, dim):
    """Bitmaps 0 and 1 allow no row of the sample: their queries have no bound and overflow - 40 of 100, every fifth and the one behind it, three groups
    of the packed pass - and they carry DIFFERENT bitmaps, which must follow them through the packing: the lists are the exact scan's under each
    query's own bitmap.  Bitmap 2 and "none" keep the prefilter."""
    block = blocks(dim)
    nq, top = 100, 10
    rng = np.random.default_rng(172)
    masks = np.stack([rng.random(N) < 0.5, rng.random(N) < 0.5, rng.random(N) < 0.3])
    masks[:2, _sample_rows(N)] = False
    filter_of = [(i % 5 if i % 5 < 3 else -1) for i in range(nq)]
    f = sum(1 for x in filter_of if x in (0, 1))
    want = _three(qa, block[0], _queries(block, nq, ()), top, f, dim, filters=(masks, filter_of), verify_max=0)
    for qi, w in enumerate(want):
        assert len(w) == top and (filter_of[qi] < 0 or masks[filter_of[qi]][w["idx"]].all()), qi
    # (the two bitmaps give different lists to the same query: a pass that mixed them up would not reproduce the exact scan's)
    assert any(not masks[1][want[qi]["idx"]].all() for qi in range(nq) if filter_of[qi] == 0)


@pytest.mark.parametrize("dim", [128, 768])
def test_one_handle_three_times(qa, blocks, dim):
    """overflow, no overflow, overflow on one query handle: a stale count, stale partial lists or stale flags would show in the middle search's
    lists (nobody overflows: the prefilter's lists must stand) or in the third's"""
    block = blocks(dim)
    hot = tuple(range(0, 40, 2)) + (127,)
    queries = _queries(block, 128, hot)
    want, _, _ = _run(qa, qa.BatchFilteredSearcher(queries, block[0], 10), {"no_split_scan": 1})
    for option in (1, 0):
        s = qa.BatchFilteredSearcher(queries, block[0], 10)
        for verify_max, f in ((2048, len(hot)), (0, 0), (2048, len(hot))):
            got, c, _ = _run(qa, s, {OPTION: option, "verify_max_per_query": verify_max})
            _same(got, want, "%s=%d, verify_max_per_query=%d" % (OPTION, option, verify_max))
            assert c.fallback_queries == f and c.prefilter_queries == 128, (option, verify_max, c.fallback_queries)


def test_1024_coordinates_keep_the_former_passes(qa, blocks):
    """the int8 scan leaves 31 744 B of LDS on its CU at 1 024 coordinates: the one-launch form does not fit, both option values run the 16- and 32-query
    passes (`bytes_read` is equal - _three asserts it with _passes(.., 1 024))"""
    block = blocks(1024)
    hot = (0, 1, 17, 18, 19, 30, 31, 32, 33, 50, 51, 52, 53, 54, 64, 65, 66, 90, 91, 127)
    want = _three(qa, block[0], _queries(block, 128, hot), 10, len(hot), 1024)
    for qi in hot:
        assert want[qi]["idx"].tolist() == block[2][:10].tolist()
