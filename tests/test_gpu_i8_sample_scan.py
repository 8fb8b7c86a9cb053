"""Option `i8_sample_scan` (default 1): the int8 prefilter takes its first bound from the int8 copy itself.  Its sample is T = S / 16 whole 16-row
tiles of the block (include/qdrant_amd.h states which; restated in `_sample_rows` below), scored by scan_i8copy_sample_kernel
(qdrant_amd/csrc/scan_i8copy.hip); the k best live sample rows of each query are scored exactly, and the smallest of those scores is the bound.
0 = the exact f32 scores of every (n / S)-th row, as before.

Every case compares ids and score bits with the exact scan (`no_split_scan` = 1) and between the two option values.  The candidate and
verified-row counters are printed, not compared: the two samples differ.

Blocks of 2^18 rows (the smallest the prefilter takes) and of 270 011 (a ragged last tile).  The inputs of the plain cases were checked against the
first launch's list capacity by running them: `fallback_queries == 0` is what an overflow would break."""
import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

N18, N_RAGGED = 1 << 18, 270_011
OPTION = "i8_sample_scan"


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    assert qdrant_amd.get_option("prescan_shift") == 10 and qdrant_amd.get_option("i8_sample_rows") == 0      # the defaults `_sample_rows` restates
    return qdrant_amd


def _sample_rows(n):
    """the rule of the header: S = max(n >> 11, 8 192) rounded down to 16, T = S / 16 tiles, tile i = row tile i * ((n / 16) / T)"""
    S = min(n, max(n >> 11, 8192)) // 16 * 16
    T = S // 16
    step = (n // 16) // T
    return (16 * step * np.arange(T)[:, None] + np.arange(16)[None, :]).reshape(-1)


def _search(qa, queries, vs, top, option=None, exact=False, allowed=None, filters=None):
    """lists and counters of one search: option = the value of i8_sample_scan, or exact = the exact scan"""
    name, value = ("no_split_scan", 1) if exact else (OPTION, option)
    qa.set_option(name, value)
    try:
        s = qa.BatchFilteredSearcher(queries, vs, top)
        if allowed is not None:
            s.scorer.set_filter(allowed)
        if filters is not None:
            s.scorer.set_filters(*filters)
        got = s.peek_top_all()
        kernel = qa._ffi.last_kernel(s.scorer._h)
    finally:
        qa.set_option(name, -1)
    assert exact or "scan_i8copy_kernel" in kernel, kernel
    return got, s.counters


def _same(got, want, what=""):
    assert len(got) == len(want)
    for qi, (g, w) in enumerate(zip(got, want)):
        assert g["idx"].tolist() == w["idx"].tolist(), (what, qi)
        assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32)), (what, qi)


def _both(qa, queries, vs, top, want, **kw):
    """both option values against the exact scan's lists `want`; returns the two counter sets"""
    out = []
    for option in (0, 1):
        got, c = _search(qa, queries, vs, top, option=option, **kw)
        _same(got, want, "i8_sample_scan=%d" % option)
        assert c.prefilter_queries == len(queries)
        print("i8_sample_scan=%d, %d queries, top %d: prefilter_candidates %d, verified_rows %d, fallback_queries %d"
              % (option, len(queries), top, c.prefilter_candidates, c.verified_rows, c.fallback_queries))
        out.append(c)
    return out


@pytest.fixture(scope="module")
def raw_rows():
    """iid rows per row length, generated once (270 011 of them; the 2^18-row block is their prefix) and left unchanged"""
    memo = {}

    def get(dim):
        if dim not in memo:
            raw = O.synth(0x5EED1600 + dim, 0, N_RAGGED, dim)
            memo[dim] = (raw, O.preprocess(O.COSINE, raw))
        return memo[dim]
    return get


# one, six and eight stages under the resident scan (64 / 64 / 16 queries per block of the sample kernel), nine under the staged scan; the short rows
# with both block sizes and both distances, the long ones with one of each
PLAIN = [(128, N18, "cosine"), (128, N_RAGGED, "dot"), (128, N18, "dot"), (128, N_RAGGED, "cosine"),
         (768, N_RAGGED, "cosine"), (768, N18, "dot"), (1024, N18, "cosine"), (1024, N_RAGGED, "dot"), (1152, N_RAGGED, "cosine"), (1152, N18, "dot")]


@pytest.mark.parametrize("dim,n,distance", PLAIN)
def test_plain_blocks(qa, raw_rows, dim, n, distance):
    """nq 1 .. 130 (130: a second tile of two queries) x top 1, 10, 64: the exact scan's lists, nobody falls back"""
    raw, cos = raw_rows(dim)
    rows = np.ascontiguousarray((cos if distance == "cosine" else raw)[:n])
    dist = qa.Distance.Cosine if distance == "cosine" else qa.Distance.Dot
    queries = O.synth(0x5EED1601 + dim, 0, 130, dim)
    vs = qa.VectorStorage(rows, dist, flags=qa._ffi.SEG_I8_COPY)
    for top in (1, 10, 64):
        want, _ = _search(qa, queries, vs, top, exact=True)
        for nq in (1, 16, 17, 64, 65, 128, 130):
            for c in _both(qa, queries[:nq], vs, top, want[:nq]):
                assert c.fallback_queries == 0 and c.prefilter_candidates > 0, (nq, top)


@pytest.fixture(scope="module")
def block128(qa, raw_rows):
    rows = np.ascontiguousarray(raw_rows(128)[1][:N18])
    return rows, O.synth(0x5EED1620, 0, 128, 128)


def test_the_sample_is_the_tiles_the_header_names(qa, block128):
    rows, queries = block128
    n, nq, top = N18, 48, 10
    queries = queries[:nq]
    sample = _sample_rows(n)
    assert len(sample) == 8192 and sample[16] == 512 and sample[-1] == 511 * 512 + 15
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    # exactly the sample deleted, then all of it but five rows (fewer than top): no bound, every query takes the exact scan
    for keep in (0, 5):
        deleted = np.zeros(n, dtype=bool)
        deleted[sample] = True
        deleted[sample[1000:1000 + keep]] = False
        vs.set_deleted(deleted, None)
        want, _ = _search(qa, queries, vs, top, exact=True)
        got, c = _search(qa, queries, vs, top, option=1)
        _same(got, want)
        assert c.fallback_queries == nq, (keep, c.fallback_queries)
    # every 32nd row deleted - the other option's whole sample at this size: this one keeps its bound, that one loses it
    deleted = np.zeros(n, dtype=bool)
    deleted[::32] = True
    vs.set_deleted(deleted, None)
    want, _ = _search(qa, queries, vs, top, exact=True)
    c0, c1 = _both(qa, queries, vs, top, want)
    assert c1.fallback_queries == 0 and c0.fallback_queries == nq


def test_deleted_rows(qa, block128):
    rows, queries = block128
    rng = np.random.default_rng(16)
    deleted, vdel = rng.random(N18) < 0.15, rng.random(N18) < 0.05
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    vs.set_deleted(deleted, vdel)
    want, _ = _search(qa, queries, vs, 10, exact=True)
    assert not (deleted | vdel)[np.concatenate([w["idx"] for w in want])].any()
    for c in _both(qa, queries, vs, 10, want):
        assert c.fallback_queries == 0


def test_per_request_filters(qa, block128):
    """Three bitmaps and "none", interleaved.  Bitmap 0 allows no row of the sample: its queries have no bound and take the exact scan - they alone, so
    every query's bound came from the live sample rows of its own bitmap."""
    rows, queries = block128
    nq, top = 100, 10
    queries = queries[:nq]
    rng = np.random.default_rng(61)
    masks = np.stack([rng.random(N18) < 0.5, rng.random(N18) < 0.5, rng.random(N18) < 0.3])
    masks[0, _sample_rows(N18)] = False
    filter_of = [(-1 if i % 4 == 3 else i % 4) for i in range(nq)]
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    want, _ = _search(qa, queries, vs, top, exact=True, filters=(masks, filter_of))
    for qi, w in enumerate(want):
        assert filter_of[qi] < 0 or masks[filter_of[qi]][w["idx"]].all(), qi
    got, c = _search(qa, queries, vs, top, option=1, filters=(masks, filter_of))
    _same(got, want)
    assert c.fallback_queries == sum(1 for f in filter_of if f == 0), c.fallback_queries
    got, c = _search(qa, queries, vs, top, option=0, filters=(masks, filter_of))
    _same(got, want)
    print("filters: fallback_queries %d with option 0" % c.fallback_queries)


def test_a_block_of_equal_rows(qa):
    n, dim, nq, top = N18, 128, 20, 10
    unit = O.preprocess(O.COSINE, O.synth(0x5EED1630, 0, 1, dim))
    rows = np.tile(unit, (n, 1))
    queries = O.synth(0x5EED1631, 0, nq, dim)
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    want, _ = _search(qa, queries, vs, top, exact=True)
    for w in want:
        assert w["idx"].tolist() == list(range(top))
    _both(qa, queries, vs, top, want)


def test_a_sample_of_copies_of_one_row(qa, block128):
    """8 192 equal approximate scores per query: more survivors than the top-k's list holds, it takes its insertion walk"""
    rows, queries = block128
    rows = rows.copy()
    rows[_sample_rows(N18)] = rows[7]
    vs = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    want, _ = _search(qa, queries, vs, 10, exact=True)
    _, c1 = _both(qa, queries, vs, 10, want)
    assert c1.prefilter_candidates > 0


def test_queries_that_are_not_finite(qa, raw_rows):
    """A NaN and an infinite query take the exact scan alone; the others keep the prefilter"""
    rows = np.ascontiguousarray(raw_rows(128)[1][:N18])
    nq, top = 96, 10
    queries = O.synth(0x5EED1640, 0, nq, 128)
    queries[5, 17] = np.nan
    queries[40, 3] = np.inf
    vs = qa.VectorStorage(rows, qa.Distance.Dot, flags=qa._ffi.SEG_I8_COPY)
    want, _ = _search(qa, queries, vs, top, exact=True)
    for option in (0, 1):
        got, c = _search(qa, queries, vs, top, option=option)
        for qi, (g, w) in enumerate(zip(got, want)):
            assert g["idx"].tolist() == w["idx"].tolist(), (option, qi)
            if qi in (5, 40):
                assert np.array_equal(np.isnan(g["score"]), np.isnan(w["score"])) and np.array_equal(np.isposinf(g["score"]), np.isposinf(w["score"]))
            else:
                assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32)), (option, qi)
        assert c.prefilter_queries == nq and 2 <= c.fallback_queries <= 4, (option, c.fallback_queries)
