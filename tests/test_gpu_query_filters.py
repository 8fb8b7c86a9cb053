"""Per-request payload filters in one batch (qmx_query_set_filters): query i of a batch is held to bitmap filter_of[i] - or to none - and
the deleted flags, on every brute-force route and on the graph walks.

The expected value is always the same: query i returns what the oracle returns for that query alone over a storage whose deleted flags are
`deleted | ~mask[filter_of[i]]` (one oracle storage per filter class, not per query), compared as tests/parity_asserts.py compares brute-force lists
and as tests/test_gpu_hnsw.py compares walks.  In every case the device is also held against itself: the queries of class f inside the mixed batch
return exactly what a batch of just those queries returns under set_filter(mask[f]).

The filter classes used throughout: 0 an all-zero bitmap (empty lists), 1 fewer than `top` live rows, 2 / 3 / 4 keep rates 0.02 / 0.3 / 0.6, and
QMX_FILTER_NONE; the bitmaps are 37 bits shorter than the block (the tail is rejected), deleted flags lie on top, and the queries' classes are
interleaved.

The oracles of the quantized storages score one (query, row) pair per call from Python: over the blocks of 2^18 rows of the wide / prefilter routes they
score the LIVE rows of two queries per filter class (what the oracle returns for that query alone); every query of those batches is held against the
single-filter batch of its class, whose lists the route suites tie to the oracle.  That is narrower than "every query i against the oracle": on those
three routes the oracle answers two queries of each class, not all of them (every query of every other case is answered by it)."""
import ctypes as C

import numpy as np
import pytest

import oracle_ffi as O
from parity_asserts import assert_reference_lists

pytestmark = pytest.mark.gpu

TOP = 10
NONE = None
PATTERN = [2, NONE, 1, 3, 0, 4]          # the class of query i is PATTERN[i % 6]: interleaved, every class within any 6 queries
TAIL = 37                                # the bitmaps are this much shorter than the block


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


def _dist(qa, d):
    return {O.COSINE: qa.Distance.Cosine, O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid, O.MANHATTAN: qa.Distance.Manhattan}[d]


def _kernel(qa, searcher):
    return qa._ffi.last_kernel(searcher.scorer._h)


class World:
    """the deleted flags, the five bitmaps and the class of every query of one case; dead[f] = what query class f may not return"""

    def __init__(self, n, nq, seed, top=TOP, keep=(0.02, 0.3, 0.6), not_allowed=(), alive=()):
        """alive: rows that are not deleted and that classes 3 and 4 allow; not_allowed: rows that classes 2, 3 and 4 reject (the stronger of the two)"""
        rng = np.random.default_rng(seed)
        self.n, self.nq, self.n_bits = n, nq, n - TAIL
        self.deleted = rng.random(n) < 0.1
        self.vdel = rng.random(n) < 0.02
        self.deleted[list(alive)] = False
        self.vdel[list(alive)] = False
        gone = self.deleted | self.vdel
        m = np.zeros((5, self.n_bits), dtype=bool)
        live = np.flatnonzero(~gone[:self.n_bits])
        m[1, rng.choice(live, top - 4, replace=False)] = True          # fewer than `top` live rows ...
        m[1, np.flatnonzero(gone[:self.n_bits])[:5]] = True            # ... and a few dead ones
        for f, p in zip((2, 3, 4), keep):
            m[f] = rng.random(self.n_bits) < p
        for f in (3, 4):
            m[f, list(alive)] = True
        for f in (2, 3, 4):
            m[f, list(not_allowed)] = False
        self.masks = m
        self.full = np.zeros((5, n), dtype=bool)
        self.full[:, :self.n_bits] = m
        self.filter_of = [PATTERN[i % len(PATTERN)] for i in range(nq)]
        self.classes = [f for f in (0, 1, 2, 3, 4, NONE) if f in self.filter_of]

    def dead(self, f):
        return (self.deleted | self.vdel) if f is NONE else (self.deleted | self.vdel | ~self.full[f])

    def of_class(self, f):
        return [i for i, g in enumerate(self.filter_of) if g == f]

    def apply(self, storage, scorer):
        storage.set_deleted(self.deleted, self.vdel)
        scorer.set_filters(self.masks, self.filter_of)

    def dense_oracle(self, dtype, distance, rows, f):
        return O.DenseStorage(dtype, distance, rows, point_deleted=self.deleted | (~self.full[f] if f is not NONE else False), vec_deleted=self.vdel)


class PairOracle:
    """The oracle of a quantized storage behind the interface assert_reference_lists reads (peek_top / score_points / rows): `score(qidx, ids)` is the
    oracle's score_points of query number qidx; the lists are its scores of the LIVE rows, best first, the lower offset first among equal scores - what
    the oracle's queue returns for that query alone over a storage whose other rows are deleted."""

    def __init__(self, score, n, dead):
        self.score, self.live_ids, self.rows = score, np.flatnonzero(~dead).astype(np.uint32), np.empty((n, 0))

    def peek_top(self, qidx, top):
        out = []
        for qi in qidx:
            sc = self.score(int(qi), self.live_ids) if len(self.live_ids) else np.zeros(0, dtype=np.float32)
            order = np.lexsort((self.live_ids, -sc.astype(np.float64)))[:top]
            r = np.zeros(len(order), dtype=O.ScoredPointOffset)
            r["idx"], r["score"] = self.live_ids[order], sc[order]
            out.append(r)
        return out

    def score_points(self, qidx, ids):
        return np.stack([self.score(int(qi), np.asarray(ids, dtype=np.uint32)) for qi in qidx])


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["idx"].tolist() == w["idx"].tolist()
        assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32))


F16_REL = 1e-5      # the f16 kernels sum in another order than the reference's AVX leaf: within 1e-5 of sum |terms| (tests/test_gpu_dense_f16_u8.py)


def _f16_lists(got, orc, queries, top, live):
    """f16 rows of 32 and more elements: the oracle's lists up to that tolerance - every listed row is live and carries the oracle's score within it, the
    list is full and sorted, and no live row left out beats the last entry by more than it"""
    n = orc.rows.shape[0]
    ids_all = np.arange(n, dtype=np.uint32)
    q16 = orc.encode_queries(queries)
    sc = orc.score_points(queries, ids_all).astype(np.float64)
    v = O.f16_to_f32(orc.rows).astype(np.float64)
    for i, g in enumerate(got):
        tol = F16_REL * np.abs(O.f16_to_f32(q16[i]).astype(np.float64)[None, :] * v).sum(-1)
        gi = g["idx"].astype(np.int64)
        assert len(g) == min(top, int(live.sum())) and live[gi].all() and len(set(gi.tolist())) == len(gi)
        assert np.all(np.abs(g["score"].astype(np.float64) - sc[i][gi]) <= tol[gi]), i
        assert np.all(np.diff(g["score"]) <= 0)
        if len(g) == top:
            out = live.copy()
            out[gi] = False
            assert np.all(sc[i][out] <= float(g["score"][-1]) + tol[out] + tol[gi[-1]]), i


def _check_brute_force(qa, w, storage, queries, got, oracle_of, top=TOP, ids=None, oracle_queries=None):
    """got: the mixed batch's lists.  oracle_of(f) -> (oracle storage of class f, how it addresses queries: 'rows' = the vectors, 'index' = their numbers).
    oracle_queries: per class how many of its queries the oracle answers (None: all)."""
    assert len(got) == w.nq
    for f in w.classes:
        idx = w.of_class(f)
        sub = [got[i] for i in idx]
        dead = w.dead(f)
        if ids is not None:
            listed = np.zeros(w.n, dtype=bool)
            listed[ids] = True
            dead = dead | ~listed
        for r in sub:
            assert not dead[r["idx"]].any(), f
        n_live = int((~dead).sum())
        assert all(len(r) == min(top, n_live) for r in sub), (f, n_live, [len(r) for r in sub])
        # the oracle, one storage per class
        orc, how = oracle_of(f)
        k = len(idx) if oracle_queries is None else min(oracle_queries, len(idx))
        if how == "f16":
            _f16_lists(sub, orc, queries[idx], top, ~dead)
        elif ids is None:
            q_arg = queries[idx[:k]] if how == "rows" else np.asarray(idx[:k])
            assert_reference_lists(sub[:k], orc, q_arg, top, live=~dead, threads=8 if how == "rows" else 0)
        else:
            _same(sub[:k], orc.peek_top(queries[idx[:k]], top, ids=ids))
        # the device against itself: just these queries under the one filter of their class
        # (f16 rows: a batch of another size takes another kernel, which sums in another order - there the whole batch runs under the one filter)
        alone = qa.BatchFilteredSearcher(queries if how == "f16" else queries[idx], storage, top)
        alone.scorer.set_filter(None if f is NONE else w.masks[f])
        lists = alone.peek_top_all() if ids is None else alone.peek_top_iter(ids)
        _same(sub, [lists[i] for i in idx] if how == "f16" else lists)


# ---- 1. exact tiles ------------------------------------------------------------------------------------------------------------------------------
def _make_small(qa, kind, n, dim, seed, nq=0):
    """(device storage, queries, oracle_of(world) -> f -> (oracle, how)) of one storage kind over n rows"""
    dist = {"f32_cosine": O.COSINE, "f32_dot": O.DOT, "f32_euclid": O.EUCLID, "f32_manhattan": O.MANHATTAN, "tq_l1": O.MANHATTAN}.get(kind, O.COSINE if kind != "u8" else O.DOT)
    raw = O.synth(seed, 0, n, dim)
    nq = nq or (70 if dim == 256 else 20)
    queries = O.synth(seed + 1, 0, nq, dim)
    if kind.startswith("f32") or kind in ("f16", "u8"):
        dtype = O.F16 if kind == "f16" else O.U8 if kind == "u8" else O.F32
        if kind == "u8":
            rng = np.random.default_rng(seed)
            rows = rng.integers(0, 256, (n, dim), dtype=np.uint8)
            queries = rng.uniform(0.0, 255.0, (nq, dim)).astype(np.float32)
            st = qa.VectorStorage(rows, _dist(qa, dist), qa.VectorStorageDatatype.Uint8)
        elif kind == "f16":
            rows = O.to_f16(O.preprocess(dist, raw))
            st = qa.VectorStorage(rows.view(np.float16), _dist(qa, dist), qa.VectorStorageDatatype.Float16)
        else:
            rows = O.preprocess(dist, raw)
            st = qa.VectorStorage(rows, _dist(qa, dist))
        return st, queries, lambda w: (lambda f: (w.dense_oracle(dtype, dist, rows, f), "f16" if kind == "f16" else "rows"))
    vecs = O.preprocess(dist, raw)
    qpre = O.preprocess(dist, queries)
    if kind == "sq":
        quant = qa.ScalarQuantizer.from_min_max(vecs, dim, _dist(qa, dist))
        orc = O.SqOracle(dist, dim, quant.alpha, quant.offset)
        codes = quant.encode(vecs)
        orc.rows = codes
        st = qa.EncodedVectorsU8(codes, quant)
    elif kind == "pq":
        cen = O.PqOracle.train(vecs, dim, 4, 64, iters=3)
        orc = O.PqOracle(dist, dim, 4, cen)
        quant = qa.ProductQuantizer(dim, _dist(qa, dist), 4, cen)
        codes = quant.encode(vecs)
        orc.codes = codes
        st = qa.EncodedVectorsPQ(codes, quant)
    elif kind == "bq":
        quant = qa.BinaryQuantizer(dim, _dist(qa, dist))
        orc = O.BqOracle(dist, dim)
        orc.encode_rows(vecs)
        st = qa.EncodedVectorsBin(quant.encode(vecs), quant)
    else:
        assert kind in ("tq", "tq_l1")      # (over Manhattan: the score matrix, then one block per query selects - tq_l1_search)
        orc = O.TqOracle(dist, dim, O.TQ_BITS4)
        quant = qa.TurboQuantizer(dim, _dist(qa, dist), O.TQ_BITS4)
        codes = quant.encode(vecs)
        orc.rows = codes
        st = qa.EncodedVectorsTQ(codes, quant)
    score = lambda qi, ids: orc.score_points(qpre[qi:qi + 1], ids)[0]      # noqa: E731
    return st, queries, lambda w: (lambda f: (PairOracle(score, n, w.dead(f)), "index"))


SMALL = [("f32_cosine", 32), ("f32_dot", 32), ("f32_euclid", 32), ("f32_manhattan", 32), ("f16", 32), ("u8", 32), ("sq", 32), ("pq", 32), ("bq", 32),
         ("tq", 32), ("tq_l1", 32), ("f32_cosine", 256)]


@pytest.mark.parametrize("kind,dim", SMALL)
def test_exact_tiles_hold_every_query_to_its_own_filter(qa, kind, dim):
    """n = 3 000: the exact scans of every storage kind (20 queries at 32 coordinates: the VALU, 4x4x1 and int8 matrix-core epilogues, the PQ, BQ and
    TurboQuant kernels) and the chain-major f32 scan's 64-query shape (70 queries at 256 coordinates: a tile of 64, then one of 6 - a filter_of that
    does not move with the tile shows there)"""
    n = 3000
    st, queries, oracle_of = _make_small(qa, kind, n, dim, 0x5EEDF100 + dim + len(kind))
    w = World(n, len(queries), seed=len(kind) * 7 + dim)
    s = qa.BatchFilteredSearcher(queries, st, TOP)
    w.apply(st, s.scorer)
    got = s.peek_top_all()
    if dim == 256:      # (the batch's last kernel is the remainder tile's: the first tile alone names the 64-query scan, and returns the same lists)
        s64 = qa.BatchFilteredSearcher(queries[:64], st, TOP)
        s64.scorer.set_filters(w.masks, w.filter_of[:64])
        _same(got[:64], s64.peek_top_all())
        assert "scan_f32_mfma16_kernel" in _kernel(qa, s64) and _kernel(qa, s64).split("(")[0].endswith(", true>"), _kernel(qa, s64)      # (the instantiation for batches with per-request filters)
    _check_brute_force(qa, w, st, queries, got, oracle_of(w))
    # replaced by the one filter, then cleared: both calls undo the per-request filters
    s.scorer.set_filter(w.masks[4])
    _same(s.peek_top_all(), _alone(qa, st, queries, w.masks[4]))
    s.scorer.set_filter(None)
    _same(s.peek_top_all(), _alone(qa, st, queries, None))


def _alone(qa, st, queries, mask, top=TOP):
    a = qa.BatchFilteredSearcher(queries, st, top)
    a.scorer.set_filter(mask)
    return a.peek_top_all()


@pytest.mark.parametrize("dim,nq", [(24, 20), (24, 2), (32, 2), (32, 1), (32, 3)])
def test_short_rows_and_batches_of_one_to_three_queries(qa, dim, nq):
    """rows below 32 elements take the one-lane-per-row kernel (scan_small_kernel: blockIdx.y is the query); batches of 1, 2 and 3 queries the
    1-, 2- and 4-query instantiations of the tiled scan"""
    n = 3000
    st, queries, oracle_of = _make_small(qa, "f32_cosine", n, dim, 0x5EEDF1A0 + dim, nq=nq)
    w = World(n, nq, seed=dim + nq)
    s = qa.BatchFilteredSearcher(queries, st, TOP)
    w.apply(st, s.scorer)
    got = s.peek_top_all()
    assert ("scan_small_kernel" in _kernel(qa, s)) == (dim < 32), _kernel(qa, s)
    _check_brute_force(qa, w, st, queries, got, oracle_of(w))


def test_exact_tiles_over_a_candidate_id_list(qa):
    n, dim = 3000, 32
    st, queries, oracle_of = _make_small(qa, "f32_cosine", n, dim, 0x5EEDF180)
    w = World(n, len(queries), seed=91)
    ids = np.random.default_rng(4).choice(n, 1700, replace=False).astype(np.uint32)      # unsorted, with rows of the rejected tail
    s = qa.BatchFilteredSearcher(queries, st, TOP)
    w.apply(st, s.scorer)
    _check_brute_force(qa, w, st, queries, s.peek_top_iter(ids), oracle_of(w), ids=ids)


# ---- 2. the prefilter and wide routes ---------------------------------------------------------------------------------------------------------------
N_BIG = 300_000                       # >= 2^18: the prefilters apply


@pytest.fixture(scope="module")
def big_rows():
    return O.preprocess(O.COSINE, O.synth(0x5EEDF200, 0, N_BIG, 128)), O.synth(0x5EEDF201, 0, 130, 128)


def test_int8_copy_two_tiles_and_selective_filters(qa, big_rows):
    """130 queries over the int8 copy: tiles of 128 + 2 - the smallest shape at which a filter_of that is not offset with the tile shows"""
    rows, queries = big_rows
    nq = 130
    w = World(N_BIG, nq, seed=21)
    st = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    s = qa.BatchFilteredSearcher(queries, st, TOP)
    w.apply(st, s.scorer)
    got = s.peek_top_all()
    assert "scan_i8copy_kernel" in _kernel(qa, s), _kernel(qa, s)
    assert s.counters.prefilter_queries == nq
    print("int8 copy, classes 0 / <top / 0.02 / 0.3 / 0.6 / none: fallback_queries", s.counters.fallback_queries, "verified_rows", s.counters.verified_rows)
    _check_brute_force(qa, w, st, queries, got, lambda f: (w.dense_oracle(O.F32, O.COSINE, rows, f), "rows"))
    # filters that all keep >= 30 % of the rows: a few hundred live rows per query pass the sample's bound - nobody falls back
    w2 = World(N_BIG, nq, seed=22, keep=(0.3, 0.45, 0.6))
    w2.filter_of = [(2, 3, 4, NONE)[i % 4] for i in range(nq)]
    w2.classes = [2, 3, 4, NONE]
    w2.apply(st, s.scorer)
    got2 = s.peek_top_all()
    print("int8 copy, every filter keeps >= 30 %: fallback_queries", s.counters.fallback_queries, "verified_rows", s.counters.verified_rows)
    assert s.counters.prefilter_queries == nq and s.counters.fallback_queries == 0
    _check_brute_force(qa, w2, st, queries, got2, lambda f: (w2.dense_oracle(O.F32, O.COSINE, rows, f), "rows"))


@pytest.mark.parametrize("route,nq", [("f32_split", 70), ("half_copy", 70), ("split_copy", 70)])
def test_f16_split_routes(qa, big_rows, route, nq):
    """the f16-pair prefilter over the f32 rows themselves (65 and more queries: its epilogue tests liveness itself) and over the derived f16 copies
    (per-wave lists, regrouped per query)"""
    rows, queries = big_rows
    F = qa._ffi
    w = World(N_BIG, nq, seed=23 + nq)
    st = qa.VectorStorage(rows, qa.Distance.Cosine, flags={"f32_split": 0, "half_copy": F.SEG_HALF_COPY, "split_copy": F.SEG_SPLIT_COPY}[route])
    s = qa.BatchFilteredSearcher(queries[:nq], st, TOP)
    w.apply(st, s.scorer)
    got = s.peek_top_all()
    assert ("scan_f32_split_kernel" if route == "f32_split" else "scan_f16pair_kernel") in _kernel(qa, s), _kernel(qa, s)
    assert s.counters.prefilter_queries == nq
    _check_brute_force(qa, w, st, queries[:nq], got, lambda f: (w.dense_oracle(O.F32, O.COSINE, rows, f), "rows"))


N_ODD = 262_144 + 1_111               # n % 4 == 3, not a multiple of the 256-row tile (tests/test_gpu_sq_wide.py)


def _clustered(n, dim, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((64, dim)).astype(np.float32)
    vecs = (centres[rng.integers(0, 64, n)] * rng.uniform(0.5, 2.0, (n, 1)) + 0.5 * rng.standard_normal((n, dim))).astype(np.float32)
    return rng, O.preprocess(O.DOT, vecs)


@pytest.mark.parametrize("route", ["sq_wide", "tq_wide", "pq_prefilter"])
def test_quantized_wide_and_prefilter_routes(qa, route):
    """SQ wide, TurboQuant wide and the PQ prefilter at their minimum batches (33, 33, 4 queries)"""
    n = N_ODD
    assert n % 4 == 3
    dim = 256 if route == "tq_wide" else 128
    rng, vecs = _clustered(n, dim, 31 + len(route))
    dist = O.DOT
    if route == "sq_wide":
        nq, kern = int(qa.get_option("sq_wide_min_queries")), "scan_sqw_kernel"
        quant = qa.ScalarQuantizer.from_min_max(vecs[:20000], dim, qa.Distance.Dot)
        orc = O.SqOracle(dist, dim, quant.alpha, quant.offset)
        codes = quant.encode(vecs)
        orc.rows = codes
        st = qa.EncodedVectorsU8(codes, quant)
    elif route == "tq_wide":
        nq, kern = int(qa.get_option("tq_wide_min_queries")), "scan_tq4w_kernel"
        orc = O.TqOracle(dist, dim, O.TQ_BITS4)
        quant = qa.TurboQuantizer(dim, qa.Distance.Dot, O.TQ_BITS4)
        codes = quant.encode(vecs)
        orc.rows = codes
        st = qa.EncodedVectorsTQ(codes, quant)
    else:
        nq, kern = int(qa.get_option("pq_prefilter_min_queries")), "pq_prefilter_kernel"
        cen = O.PqOracle.train(vecs[:3000], dim, 8, 256, iters=3)
        orc = O.PqOracle(dist, dim, 8, cen)
        quant = qa.ProductQuantizer(dim, qa.Distance.Dot, 8, cen)
        codes = quant.encode(vecs)
        orc.codes = codes
        st = qa.EncodedVectorsPQ(codes, quant)
    assert nq == (4 if route == "pq_prefilter" else 33)
    queries = (vecs[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, dim))).astype(np.float32)
    qpre = O.preprocess(dist, queries)
    w = World(n, nq, seed=41 + len(route))
    s = qa.BatchFilteredSearcher(queries, st, TOP)
    w.apply(st, s.scorer)
    got = s.peek_top_all()
    assert kern in _kernel(qa, s), _kernel(qa, s)
    assert s.counters.prefilter_queries == nq
    score = lambda qi, ids: orc.score_points(qpre[qi:qi + 1], ids)[0]      # noqa: E731
    _check_brute_force(qa, w, st, queries, got, lambda f: (PairOracle(score, n, w.dead(f)), "index"), oracle_queries=2)


# ---- 3. the packed exact passes of overflowed queries -------------------------------------------------------------------------------------------------
def test_packed_overflow_passes_carry_each_query_s_filter(qa):
    """The mass-tie block of test_int8_copy_falls_back_when_scores_tie_in_masses (every row 30 000 times, 70 queries): the queries whose lists overflow are
    re-scanned packed, in another order than the batch's - each must keep its own bitmap.  Every result score is a mass of ties: the lists are the LOWEST
    live offsets of each query."""
    dim, nq, rep = 128, 70, 30_000
    base = O.preprocess(O.COSINE, O.synth(0x5EED0730, 0, N_BIG // rep, dim))
    rows = np.tile(base, (rep, 1))
    n = rows.shape[0]
    queries = O.synth(0x5EED0731, 0, nq, dim)
    w = World(n, nq, seed=51)
    st = qa.VectorStorage(rows, qa.Distance.Cosine, flags=qa._ffi.SEG_I8_COPY)
    s = qa.BatchFilteredSearcher(queries, st, TOP)
    w.apply(st, s.scorer)
    got = s.peek_top_all()
    assert "scan_i8copy_kernel" in _kernel(qa, s)
    assert s.counters.prefilter_queries == nq and 0 < s.counters.fallback_queries <= nq
    _check_brute_force(qa, w, st, queries, got, lambda f: (w.dense_oracle(O.F32, O.COSINE, rows, f), "rows"))
    # the lowest live offsets, spelled out: the rows of a result score are the copies base_row + k * (n / rep) of one base row
    n_base = n // rep
    for i in (1, 3, 5):                     # classes none, 0.3, 0.6
        dead = w.dead(w.filter_of[i])
        best = int(got[i]["idx"][0]) % n_base
        copies = np.arange(best, n, n_base)
        want = copies[~dead[copies]][:(got[i]["score"] == got[i]["score"][0]).sum()]
        assert got[i]["idx"][:len(want)].tolist() == want.tolist()


# ---- 4. the graph walks ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph_world():
    n, dim, m, nq = 3000, 32, 8, 20
    rows = O.preprocess(O.COSINE, O.synth(0x5EEDF400, 0, n, dim))
    st = O.DenseStorage(O.F32, O.COSINE, rows)
    g = O.Hnsw(st, m=m, ef_construct=64, seed=7, threads=0)
    plain = g.export_plain()
    queries = O.synth(0x5EEDF401, 0, nq, dim)
    # classes 2, 3 and 4 reject every entry point of the graph's list (one, here); get_entry_point then takes the live extra entry point of the highest
    # level, which classes 3 and 4 allow - the searches of those classes start elsewhere than their neighbours in the batch
    eps, xps = [int(i) for i in plain.ep_ids], [int(i) for i in plain.xp_ids]
    assert eps and xps and max(eps + xps) < n - TAIL
    w = World(n, nq, seed=61, not_allowed=eps, alive=eps + xps)
    assert not any(w.full[f][eps].any() for f in range(5)) and not w.dead(NONE)[eps].any() and not w.dead(3)[xps].any() and not w.dead(4)[xps].any()
    return rows, g, plain, queries, w


def _same_modulo_ties(got, want):
    """tests/test_gpu_hnsw.py: score lists bit-equal; ids equal wherever the score is unique in the list and above the last (boundary) score"""
    for g, x in zip(got, want):
        assert np.array_equal(g["score"].view(np.uint32), x["score"].view(np.uint32))
        sc = x["score"]
        for i in range(len(x)):
            if (sc == sc[i]).sum() == 1 and sc[i] != sc[-1]:
                assert g["idx"][i] == x["idx"][i]


@pytest.mark.parametrize("acorn", [False, True])
def test_dense_walks_hold_every_search_to_its_own_filter(qa, graph_world, acorn):
    rows, g, plain, queries, w = graph_world
    top, ef = TOP, 64
    vs = qa.VectorStorage(rows, qa.Distance.Cosine)
    scorer = qa.new_raw_scorer(queries, vs)
    w.apply(vs, scorer)
    graph = qa.GraphLayers.from_plain(plain)
    got, scored = graph.search(top, ef, scorer, with_scored=True, acorn=acorn)
    want_scored = 0
    g.algorithm = 1 if acorn else 0
    try:
        for f in w.classes:
            idx = w.of_class(f)
            want, stats = g.search_dense(w.dense_oracle(O.F32, O.COSINE, rows, f), queries[idx], top, ef, with_stats=True)
            want_scored += sum(stats)
            sub = [got[i] for i in idx]
            _same_modulo_ties(sub, want)
            for r in sub:
                assert not w.dead(f)[r["idx"]].any()
            if f in (3, 4):       # every entry point of these searches is rejected by their filter: they still return their live result
                assert all(len(r) == top for r in sub), f
            # the device against itself
            alone = qa.new_raw_scorer(queries[idx], vs)
            alone.set_filter(None if f is NONE else w.masks[f])
            _same(sub, graph.search(top, ef, alone, acorn=acorn))
    finally:
        g.algorithm = 0
    assert scored == want_scored
    assert all(len(got[i]) == 0 for i in w.of_class(0))
    # the asynchronous and the traced call walk the same walk
    import torch
    F = qa._ffi
    nq = len(queries)
    if not acorn:
        out = torch.zeros((nq, top, 2), dtype=torch.int32, device="cuda")
        counts = torch.zeros(nq, dtype=torch.int32, device="cuda")
        F.check(F.lib().qmx_hnsw_search_async(graph._h, scorer._h, top, ef, F.ptr(out), F.ptr(counts), None))
        F.check(F.lib().qmx_query_synchronize(scorer._h))
        o, c = out.cpu().numpy(), counts.cpu().numpy()
        for i in range(nq):
            assert int(c[i]) == len(got[i]) and o[i, :c[i], 0].view(np.uint32).tolist() == got[i]["idx"].tolist()
        traced, _pops = graph.search_traced(top, ef, scorer)
        _same(traced, got)


@pytest.mark.parametrize("acorn", [False, True])
def test_sq_walks_and_the_graph_stage_of_search_quantized(qa, graph_world, acorn):
    rows, g, plain, queries, w = graph_world
    top, ef, dim = TOP, 64, rows.shape[1]
    qpre = O.preprocess(O.COSINE, queries)
    quant = qa.ScalarQuantizer.from_min_max(rows, dim, qa.Distance.Cosine)
    osq = O.SqOracle(O.COSINE, dim, quant.alpha, quant.offset)
    osq.encode_rows(rows)
    enc = qa.EncodedVectorsU8(quant.encode(rows), quant)
    scorer = qa.new_raw_scorer(queries, enc)
    w.apply(enc, scorer)
    graph = qa.GraphLayers.from_plain(plain)
    got = graph.search(top, ef, scorer, acorn=acorn)
    g.algorithm = 1 if acorn else 0
    try:
        for f in w.classes:
            idx = w.of_class(f)
            want = g.search_sq(w.dense_oracle(O.F32, O.COSINE, rows, f), osq, qpre[idx], top, ef)
            sub = [got[i] for i in idx]
            _same_modulo_ties(sub, want)
            for r in sub:
                assert not w.dead(f)[r["idx"]].any()
            alone = qa.new_raw_scorer(queries[idx], enc)
            alone.set_filter(None if f is NONE else w.masks[f])
            _same(sub, graph.search(top, ef, alone, acorn=acorn))
    finally:
        g.algorithm = 0
    if not acorn:
        # integer scores tie, and which of two equal candidates a walk expands is the heap's choice: with the reference's heaps on the device (a mode of
        # the plain walk only) lists and the number of scored points are the oracle's, search by search
        qa.set_option("hnsw_reference_heap_order", 1)
        try:
            exact, scored = graph.search(top, ef, scorer, with_scored=True)
        finally:
            qa.set_option("hnsw_reference_heap_order", -1)
        want_scored = 0
        for f in w.classes:
            idx = w.of_class(f)
            st_f = w.dense_oracle(O.F32, O.COSINE, rows, f)
            for i in idx:
                codes, off = osq.encode_query(qpre[i])
                sc = O.Scorer()
                sc.kind, sc.st, sc.sq, sc.sq_rows = 1, C.pointer(st_f.st), C.pointer(osq.sq), osq.rows.ctypes.data
                sc.sq_query, sc.sq_query_offset, sc.isa = codes.ctypes.data, off, osq.isa
                want, n_scored = g._run(sc, top, ef)      # (Hnsw.search_sq, keeping the walk's count of scored points)
                want_scored += n_scored
                _same([exact[i]], [want])
        assert scored == want_scored
    # qmx_search_quantized: the walk of the quantized batch under ITS per-request filters, oversampled, then the raw batch's exact scores
    vs = qa.VectorStorage(rows, qa.Distance.Cosine)
    raw = qa.new_raw_scorer(queries, vs)
    fused = qa.search_quantized(scorer, raw, top, oversampling=2.0, rescore=True, graph=graph, hnsw_ef=ef, acorn=acorn)
    walk = graph.search(2 * top, ef, scorer, acorn=acorn)
    ids = np.zeros((len(queries), 2 * top), dtype=np.uint32)
    cnt = np.zeros(len(queries), dtype=np.uint32)
    for i, r in enumerate(walk):
        ids[i, :len(r)] = r["idx"]
        cnt[i] = len(r)
        assert not w.dead(w.filter_of[i])[r["idx"]].any()
    for a_, b_ in zip(fused, raw.rescore(ids, top, cnt)):
        assert np.array_equal(a_, b_)


def test_pq_walk_takes_the_per_query_instantiation_of_its_own_policy(qa, graph_world):
    """every single-vector hop policy has a per-request instantiation (HopPerQuery<H>, picked by launch_hnsw_hop); the PQ walk stands for the quantized ones:
    lists and the number of scored points are the oracle's, class by class"""
    rows, g, plain, queries, w = graph_world
    top, ef, dim = TOP, 64, rows.shape[1]
    qpre = O.preprocess(O.COSINE, queries)
    cen = O.PqOracle.train(rows, dim, 4, 64, iters=3)
    opq = O.PqOracle(O.COSINE, dim, 4, cen)
    quant = qa.ProductQuantizer(dim, qa.Distance.Cosine, 4, cen)
    codes = quant.encode(rows)
    opq.codes = codes
    enc = qa.EncodedVectorsPQ(codes, quant)
    scorer = qa.new_raw_scorer(queries, enc)
    w.apply(enc, scorer)
    graph = qa.GraphLayers.from_plain(plain)
    got, scored = graph.search(top, ef, scorer, with_scored=True)
    want_scored = 0
    for f in w.classes:
        idx = w.of_class(f)
        want, stats = g.search_pq(w.dense_oracle(O.F32, O.COSINE, rows, f), opq, qpre[idx], top, ef, with_stats=True)
        want_scored += sum(stats)
        sub = [got[i] for i in idx]
        _same_modulo_ties(sub, want)
        for r in sub:
            assert not w.dead(f)[r["idx"]].any()
        alone = qa.new_raw_scorer(queries[idx], enc)
        alone.set_filter(None if f is NONE else w.masks[f])
        _same(sub, graph.search(top, ef, alone))
    assert scored == want_scored
    assert "HopPerQuery" in qa._ffi.last_kernel(scorer._h), qa._ffi.last_kernel(scorer._h)


# ---- 5. the calls that do not serve per-request filters refuse them ---------------------------------------------------------------------------------
def test_unsupported_calls_refuse_per_request_filters_and_work_again_once_cleared(qa, graph_world):
    rows, g, plain, queries, w = graph_world
    n, dim = rows.shape
    nq = len(queries)
    F = qa._ffi
    lib = F.lib()
    vs = qa.VectorStorage(rows, qa.Distance.Cosine)
    graph = qa.GraphLayers.from_plain(plain)
    scorer = qa.new_raw_scorer(queries, vs)
    base = qa.new_raw_scorer(queries, vs)
    keys = qa.GroupKeys(n, np.arange(n, dtype=np.uint32) % 50)
    custom = qa.CustomRawScorer([qa.CustomQuery.recommend_best_score([rows[0], rows[1]], [rows[2]]), qa.CustomQuery.recommend_best_score([rows[3]], [])], vs)
    n_ex = custom.examples.nq
    out = np.zeros((nq, TOP), dtype=O.ScoredPointOffset)
    counts = np.zeros(nq, dtype=np.uint32)
    first = np.arange(nq + 1, dtype=np.uint32)            # every query one token, every inner row its own point: the dense search again
    efirst = np.arange(n_ex + 1, dtype=np.uint32)
    offsets = np.arange(n + 1, dtype=np.uint64)
    ex = custom.examples
    calls = {      # name -> (the batch that carries the filters, the call)
        "search_with_vectors (links)": (scorer, lambda: graph.search_with_vectors(TOP, 64, scorer, base)),
        "search_with_vectors (base)": (base, lambda: graph.search_with_vectors(TOP, 64, scorer, base)),
        "group_search": (scorer, lambda: qa.search_groups(scorer, None, keys, 3, 2)),
        "custom_search_topk": (ex, lambda: custom.peek_top(TOP)),
        "custom_hnsw_search": (ex, lambda: custom.search_hnsw(graph, TOP, 64)),
        "multi_search_topk": (scorer, lambda: F.check(lib.qmx_multi_search_topk(scorer._h, F.ptr(first), nq, F.ptr(offsets), n, None, 0, TOP, None, 0, F.ptr(out),
                                                                                F.ptr(counts)))),
        "multi_hnsw_search": (scorer, lambda: F.check(lib.qmx_multi_hnsw_search(graph._h, scorer._h, F.ptr(first), nq, F.ptr(offsets), n, None, 0, TOP, 64, F.ptr(out),
                                                                                F.ptr(counts), None))),
        "multi_custom_search_topk": (ex, lambda: F.check(lib.qmx_multi_custom_search_topk(ex._h, F.ptr(efirst), n_ex, custom._descs, custom.nq, F.ptr(offsets), n, None,
                                                                                          0, TOP, None, 0, F.ptr(out), F.ptr(counts)))),
        "multi_custom_hnsw_search": (ex, lambda: F.check(lib.qmx_multi_custom_hnsw_search(graph._h, ex._h, F.ptr(efirst), n_ex, custom._descs, custom.nq, F.ptr(offsets),
                                                                                          n, None, 0, TOP, 64, F.ptr(out), F.ptr(counts), None))),
    }
    # a sparse batch, and custom queries over sparse examples
    rng = np.random.default_rng(5)
    srows = [(np.sort(rng.choice(50, 6, replace=False)).astype(np.uint32), rng.standard_normal(6).astype(np.float32)) for _ in range(200)]
    sparse = qa.SparseVectorStorage(srows)
    sq = qa.new_raw_scorer(srows[:3], sparse)
    sout = np.zeros((3, 5), dtype=O.ScoredPointOffset)
    scounts = np.zeros(3, dtype=np.uint32)
    scustom = qa.CustomRawScorer([qa.CustomQuery.recommend_best_score([srows[0]], [srows[1]])], sparse)
    calls["sparse search_topk"] = (sq, lambda: F.check(lib.qmx_search_topk(sq._h, 5, None, 0, F.ptr(sout), F.ptr(scounts), None, None)))
    calls["sparse_custom_search_topk"] = (scustom.examples, lambda: scustom.peek_top(5))
    for name, (batch, call) in calls.items():
        call()                                             # served without filters ...
        n_points = 200 if "sparse" in name else n
        batch.set_filters(np.ones((2, n_points), dtype=bool), [i % 2 for i in range(batch.nq)])
        with pytest.raises(F.QmxError) as e:               # ... refused with them, never served without applying them ...
            call()
        assert e.value.status == F.ERR_NOT_SUPPORTED and "per-request filters" in str(e.value), (name, e.value)
        batch.set_filter(None)
        call()                                             # ... and served again once they are cleared
    assert scounts.tolist() == [5, 5, 5]
    # the scoring calls ignore filters, as they ignore the one filter
    scorer.set_filters(np.zeros((1, n), dtype=bool), [0] * nq)
    want = qa.new_raw_scorer(queries, vs).score_points([1, 2, 3])
    assert np.array_equal(scorer.score_points([1, 2, 3]), want)


# ---- 6. bad arguments -------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(qa):
    F = qa._ffi
    lib = F.lib()
    n, dim, nq = 500, 32, 6
    rows = O.preprocess(O.COSINE, O.synth(0x5EEDF600, 0, n, dim))
    queries = O.synth(0x5EEDF601, 0, nq, dim)
    vs = qa.VectorStorage(rows, qa.Distance.Cosine)
    s = qa.BatchFilteredSearcher(queries, vs, TOP)
    want = s.peek_top_all()
    masks = np.ones((2, n), dtype=bool)
    words, n_bits, n_filters, fof = qa.pack_filters(masks, [0, 1, NONE, 0, 1, NONE], nq)
    bad = fof.copy()
    bad[4] = 2                                   # == n_filters
    assert lib.qmx_query_set_filters(s.scorer._h, F.ptr(words), n_bits, n_filters, F.ptr(bad)) == F.ERR_OUT_OF_BOUNDS
    assert "filter_of_query[4]" in F.last_error()
    assert lib.qmx_query_set_filters(s.scorer._h, F.ptr(words), n_bits, 0, F.ptr(fof)) == F.ERR_BAD_ARG
    assert lib.qmx_query_set_filters(s.scorer._h, None, n_bits, n_filters, F.ptr(fof)) == F.ERR_BAD_ARG
    assert lib.qmx_query_set_filters(s.scorer._h, F.ptr(words), n_bits, n_filters, None) == F.ERR_BAD_ARG
    assert lib.qmx_query_set_filters(None, F.ptr(words), n_bits, n_filters, F.ptr(fof)) == F.ERR_BAD_ARG
    with pytest.raises(ValueError):
        s.scorer.set_filters(masks, [0, 1])      # one entry per query
    # a refused call leaves the batch as it was: no filter
    _same(s.peek_top_all(), want)
    # device memory for both arrays
    import torch
    masks[0, ::2] = False
    words, n_bits, n_filters, fof = qa.pack_filters(masks, [0, 1, NONE, 0, 1, NONE], nq)
    d_words = torch.from_numpy(words.view(np.int64)).cuda()
    d_fof = torch.from_numpy(fof.view(np.int32)).cuda()
    F.check(lib.qmx_query_set_filters(s.scorer._h, F.ptr(d_words), n_bits, n_filters, F.ptr(d_fof)))
    got = s.peek_top_all()
    s.scorer.set_filters(masks, [0, 1, NONE, 0, 1, NONE])
    _same(got, s.peek_top_all())
    assert all((r["idx"] % 2 == 1).all() for r in (got[0], got[3])) and not all((r["idx"] % 2 == 1).all() for r in (got[1], got[2]))
