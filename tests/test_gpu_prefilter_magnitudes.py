"""Inputs whose magnitudes are far apart, on every prefilter route: the f16 split over the f32 rows, the split and half copies, the int8 copy, TurboQuant
wide, SQ wide and the PQ prefilter.  Each route rejects rows by a bound it derives from a few statistics - the block's largest |x|, the batch's largest
|q|, the sf / l2 ranges, the LUT ranges - and the exact re-scoring behind the scan repairs only what the bound lets through.  Here one member of the
batch or of the block owns those statistics:
  A  queries 2^e times a near-copy of a row, e = 0, -10, -20, -30, -40, +20 in turn: one query of every tile sets the batch's scale;
  B  rows 2^k times a Gaussian, k in [-30, 0]; queries near rows of the k = 0, -15 and -30 groups (under Euclid the small rows are the near ones);
  C  the whole block times 2^-110 and 2^100 (dense routes: below and above the clamp of the split's power-of-two scale), 2^-50 and 2^50 (quantized);
  D  rows |Gaussian|, queries -|Gaussian|: every score is negative;
  E  one column of the rows times 2^20.
A block of 2^18 + 87 rows (the routes' minimum, a partial last tile), every route at its minimum batch or the number of queries a case plants.  The dense
routes return the oracle's lists (parity_asserts.assert_reference_lists); the quantized ones their own option-off scans' - ids, score bits, order - and,
for the first two queries, the lists the oracle's scores of every row give.  The queries of C are near-copies of the rows BEFORE the block's factor, so
that no score leaves the f32 range."""
import numpy as np
import pytest

import oracle_ffi as O
from parity_asserts import assert_reference_lists
from test_gpu_sq_wide import _segment as sq_segment

pytestmark = pytest.mark.gpu

N, DIM, DIM_TQ, TOP = (1 << 18) + 87, 128, 256, 10
DENSE = ["f32_split", "split_copy", "half_copy", "i8_copy"]
QUANT = ["tq_wide", "sq_wide", "pq_prefilter"]
ROUTES = DENSE + QUANT
KERNEL = {"f32_split": "scan_f32_split_kernel", "split_copy": "scan_f16pair_kernel<false>", "half_copy": "scan_f16pair_kernel<true>", "i8_copy": "scan_i8copy_kernel",
          "tq_wide": "scan_tq4w_kernel", "sq_wide": "scan_sqw_kernel", "pq_prefilter": "pq_prefilter_kernel"}
OPTION_OFF = {"tq_wide": ("tq_wide_min_queries", 0), "sq_wide": ("sq_wide_min_queries", 0), "pq_prefilter": ("no_pq_prefilter", 1)}
EXPONENTS = (0, -10, -20, -30, -40, 20)
COLUMN = 5


def _dim(route):
    return DIM_TQ if route == "tq_wide" else DIM


def _block(name, dim):
    """the rows of a case, as stored (Dot and Euclid keep a vector as it is)"""
    rng = np.random.default_rng([dim, sum(name.encode())])
    x = rng.standard_normal((N, dim)).astype(np.float32)
    if name.startswith("scaled"):
        x *= np.float32(2.0) ** int(name[6:])
    elif name == "mixed":
        x *= (np.float32(2.0) ** _mixed_exponents()).astype(np.float32)[:, None]
    elif name == "positive":
        np.abs(x, out=x)
    elif name == "column":
        x[:, COLUMN] *= np.float32(2.0 ** 20)
    else:
        assert name == "unit"
    return x


def _mixed_exponents():
    return np.random.default_rng(0xB10C).integers(-30, 1, N)


class _World:
    """every block, oracle and segment once, when the first test asks for it"""

    def __init__(self, qa):
        self.qa, self.F = qa, qa._ffi
        self.min_batch = {"f32_split": 70, "split_copy": 5, "half_copy": 5, "i8_copy": 5, "tq_wide": int(qa.get_option("tq_wide_min_queries")),
                          "sq_wide": int(qa.get_option("sq_wide_min_queries")), "pq_prefilter": max(int(qa.get_option("pq_prefilter_min_queries")), 8)}
        assert self.min_batch["tq_wide"] == 33 and self.min_batch["sq_wide"] == 33 and self.min_batch["pq_prefilter"] == 8      # what the cases are sized for
        self.blocks, self.dense, self.segments = {}, {}, {}

    def rows(self, name, dim):
        if (name, dim) not in self.blocks:
            self.blocks[name, dim] = _block(name, dim)
        return self.blocks[name, dim]

    def oracle(self, name, dim, dist=O.DOT):
        """the dense oracle over the rows of a block"""
        if (name, dim, dist) not in self.dense:
            self.dense[name, dim, dist] = O.DenseStorage(O.F32, dist, self.rows(name, dim))
        return self.dense[name, dim, dist]

    def segment(self, name, route, dist=O.DOT):
        """-> (device storage, scores of every row by the route's oracle for preprocessed queries | None for a dense route)"""
        key = (name, route, dist)
        if key in self.segments:
            return self.segments[key]
        qa, F = self.qa, self.F
        rows = self.rows(name, _dim(route))
        d = {O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid}[dist]
        ids = np.arange(N, dtype=np.uint32)
        if route in DENSE:
            flags = {"f32_split": 0, "split_copy": F.SEG_SPLIT_COPY, "half_copy": F.SEG_HALF_COPY, "i8_copy": F.SEG_I8_COPY}[route]
            out = (qa.VectorStorage(rows, d, flags=flags), None)
        elif route == "tq_wide":
            tq = qa.TurboQuantizer(DIM_TQ, d, O.TQ_BITS4)
            codes = tq.encode(rows)
            orc = O.TqOracle(dist, DIM_TQ, O.TQ_BITS4)
            orc.rows = codes
            out = (qa.EncodedVectorsTQ(codes, tq), lambda qpre: orc.score_points(qpre, ids))
        elif route == "sq_wide":
            _, osq, codes, st = sq_segment(qa, dist, DIM, N, seed=0, vecs=rows)

            def sq_scores(qpre):
                osq.rows = codes
                return osq.score_points(qpre, ids)
            out = (st, sq_scores)
        else:
            centroids = O.PqOracle.train(rows[:3000], DIM, 8, 256, iters=3)
            pq = qa.ProductQuantizer(DIM, d, 8, centroids)
            opq = O.PqOracle(dist, DIM, 8, centroids)
            opq.codes = pq.encode(rows)
            out = (qa.EncodedVectorsPQ(opq.codes, pq), lambda qpre: opq.score_points(qpre, ids))
        self.segments[key] = out
        return out


@pytest.fixture(scope="module")
def world():
    import qdrant_amd as qa
    assert qa.device_count() >= 1
    assert N % 256 == 87
    return _World(qa)


def _near_copies(rows, picks, seed, noise=0.3):
    """queries: the picked rows plus noise of `noise` times each row's own spread (its median |x| / 0.6745: one outlying column does not set it)"""
    rng = np.random.default_rng(seed)
    base = rows[picks].astype(np.float64)
    sd = np.median(np.abs(base), axis=1, keepdims=True) / 0.6745
    return (base + noise * sd * rng.standard_normal(base.shape)).astype(np.float32)


def _near_copies_before_the_factor(world, route, exponent, seed):
    """case C: near-copies of rows of the block as it was before its factor 2^exponent (a score is then 2^exponent times a unit-scale one)"""
    rows = world.rows("scaled%d" % exponent, _dim(route))
    picks = np.random.default_rng(seed).integers(0, N, world.min_batch[route])
    return _near_copies(rows[picks].astype(np.float64) * 2.0 ** -exponent, np.arange(len(picks)), seed + 1)


def _run(world, name, route, queries, dist=O.DOT):
    """the search of a case on a route, with every check the cases share; -> its counters"""
    qa, F = world.qa, world.F
    st, oracle_scores = world.segment(name, route, dist)
    nq = len(queries)
    s = qa.BatchFilteredSearcher(queries, st, TOP)
    got = s.peek_top_all()
    counters = s.counters
    print("%s / %s / distance %d: %d queries, fallback_queries = %d" % (name, route, dist, nq, counters.fallback_queries))
    assert KERNEL[route] in F.last_kernel(s.scorer._h), F.last_kernel(s.scorer._h)
    assert counters.prefilter_queries == nq
    assert all(len(g) == TOP for g in got)
    if route in DENSE:
        assert_reference_lists(got, world.oracle(name, DIM, dist), queries, TOP)
        return counters
    option, value = OPTION_OFF[route]
    qa.set_option(option, value)
    try:
        s2 = qa.BatchFilteredSearcher(queries, st, TOP)
        want = s2.peek_top_all()
        assert KERNEL[route] not in F.last_kernel(s2.scorer._h)
    finally:
        qa.set_option(option, -1)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["idx"].tolist() == w["idx"].tolist()
        assert np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32))
    sc = oracle_scores(O.preprocess(dist, queries[:2]))
    for g, scores in zip(got[:2], sc):
        order = np.lexsort((np.arange(N), -scores.astype(np.float64)))[:TOP]      # descending score, ties -> lower id
        assert g["idx"].tolist() == order.tolist()
        assert np.array_equal(g["score"].view(np.uint32), scores[order].view(np.uint32))
    return counters


@pytest.mark.parametrize("route", ROUTES)
def test_a_queries_of_mixed_magnitudes_in_one_batch(world, route):
    """query j is 2^e times a near-copy of a row, e = EXPONENTS[j % 6].  The queries of e <= -20 - 2^-40 and less of the batch's largest - may take the exact
    scan; nobody else: the case does not pass by sending everybody there."""
    nq = max(world.min_batch[route], len(EXPONENTS))
    rows = world.rows("unit", _dim(route))
    e = np.array([EXPONENTS[j % len(EXPONENTS)] for j in range(nq)])
    base = _near_copies(rows, np.random.default_rng(11).integers(0, N, nq), seed=12)
    factor = (np.float32(2.0) ** e).astype(np.float32)
    queries = base * factor[:, None]
    # the inputs hold no subnormal or rounded score: the oracle's list of 2^e q is q's list, every score times 2^e
    dense = world.oracle("unit", _dim(route))
    for a, b, f in zip(dense.peek_top(base, TOP, threads=8), dense.peek_top(queries, TOP, threads=8), factor):
        assert a["idx"].tolist() == b["idx"].tolist()
        assert np.array_equal((a["score"] * f).view(np.uint32), b["score"].view(np.uint32))
    counters = _run(world, "unit", route, queries)
    assert counters.fallback_queries <= int((e <= -20).sum()), (counters.fallback_queries, int((e <= -20).sum()))


def _mixed_queries(world, route):
    rows = world.rows("mixed", _dim(route))
    k = _mixed_exponents()
    nq = max(world.min_batch[route], 6)
    rng = np.random.default_rng(21)
    picks = np.array([rng.choice(np.flatnonzero(k == (0, -15, -30)[j % 3])) for j in range(nq)])
    return _near_copies(rows, picks, seed=22)


@pytest.mark.parametrize("route", ROUTES)
def test_b_rows_of_mixed_magnitudes(world, route):
    _run(world, "mixed", route, _mixed_queries(world, route))


@pytest.mark.parametrize("route", QUANT)
def test_b_rows_of_mixed_magnitudes_euclid(world, route):
    _run(world, "mixed", route, _mixed_queries(world, route), dist=O.EUCLID)


@pytest.mark.parametrize("exponent", [-110, 100])
@pytest.mark.parametrize("route", DENSE)
def test_c_whole_block_scaled_dense(world, route, exponent):
    _run(world, "scaled%d" % exponent, route, _near_copies_before_the_factor(world, route, exponent, seed=31))


@pytest.mark.parametrize("exponent", [-50, 50])
@pytest.mark.parametrize("route", QUANT)
def test_c_whole_block_scaled_quantized(world, route, exponent):
    _run(world, "scaled%d" % exponent, route, _near_copies_before_the_factor(world, route, exponent, seed=33))


@pytest.mark.parametrize("route", ROUTES)
def test_d_every_score_negative(world, route):
    nq = world.min_batch[route]
    dim = _dim(route)
    queries = -np.abs(np.random.default_rng(41).standard_normal((nq, dim))).astype(np.float32)
    best = world.oracle("positive", dim).peek_top(queries, 1, threads=8)
    assert all(float(b["score"][0]) < 0.0 for b in best)
    _run(world, "positive", route, queries)


@pytest.mark.parametrize("route", ["i8_copy", "half_copy", "pq_prefilter", "tq_wide"])
def test_e_one_row_column_scaled(world, route):
    nq = world.min_batch[route]
    rows = world.rows("column", _dim(route))
    queries = _near_copies(rows, np.random.default_rng(51).integers(0, N, nq), seed=52)
    _run(world, "column", route, queries)
