"""The band of the f16 split prefilter (qdrant_amd/csrc/scan_split.hip, split_rel_band / split_abs_band in api_search.hip), restated in numpy and
checked on the CPU: for every (query, row) the approximate score the pass forms - rows and queries scaled by one power of two each, split into f16
pairs, three products (the f32 rows, the split copy) or one (the half copy) - lies within band[query] of the f64 dot of the f32 values.  The model
restates, line by line: sp_pow2_scale / split_row_scale with the clamp at 2^+-100, the batch's scale from max |q| over the tile (sp_batch_scale),
h = f16(x s) and l = f16(x s - h) rounded to nearest even (sp_split4, sp_pack_queries_kernel), the sums of the products divided by row_scale *
query_scale, and the band of sp_thresholds_kernel.  The products are summed in f64: the f32 accumulation of the matrix cores is the band's dim * 2^-23
term, which the model leaves unused.

Every case runs twice: with f16 subnormal operands kept - what the matrix cores of gfx950 do (measured), the variant the band is made for and the one
asserted everywhere - and with them flushed to zero, an operand below 2^-14 lost whole.  The flushed variant is asserted wherever no operand that
matters is subnormal; where it parts from the kept one - a query 2^-20 and less of its batch's largest, a block below the scale's clamp - the band
would have to be 2^10 wider, and test_flushed_operands_would_need_a_wider_band pins the figures: a chip that flushed would need split_abs_band at 2^-14.

The cases: a uniform batch; the block times 2^100 and 2^-110 (beyond the clamp: the rows reach f16 at 2^-8 and below); rows times 2^k, k in [-30, 0];
one column of the rows, or of the queries, times 2^20; a batch whose queries are 2^e of its largest, e down to -40.  The relative band alone - the
formula before the absolute term - loses the last case from e = -25 on: test_the_relative_band_alone_does_not_cover_a_small_query_beside_a_big_one."""
import numpy as np
import pytest

N_ROWS = 20_000
F16_MIN_NORMAL = 2.0 ** -14
E_SMALL = (0, -10, -20, -25, -30, -40)


def pow2_scale(maxabs):
    """sp_pow2_scale / split_row_scale: the power of two that brings maxabs to [8192, 16384), its exponent clamped to +-100"""
    maxabs = np.float32(maxabs)
    if not (maxabs > 0.0) or not (maxabs < np.float32(3.0e38)):
        return np.float32(1.0)
    _, e = np.frexp(maxabs)
    return np.float32(np.ldexp(1.0, int(np.clip(14 - int(e), -100, 100))))


def split(x, scale, flush):
    """x * scale = h + l + residual, both parts f16 (round to nearest even); flush: the matrix cores read a subnormal f16 operand as zero"""
    xs = x.astype(np.float32) * np.float32(scale)      # (a power of two: exact)
    assert np.isfinite(xs).all()
    h = xs.astype(np.float16)
    l = (xs - h.astype(np.float32)).astype(np.float16)
    h, l = h.astype(np.float64), l.astype(np.float64)
    if flush:
        h[np.abs(h) < F16_MIN_NORMAL] = 0.0
        l[np.abs(l) < F16_MIN_NORMAL] = 0.0
    return h, l


def rel_band(half, dim):
    """split_rel_band"""
    acc = np.float32(dim) * np.float32(1.1920929e-7)
    return (np.float32(9.765625e-4) + np.float32(9.5367432e-7) if half else np.float32(1.9073486e-6)) + acc


ABS_UNIT = 2.0 ** -24             # split_abs_band's resolution: the spacing of f16 subnormals
ABS_UNIT_FLUSHED = 2.0 ** -14     # ... what it would have to be on matrix cores that read subnormal operands as zero: the smallest normal f16


def abs_band(dim, unit=ABS_UNIT):
    """split_abs_band: 2^-24 sqrt(dim), accumulator units of one side"""
    return np.float32(unit) * np.sqrt(np.float32(dim))


def bands(rows, queries, half, with_abs=True, unit=ABS_UNIT):
    """sp_thresholds_kernel: band[q] in score units (f32 arithmetic in the kernel's order); -> band, row_scale, query_scale"""
    dim = rows.shape[1]
    rs, qs = pow2_scale(np.abs(rows).max()), pow2_scale(np.abs(queries).max())
    # segment_split_stats: sqrtf of the largest sum of the squares of x * row_scale, divided by row_scale
    row_norm_max = np.sqrt(np.float32(((rows.astype(np.float64) * float(rs)) ** 2).sum(axis=1).max())) / rs
    qnorm = np.sqrt((queries.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    with np.errstate(over="ignore"):
        b = rel_band(half, dim) * row_norm_max * qnorm
        if with_abs:
            b = b + abs_band(dim, unit) * (row_norm_max / qs + qnorm / rs)
            b = np.where(b < row_norm_max * qnorm, b, np.float32(np.inf))      # a band as wide as the scores' range rejects nothing: the exact scan
    return b.astype(np.float32), rs, qs


def approximate(rows, queries, half, flush, rs, qs):
    """[query, row]: the pass's score, the products summed in f64"""
    rh, rl = split(rows, rs, flush)
    qh, ql = split(queries, qs, flush)
    acc = qh @ rh.T
    if not half:
        acc += qh @ rl.T + ql @ rh.T
    return acc / (float(rs) * float(qs))


def worst_ratio(rows, queries, half, flush, with_abs=True, unit=ABS_UNIT):
    """max over the pairs of |approximate - exact| / band[query]; 0 for a query whose band is infinite (it takes the exact scan)"""
    band, rs, qs = bands(rows, queries, half, with_abs, unit)
    exact = queries.astype(np.float64) @ rows.astype(np.float64).T
    err = np.abs(approximate(rows, queries, half, flush, rs, qs) - exact).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(np.isinf(band), 0.0, err / band.astype(np.float64))
    return ratio, band


def gaussian(seed, n, dim):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def make_case(kind, dim):
    rows, queries = gaussian(dim + 1, N_ROWS, dim), gaussian(dim + 2, 12, dim)
    if kind == "uniform":
        pass
    elif kind in ("block_x2^100", "block_x2^-110"):
        rows *= np.float32(2.0) ** int(kind[9:])
    elif kind == "rows_x2^k":
        rows *= (np.float32(2.0) ** np.random.default_rng(dim + 3).integers(-30, 1, N_ROWS)).astype(np.float32)[:, None]
    elif kind == "row_column_x2^20":
        rows[:, 3] *= np.float32(2.0 ** 20)
    elif kind == "query_column_x2^20":
        queries[:, 3] *= np.float32(2.0 ** 20)
    else:
        assert kind == "small_queries"
        queries *= (np.float32(2.0) ** np.array([E_SMALL[j % len(E_SMALL)] for j in range(len(queries))])).astype(np.float32)[:, None]
    return rows, queries


FLUSH_SENSITIVE = ("block_x2^-110", "small_queries")
KINDS = ["uniform", "block_x2^100", "block_x2^-110", "rows_x2^k", "row_column_x2^20", "query_column_x2^20", "small_queries"]


@pytest.mark.parametrize("flush", [False, True], ids=["subnormals_kept", "subnormals_flushed"])
@pytest.mark.parametrize("half", [False, True], ids=["pair", "half"])
@pytest.mark.parametrize("dim", [128, 256])
@pytest.mark.parametrize("kind", KINDS)
def test_every_pair_lies_within_its_querys_band(kind, dim, half, flush):
    """subnormal operands kept: the band as the device computes it, every case.  Flushed: the same band wherever the operands that matter are normal
    numbers; in the two cases where they are not, the band with the absolute term at the resolution flushing leaves (2^-14) - and
    test_flushed_operands_would_need_a_wider_band shows that nothing less would do"""
    rows, queries = make_case(kind, dim)
    wider = flush and kind in FLUSH_SENSITIVE
    ratio, band = worst_ratio(rows, queries, half, flush, unit=ABS_UNIT_FLUSHED if wider else ABS_UNIT)
    print("%s dim %d %s %s: worst |approx - exact| / band = %.3g, %d infinite bands" % (kind, dim, "half" if half else "pair", "flushed" if flush else "kept", ratio.max(),
                                                                                      int(np.isinf(band).sum())))
    assert (ratio <= 1.0).all(), ratio.tolist()
    # the band still selects: only a query 2^-20 and less of its batch's largest gives up (and no row-side term does: the queries of the other cases keep theirs)
    small = kind == "small_queries"
    for j, b in enumerate(band):
        assert wider or np.isfinite(b) or (small and E_SMALL[j % len(E_SMALL)] <= -20), (j, float(b))


@pytest.mark.parametrize("dim", [128, 256])
def test_an_ordinary_batch_pays_the_added_term_only(dim):
    """unit-scale rows and queries: the absolute term is below 2^-8 of the relative band of the pair (2^-17 of the half copy's)"""
    rows, queries = make_case("uniform", dim)
    for half in (False, True):
        new, _, _ = bands(rows, queries, half)
        old, _, _ = bands(rows, queries, half, with_abs=False)
        assert (new >= old).all() and (new <= old * (1.0 + 2.0 ** -8)).all(), float((new / old).max())


@pytest.mark.parametrize("dim", [128, 256])
def test_the_relative_band_alone_does_not_cover_a_small_query_beside_a_big_one(dim):
    """what the absolute term is for: rel_band * row_norm_max * |q| alone is exceeded by the pair for a query 2^-25 and less of its batch's largest with subnormal
    operands kept - the resolution the batch's scale leaves such a query is 2^-24 in accumulator units, whatever its own size - and from 2^-20 on, and
    by a whole block below the scale's clamp, when they flush"""
    rows, queries = make_case("small_queries", dim)
    e = np.array([E_SMALL[j % len(E_SMALL)] for j in range(len(queries))])
    kept, _ = worst_ratio(rows, queries, False, False, with_abs=False)
    flushed, _ = worst_ratio(rows, queries, False, True, with_abs=False)
    print("pair, relative band alone, dim %d: e -> worst ratio kept / flushed: %s" % (dim, {int(x): (float("%.3g" % a), float("%.3g" % b)) for x, a, b in zip(e[:6], kept[:6], flushed[:6])}))
    assert (kept[e >= -20] <= 1.0).all() and (kept[e <= -30] > 1.0).all()
    assert (flushed[e >= -10] <= 1.0).all() and (flushed[e <= -20] > 1.0).all()
    rows, queries = make_case("block_x2^-110", dim)
    assert worst_ratio(rows, queries, False, False, with_abs=False)[0].max() <= 1.0
    assert worst_ratio(rows, queries, False, True, with_abs=False)[0].max() > 1.0


@pytest.mark.parametrize("half", [False, True], ids=["pair", "half"])
@pytest.mark.parametrize("dim", [128, 256])
@pytest.mark.parametrize("kind", FLUSH_SENSITIVE)
def test_flushed_operands_would_need_a_wider_band(kind, dim, half):
    """the device's band (absolute term at 2^-24) against operands flushed below 2^-14: exceeded by a block below the scale's clamp and by the queries 2^-20
    and 2^-25 of their batch's largest (those below have infinite bands either way).  gfx950 does not flush; this pins what to change on a chip that does"""
    rows, queries = make_case(kind, dim)
    ratio, band = worst_ratio(rows, queries, half, True)
    print("%s dim %d %s, flushed operands against the 2^-24 band: worst ratio %.3g" % (kind, dim, "half" if half else "pair", ratio.max()))
    assert ratio.max() > 1.0
    if kind == "small_queries":
        e = np.array([E_SMALL[j % len(E_SMALL)] for j in range(len(queries))])
        assert (ratio[e >= -10] <= 1.0).all()
