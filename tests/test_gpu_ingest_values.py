"""Ingest and query encoding on the device against the CPU oracle, by number class: `cosine_preprocess_lds_kernel` / `cosine_preprocess_kernel`
(`CosineMetric::preprocess`), `cast_f32_kernel` and `pack_queries_kernel` (csrc/preprocess.hip), and the exact scans over what they store.  Every input
is built here from explicit bit patterns plus a seeded generator, the oracle runs with `isa=ISA_AUTO` (the reference's live dispatch), and a failure
names the case, the row and the element.

1. Cosine preprocess.  Dimensions 1, 3, 15 (scalar leaf), 16, 17, 31 (SSE leaf, remainder 0 / 1 / 15), 32, 36, 64 (AVX leaf, tail 0 / 4 / 0, a multiple
   of 4), 33, 63, 65 (AVX leaf, no multiple of 4), 4096 and 4100 (the last dimension whose 4 rows fit 64 KiB of LDS, and the first past it).  9 rows per
   call: the kernels take 4 rows per block, so the last block holds one.  The rows of every dimension (`_preprocess_cases`): Gaussian; zero; a sum of
   squares one step below and one step at or above f32::EPSILON; a row the oracle normalised, fed again; sums of squares one step inside and one step
   outside 1 -+ 1e-6; elements of 2e19 (the sum is +inf, every quotient a signed zero); one large element beside subnormals and beside tiny normals
   (subnormal quotients); all subnormal; a NaN in the body and in the tail; a +inf; -0.0 in a copied and in a divided row.  Which side of a threshold a
   row lies on is READ from the oracle (a copied row comes back with its own bits), and `test_preprocess_inputs_reach_every_branch` asserts for every
   dimension that copy-because-zero, copy-because-normalised, divide and infinite length all occur and that the threshold pairs differ by one step of
   one multiplier.  Placements: host to host, device to device, device in place, and at dimension 64 an input 4 bytes past a 16-byte boundary.  The
   same rows as queries of a Cosine f32 segment (`encoded_query`), 9 and 27 at a time.
   Which kernel a call reaches is not observable through the API; it is the gate of `launch_cosine_preprocess_f32`, restated in `_takes_lds_kernel`:
   dimensions 32, 36, 64 and 4096 the LDS kernel, every other dimension and the unaligned input the plain one.  The mutation check confirmed it: with the
   division of the LDS kernel alone replaced by a multiplication by the reciprocal exactly those four dimensions (and the query dimensions 36 and 64)
   turned red, with the plain kernel's alone every other dimension, the unaligned call and the other six query dimensions.
2. Casts.  f16: +-0, the smallest and largest f32 subnormal, the ties at f16 subnormal spacing (2^-25 -> 0, 3 x 2^-25 -> 2 x 2^-24, ...), the
   subnormal / normal boundary 2^-14 and its f32 neighbours, ties between normal f16 values over an even and an odd lower neighbour, 65504, the last f32
   below 65520, 65520 (-> inf), 65536, f32::MAX, inf, 4096 seeded values 2^e (1 + m / 2^23) with e in -30 .. 17, all of it negated; through
   `qmx_cast_f32` and as queries of a Dot f16 segment.  `test_cast_inputs_are_what_they_claim` asserts on the host that the ties are ties.
   NaN: the device returns a NaN of the same sign for quiet and signalling inputs of both signs.  MEASURED on gfx950: the payload is F16C's too - the
   top ten mantissa bits with the quiet bit set, so a signalling NaN whose payload sits in the low 13 bits alone becomes 0x7E00 - and the test asserts
   the oracle's bits.
   u8: NaN, +-inf, -0.0, -0.5, 0.99999994, 1.0, 254.99998, 255.0, 255.5, 256, 1e10, subnormals and k + {0, 0.5, 0.99999} for k = 0 .. 255; through
   `qmx_cast_f32`, as queries of a Dot u8 segment at dimension 33, and - the `norm1` block of `pack_queries_kernel` at a dimension with a remainder -
   as scores of a Cosine u8 segment.
3. Scores over stored extremes, 64 rows.  f32 Dot and Euclid at dimensions 128 and 100 with elements of 2^-70 x Gaussian on both sides (every product and
   every sum subnormal: asserted), with half the rows and queries at unit scale, and with subnormal rows against unit queries; 1, 16, 32 and (dimension
   128) 64 queries, `score_points` bit for bit and `peek_top` lists.  `test_f32_extremes_reach_three_kernel_families` reads `qmx_query_last_kernel` and
   asserts that the VALU scan, `scan_f32_mfma_kernel` and `scan_f32_mfma16_kernel` each served a case.
   f16 rows holding subnormals, +-65504, +-0 and +-inf against unit, subnormal and +-65504 queries, all four distances: bits at dimension 24, and at
   dimension 64 the bar of `test_f16_score_points`, 1e-5 x sum|terms|, with the class and sign of every infinite or NaN score.  That bar would hide a
   unit that flushes f16 subnormals wherever other terms dominate: a subnormal element times 65504 is at most 4, and beside 63 products of unit-scale
   elements with 65504 the bar is 1e-5 x 4e6 = 40.  So rows with ONE nonzero, subnormal element are there too: a single product of two f16 values is
   exact in f32 and the sum of it and zeros is exact in any order, and their Dot and Cosine scores are asserted bit for bit at both dimensions.
   A block of +-2e19 elements normalised by `qmx_preprocess_f32` on the device is all signed zeros and scores 0.0 against every query.

Mutation check (scratch copies of preprocess.hip with one change each, run on gfx950; not committed).  `x / length` -> `x * (1.0f / length)`, one kernel
at a time as told above: test_preprocess_rows at all 14 dimensions, test_preprocess_unaligned_input_at_dim_64 and test_preprocess_queries at all 8 turn
red between the two.  `1.0e-6f` -> `1.0e-5f`: the same 23 cases, each through the row "e one step below 1 - 1e-6" first.  `__float2half_rn` ->
`__float2half_rz`: test_cast_f16 (3912 of 8248 values, the first 2^-25 (1 + 2^-23)), test_cast_f16_as_queries and the encoded queries of
test_f16_scores_over_extremes.  Two of the changes the issue lists cannot be seen by any input, so nothing can turn red for them: `x >= 255.0f` ->
`x > 255.0f` routes 255.0 alone to the conversion, which gives 255 as well (the threshold may stand anywhere in (254, 256]; `x >= 254.0f` turns
test_cast_u8 and test_cast_u8_as_queries red at 254.99998); and `length = -0.0f` -> `0.0f` in the scalar leaf, because the first term added is a
square, +0.0 or greater or NaN, and -0.0 + x equals +0.0 + x for every such x."""
import functools

import numpy as np
import pytest

import oracle_ffi as O

gpu = pytest.mark.gpu

DIMS = [1, 3, 15, 16, 17, 31, 32, 36, 64, 33, 63, 65, 4096, 4100]
QUERY_DIMS = [3, 15, 17, 31, 36, 64, 33, 65]      # two per leaf and kernel
ROWS_PER_CALL = 9
SENTINEL = 0xA5
EPSILON = float(np.float32(1.1920929e-7))


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


def _dist(qa, d):
    return {O.COSINE: qa.Distance.Cosine, O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid, O.MANHATTAN: qa.Distance.Manhattan}[d]


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _frozen(a):
    a.setflags(write=False)
    return a


def _assert_same_f32(got, want, names, what):
    """Bit equality of two [rows, dim] f32 arrays; a NaN equals a NaN.  The message names the first differing row's case and element."""
    got, want = np.asarray(got, dtype=np.float32).reshape(np.shape(want)), np.asarray(want, dtype=np.float32)
    ok = (_u32(got) == _u32(want)) | (np.isnan(got) & np.isnan(want))
    if not ok.all():
        r, c = np.argwhere(~ok)[0]
        raise AssertionError("%s: row %d (%s), element %d: got 0x%08X, the oracle 0x%08X; %d elements of %d rows differ"
                             % (what, r, names[r], c, _u32(got)[r, c], _u32(want)[r, c], int((~ok).sum()), int((~ok).any(axis=1).sum())))


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. Cosine preprocess
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _takes_lds_kernel(dim, aligned=True):
    """the gate of launch_cosine_preprocess_f32 (csrc/preprocess.hip)"""
    return dim >= 32 and dim % 4 == 0 and dim * 16 <= 64 * 1024 and aligned


def _oracle_copies(row):
    """Whether CosineMetric::preprocess returns the row as it is (is_length_zero_or_normalized): read from the oracle, not computed here."""
    return np.array_equal(_u32(O.preprocess(O.COSINE, row[None, :])[0]), _u32(row))


def _step_pair(base, lo, hi):
    """f32 multipliers lo < hi whose rows base * lo and base * hi lie on different sides of a threshold -> the two rows of ADJACENT multipliers that still do
    (bisection over the multiplier's bit pattern), in the order (row of the smaller multiplier, row of the larger)."""
    a, b = int(np.float32(lo).view(np.uint32)), int(np.float32(hi).view(np.uint32))
    row = lambda t: base * _f32([t])[0]
    side_a, side_b = _oracle_copies(row(a)), _oracle_copies(row(b))
    assert side_a != side_b, "the multipliers %r and %r do not straddle a threshold" % (lo, hi)
    while b - a > 1:
        m = (a + b) // 2
        if _oracle_copies(row(m)) == side_a:
            a = m
        else:
            b = m
    return row(a), row(b)


def _nudged(row, ulps):
    """the row with its largest element moved by `ulps` steps of its own spacing"""
    out = row.copy()
    i = int(np.argmax(np.abs(row)))
    out.view(np.uint32)[i] = int(out.view(np.uint32)[i]) + ulps      # (sign and magnitude: a step of the bits is a step of the magnitude)
    return out


def _subnormals(rng, size):
    return _f32(rng.integers(1, 0x800000, size=size, dtype=np.uint32) | (rng.integers(0, 2, size=size, dtype=np.uint32) << np.uint32(31)))


@functools.lru_cache(maxsize=None)
def _preprocess_cases(dim):
    """(names, rows [27, dim] f32, the oracle's preprocess of them): every case of the module's docstring, padded with Gaussian rows of other scales to
    whole calls of 9 rows."""
    rng = np.random.default_rng(7700 + dim)
    gauss = lambda: rng.standard_normal(dim).astype(np.float32)
    names, rows = [], []

    def add(name, row):
        names.append(name)
        rows.append(np.ascontiguousarray(row, dtype=np.float32))

    add("a gaussian", gauss() * np.float32(1.5))
    add("b zero", np.zeros(dim, dtype=np.float32))
    g = gauss()
    g[g == 0] = 1.0
    unit = (g.astype(np.float64) / np.sqrt((g.astype(np.float64) ** 2).sum())).astype(np.float32)      # sum of squares 1 within rounding
    # (c) sum of squares 2^-22 at the multiplier 1, 2^-24 at 0.5: f32::EPSILON = 2^-23 lies between
    below, above = _step_pair(unit * np.float32(2.0 ** -11), 0.5, 1.0)
    add("c below epsilon", below)
    add("c at or above epsilon", above)
    add("c below epsilon, largest element 1 step up", _nudged(below, 1))
    add("c above epsilon, largest element 1 step down", _nudged(above, -1))
    add("d normalised by the oracle, fed again", O.preprocess(O.COSINE, (gauss() * np.float32(3.0))[None, :])[0])
    # (e) |sum of squares - 1| <= 1e-6
    outside, inside = _step_pair(unit, 1.0 - 2e-6, 1.0)
    add("e one step below 1 - 1e-6", outside)
    add("e one step inside 1 - 1e-6", inside)
    inside, outside = _step_pair(unit, 1.0, 1.0 + 2e-6)
    add("e one step inside 1 + 1e-6", inside)
    add("e one step above 1 + 1e-6", outside)
    add("e above 1 + 1e-6, largest element 1 step down", _nudged(outside, -1))
    add("f sum of squares +inf", np.where(rng.integers(0, 2, dim) == 1, np.float32(-2e19), np.float32(2e19)))
    if dim >= 2:
        row = _subnormals(rng, dim)
        row[dim // 2] = np.float32(3.0)
        add("g one large element, the rest subnormal", row)
        row = gauss() * np.float32(2.0 ** -122)
        row[dim - 1] = np.float32(-1000.0)
        add("g one large element, the rest tiny normals (subnormal quotients)", row)
    else:
        add("g a lone large element", np.full(dim, 3.0, dtype=np.float32))
    add("h all subnormal", _subnormals(rng, dim))
    row = gauss()
    row[0] = np.nan
    add("i NaN in the body", row)
    row = gauss()
    row[dim - 1] = _f32([0xFFC00001])[0]
    add("i NaN in the last element (the tail where the leaf has one)", row)
    row = gauss()
    row[dim // 3] = np.inf
    add("j +inf element", row)
    add("k zeros of both signs", _f32(rng.integers(0, 2, dim, dtype=np.uint32) << np.uint32(31)))
    if dim >= 2:
        row = gauss()
        row[1::2] = -0.0
        if dim >= 3:
            row[2] = 0.0
        add("k -0.0 among gaussian elements", row)
    scale = 0
    while len(rows) % ROWS_PER_CALL:
        add("a gaussian x 1e%d" % (3 * scale - 3), gauss() * np.float32(10.0 ** (3 * scale - 3)))
        scale += 1
    rows = np.stack(rows)
    return tuple(names), _frozen(rows), _frozen(O.preprocess(O.COSINE, rows))


def _branch(row, out):
    """Which way CosineMetric::preprocess took for the row, from the oracle's output (copied or not) and the sum of squares in f64."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = float((row.astype(np.float64) ** 2).sum())
    if np.isnan(s):
        return "nan"
    if np.array_equal(_u32(out), _u32(row)):
        return "copy: zero" if s < 0.5 else "copy: normalised"
    return "inf length" if s > float(np.finfo(np.float32).max) else "divide"


@pytest.mark.parametrize("dim", DIMS)
def test_preprocess_inputs_reach_every_branch(dim):
    """Host only: the oracle puts the threshold rows on both sides, one multiplier step apart, and the rows of every dimension take every branch."""
    names, rows, want = _preprocess_cases(dim)
    assert len(rows) % ROWS_PER_CALL == 0 and len(rows) // ROWS_PER_CALL >= 2
    by_name = {n: i for i, n in enumerate(names)}
    taken = {n: _branch(rows[i], want[i]) for n, i in by_name.items()}
    assert {"copy: zero", "copy: normalised", "divide", "inf length", "nan"} <= set(taken.values()), taken
    expect = {"b zero": "copy: zero", "c below epsilon": "copy: zero", "c at or above epsilon": "divide",
              "d normalised by the oracle, fed again": "copy: normalised", "e one step below 1 - 1e-6": "divide",
              "e one step inside 1 - 1e-6": "copy: normalised", "e one step inside 1 + 1e-6": "copy: normalised", "e one step above 1 + 1e-6": "divide",
              "f sum of squares +inf": "inf length", "h all subnormal": "copy: zero", "k zeros of both signs": "copy: zero",
              "j +inf element": "inf length"}
    if dim >= 2:
        expect["k -0.0 among gaussian elements"] = "divide"
    for name, branch in expect.items():
        assert taken[name] == branch, (dim, name, taken[name])
    for a, b in (("c below epsilon", "c at or above epsilon"), ("e one step below 1 - 1e-6", "e one step inside 1 - 1e-6"),
                 ("e one step inside 1 + 1e-6", "e one step above 1 + 1e-6")):
        ra, rb = rows[by_name[a]], rows[by_name[b]]      # one step of a multiplier in [0.5, 1.000002] is at most 2^-23 of it: two steps of an element at the most
        assert np.abs(_u32(ra).astype(np.int64) - _u32(rb).astype(np.int64)).max() <= 2, (dim, a, b)
    # the sums of squares are where they are meant to be (f64; the f32 chains differ from it by rounding only)
    s = lambda n: float((rows[by_name[n]].astype(np.float64) ** 2).sum())
    assert abs(s("c below epsilon") / EPSILON - 1) < 1e-4 and abs(s("c at or above epsilon") / EPSILON - 1) < 1e-4
    # (one multiplier step moves the sum by 2.4e-7 above 1, and the f32 sum is 1.2e-7 apart from its neighbours there)
    assert abs(abs(s("e one step below 1 - 1e-6") - 1) - 1e-6) < 4e-7 and abs(abs(s("e one step above 1 + 1e-6") - 1) - 1e-6) < 4e-7
    # infinite length: signed zeros, and NaN for inf / inf; subnormal quotients where the case says so
    f = want[by_name["f sum of squares +inf"]]
    assert np.array_equal(_u32(f), _u32(rows[by_name["f sum of squares +inf"]]) & np.uint32(0x80000000))
    if dim >= 2:
        for name in ("g one large element, the rest subnormal", "g one large element, the rest tiny normals (subnormal quotients)"):
            out = want[by_name[name]]
            tiny = np.abs(out) < np.finfo(np.float32).tiny
            assert tiny.sum() == dim - 1 and (out[tiny] != 0).sum() >= (dim - 1) // 2, (dim, name)
        k = by_name["k -0.0 among gaussian elements"]
        assert (_u32(want[k])[1::2] == 0x80000000).all() and (_u32(want[k])[0] & 0x7FFFFFFF) != 0
    # both kernels are asked for
    assert {_takes_lds_kernel(d) for d in DIMS} == {True, False} and [d for d in DIMS if _takes_lds_kernel(d)] == [32, 36, 64, 4096]


def _on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _preprocess_on_device(qa, chunk, placement):
    """qmx_preprocess_f32 of a [n, dim] block: placement "host" (host to host), "device" (device to device, out of place) or "in place"."""
    import torch
    from qdrant_amd import _ffi as F
    n, dim = chunk.shape
    call = lambda i, o: F.check(F.lib().qmx_preprocess_f32(0, int(qa.Distance.Cosine), F.ptr(i), n, dim, F.ptr(o)))
    if placement == "host":
        src, out = np.ascontiguousarray(chunk), np.full(chunk.nbytes, SENTINEL, dtype=np.uint8)
        call(src, out)
        assert np.array_equal(_u32(src), _u32(chunk)), "the input changed"
        return out.view(np.float32).reshape(n, dim)
    src = _on_device(chunk)
    if placement == "in place":
        call(src, src)
        return src.cpu().numpy().view(np.float32).reshape(n, dim)
    out = torch.full((chunk.nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    call(src, out)
    assert np.array_equal(src.cpu().numpy(), np.ascontiguousarray(chunk).view(np.uint8).reshape(-1)), "the input changed"
    return out.cpu().numpy().view(np.float32).reshape(n, dim)


@gpu
@pytest.mark.parametrize("dim", DIMS)
def test_preprocess_rows(qa, dim):
    names, rows, want = _preprocess_cases(dim)
    for r0 in range(0, len(rows), ROWS_PER_CALL):
        sl = slice(r0, r0 + ROWS_PER_CALL)
        for placement in ("host", "device", "in place"):
            got = _preprocess_on_device(qa, rows[sl], placement)
            _assert_same_f32(got, want[sl], names[sl], "dim %d (%s kernel), rows %d.., %s" % (dim, "LDS" if _takes_lds_kernel(dim) else "plain", r0, placement))


@gpu
def test_preprocess_unaligned_input_at_dim_64(qa):
    """An input 4 bytes past a 16-byte boundary: the plain kernel at a dimension the LDS kernel takes otherwise; out of place and in place."""
    import torch
    from qdrant_amd import _ffi as F
    dim = 64
    names, rows, want = _preprocess_cases(dim)
    assert _takes_lds_kernel(dim) and not _takes_lds_kernel(dim, aligned=False)
    for r0 in range(0, len(rows), ROWS_PER_CALL):
        sl = slice(r0, r0 + ROWS_PER_CALL)
        chunk = np.ascontiguousarray(rows[sl])
        for in_place in (False, True):
            buf = torch.full((chunk.nbytes + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            buf[4:4 + chunk.nbytes] = _on_device(chunk)
            out = buf if in_place else torch.full((chunk.nbytes + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
            off = 4 if in_place else 0
            F.check(F.lib().qmx_preprocess_f32(0, int(qa.Distance.Cosine), F.ptr(buf.data_ptr() + 4), ROWS_PER_CALL, dim, F.ptr(out.data_ptr() + off)))
            host = out.cpu().numpy()
            got = host[off:off + chunk.nbytes].copy().view(np.float32).reshape(ROWS_PER_CALL, dim)
            _assert_same_f32(got, want[sl], names[sl], "dim 64, input at +4 bytes, rows %d.., %s" % (r0, "in place" if in_place else "out of place"))
            assert (host[:off] == SENTINEL).all() and (host[off + chunk.nbytes:] == SENTINEL).all(), "bytes outside the block were written"
            if not in_place:
                assert np.array_equal(buf.cpu().numpy()[4:4 + chunk.nbytes], chunk.view(np.uint8).reshape(-1)), "the input changed"


@gpu
@pytest.mark.parametrize("dim", QUERY_DIMS)
def test_preprocess_queries(qa, dim):
    """The same rows as queries of a Cosine f32 segment: the query path stages and normalises on its own stream (query_encode), 9 and 27 at a time."""
    names, rows, want = _preprocess_cases(dim)
    stored = O.preprocess(O.COSINE, np.random.default_rng(dim).standard_normal((4, dim)).astype(np.float32))
    st = qa.VectorStorage(stored, qa.Distance.Cosine)
    batches = [slice(r0, r0 + ROWS_PER_CALL) for r0 in range(0, len(rows), ROWS_PER_CALL)] + [slice(0, len(rows))]
    for sl in batches:
        scorer = qa.new_raw_scorer(rows[sl], st)
        got = np.stack([scorer.encoded_query(i) for i in range(scorer.nq)])
        _assert_same_f32(got, want[sl], names[sl], "dim %d, queries %d..%d" % (dim, sl.start, sl.stop))
        scorer.close()
    st.close()


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. casts
# ------------------------------------------------------------------------------------------------------------------------------------------------------
# (name, f32 bits, lower f16 neighbour of a tie or None, the f16 the tie rounds to)
F16_SPECIALS = [
    ("+0", 0x00000000, None, None),
    ("smallest f32 subnormal", 0x00000001, None, None),
    ("largest f32 subnormal", 0x007FFFFF, None, None),
    ("below 2^-25", 0x32FFFFFF, None, None),
    ("2^-25: tie between 0 and 2^-24", 0x33000000, 0x0000, 0x0000),
    ("2^-25 (1 + 2^-23)", 0x33000001, None, None),
    ("2^-24", 0x33800000, None, None),
    ("3 x 2^-25: tie over an odd neighbour", 0x33C00000, 0x0001, 0x0002),
    ("5 x 2^-25: tie over an even neighbour", 0x34200000, 0x0002, 0x0002),
    ("7 x 2^-25: tie over an odd neighbour", 0x34600000, 0x0003, 0x0004),
    ("1023.5 x 2^-24: tie between the largest subnormal and 2^-14", 0x387FE000, 0x03FF, 0x0400),
    ("below 2^-14", 0x387FFFFF, None, None),
    ("2^-14", 0x38800000, None, None),
    ("above 2^-14", 0x38800001, None, None),
    ("below the tie over 1.0", 0x3F800FFF, None, None),
    ("tie over 1.0 (even)", 0x3F801000, 0x3C00, 0x3C00),
    ("above the tie over 1.0", 0x3F801001, None, None),
    ("below the tie over 1 + 2^-10", 0x3F802FFF, None, None),
    ("tie over 1 + 2^-10 (odd)", 0x3F803000, 0x3C01, 0x3C02),
    ("above the tie over 1 + 2^-10", 0x3F803001, None, None),
    ("tie over 2 - 2^-10 (odd): carries into the exponent", 0x3FFFF000, 0x3FFF, 0x4000),
    ("tie at subnormal / normal spacing change, over 2^-14 (even)", 0x38801000, 0x0400, 0x0400),
    ("65504", 0x477FE000, None, None),
    ("largest f32 below 65520", 0x477FEFFF, None, None),
    ("65520: tie between 65504 and 2^16", 0x477FF000, 0x7BFF, 0x7C00),
    ("65536", 0x47800000, None, None),
    ("f32::MAX", 0x7F7FFFFF, None, None),
    ("+inf", 0x7F800000, None, None),
]
# quiet / signalling, both signs, payload in the high mantissa bits only and in the low 13 bits only
F16_NANS = [("quiet", 0x7FC00000), ("quiet, negative", 0xFFC00000), ("quiet, high payload", 0x7FE00000), ("quiet, low payload", 0x7FC00001),
            ("signalling, high payload", 0x7FA00000), ("signalling, high payload, negative", 0xFFA00000), ("signalling, low payload", 0x7F800001),
            ("signalling, low payload, negative", 0xFF800001), ("signalling, bit 12 alone", 0x7F801000), ("all mantissa bits", 0x7FFFFFFF)]


@functools.lru_cache(maxsize=None)
def _f16_inputs():
    rng = np.random.default_rng(1616)
    e = rng.integers(-30, 18, size=4096, dtype=np.int64)
    m = rng.integers(0, 1 << 23, size=4096, dtype=np.int64)
    bits = np.concatenate([np.array([b for _, b, _, _ in F16_SPECIALS], dtype=np.uint32), (((e + 127) << 23) | m).astype(np.uint32)])
    names = [n for n, _, _, _ in F16_SPECIALS] + ["2^%d (1 + %d / 2^23)" % (a, b) for a, b in zip(e.tolist(), m.tolist())]
    bits = np.concatenate([bits, bits | np.uint32(0x80000000)])
    return tuple(names + ["-(%s)" % n for n in names]), _frozen(_f32(bits).copy())


@functools.lru_cache(maxsize=None)
def _u8_inputs():
    named = [("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("-0.0", -0.0), ("-0.5", -0.5), ("0.99999994", _f32([0x3F7FFFFF])[0]), ("1.0", 1.0),
             ("254.99998", _f32([0x437EFFFF])[0]), ("255.0", 255.0), ("255.00002", _f32([0x437F0001])[0]), ("255.5", 255.5), ("256", 256.0), ("1e10", 1e10),
             ("-1e10", -1e10), ("f32::MAX", _f32([0x7F7FFFFF])[0]), ("negative NaN", _f32([0xFFC00000])[0]), ("signalling NaN", _f32([0x7F800001])[0]),
             ("smallest subnormal", _f32([0x00000001])[0]), ("largest subnormal", _f32([0x007FFFFF])[0]), ("negative subnormal", _f32([0x80000001])[0])]
    names, vals = [n for n, _ in named], [np.float32(v) for _, v in named]
    for k in range(256):
        for frac in (0.0, 0.5, 0.99999):
            names.append("%d + %g" % (k, frac))
            vals.append(np.float32(k + frac))
    return tuple(names), _frozen(np.array(vals, dtype=np.float32))


def test_cast_inputs_are_what_they_claim():
    """Host only: every listed tie lies exactly half way between two adjacent f16 values and the oracle rounds it to the even one; the boundary values
    are the numbers their names say; the u8 list holds values on both sides of 0, 1, 255 and 256."""
    for name, bits, lower, rounded in F16_SPECIALS:
        if lower is None:
            continue
        x = float(_f32([bits])[0])
        lo = float(O.f16_to_f32(np.array([lower], dtype=np.uint16))[0])
        hi = 65536.0 if lower == 0x7BFF else float(O.f16_to_f32(np.array([lower + 1], dtype=np.uint16))[0])
        assert lo < x < hi and x - lo == hi - x, name
        assert rounded in (lower, lower + 1) and rounded % 2 == 0, name
        assert int(O.to_f16(_f32([bits]))[0]) == rounded and int(O.to_f16(_f32([bits | 0x80000000]))[0]) == rounded | 0x8000, name
    value = {n: float(_f32([b])[0]) for n, b, _, _ in F16_SPECIALS}
    assert value["2^-25: tie between 0 and 2^-24"] == 2.0 ** -25 and value["2^-24"] == 2.0 ** -24 and value["2^-14"] == 2.0 ** -14
    assert value["3 x 2^-25: tie over an odd neighbour"] == 3 * 2.0 ** -25 and value["65504"] == 65504.0 and value["65536"] == 65536.0
    assert value["65520: tie between 65504 and 2^16"] == 65520.0 and value["largest f32 below 65520"] == 65520.0 - 2.0 ** -8
    names, x = _f16_inputs()
    assert len(x) == 2 * (len(F16_SPECIALS) + 4096) and np.isfinite(x).sum() == len(x) - 2
    h = O.to_f16(x)
    assert ((h & 0x7C00) == 0).sum() > 1000 and ((h & 0x7FFF) == 0x7C00).sum() > 100      # subnormal / zero results and overflows among the seeded values
    for _, bits in F16_NANS:
        assert np.isnan(_f32([bits])[0])
    names, u = _u8_inputs()
    assert len(u) == 20 + 3 * 256
    want = O.to_u8(u)
    by_name = dict(zip(names, want.tolist()))
    assert by_name["NaN"] == 0 and by_name["0.99999994"] == 0 and by_name["1.0"] == 1 and by_name["254.99998"] == 254 and by_name["255.0"] == 255
    assert by_name["256"] == 255 and by_name["-0.5"] == 0 and by_name["+inf"] == 255 and by_name["-inf"] == 0 and by_name["255 + 0.99999"] == 255
    assert sorted(set(want.tolist())) == list(range(256))


def _cast_on_device(qa, x, dtype, width, on_device):
    import torch
    from qdrant_amd import _ffi as F
    x = np.ascontiguousarray(x, dtype=np.float32)
    if on_device:
        src, out = _on_device(x), torch.full((x.size * width,), SENTINEL, dtype=torch.uint8, device="cuda")
    else:
        src, out = x, np.full(x.size * width, SENTINEL, dtype=np.uint8)
    F.check(F.lib().qmx_cast_f32(0, dtype, F.ptr(src), x.size, F.ptr(out)))
    return out.cpu().numpy() if on_device else out


def _assert_same_ints(got, want, names, x, what):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if len(bad):
        i = int(bad[0])
        raise AssertionError("%s: element %d (%s, f32 0x%08X): got 0x%X, the oracle 0x%X; %d of %d differ"
                             % (what, i, names[i], _u32(x)[i], int(got[i]), int(want[i]), len(bad), len(want)))


@gpu
@pytest.mark.parametrize("on_device", [False, True])
def test_cast_f16(qa, on_device):
    from qdrant_amd import _ffi as F
    names, x = _f16_inputs()
    got = _cast_on_device(qa, x, F.DTYPE_F16, 2, on_device).view(np.uint16)
    _assert_same_ints(got, O.to_f16(x), names, x, "qmx_cast_f32 to f16, %s" % ("device" if on_device else "host"))


def _nan_report(got, want, what):
    for (name, bits), g, w in zip(F16_NANS, got.tolist(), want.tolist()):
        print("%s: %-36s f32 0x%08X -> device 0x%04X, oracle (F16C) 0x%04X" % (what, name, bits, g, w))


@gpu
def test_cast_f16_nan(qa):
    """NaN stays NaN with its sign, through the cast entry point and the query path.  Measured on gfx950: the payload bits are the oracle's (F16C's: the
    top ten mantissa bits, quiet bit set), for signalling inputs and for payloads in the low 13 bits alone as well - asserted."""
    from qdrant_amd import _ffi as F
    x = _f32([b for _, b in F16_NANS]).copy()
    want = O.to_f16(x)
    assert (((want & 0x7C00) == 0x7C00) & ((want & 0x03FF) != 0)).all()
    st = qa.VectorStorage(np.zeros((1, len(x)), dtype=np.float16), qa.Distance.Dot, qa.VectorStorageDatatype.Float16)
    scorer = qa.new_raw_scorer(x[None, :], st)
    for what, got in (("qmx_cast_f32", _cast_on_device(qa, x, F.DTYPE_F16, 2, True).view(np.uint16)), ("query", scorer.encoded_query(0).view(np.uint16))):
        _nan_report(got, want, what)
        assert (((got & 0x7C00) == 0x7C00) & ((got & 0x03FF) != 0)).all(), (what, [hex(v) for v in got])
        assert np.array_equal(got & 0x8000, (_u32(x) >> 16) & 0x8000), (what, [hex(v) for v in got])
        assert np.array_equal(got, want), (what, [hex(v) for v in got], [hex(v) for v in want])


@gpu
def test_cast_f16_as_queries(qa):
    """pack_queries_kernel: the same values as queries of a Dot f16 segment (no normalisation), dim = the chunk's length, chunks of at most 2048."""
    names, x = _f16_inputs()
    want = O.to_f16(x)
    for c0 in range(0, len(x), 2048):
        chunk = x[c0:c0 + 2048]
        st = qa.VectorStorage(np.zeros((1, len(chunk)), dtype=np.float16), qa.Distance.Dot, qa.VectorStorageDatatype.Float16)
        scorer = qa.new_raw_scorer(chunk[None, :], st)
        got = scorer.encoded_query(0).view(np.uint16)
        assert len(got) == len(chunk)
        _assert_same_ints(got, want[c0:c0 + 2048], names[c0:c0 + 2048], chunk, "f16 query of dim %d, values %d.." % (len(chunk), c0))
        scorer.close()
        st.close()


@gpu
@pytest.mark.parametrize("on_device", [False, True])
def test_cast_u8(qa, on_device):
    from qdrant_amd import _ffi as F
    names, x = _u8_inputs()
    got = _cast_on_device(qa, x, F.DTYPE_U8, 1, on_device)
    _assert_same_ints(got, O.to_u8(x), names, x, "qmx_cast_f32 to u8, %s" % ("device" if on_device else "host"))


def _u8_queries(dim):
    """the u8 inputs as rows of `dim` values (the last row padded with zeros) + the name of every element"""
    names, x = _u8_inputs()
    nq = -(-len(x) // dim)
    q = np.zeros(nq * dim, dtype=np.float32)
    q[:len(x)] = x
    return list(names) + ["padding"] * (nq * dim - len(x)), q.reshape(nq, dim)


@gpu
def test_cast_u8_as_queries(qa):
    """pack_queries_kernel at dim 33: the saturating cast of the queries of a Dot u8 segment, and - Cosine, dim >= 32 with a remainder - its norm1 block,
    through the scores of a Cosine u8 segment against the oracle's, bit for bit."""
    dim = 33
    names, queries = _u8_queries(dim)
    rng = np.random.default_rng(33)
    rows = rng.integers(0, 256, (64, dim), dtype=np.uint8)
    rows[0], rows[1], rows[2, :32], rows[3, 32] = 0, 255, 0, 0
    ids = np.arange(len(rows), dtype=np.uint32)
    for dist in (O.DOT, O.COSINE):
        st = qa.VectorStorage(rows, _dist(qa, dist), qa.VectorStorageDatatype.Uint8)
        ost = O.DenseStorage(O.U8, dist, rows)
        want_q = ost.encode_queries(queries)
        scorer = qa.new_raw_scorer(queries, st)
        got_q = np.stack([scorer.encoded_query(i) for i in range(len(queries))])
        _assert_same_ints(got_q.reshape(-1), want_q.reshape(-1), names, queries.reshape(-1), "u8 queries of dim 33, distance %d" % dist)
        got, want = scorer.score_points(ids), ost.score_points(queries, ids)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, "distance %d: query %d (values %s ..) x row %d: got %r, the oracle %r; %d scores differ" % (
            dist, bad[0][0], names[bad[0][0] * dim], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))
        scorer.close()
        st.close()


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. scores over the stored extremes
# ------------------------------------------------------------------------------------------------------------------------------------------------------
N_ROWS = 64
TINY = np.float32(2.0 ** -70)
F32_BLOCKS = ["tiny", "mixed", "subnormal rows"]
F32_TINY_NORMAL = float(np.finfo(np.float32).tiny)


@functools.lru_cache(maxsize=None)
def _f32_block(kind, dim):
    """(rows [64, dim], queries [64, dim]) f32: "tiny" = 2^-70 x Gaussian on both sides; "mixed" = every other row and query at unit scale; "subnormal rows" =
    f32 subnormal elements against unit queries."""
    rng = np.random.default_rng(3000 + dim + 17 * F32_BLOCKS.index(kind))
    rows = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    queries = rng.standard_normal((64, dim)).astype(np.float32)
    if kind == "tiny":
        rows, queries = rows * TINY, queries * TINY
    elif kind == "mixed":
        rows[::2] *= TINY
        queries[1::2] *= TINY
    else:
        rows = _subnormals(rng, (N_ROWS, dim)).copy()
    return _frozen(np.ascontiguousarray(rows)), _frozen(np.ascontiguousarray(queries))


@pytest.mark.parametrize("dist", [O.DOT, O.EUCLID])
@pytest.mark.parametrize("dim", [128, 100])
def test_f32_extreme_inputs_are_subnormal_where_they_claim(dist, dim):
    """Host only: in the tiny block every single product (squared difference) and every whole score is an f32 subnormal, nearly all of them nonzero; the
    subnormal rows give subnormal products; the mixed block spans both ranges."""
    rows, queries = _f32_block("tiny", dim)
    with np.errstate(under="ignore"):
        terms = (rows[:8, None, :] * queries[None, :8, :]) if dist == O.DOT else (rows[:8, None, :] - queries[None, :8, :]) ** 2
    assert (np.abs(terms) < F32_TINY_NORMAL).all() and (terms != 0).mean() > 0.95
    ids = np.arange(N_ROWS, dtype=np.uint32)
    want = O.DenseStorage(O.F32, dist, rows).score_points(queries, ids)
    assert (np.abs(want) < F32_TINY_NORMAL).all() and (want != 0).mean() > 0.99
    rows, queries = _f32_block("subnormal rows", dim)
    assert (np.abs(rows) < F32_TINY_NORMAL).all() and (rows != 0).all()
    want = O.DenseStorage(O.F32, dist, rows).score_points(queries, ids)
    assert (want != 0).all() if dist == O.DOT else (np.abs(want) > 1).all()      # (Euclid: the rows vanish beside unit queries, their bits must not change the sum)
    rows, queries = _f32_block("mixed", dim)
    want = np.abs(O.DenseStorage(O.F32, dist, rows).score_points(queries, ids))
    assert (want < F32_TINY_NORMAL).any() and (want > 1).any()


def _assert_lists(got, want, what):
    """peek_top lists: the oracle's score bits in the oracle's order (NaN first), the oracle's ids wherever a score occurs once."""
    assert len(got) == len(want), what
    for qi, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (what, qi)
        gs, ws = g["score"], w["score"]
        same = (gs.view(np.uint32) == ws.view(np.uint32)) | (np.isnan(gs) & np.isnan(ws))
        assert same.all(), "%s, query %d: scores %r, the oracle's %r" % (what, qi, gs, ws)
        uniq = np.array([not np.isnan(x) and (ws == x).sum() == 1 for x in ws], dtype=bool)
        assert np.array_equal(g["idx"][uniq], w["idx"][uniq]), "%s, query %d: ids %r, the oracle's %r" % (what, qi, g["idx"], w["idx"])


def _assert_top_of(lst, scores, what):
    """A peek_top list against the scan's own scores of all 64 rows: their greatest entries in order (NaN greatest, types.rs:21-25), bit for bit, each
    under an id that has that score."""
    nan = np.isnan(scores)
    order = sorted(range(len(scores)), key=lambda i: (not nan[i], 0.0 if nan[i] else -float(scores[i]), i))[:len(lst)]
    top = scores[order]
    same = (lst["score"].view(np.uint32) == top.view(np.uint32)) | (np.isnan(lst["score"]) & np.isnan(top))
    assert same.all(), "%s: scores %r, the greatest of the scan's scores %r" % (what, lst["score"], top)
    mine = scores[lst["idx"]]
    assert ((mine.view(np.uint32) == lst["score"].view(np.uint32)) | (np.isnan(mine) & np.isnan(lst["score"]))).all(), "%s: ids %r do not carry their scores" % (what, lst["idx"])
    assert len(set(lst["idx"].tolist())) == len(lst), what


def _run_f32_block(qa, dist, dim, kind):
    """Every batch size of one block through score_points and peek_top against the oracle; returns the kernels that served, by (call, nq)."""
    from qdrant_amd import _ffi as F
    rows, queries = _f32_block(kind, dim)
    st = qa.VectorStorage(rows, _dist(qa, dist))
    ost = O.DenseStorage(O.F32, dist, rows)
    ids = np.concatenate([np.arange(N_ROWS, dtype=np.uint32), np.array([63, 0, 31], dtype=np.uint32)])
    want_all = ost.score_points(queries, ids)
    served = {}
    for nq in (1, 16, 32) + ((64,) if dim == 128 else ()):
        what = "f32 %s block, distance %d, dim %d, %d queries" % (kind, dist, dim, nq)
        scorer = qa.new_raw_scorer(queries[:nq], st)
        got = scorer.score_points(ids)
        served[("score_points", nq)] = F.last_kernel(scorer._h)
        bad = np.argwhere(got.view(np.uint32) != want_all[:nq].view(np.uint32))
        assert len(bad) == 0, "%s (%s): query %d x row %d: got 0x%08X, the oracle 0x%08X; %d of %d scores differ" % (
            what, served[("score_points", nq)].split("<")[0], bad[0][0], ids[bad[0][1]], got.view(np.uint32)[tuple(bad[0])],
            want_all.view(np.uint32)[tuple(bad[0])], len(bad), got.size)
        scorer.close()
        s = qa.BatchFilteredSearcher(queries[:nq], st, 10)
        lists = s.peek_top_all()
        served[("peek_top", nq)] = F.last_kernel(s.scorer._h)
        _assert_lists(lists, ost.peek_top(queries[:nq], 10), what + " (%s)" % served[("peek_top", nq)].split("<")[0])
        s.scorer.close()
    st.close()
    return served


@gpu
@pytest.mark.parametrize("kind", F32_BLOCKS)
@pytest.mark.parametrize("dim", [128, 100])
@pytest.mark.parametrize("dist", [O.DOT, O.EUCLID])
def test_f32_scores_over_subnormals(qa, dist, dim, kind):
    _run_f32_block(qa, dist, dim, kind)


def _family(kernel):
    if "scan_f32_mfma16_kernel<" in kernel:
        return "scan_mfma16.hip"
    if "scan_f32_mfma_kernel<" in kernel:
        return "scan_mfma.hip"
    if ("scan_kernel<" in kernel or "scan_small_kernel<" in kernel) and "mfma" not in kernel:
        return "scan_common.hpp"
    return "other: " + kernel


@gpu
@pytest.mark.parametrize("kind", F32_BLOCKS)
def test_f32_extremes_reach_three_kernel_families(qa, kind):
    """The Dot block at dim 128 is served by the VALU scan, the 4x4x1 matrix-core scan and the chain-major 16x16x4 scan (64-query shape included): a
    re-routing that takes one of them away from these inputs fails here instead of emptying the comparison."""
    served = _run_f32_block(qa, O.DOT, 128, kind)
    families = {k: _family(v) for k, v in served.items()}
    assert {"scan_common.hpp", "scan_mfma.hip", "scan_mfma16.hip"} <= set(families.values()), served
    assert families[("score_points", 1)] == "scan_common.hpp", served
    assert families[("peek_top", 64)] == "scan_mfma16.hip", served
    # Euclid has no matrix-core scan: the VALU kernel serves every batch size
    assert {_family(v) for v in _run_f32_block(qa, O.EUCLID, 128, kind).values()} == {"scan_common.hpp"}


F16_SINGLE = slice(56, 64)      # the rows with one nonzero, subnormal element


@functools.lru_cache(maxsize=None)
def _f16_block(dim):
    """(rows [64, dim] f16 bits, queries [12, dim] f32).  Rows 0-15: Gaussian with subnormals and +-0 sprinkled in; 16-31: all subnormal; 32-39: a quarter
    of the elements +-65504; 40-43 a +inf, 44-47 a -inf, 48-51 both; 52-55 all +-65504; 56-63 one subnormal element, the rest +-0.  Queries 0-5 unit
    scale, 6-9 at 2^-20 (f16 subnormals after the cast), 10 all 65504, 11 +-65504."""
    rng = np.random.default_rng(1600 + dim)
    sign = lambda size: rng.integers(0, 2, size=size, dtype=np.uint16) << np.uint16(15)
    sub = lambda size: rng.integers(1, 0x400, size=size, dtype=np.uint16) | sign(size)
    rows = O.to_f16(rng.standard_normal((N_ROWS, dim)).astype(np.float32))
    pick = rng.random((16, dim))
    rows[:16] = np.where(pick < 0.25, sub((16, dim)), np.where(pick < 0.35, sign((16, dim)), rows[:16]))
    rows[16:32] = sub((16, dim))
    rows[32:40] = np.where(rng.random((8, dim)) < 0.25, np.uint16(0x7BFF) | sign((8, dim)), rows[32:40])
    for r in range(40, 52):
        cols = rng.permutation(dim)[:2]
        if r < 44 or r >= 48:
            rows[r, cols[0]] = 0x7C00
        if r >= 44:
            rows[r, cols[1]] = 0xFC00
    rows[52:56] = np.uint16(0x7BFF) | sign((4, dim))
    rows[F16_SINGLE] = sign((8, dim))
    for k, r in enumerate(range(56, 64)):
        rows[r, (k * 5 + 1) % dim] = [0x0001, 0x83FF, 0x0200, 0x8155, 0x03FF, 0x8001, 0x02AB, 0x0100][k]
    queries = rng.standard_normal((12, dim)).astype(np.float32)
    queries[6:10] *= np.float32(2.0 ** -20)
    queries[10] = 65504.0
    queries[11] = np.where(rng.integers(0, 2, dim) == 1, np.float32(-65504.0), np.float32(65504.0))
    return _frozen(rows), _frozen(queries)


def _f16_scale(dist, q16, rows16):
    """sum(abs(terms)) per (query, row) in f64: what the 1e-5 of the f16 bar is relative to (test_gpu_dense_f16_u8.py)"""
    with np.errstate(over="ignore", invalid="ignore"):
        q, v = O.f16_to_f32(q16).astype(np.float64), O.f16_to_f32(rows16).astype(np.float64)
        if dist in (O.DOT, O.COSINE):
            return np.abs(q[:, None, :] * v[None, :, :]).sum(-1)
        if dist == O.EUCLID:
            return ((q[:, None, :] - v[None, :, :]) ** 2).sum(-1)
        return np.abs(q[:, None, :] - v[None, :, :]).sum(-1)


def _assert_f16_scores(got, want, scale, exact, what):
    """Bits where `exact`; elsewhere the class and sign of every non-finite score and 1e-5 x sum|terms| for the finite ones."""
    same_bits = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    bad = np.argwhere(exact & ~same_bits)
    assert len(bad) == 0, "%s: query %d x row %d: got 0x%08X, the oracle 0x%08X (bits asserted); %d differ" % (
        what, bad[0][0], bad[0][1], got.view(np.uint32)[tuple(bad[0])], want.view(np.uint32)[tuple(bad[0])], len(bad))
    finite = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN scores at %r, the oracle's at %r" % (what, np.argwhere(np.isnan(got)).tolist(), np.argwhere(np.isnan(want)).tolist())
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), "%s: infinite scores differ in place or sign" % what
    assert np.isfinite(scale[finite]).all()
    err = np.abs(got[finite].astype(np.float64) - want[finite].astype(np.float64))
    worst = float((err / np.maximum(scale[finite], 1e-300)).max()) if finite.any() else 0.0
    assert (err <= 1e-5 * scale[finite] + 1e-30).all(), "%s: worst |error| / sum|terms| = %.3g" % (what, worst)


@gpu
@pytest.mark.parametrize("dim", [24, 64])
@pytest.mark.parametrize("dist", [O.DOT, O.COSINE, O.EUCLID, O.MANHATTAN])
def test_f16_scores_over_extremes(qa, dist, dim):
    rows16, queries = _f16_block(dim)
    st = qa.VectorStorage(rows16.view(np.float16), _dist(qa, dist), qa.VectorStorageDatatype.Float16)
    ost = O.DenseStorage(O.F16, dist, rows16)
    q16 = ost.encode_queries(queries)
    ids = np.arange(N_ROWS, dtype=np.uint32)
    want_all = ost.score_points(queries, ids)
    scale_all = _f16_scale(dist, q16, rows16)
    assert np.isnan(want_all).any() == (dist in (O.DOT, O.COSINE)) and np.isinf(want_all).any()
    # a single product of two f16 values is exact in f32, and so is its sum with zeros in any order: Dot / Cosine scores of the single-element rows
    exact = np.zeros(want_all.shape, dtype=bool)
    if dim < 32:
        exact[:] = True
    if dist in (O.DOT, O.COSINE):
        exact[:, F16_SINGLE] = True
        single = want_all[:, F16_SINGLE]
        assert np.isfinite(single).all() and (single != 0).mean() > 0.9      # (a subnormal times a query element that the cast took to zero is zero)
        assert dist == O.COSINE or (single[10:12] != 0).all()                # 65504 x subnormal: the product a flushing unit would lose
    for sel in ([0, 6, 10], list(range(12))):      # 3 queries: the VALU scan; 12: the f16 matrix-core scan where the distance has one
        what = "f16 extremes, distance %d, dim %d, queries %r" % (dist, dim, sel)
        scorer = qa.new_raw_scorer(queries[sel], st)
        for k, qi in enumerate(sel):
            _assert_same_ints(scorer.encoded_query(k).view(np.uint16), q16[qi], ["element %d" % i for i in range(dim)], queries[qi], what + ": encoded query %d" % qi)
        got = scorer.score_points(ids)
        _assert_f16_scores(got, want_all[sel], scale_all[sel], exact[sel], what)
        scorer.close()
        s = qa.BatchFilteredSearcher(queries[sel], st, 10)
        lists = s.peek_top_all()
        want_lists = ost.peek_top(queries[sel], 10)
        if dim < 32:
            _assert_lists(lists, want_lists, what)
        else:      # the scores above are the oracle's within the bar; the lists must be the ten greatest of exactly those scores, NaN greatest
            for k, (g, w) in enumerate(zip(lists, want_lists)):
                assert len(g) == len(w) == 10
                _assert_top_of(g, got[k], what + ": peek_top of query %d" % sel[k])
                assert np.isnan(g["score"]).sum() == np.isnan(w["score"]).sum() and np.array_equal(np.isposinf(g["score"]), np.isposinf(w["score"])), (what, k)
        s.scorer.close()
    st.close()


@gpu
def test_rows_of_2e19_normalise_to_zeros_and_score_zero(qa):
    """Cosine ingest on the device of rows whose sum of squares is +inf: stored as signed zeros (x / inf), 0.0 against every query, the oracle's bits."""
    import torch
    from qdrant_amd import _ffi as F
    dim, nq = 128, 16
    rng = np.random.default_rng(219)
    raw = np.where(rng.integers(0, 2, (N_ROWS, dim)) == 1, np.float32(-2e19), np.float32(2e19)).astype(np.float32)
    t = torch.from_numpy(raw.copy()).cuda()
    F.check(F.lib().qmx_preprocess_f32(0, int(qa.Distance.Cosine), F.ptr(t), N_ROWS, dim, F.ptr(t)))
    stored = O.preprocess(O.COSINE, raw)
    assert np.array_equal(_u32(stored), _u32(raw) & np.uint32(0x80000000))
    assert np.array_equal(_u32(t.cpu().numpy()), _u32(stored))
    st = qa.VectorStorage(t, qa.Distance.Cosine)
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    queries[1] = 2e19
    ids = np.arange(N_ROWS, dtype=np.uint32)
    want = O.DenseStorage(O.F32, O.COSINE, stored).score_points(queries, ids)
    assert (want == 0).all()
    for sel in ([0], [1], list(range(nq))):
        scorer = qa.new_raw_scorer(queries[sel], st)
        got = scorer.score_points(ids)
        assert (got == 0).all() and np.array_equal(got.view(np.uint32), want[sel].view(np.uint32)), sel
        scorer.close()
    st.close()
