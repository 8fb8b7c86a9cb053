"""The Euclid int8 prefilter's band (qdrant_amd/csrc/l2i8_band.hpp) at 1 152 coordinates, where the integer of a pair passes 2^24 and the epilogue's
fl32(I) is rounded (term (6), e_I = 1): test_l2i8_band.py's check with the score formed from the ROUNDED integer, as scan_l2i8_staged_kernel forms it."""
import ctypes as C

import numpy as np
import pytest

import oracle_ffi as O
from test_l2i8_band import _codes, _ru32, band_lib      # noqa: F401  (the fixture compiles tools/l2i8_band_check.cpp)

N, DIM, NQ, TOP, U = 2000, 1152, 16, 10, 2.0 ** -24


def test_every_pair_lies_inside_the_band_when_the_integer_is_rounded(band_lib):
    """Rows sign * (1 + 0.01 synth) with as many rows of either sign per column (mu = 0: both signs keep codes near +-122), queries = stored rows + 0.01
    synth: I of a query and its source row is above 17 M > 2^24.  The band is a worst case (|A - R| reaches 6 % of it here), so no pair of any seed leaves
    it for want of 2 t e_I alone; what fails without term (6) is the first assertion: the band covers the float64 sum of the derivation's six terms."""
    signs = np.random.default_rng(5).permuted(np.tile(np.array([[1.0], [-1.0]], dtype=np.float32), (N // 2, DIM)), axis=0)
    rows = np.ascontiguousarray(signs * (np.float32(1.0) + np.float32(0.01) * O.synth(0x5EED0B40, 0, N, DIM)), dtype=np.float32)
    queries = np.ascontiguousarray(rows[::N // NQ][:NQ] + 0.01 * O.synth(0x5EED0B41, 0, NQ, DIM), dtype=np.float32)
    ref = O.DenseStorage(O.F32, O.EUCLID, rows).score_points(queries, np.arange(N, dtype=np.uint32)).astype(np.float64)
    mu = (rows.astype(np.float64).sum(0) / N).astype(np.float32).astype(np.float64)      # the segment's side, as l2_colsum_kernel .. l2_copy_kernel
    y = rows.astype(np.float64) - mu
    s = (_ru32(np.abs(y).max(0)) / np.float32(127.0)).astype(np.float32).astype(np.float64)
    c, n_r = _codes(y / s), (y * y).sum(1)
    n32, c1, c2, n_max = n_r.astype(np.float32).astype(np.float64), np.abs(c).sum(1).max(), np.sqrt((c * c).sum(1).max()), float(_ru32(n_r).max())
    u = (queries.astype(np.float64) - mu) * s                                             # the queries' side, as l2i8_pack_kernel
    q_n = ((queries.astype(np.float64) - mu) ** 2).sum(1)
    t = _ru32(np.abs(u).max(1) / 127.0).astype(np.float64)
    d = _codes(u / t[:, None])
    sum_d, f_norm = np.abs(d).sum(1), np.sqrt(((u / t[:, None] - d) ** 2).sum(1))
    band = np.array([band_lib.qmx_l2i8_band(t[j], sum_d[j], f_norm[j], q_n[j], c1, c2, n_max, DIM) for j in range(NQ)], dtype=np.float64)
    dot2, sq = 2.0 * t * (np.minimum(0.5 * c1, c2 * f_norm) + 0.5 * sum_d + 0.25 * DIM) * 1.001, n_max + q_n      # terms (1) .. (6), e_I = 1
    assert np.all(band >= dot2 + U * sq + 2.0 ** -36 * sq + (DIM + 16.0) * 4.0 * U * sq + 2.0 * U * (2.0 * sq + dot2 + 2.0 * t) + 2.0 * t)
    dot = d @ c.T
    fi = dot.astype(np.float32).astype(np.float64)                                        # the epilogue: even integers above 2^24
    assert np.all(np.abs(dot).max(1) > 2 ** 24) and np.abs(dot).max() < 2 ** 25 and np.any(fi != dot)
    a = ((2.0 * t[:, None] * fi - n32).astype(np.float32) - q_n.astype(np.float32)[:, None]).astype(np.float64)
    assert np.all(np.abs(a - ref) <= band[:, None]), float((np.abs(a - ref) / band[:, None]).max())
    cut = np.sort(ref[:, ::8], axis=1)[:, -TOP] - band                                    # T_q of a strided sample, less the band
    for j in range(NQ):
        assert np.all(a[j, np.argsort(-ref[j], kind="stable")[:TOP]] >= cut[j])
        ca, cb = C.c_float(), C.c_float()
        band_lib.qmx_l2i8_compare_coefs(cut[j], t[j], q_n[j], n_max, DIM, C.byref(ca), C.byref(cb))
        admitted = (fi[j] - float(cb.value) * n32).astype(np.float32) >= np.float32(ca.value)
        assert np.all(admitted[(a[j] >= cut[j]) | (2.0 * t[j] * dot[j] - n32 - q_n[j] >= cut[j])]) and admitted.sum() < N      # (the rounded and the exact integer's score)


# the bits of the header before term (6) existed, for t = 5 / 1024, sum |d| = 40 dim, |f| = 0.29 sqrt(dim), Q = 1.5 dim, C1 = 45 dim, C2 = 60 sqrt(dim),
# max N = 2.25 dim, cut = -0.75 dim: (band, compare a, compare b)
@pytest.mark.parametrize("dim,bits", [(128, (0x423C8145, 0x46199495, 0x42CCCCCD)), (768, (0x438D9934, 0x476663DF, 0x42CCCCCD)),
                                      (1024, (0x43BCEA45, 0x47999815, 0x42CCCCCD))])
def test_rows_of_up_to_1024_coordinates_keep_their_bits(band_lib, dim, bits):
    b = band_lib.qmx_l2i8_band(5.0 / 1024.0, 40.0 * dim, 0.29 * dim ** 0.5, 1.5 * dim, 45.0 * dim, 60.0 * dim ** 0.5, 2.25 * dim, dim)
    ca, cb = C.c_float(), C.c_float()
    band_lib.qmx_l2i8_compare_coefs(-0.75 * dim, 5.0 / 1024.0, 1.5 * dim, 2.25 * dim, dim, C.byref(ca), C.byref(cb))
    assert tuple(int(np.float32(v).view(np.uint32)) for v in (b, ca.value, cb.value)) == bits
