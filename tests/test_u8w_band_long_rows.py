"""The band and the compare of the dense-u8 128-query pass (qdrant_amd/csrc/u8w_band.hpp) at the rows of the staged scan: dim 1088, its shortest, and 2048,
where the derivation ends (a lane total of the AVX2 leaf just under 2^24, a total just under 2^27).  test_u8w_band.py's every-pair condition against the
oracle's u8 leaves in both summation orders; a condition, not a tolerance: no pair is left out."""
import numpy as np
import pytest

import oracle_ffi as O
from test_u8w_band import METRIC, band_lib  # noqa: F401  (the fixture builds tools/u8w_band_check.cpp)

N, NQ, TOP = 300, 12, 10


def _block(kind, dim):
    rng = np.random.default_rng(dim + len(kind))
    lo = 200 if kind == "hot" else 0
    rows = rng.integers(lo, 256, (N, dim), dtype=np.uint8)
    queries = rng.integers(lo, 256, (NQ, dim), dtype=np.uint8)
    rows[0], rows[1], rows[2], rows[3] = 0, 255, 127, 128
    queries[0], queries[1], queries[2] = 255, 0, 128
    return np.ascontiguousarray(rows), np.ascontiguousarray(queries)


@pytest.mark.parametrize("scalar_order", [False, True])
@pytest.mark.parametrize("dim", [1088, 2048])
@pytest.mark.parametrize("kind", ["hot", "uniform"])
@pytest.mark.parametrize("dist", [O.DOT, O.EUCLID, O.COSINE])
def test_every_pair_of_a_long_row_lies_inside_the_band_and_the_compare_admits_the_cut(band_lib, dist, kind, dim, scalar_order):  # noqa: F811
    rows, queries = _block(kind, dim)
    ost = O.DenseStorage(O.U8, dist, rows, u8_isa=O.ISA_SCALAR if scalar_order else O.ISA_AVX)
    ref = ost.score_points(queries, np.arange(N, dtype=np.uint32), encoded=True).astype(np.float64)      # R, [NQ][N]
    rejected = 0
    for j in range(NQ):
        band = float(band_lib.qmx_u8w_band(METRIC[dist], int(scalar_order), queries[j].ctypes.data, dim))
        cut = float(np.sort(ref[j, ::4])[-TOP]) - band      # T_q of a strided sample, less the band
        a, admit = np.empty(N, dtype=np.float32), np.empty(N, dtype=np.uint8)
        band_lib.qmx_u8w_pass(METRIC[dist], queries[j].ctypes.data, rows.ctypes.data, N, dim, cut, a.ctypes.data, admit.ctypes.data)
        a = a.astype(np.float64)
        assert np.all(np.abs(a - ref[j]) <= band), (j, float(np.abs(a - ref[j]).max()), band)
        assert np.all(admit[a >= cut] == 1)
        rejected += int((admit == 0).sum())
    assert rejected > 0      # (the compare is not vacuous)
