"""The band and the compare of the dense-u8 128-query pass (qdrant_amd/csrc/u8w_band.hpp, derived there term by term) against the oracle's u8 leaves: for
every (query, row) pair of small adversarial blocks the pass's score lies within the band of the oracle's f32 score in both summation orders, and the
scan's integer / float compare admits every pair the cut admits.  A condition, not a tolerance: no pair is left out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRIC = {O.DOT: 0, O.EUCLID: 1, O.COSINE: 3}      # u8w_band.hpp U8W_*
N, NQ, TOP = 300, 12, 10


@pytest.fixture(scope="module")
def band_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("u8w") / "u8w_band_check.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "qdrant_amd", "csrc"),
                           os.path.join(ROOT, "tools", "u8w_band_check.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.qmx_u8w_band.restype = C.c_float
    lib.qmx_u8w_band.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint32]
    lib.qmx_u8w_pass.restype = None
    lib.qmx_u8w_pass.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p]
    return lib


def _block(kind, dim):
    """uniform: every byte value, the bias' corners (0, 127, 128, 255) planted as whole rows; hot: 200..255 - at dim 1024 the totals pass 2^24, where the
    AVX2 leaf's f32 sums stop being a function of the integer; ties: nine distinct rows"""
    rng = np.random.default_rng(dim + len(kind))
    lo = 200 if kind == "hot" else 0
    rows = rng.integers(lo, 256, (N, dim), dtype=np.uint8)
    queries = rng.integers(lo, 256, (NQ, dim), dtype=np.uint8)
    if kind == "ties":
        rows = rows[rng.integers(0, 9, N)]
    rows[0], rows[1], rows[2], rows[3] = 0, 255, 127, 128
    queries[0], queries[1], queries[2] = 255, 0, 128
    queries[3] = rows[7]
    return np.ascontiguousarray(rows), np.ascontiguousarray(queries)


@pytest.mark.parametrize("scalar_order", [False, True])
@pytest.mark.parametrize("kind,dim", [("uniform", 64), ("uniform", 192), ("hot", 1024), ("ties", 1024)])
@pytest.mark.parametrize("dist", [O.DOT, O.EUCLID, O.COSINE])
def test_every_pair_lies_inside_the_band_and_the_compare_admits_the_cut(band_lib, dist, kind, dim, scalar_order):
    rows, queries = _block(kind, dim)
    ost = O.DenseStorage(O.U8, dist, rows, u8_isa=O.ISA_SCALAR if scalar_order else O.ISA_AVX)
    ref = ost.score_points(queries, np.arange(N, dtype=np.uint32), encoded=True).astype(np.float64)      # R, [NQ][N]
    rejected = 0
    for j in range(NQ):
        band = float(band_lib.qmx_u8w_band(METRIC[dist], int(scalar_order), queries[j].ctypes.data, dim))
        if scalar_order and dist != O.COSINE:
            assert band == 0.0
        # T_q: the k-th best exact score of a strided sample, a lower bound of the final k-th best
        cut = float(np.sort(ref[j, ::4])[-TOP]) - band
        a, admit = np.empty(N, dtype=np.float32), np.empty(N, dtype=np.uint8)
        band_lib.qmx_u8w_pass(METRIC[dist], queries[j].ctypes.data, rows.ctypes.data, N, dim, cut, a.ctypes.data, admit.ctypes.data)
        a = a.astype(np.float64)
        assert np.all(np.abs(a - ref[j]) <= band), (j, float(np.abs(a - ref[j]).max()), band)
        best = np.argsort(-ref[j], kind="stable")[:TOP]
        assert np.all(a[best] >= cut)
        assert np.all(admit[a >= cut] == 1)
        rejected += int((admit == 0).sum())
    assert rejected > 0      # (the compare is not vacuous)
