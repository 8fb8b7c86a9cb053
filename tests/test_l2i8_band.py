"""The band of the Euclid int8 prefilter (qdrant_amd/csrc/l2i8_band.hpp, derived there term by term) against float64: blocks quantised in numpy as
scan_l2i8.hip's kernels do it, every (query, row) pair within the band of the oracle's f32 Euclid score, the true top-k inside the cut, and the
epilogue's compare admitting every pair the cut admits.  A condition, not a tolerance: no pair is left out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DIM, NQ, TOP = 2000, 128, 32, 10


@pytest.fixture(scope="module")
def band_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("l2i8") / "l2i8_band_check.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "qdrant_amd", "csrc"),
                           os.path.join(ROOT, "tools", "l2i8_band_check.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.qmx_l2i8_band.restype = C.c_float
    lib.qmx_l2i8_band.argtypes = [C.c_double] * 7 + [C.c_uint32]
    lib.qmx_l2i8_compare_coefs.restype = None
    lib.qmx_l2i8_compare_coefs.argtypes = [C.c_double] * 4 + [C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    return lib


def _ru32(x):
    """f64 -> f32, rounded up"""
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f)


def _codes(v):
    return np.clip(np.rint(v), -127.0, 127.0)


@pytest.mark.parametrize("kind", ["plain", "shifted", "outlier_columns"])
def test_every_pair_lies_inside_the_band(band_lib, kind):
    rows = O.synth(0x5EED0A00, 0, N, DIM)
    if kind == "shifted":
        rows = rows + np.float32(50.0)
    elif kind == "outlier_columns":
        rows[:, :3] *= 40.0
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    queries = np.ascontiguousarray(rows[::N // NQ][:NQ] + 0.1 * O.synth(0x5EED0A01, 0, NQ, DIM), dtype=np.float32)
    ref = O.DenseStorage(O.F32, O.EUCLID, rows).score_points(queries, np.arange(N, dtype=np.uint32)).astype(np.float64)      # R, [NQ][N]
    # the segment's side (l2_colsum_kernel .. l2_copy_kernel)
    mu = (rows.astype(np.float64).sum(0) / N).astype(np.float32).astype(np.float64)
    y = rows.astype(np.float64) - mu
    colmax = _ru32(np.abs(y).max(0))
    s = np.where(colmax > 1e-30, colmax / np.float32(127.0), np.float32(1.0)).astype(np.float32).astype(np.float64)
    c = _codes(y / s)
    n_r = (y * y).sum(1)
    n32 = n_r.astype(np.float32)
    c1, c2, n_max = np.abs(c).sum(1).max(), np.sqrt((c * c).sum(1).max()), float(_ru32(n_r).max())
    # the queries' side (l2i8_pack_kernel)
    p = queries.astype(np.float64) - mu
    u = p * s
    t32 = _ru32(np.abs(u).max(1) / 127.0)
    t = t32.astype(np.float64)[:, None]
    d = _codes(u / t)
    f = u / t - d
    q_n = (p * p).sum(1)
    band = np.array([band_lib.qmx_l2i8_band(float(t[j, 0]), float(np.abs(d[j]).sum()), float(np.sqrt((f[j] * f[j]).sum())), float(q_n[j]), c1, c2, n_max, DIM)
                     for j in range(NQ)], dtype=np.float64)
    # the epilogue (scan_l2i8_kernel): I exact, A = fma(2 t, I, -N_r) - Q in f32
    dot = d @ c.T
    assert np.abs(dot).max() < 2 ** 24
    a = ((2.0 * t * dot - n32.astype(np.float64)).astype(np.float32) - q_n.astype(np.float32)[:, None]).astype(np.float64)
    assert np.all(np.abs(a - ref) <= band[:, None]), float((np.abs(a - ref) / band[:, None]).max())
    # T_q: the k-th best exact score of a strided sample; the true top-k lies inside A >= T_q - band, and the compare admits every such pair
    t_q = np.sort(ref[:, ::8], axis=1)[:, -TOP]
    cut = t_q - band
    for j in range(NQ):
        best = np.argsort(-ref[j], kind="stable")[:TOP]
        assert np.all(a[j, best] >= cut[j])
        ca, cb = C.c_float(), C.c_float()
        band_lib.qmx_l2i8_compare_coefs(float(cut[j]), float(t[j, 0]), float(q_n[j]), n_max, DIM, C.byref(ca), C.byref(cb))
        admitted = (dot[j] - float(cb.value) * n32.astype(np.float64)).astype(np.float32) >= np.float32(ca.value)
        assert np.all(admitted[a[j] >= cut[j]])
        assert admitted.sum() < N      # (and it does reject: the compare is not vacuous)
