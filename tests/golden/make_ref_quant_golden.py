#!/usr/bin/env python3
"""Records what the reference's own C quantization kernels (lib/quantization/cpp/avx2.c, sse.c, compiled unchanged into oracle/_ref by
oracle/Makefile where the reference tree is present) return on the inputs of the tests that pin the oracle and the device to them, into
tests/golden/ref_quant_kernels.npz.  The tests read that file, so they need no oracle/_ref; where it is built they check the live kernels
against the recorded bits as well.

  make -C oracle && python tests/golden/make_ref_quant_golden.py

Keys (all uint32):
  sq_leaves               [10 dims, 20 draws, 4]  f32 bits of impl_score_{dot,l1}_{avx,sse}   (test_oracle_golden.test_sq_leaves_match_reference_c_kernels)
  sq_leaf_dot_avx_worst   [1]                     impl_score_dot_avx on all-127 codes, dim 2064
  bq_xor_popcnt_sse       [7 word counts, 20]     impl_xor_popcnt_sse_uint128                 (test_oracle_bq.test_xor_popcnt_matches_the_reference_c_kernel)
  bq_xor_popcnt_scalar{4,8} [8 word counts, 20, 2] impl_xor_popcnt_scalar{4,8}_{avx,sse}_uint128 (test_oracle_bq.test_scalar_xor_popcnt_matches_the_reference_c_kernels)
  sq_scores_<case>        [queries, ids]          f32 bits of the oracle's SQ scores with the reference's leaves (test_gpu_sq.test_sq_matches_reference_c_kernels)
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import oracle_ffi as O  # noqa: E402
import test_gpu_sq  # noqa: E402
import test_oracle_bq  # noqa: E402
import test_oracle_golden  # noqa: E402


def _bits(x):
    return np.float32(x).view(np.uint32)


def main():
    ref = O.load_ref_quant()
    if ref is None:
        sys.exit("oracle/_ref/libqdrant_ref_quant.so is not built (make -C oracle, with the reference tree present)")
    out = {}
    g = test_oracle_golden
    leaves = np.zeros((len(g.SQ_LEAF_DIMS), 20, len(g.SQ_LEAF_NAMES)), dtype=np.uint32)
    for di, it, dim, q, v in g.sq_leaf_cases():
        pq, pv = C.c_void_p(q.ctypes.data), C.c_void_p(v.ctypes.data)
        leaves[di, it] = [_bits(getattr(ref, f)(pq, pv, dim)) for f in g.SQ_LEAF_NAMES]
    out["sq_leaves"] = leaves
    worst = np.full(2064, 127, dtype=np.uint8)
    pw = C.c_void_p(worst.ctypes.data)
    out["sq_leaf_dot_avx_worst"] = np.array([_bits(ref.impl_score_dot_avx(pw, pw, 2064))], dtype=np.uint32)

    b = test_oracle_bq
    fn = b._ref_xor_fn(ref, "impl_xor_popcnt_sse_uint128")
    xs = np.zeros((len(b.XOR_WORDS), 20), dtype=np.uint32)
    for wi, it, words, q, v in b.xor_popcnt_cases():
        xs[wi, it] = fn(q.ctypes.data, v.ctypes.data, words)
    out["bq_xor_popcnt_sse"] = xs
    for bits in (4, 8):
        fns = [b._ref_xor_fn(ref, "impl_xor_popcnt_scalar%d_%s_uint128" % (bits, isa)) for isa in ("avx", "sse")]
        sx = np.zeros((len(b.SCALAR_XOR_WORDS), 20, 2), dtype=np.uint32)
        for wi, it, words, v, q in b.scalar_xor_popcnt_cases(bits):
            sx[wi, it] = [f(q.ctypes.data, v.ctypes.data, words) for f in fns]
        out["bq_xor_popcnt_scalar%d" % bits] = sx

    import qdrant_amd as qa       # (host-side quantizer parameters only: no device is used)
    for key, rows, quant, queries, qpre, osq, ids in test_gpu_sq.ref_kernel_cases(qa, O.ISA_REF):
        out["sq_scores_" + key] = osq.score_points(qpre, ids).view(np.uint32)

    path = O.REF_GOLDEN_PATH
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes): %s" % (path, os.path.getsize(path), ", ".join("%s %s" % (k, v.shape) for k, v in out.items())))


if __name__ == "__main__":
    main()
