"""The numpy restatement of sparse scoring (tests/sparse_reference.py) against the reference's literal cases and against the per-pair merge
loop of score_vectors; and the library's refusal without a device.  CPU only."""
import json
import os

import numpy as np
import pytest

import sparse_reference as SR

HERE = os.path.dirname(os.path.abspath(__file__))


def _literals():
    with open(os.path.join(HERE, "golden", "sparse_vector_literals.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _literals(), ids=lambda c: c["name"])
def test_restatement_reproduces_the_reference_literals(case):
    (ai, av), (bi, bv) = case["a"], case["b"]
    s, ov = SR.score_pair(*SR.sort_vector(ai, av), *SR.sort_vector(bi, bv))
    if case["score"] is None:
        assert not ov
    else:
        assert ov and s == np.float32(case["score"])
    st = SR.Restatement([(ai, av)])
    sc, overlap = st.score_matrix([st.prepare_query(bi, bv)])
    assert bool(overlap[0, 0]) == (case["score"] is not None)
    assert sc[0, 0] == np.float32(case["score"] if case["score"] is not None else 0.0)


def _random_rows(rng, n, n_dims, nnz, signed):
    rows = []
    for _ in range(n):
        k = int(rng.integers(0, nnz + 1))
        ix = rng.choice(n_dims, size=k, replace=False).astype(np.uint32)
        vx = rng.standard_normal(k).astype(np.float32) if signed else rng.lognormal(0.0, 1.0, k).astype(np.float32)
        rows.append((ix, vx))
    return rows


@pytest.mark.parametrize("signed", [False, True])
def test_dimension_major_sums_equal_the_pair_merge_loop(signed):
    rng = np.random.default_rng(7 + signed)
    rows = _random_rows(rng, 300, 60, 25, signed)
    queries = _random_rows(rng, 6, 60, 20, signed)
    st = SR.Restatement(rows)
    prepared = [st.prepare_query(*q) for q in queries]
    sc, overlap = st.score_matrix(prepared)
    for qi, (qx, qv) in enumerate(prepared):
        for p, (rx, rv) in enumerate(st.rows):
            s, ov = SR.score_pair(rx, rv, qx, qv)
            assert ov == overlap[qi, p]
            assert np.float32(s).view(np.uint32) == sc[qi, p].view(np.uint32), (qi, p)


def test_remap_vector_drops_unknown_and_resorts():
    ix, vx = SR.remap_vector([5, 1, 9], [1.0, 2.0, 3.0], {1: 7, 5: 2})
    assert ix.tolist() == [2, 7] and vx.tolist() == [1.0, 2.0]


def test_duplicates_and_length_mismatch_are_invalid():
    with pytest.raises(ValueError):
        SR.sort_vector([1, 1], [1.0, 2.0])
    with pytest.raises(ValueError):
        SR.sort_vector([1, 2], [1.0])


def test_search_returns_only_overlapping_points():
    st = SR.Restatement([([1, 2], [1.0, 1.0]), ([3], [5.0]), ([2, 3], [-1.0, 1.0])])
    got = st.search([st.prepare_query([2, 3], [1.0, 1.0])], 10)[0]
    assert got["idx"].tolist() == [1, 0, 2] and got["score"].tolist() == [5.0, 1.0, 0.0]    # the exact 0.0 of row 2 overlaps: returned


def test_sparse_storage_without_a_device_is_refused():
    import qdrant_amd as qa
    from qdrant_amd import _ffi as F
    try:
        have = qa.device_count()
    except F.QmxError:
        have = 0
    if have > 0:
        pytest.skip("a device is present: tests/test_gpu_sparse.py covers the storage")
    with pytest.raises(F.QmxError) as e:
        qa.SparseVectorStorage([([1, 2], [1.0, 2.0])])
    assert e.value.status == F.ERR_NO_DEVICE
