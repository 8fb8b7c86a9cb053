"""tests/matrix_reference.py against the reference's own unit-test fixture and hand-written cases (no device): the sampler's key in its two forms, the
nearest lists of a score matrix, the two response conversions - and the same conversions as qdrant_amd.SearchMatrix makes them."""
import json
import os

import numpy as np

import matrix_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrix_conversion.json")


def _fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def test_key_numpy_and_python_int_forms_agree():
    for seed in (0, 1, 0x5EED0001, R.M64, 1 << 63):
        offsets = np.concatenate([np.arange(9000), np.arange(0xFFFFFFFF - 1000, 0xFFFFFFFF)]).astype(np.uint64)
        assert len(offsets) == 10000
        got = R.sample_keys_np(seed, offsets)
        want = np.array([R.sample_key_int(seed, int(o)) for o in offsets], dtype=np.uint64)
        assert np.array_equal(got, want)


def test_key_frozen_values():
    for seed, offset, key in R.FROZEN_KEYS:
        assert R.sample_key_int(seed, offset) == key
        assert int(R.sample_keys_np(seed, [offset])[0]) == key


def test_keys_of_distinct_offsets_differ():
    keys = R.sample_keys_np(7, np.arange(200000))
    assert len(np.unique(keys)) == len(keys)


def test_sample_reference():
    live = np.ones(100, dtype=bool)
    live[::3] = False
    cand = np.flatnonzero(live)
    keys = {int(o): R.sample_key_int(5, int(o)) for o in cand}
    want = sorted(sorted(cand.tolist(), key=lambda o: (keys[o], o))[:10])
    assert R.sample_reference(live, 10, 5).tolist() == want
    assert R.sample_reference(live, 1000, 5).tolist() == cand.tolist()      # n past the candidates: all of them, ascending
    assert R.sample_reference(live, 0, 5).tolist() == []
    assert R.sample_reference(np.zeros(10, dtype=bool), 3, 5).tolist() == []
    assert R.sample_reference(live, 10, 6).tolist() != want                  # (the seed matters)


def test_matrix_reference_hand_written():
    # dot products of rows of very different length: self is not the best of row 0 and 1; rows 2 and 3 are duplicates, so self ties with the twin
    v = np.array([[1, 0], [2, 0], [3, 1], [3, 1]], dtype=np.float32)
    sc = v @ v.T
    live = np.ones(4, dtype=bool)
    got = R.matrix_reference(sc, live, 2)
    assert [c.tolist() for c, _ in got] == [[2, 3], [2, 3], [3, 1], [2, 1]]
    assert [s.tolist() for _, s in got] == [[3.0, 3.0], [6.0, 6.0], [10.0, 6.0], [10.0, 6.0]]
    # limit past the others: clipped to S - 1, order kept
    got = R.matrix_reference(sc, live, 7)
    assert [c.tolist() for c, _ in got] == [[2, 3, 1], [2, 3, 0], [3, 1, 0], [2, 1, 0]]
    # a deleted point keeps its row and is nobody's neighbour
    live[2] = False
    got = R.matrix_reference(sc, live, 2)
    assert [c.tolist() for c, _ in got] == [[3, 1], [3, 0], [3, 1], [1, 0]]


def test_matrix_reference_empty_cases():
    assert R.matrix_reference(np.zeros((0, 0), np.float32), [], 3) == []
    one = R.matrix_reference(np.ones((1, 1), np.float32), [True], 3)
    assert len(one) == 1 and len(one[0][0]) == 0
    assert all(len(c) == 0 for c, _ in R.matrix_reference(np.ones((3, 3), np.float32), [True] * 3, 0))
    assert all(len(c) == 0 for c, _ in R.matrix_reference(np.ones((3, 3), np.float32), [False] * 3, 2))


def test_pairs_conversion_on_the_reference_fixture():
    fx = _fixture()
    got = R.pairs_reference(fx["sample_ids"], fx["nearests"])
    assert [(int(a), int(b)) for a, b, _ in got] == [(a, b) for a, b, _ in fx["pairs"]]
    assert np.array_equal(got["score"], np.array([s for _, _, s in fx["pairs"]], dtype=np.float32))


def test_offsets_conversion_on_the_reference_fixture():
    fx = _fixture()
    rows, cols, scores, ids = R.offsets_reference(fx["sample_ids"], fx["nearests"])
    assert rows.tolist() == fx["offsets_row"] and cols.tolist() == fx["offsets_col"]
    assert np.array_equal(scores, np.array(fx["scores"], dtype=np.float32)) and list(ids) == fx["sample_ids"]


def test_search_matrix_class_converts_as_the_reference_does():
    import qdrant_amd as qa
    fx = _fixture()
    ids = np.array(fx["sample_ids"], dtype=np.uint32)
    nearests = [np.array([(b, s) for b, s in row], dtype=qa.ScoredPointOffset) for row in fx["nearests"]]
    cols = [np.array([fx["sample_ids"].index(b) for b, _ in row], dtype=np.uint32) for row in fx["nearests"]]
    m = qa.SearchMatrix(ids, nearests, cols)
    assert np.array_equal(m.pairs(), R.pairs_reference(fx["sample_ids"], fx["nearests"]))
    for got, want in zip(m.offsets(), R.offsets_reference(fx["sample_ids"], fx["nearests"])):
        assert np.array_equal(got, want)
