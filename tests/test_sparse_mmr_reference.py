"""The restatement of MMR over sparse vectors (tests/sparse_mmr_reference.py) against the reference's own sparse MMR test and a hand-made case
in which the order of the sum decides the picks.  CPU only."""
import json
import os

import numpy as np

import fusion_reference as FR
import sparse_mmr_reference as SM

SPO = FR.ScoredPointOffset
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mmr_sparse_literals.json")

# the map case: under the map {1: 0, 3: 1, 2: 2} ascending remapped id visits the original dimensions as 1, 3, 2
MAP_POINTS = [([1, 2, 3], [1.0, 1.0, 1.0]), ([1, 2, 3], [1e8, 3.0, -1e8]), ([2], [0.5]), ([2], [1.0])]
MAP = {1: 0, 3: 1, 2: 2}
MAP_LAMBDA = 0.5
MAP_REQUESTS = [      # (query, candidate ids, limit, picks in original order, picks in remapped order)
    (([2], [1.0]), [0, 1, 2], 3, [1, 0, 2], [1, 2, 0]),
    (([1, 2, 3], [1.0, 1.0, 1.0]), [1, 3], 2, [3, 1], [1, 3]),
]


def candidates(ids, scores=None):
    c = np.zeros(len(ids), dtype=SPO)
    c["idx"] = ids
    c["score"] = np.arange(len(ids), 0, -1) if scores is None else scores
    return c


def literal_case():
    g = json.load(open(GOLDEN))
    points = {p["id"]: (p["indices"], p["values"]) for p in g["points"]}
    cand = candidates([p["id"] for p in g["points"]], [p["score"] for p in g["points"]])
    return g, points, (g["query"]["indices"], g["query"]["values"]), cand


def test_the_references_sparse_mmr_test():
    g, points, query, cand = literal_case()
    got = SM.mmr(points, query, cand, g["lambda"], g["limit"])
    assert len(got) == g["asserted_by_the_reference"]["result_len"]
    assert got["idx"].tolist() == g["derived_by_hand"]["order"]
    assert got["score"].tolist() == [0.0, 0.0, 0.0]      # the input scores
    # the tie the derivation rests on: after point 4, points 5 and 6 both score exactly 0.0
    rel6, sim64 = SM.score(query, points[6]), SM.score(points[6], points[4])
    assert np.float32(0.5) * rel6 - np.float32(0.5) * sim64 == 0.0
    assert SM.score(query, points[5]) == 0.0 and SM.score(points[5], points[4]) == 0.0


def test_no_overlap_and_empty_vectors_score_plus_zero():
    for a, b in ((([1], [-1.0]), ([2], [1.0])), (([], []), ([2], [1.0])), (([], []), ([], []))):
        s = SM.score(a, b)
        assert s == 0.0 and not np.signbit(s)


def test_the_order_of_the_sum_is_the_original_index_order():
    for query, ids, limit, original, remapped in MAP_REQUESTS:
        got = SM.mmr(MAP_POINTS, query, candidates(ids), MAP_LAMBDA, limit)
        wrong = SM.mmr(MAP_POINTS, query, candidates(ids), MAP_LAMBDA, limit, remapped_order=MAP)
        assert got["idx"].tolist() == original
        assert wrong["idx"].tolist() == remapped
        assert original != remapped      # the device test over this case discriminates between the two rules
    # the sums behind request 2: 1e8 + 3 - 1e8 in original order loses the 3, in remapped order (1e8 - 1e8 + 3) keeps it
    assert SM.score(MAP_REQUESTS[1][0], MAP_POINTS[1]) == 0.0
    assert SM.score(MAP_REQUESTS[1][0], MAP_POINTS[1], remapped_order=MAP) == 3.0


def test_the_column_restatement_equals_the_pair_restatement():
    """mmr_columns (what the device tests use for long candidate lists) against mmr, on rows whose scores tie (small integer weights) and on
    float weights, with duplicated ids, an empty row, and limits below, at and above the number of candidates."""
    rng = np.random.default_rng(5)
    n, n_dims = 60, 12
    for weights in ("integer", "float"):
        points = [([], [])]
        for _ in range(n - 1):
            k = int(rng.integers(0, 7))
            ix = rng.choice(n_dims, size=k, replace=False)
            vx = rng.choice([-2.0, -1.0, 1.0, 2.0], size=k) if weights == "integer" else rng.standard_normal(k)
            points.append((ix.astype(np.uint32), vx.astype(np.float32)))
        dense = SM.Dense(points, n_dims)
        for c, limit in ((0, 3), (1, 3), (2, 1), (25, 6), (25, 25), (40, 43)):
            ids = rng.choice(n, size=c, replace=True)
            cand = candidates(ids, np.sort(rng.standard_normal(c).astype(np.float32))[::-1])
            query = points[int(rng.integers(1, n))]
            for lambda_ in (0.0, 0.5, 1.0):
                want = SM.mmr(points, query, cand, lambda_, limit)
                for matrix in (True, False):
                    got = SM.mmr_columns(dense, query, cand, lambda_, limit, matrix=matrix)
                    assert got["idx"].tolist() == want["idx"].tolist(), (weights, c, limit, lambda_, matrix)
                    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32))
