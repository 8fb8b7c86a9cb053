"""The numpy restatement of the reference's fusion and MMR code (tests/fusion_reference.py) reproduces the literals of the reference's own unit tests
(tests/golden/fusion_literals.json), its Welford recurrence agrees with float64 within the reference's own assert_close, and a hand-made MMR
case with exact ties pins the IndexSet / last-max order.  CPU only."""
import json
import os

import numpy as np
import pytest

import fusion_reference as FR
import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIT = json.load(open(os.path.join(ROOT, "tests", "golden", "fusion_literals.json")))
DIST = {"Cosine": O.COSINE, "Euclid": O.EUCLID, "Dot": O.DOT, "Manhattan": O.MANHATTAN}


def _lists(responses):
    return [np.array([(i, s) for i, s in r], dtype=FR.ScoredPointOffset) for r in responses]


@pytest.mark.parametrize("case", LIT["rrf"], ids=[c["name"] for c in LIT["rrf"]])
def test_rrf_literals(case):
    got = FR.rrf_scoring(_lists(case["responses"]), case["k"], case["weights"])
    if "expected" in case:
        assert got["idx"].tolist() == [e[0] for e in case["expected"]]
        assert np.array_equal(got["score"].view(np.uint32), np.array([e[1] for e in case["expected"]], dtype=np.float32).view(np.uint32))
    if "expected_equal_scores" in case:
        assert sorted(got["idx"].tolist()) == sorted(case["expected_equal_scores"]) and len(set(got["score"].view(np.uint32).tolist())) == 1
    if "expected_order" in case:
        assert got["idx"].tolist() == case["expected_order"]
        assert bool(np.all(np.diff(got["score"]) < 0)) == case["expected_strictly_descending"]


@pytest.mark.parametrize("case", LIT["rrf_errors"], ids=[c["name"] for c in LIT["rrf_errors"]])
def test_rrf_weights_length_mismatch(case):
    with pytest.raises(ValueError):
        FR.rrf_scoring(_lists(case["responses"]), case["k"], case["weights"])


def test_rrf_empty():      # test_rrf_scoring_empty, reciprocal_rank_fusion.rs:118-123
    assert len(FR.rrf_scoring([], 2, None)) == 0


def mmr_case(case):
    """A literal MMR case through the restatement, the similarities by the oracle's f32 scorer on the rows as given."""
    dist = DIST[case["distance"]]
    vec = {}
    for pid, v in case["points"]:
        vec.setdefault(pid, np.array(v, dtype=np.float32))      # unique_by keeps the first
    cand = np.array([(pid, 0.0) for pid, _ in case["points"]], dtype=FR.ScoredPointOffset)
    query = np.array(case["vector"], dtype=np.float32)

    def rel(pid):      # (test_mmr_less_than_two_points hands a 2-d vector to 3-d points: never scored, fewer than two candidates)
        return O.similarity(O.F32, dist, query, vec[pid])
    return FR.mmr_from_points(cand, rel, lambda a, b: O.similarity(O.F32, dist, vec[a], vec[b]), case["lambda"], case["limit"])


@pytest.mark.parametrize("case", LIT["mmr"], ids=[c["name"] for c in LIT["mmr"]])
def test_mmr_literals(case):
    got = mmr_case(case)
    if "expected_ids" in case:
        assert got["idx"].tolist() == case["expected_ids"]
    else:
        assert len(got) == len(case["expected_id_set"]) and sorted(got["idx"].tolist()) == case["expected_id_set"]


def _assert_close(a, b):      # score_fusion.rs:184-197
    diff = abs(float(a) - float(b))
    tol = max(1e-5, 1e-4 * max(abs(float(a)), abs(float(b))))
    assert diff <= tol, (a, b, diff, tol)


def test_welford_against_float64():      # welford_calc_vs_naive, score_fusion.rs:199-216
    rng = np.random.default_rng(0xF05E)
    for n in [2, 3, 7, 64, 999] + rng.integers(2, 1000, 60).tolist():
        scores = rng.uniform(-100.0, 100.0, n).astype(np.float32)
        mean, var = FR.welfords_mean_variance(scores)
        assert mean.dtype == np.float32 and var.dtype == np.float32
        x = scores.astype(np.float64)
        _assert_close(mean, x.mean())
        _assert_close(var, x.var(ddof=1))


def test_distr_norm_branches():
    assert FR.distr_norm([]).tolist() == [] and FR.distr_norm([3.0]).tolist() == [0.5]
    assert FR.distr_norm([2.0, 2.0, 2.0]).tolist() == [0.5, 0.5, 0.5]      # variance 0: min == max
    got = FR.distr_norm([1.0, 2.0, 3.0])                                      # mean 2, sample variance 1: extremes -1 and 5
    assert np.array_equal(got, np.array([2, 3, 4], dtype=np.float32) / np.float32(6))


def test_score_fusion_starts_at_the_first_contribution_and_counts_duplicates():
    a = np.array([(7, 1.0), (8, 2.0), (7, 3.0)], dtype=FR.ScoredPointOffset)      # id 7 twice inside one list
    b = np.array([(8, 5.0)], dtype=FR.ScoredPointOffset)                           # one entry: 0.5
    got = FR.score_fusion([a, b], weights=[1.0])                                   # the second weight is missing: 1.0
    na = FR.distr_norm(a["score"])
    want = {7: np.float32(na[0] + na[2]), 8: np.float32(na[1] + np.float32(0.5))}
    assert got["idx"].tolist() == sorted(want, key=lambda i: (-float(want[i]), i))
    assert all(np.float32(s).view(np.uint32) == want[i].view(np.uint32) for i, s in zip(got["idx"].tolist(), got["score"]))


# A hand-made MMR case in which the order rule decides.  Dot product, integer coordinates: every score is exact.  Query (1, 0), lambda 0.5.
#   candidate  row     relevance
#   0          (2, 0)  2
#   1          (2, 1)  2
#   2          (2, 0)  2      a duplicate of row 0
#   3          (1, 3)  1
#   4          (1, 3)  1      a duplicate of row 3
#   5          (0, 1)  0
# pick 1: relevance 2 three times (0, 1, 2): the last maximal element, 2.          remaining [0, 1, 2, 3, 4, 5] -> [0, 1, 5, 3, 4]   (5 moved into the slot of 2)
# pick 2: sims to 2 = (4, 4, 0, 2, 2) for (0, 1, 5, 3, 4): scores (-1, -1, 0, -.5, -.5): 5.          -> [0, 1, 4, 3]   (4 moved into the slot of 5)
# pick 3: sims to 5 = (0, 1, 3, 3) for (0, 1, 4, 3): maxima (4, 4, 3, 3): scores (-1, -1, -1, -1), all tied: the last in THIS order, 3 - an ascending
#         order would give 4, a first-maximum rule 0.                                                  -> [0, 1, 4]
# pick 4: sims to 3 = (2, 5, 10): maxima (4, 5, 10): scores (-1, -1.5, -4.5): 0.                      -> [4, 1]
# pick 5: sims to 0 = (2, 4) for (4, 1): maxima (10, 5): scores (-4.5, -1.5): 1.
TIE_ROWS = np.array([[2, 0], [2, 1], [2, 0], [1, 3], [1, 3], [0, 1]], dtype=np.float32)
TIE_QUERY = np.array([1, 0], dtype=np.float32)
TIE_EXPECTED = [2, 5, 3, 0, 1]


def test_mmr_exact_ties_follow_the_swap_remove_order():
    got = FR.maximal_marginal_relevance(len(TIE_ROWS), lambda c: O.similarity(O.F32, O.DOT, TIE_QUERY, TIE_ROWS[c]),
                                        lambda c, s: O.similarity(O.F32, O.DOT, TIE_ROWS[c], TIE_ROWS[s]), 0.5, 5)
    assert got == TIE_EXPECTED
    assert FR.maximal_marginal_relevance(len(TIE_ROWS), lambda c: float(TIE_QUERY @ TIE_ROWS[c]), lambda c, s: float(TIE_ROWS[c] @ TIE_ROWS[s]), 0.5, 3) == TIE_EXPECTED[:3]
    assert FR.maximal_marginal_relevance(len(TIE_ROWS), lambda c: 0.0, lambda c, s: 0.0, 0.5, 0) == []
