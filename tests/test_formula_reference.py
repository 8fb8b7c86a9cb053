"""tests/formula_reference.py (the float64 restatement of FormulaScorer and do_rescore_with_formula the device is compared with) against the
reference's own literals (tests/golden/formula_literals.json), plus what the GPU comparisons rest on: the decay lambdas, the short circuits,
last-duplicate-wins for $score, and - on the reference alone - that the fixed inputs of the libm comparisons hold no fragile value.  CPU only."""
import json
import math
import os

import numpy as np
import pytest

import qdrant_amd as qa
import formula_reference as FR
import formula_cases as FC

LIT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "formula_literals.json")))
CODES = {"NON_FINITE": FR.NON_FINITE, "NO_VALUE": FR.NO_VALUE, "BAD_VALUE": FR.BAD_VALUE}


def _fixture():
    fx = LIT["fixture"]
    scores = [{int(i): np.float32(s) for i, s in prefetch} for prefetch in fx["scores"]]
    payload = {name: FR.Column("number", [v]) for name, v in fx["numbers"].items()}
    for name in fx["invalid_numbers"]:
        payload[name] = FR.Column("number", [0.0], invalid=[True])
    for name, (lat, lon) in fx["geo"].items():
        payload[name] = FR.Column("geo", [lat], [lon])
    for name, flag in fx["conditions"].items():
        payload[name] = FR.Column("condition", [flag])
    return scores, payload


def _defaults():
    d = dict(LIT["defaults"]["values"])
    out = {("score", int(i)): v for i, v in d.pop("score").items()}
    out.update({k: tuple(v) if isinstance(v, list) else v for k, v in d.items()})
    return out


def _run(case, defaults):
    scores, payload = _fixture()
    if "error" in case:
        with pytest.raises(FR.EvalError) as e:
            FR.eval_expression(case["expr"], 0, scores, payload, defaults)
        assert e.value.code == CODES[case["error"]], case
    else:
        got = FR.eval_expression(case["expr"], 0, scores, payload, defaults)
        assert np.float64(got).view(np.uint64) == np.float64(case["expected"]).view(np.uint64), (case, got)      # assert_eq! on f64, and bit for bit


@pytest.mark.parametrize("case", LIT["evaluation"], ids=lambda c: c["at"])
def test_evaluation_literals(case):
    _run(case, {})


@pytest.mark.parametrize("case", LIT["default_values"], ids=lambda c: c["at"])
def test_default_value_literals(case):
    _run(case, _defaults())


def test_haversine_reproduces_both_literals_exactly():
    assert FR.haversine(25.717877679163667, -100.43383200156751, 25.628482424190565, -100.23881855976) == 21926.494151786308
    assert FR.haversine(25.717877679163667, -100.43383200156751, 25.0, -100.0) == 90951.29600298218


def test_decay_lambda_round_trip_ranges_and_the_builders_agree():
    """parsed_formula.rs:186-224: the validation ranges, the three formulas, and qdrant_amd's restatement bit for bit."""
    for kind, midpoint, scale in [("lin", 0.5, 1.0), ("lin", 0.0, 3.0), ("lin", 1.0, 0.25), ("gauss", 0.5, 1.0), ("gauss", 0.01, 5e6), ("gauss", 0.99, 0.1),
                                  ("exp", 0.3, 120.0), ("exp", 0.5, None), ("exp", None, 2.0), ("lin", None, None)]:
        lam = FR.decay_params_to_lambda(kind, midpoint, scale)
        assert np.float64(lam).view(np.uint64) == np.float64(qa.decay_params_to_lambda(kind, midpoint, scale)).view(np.uint64)
        m, s = float(np.float32(0.5 if midpoint is None else midpoint)), float(np.float32(1.0 if scale is None else scale))
        # the decay at distance `scale` from the target is the midpoint
        x = ("const", s)
        got = FR.eval_expression(("decay", kind, x, None, lam), 0, [], {}, {})
        assert got == pytest.approx(m, rel=1e-12, abs=1e-15)
    assert FR.decay_params_to_lambda("lin", 0.25, 2.0) == (1.0 - 0.25) / 2.0
    assert FR.decay_params_to_lambda("exp", 0.25, 2.0) == math.log(0.25) / 2.0
    assert FR.decay_params_to_lambda("gauss", 0.25, 2.0) == math.log(0.25) / 4.0
    for fn in (FR.decay_params_to_lambda, qa.decay_params_to_lambda):
        for kind, midpoint, scale in [("lin", -0.1, 1.0), ("lin", 1.5, 1.0), ("gauss", 0.0, 1.0), ("gauss", 1.0, 1.0), ("exp", 0.0, 1.0), ("exp", 1.0, 1.0),
                                      ("lin", 0.5, 0.0), ("exp", 0.5, -1.0)]:
            with pytest.raises(ValueError):
                fn(kind, midpoint, scale)
    assert qa.gauss_decay(qa.score(0), scale=5e6) == ("decay", "gauss", ("score", 0), None, FR.decay_params_to_lambda("gauss", None, 5e6))


def test_decay_bodies():
    ev = lambda e: FR.eval_expression(e, 0, [], {}, {})      # noqa: E731
    assert ev(("decay", "lin", ("const", 3.0), ("const", 1.0), 0.25)) == -0.25 * 2.0 + 1.0
    assert ev(("decay", "lin", ("const", 30.0), None, 0.25)) == 0.0                      # max(0.0)
    assert ev(("decay", "exp", ("const", -3.0), ("const", 1.0), -0.5)) == math.exp(-0.5 * 4.0)
    assert ev(("decay", "gauss", ("const", 3.0), ("const", 1.0), -0.5)) == math.exp(-0.5 * 2.0 * 2.0)


def test_short_circuits():
    ev = lambda e: FR.eval_expression(e, 0, [], {}, {})      # noqa: E731
    ln0 = ("ln", ("const", 0.0))
    assert ev(("mult", [("const", 0.0), ln0])) == 0.0                                    # 0 * ln(0): the rest is never evaluated
    with pytest.raises(FR.EvalError):
        ev(("mult", [ln0, ("const", 0.0)]))                                              # ... in order
    assert ev(("div", ("const", 0.0), ("const", 0.0), None)) == 0.0                      # 0 / 0: the divisor is never evaluated
    assert ev(("div", ("const", 0.0), ln0, None)) == 0.0
    assert math.copysign(1.0, ev(("div", ("const", -0.0), ("const", 2.0), None))) == 1.0  # ... and the zero is +0.0
    assert ev(("div", ("const", 3.0), ("const", 0.0), 7.5)) == 7.5                       # by_zero_default
    assert ev(("div", ("const", 3.0), ("const", -0.0), 7.5)) == 7.5
    assert ev(("div", ("const", 3.0), ("const", 2.0), 7.5)) == 1.5                       # ... only when right == 0.0
    with pytest.raises(FR.EvalError) as e:
        ev(("div", ("const", 1e308), ("const", 1e-308), 7.5))                            # a non-finite quotient of a non-zero divisor still fails
    assert e.value.code == FR.NON_FINITE
    assert math.copysign(1.0, ev(("sum", [("const", -0.0)]))) == 1.0                     # Sum folds from 0.0
    assert ev(("sum", [])) == 0.0 and ev(("mult", [])) == 1.0
    with pytest.raises(FR.EvalError) as e:
        FR.score(("const", 1e39), 0, [], {}, {})                                         # finite in f64, infinite as f32
    assert e.value.code == FR.NON_FINITE


def test_last_duplicate_wins_for_score_and_candidates_are_the_distinct_ids():
    a = np.array([(7, 0.9), (3, 0.8), (7, 0.1)], dtype=FR.ScoredPointOffset)      # id 7 twice: the map keeps 0.1
    b = np.array([(3, 0.5), (9, 0.4)], dtype=FR.ScoredPointOffset)
    e = ("sum", [("score", 0), ("mult", [("const", 10.0), ("score", 1)])])
    got = FR.rescore(e, [a, b], {}, {("score", 1): 1.0}, 10)
    want = {7: np.float32(np.float64(np.float32(0.1)) + 10.0), 3: np.float32(np.float64(np.float32(0.8)) + 10.0 * np.float64(np.float32(0.5))),
            9: np.float32(0.0 + 10.0 * np.float64(np.float32(0.4)))}
    assert sorted(got["idx"].tolist()) == [3, 7, 9]
    for p, s in zip(got["idx"].tolist(), got["score"]):
        assert s.view(np.uint32) == want[p].view(np.uint32)
    assert got["score"].tolist() == sorted(got["score"].tolist(), reverse=True)
    assert FR.rescore(e, [a, b], {}, {("score", 1): 1.0}, 2)["idx"].tolist() == got["idx"].tolist()[:2]
    thr = FR.rescore(e, [a, b], {}, {("score", 1): 1.0}, 10, score_threshold=float(got["score"][1]))
    assert thr["idx"].tolist() == got["idx"].tolist()[:2]                          # score >= threshold keeps the tie
    # equal scores: the lower offset first; the first error of the lowest failing offset
    tie = FR.rescore(("const", 1.0), [a, b], {}, {}, 10)
    assert tie["idx"].tolist() == [3, 7, 9]
    with pytest.raises(FR.RequestError) as err:
        FR.rescore(("ln", ("sum", [("score", 1), ("const", -0.4)])), [a, b], {}, {}, 10)      # 3: ln(0.1); 7: ln(-0.4); 9: ln(0.0) up to f32
    assert (err.value.point, err.value.code) == (7, FR.NON_FINITE)


def test_error_formula_of_the_shared_cases_fails_where_planted():
    cols = FC.payload()
    for at, code in [(FC.NO_GAP[0], FR.NO_VALUE), (FC.BAD_STRICT[0], FR.BAD_VALUE), (FC.ZERO_A[0], FR.NON_FINITE), (FC.NEG_B[0], FR.NON_FINITE),
                     (FC.ZERO_C[0], FR.NON_FINITE), (FC.HUGE_D[0], FR.NON_FINITE), (710, FR.NO_VALUE)]:
        v, status = FR.precise_and_status(FC.ERRORS, at, [], cols, {})
        assert status == code, at
        assert (v is not None and math.isfinite(v)) == (at == FC.HUGE_D[0])      # the overflow is the cast's alone
    assert FR.precise_and_status(FC.ERRORS, 5, [{5: np.float32(0.25)}], cols, {}) == (cols["gap"].values[5] + 2.0 + 0.0 + 2.0 + 0.5 + 1e-3 + 0.25, 0)


def test_libm_cases_hold_no_fragile_value_and_no_threshold_tie():
    """The GPU test compares these requests bit for bit although the device's exp / ln / log10 / pow / sin / cos / asin are another implementation
    than glibc's: an f32 cast can differ only where the f64 value lies next to an f32 rounding midpoint.  The published bound for the worst of
    these functions is 16 ulp (2^-48 relative); the formulas chain at most six such nodes, subtract no near-equal terms and keep the libm results
    in the normal range; the guard, 2^-40, is 32 x over that.  No value of the fixed inputs may lie inside the guard - if a seed ever does, the
    seed changes, never the guard."""
    cols = FC.payload()
    for name, formula, defaults, seed, n_sources, nq in FC.LIBM_CASES:
        ls = FC.libm_lists(seed, n_sources, nq)
        n_values = 0
        for qi in range(nq):
            scores = FR.prefetch_maps([src[qi] for src in ls])
            for p in sorted(set().union(*[set(m) for m in scores])):
                v = FR.eval_expression(formula, p, scores, cols, defaults)
                assert not FR.is_fragile(v), (name, qi, p, v)
                assert np.float32(v) != np.float32(FC.LIBM_THRESHOLD), (name, qi, p, v)
                n_values += 1
        assert n_values > (1000 if nq > 1 else 10), name
    kept = [len(FR.rescore(FC.LIBM_MIX, [src[qi] for src in FC.libm_lists(502, 2, 33)], cols, FC.LIBM_MIX_DEFAULTS, 400, FC.LIBM_THRESHOLD)) for qi in range(33)]
    full = [len(FR.rescore(FC.LIBM_MIX, [src[qi] for src in FC.libm_lists(502, 2, 33)], cols, FC.LIBM_MIX_DEFAULTS, 400)) for qi in range(33)]
    assert any(0 < k < f for k, f in zip(kept, full)), (kept, full)      # the threshold cuts mid-list
    assert FR.is_fragile(1.0 + 2.0 ** -24 + 2.0 ** -45) and not FR.is_fragile(1.0 + 2.0 ** -30)


def test_node_kind_formulas_stay_in_the_normal_range():
    cols = FC.payload()
    for name, formula in FC.NODE_KINDS.items():
        for p in range(0, FC.N_POINTS, 7):
            v, status = FR.precise_and_status(formula, p, [], cols, FC.LIBM_GEO_DEFAULTS)
            assert status == 0 and v != 0.0 and 1e-300 < abs(v) < 1e300, (name, p, v)
