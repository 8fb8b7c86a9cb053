"""The restatement of tests/sparse_weights_reference.py against literals: the u8 arithmetic, the reference's own search_context_tests.rs
cases over f32 / f16 / u8 index weights, fancy_idf, and the two corpus representations.  CPU only."""
import json
import math
import os

import numpy as np
import pytest

import sparse_weights_reference as SW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_index_literals.json")


def test_u8_round_is_half_away_from_zero():
    # min 0, diff256 1: the quotient is the weight itself
    assert SW.u8_encode(np.array([0.5, 1.5, 2.5, 0.49999997], dtype=np.float32), 0.0, 1.0).tolist() == [1, 2, 3, 0]
    assert SW.round_half_away(np.array([-0.5, -1.5, 254.5], dtype=np.float32)).tolist() == [-1.0, -2.0, 255.0]
    assert SW.u8_encode(np.array([-3.0, 300.0], dtype=np.float32), 0.0, 1.0).tolist() == [0, 255]      # clamp


def test_u8_all_equal_list_is_code_zero_and_decodes_to_min():
    w = np.array([7.25, 7.25, 7.25], dtype=np.float32)
    mn, d = SW.u8_params(w)
    assert (mn, d) == (np.float32(7.25), np.float32(0.0))
    codes = SW.u8_encode(w, mn, d)                       # 0 / 0 = NaN -> 0
    assert codes.tolist() == [0, 0, 0]
    assert SW.u8_decode(codes, mn, d).tolist() == [7.25] * 3
    mn, d = SW.u8_params(np.array([3.0], dtype=np.float32))
    assert SW.u8_decode(SW.u8_encode([3.0], mn, d), mn, d).tolist() == [3.0]


def test_u8_posting_10_20_30():
    w = np.array([10.0, 20.0, 30.0], dtype=np.float32)
    mn, d = SW.u8_params(w)
    assert mn == np.float32(10.0) and d == np.float32(0.078431375)
    codes = SW.u8_encode(w, mn, d)
    assert codes.tolist() == [0, 127, 255]
    assert np.array_equal(SW.u8_decode(codes, mn, d), np.array([10.0, 19.960785, 30.0], dtype=np.float32))


def test_f16_decode_rounds_to_nearest_even_and_overflows_to_inf():
    got = SW.f16_decode(np.array([1.0, 2049.0, 2051.0, 1e-8, 70000.0, -0.1], dtype=np.float32))
    assert got.tolist() == [1.0, 2048.0, 2052.0, 0.0, math.inf, float(np.float16(-0.1))]


def _cases():
    with open(GOLDEN) as f:
        data = json.load(f)
    return data["cases"], data["round_step_u8"]


@pytest.mark.parametrize("weights", [SW.F32, SW.F16, SW.U8])
def test_reference_search_context_literals(weights):
    cases, step = _cases()
    assert len(cases) == 5
    for case in cases:
        n = max(p for p, _ in case["points"]) + 1
        rows = [([], [])] * n
        for p, vec in case["points"]:
            rows[p] = ([d for d, _ in vec], [w for _, w in vec])
        ref = SW.WeightsRestatement(rows, weights=weights)
        q = ref.prepare_query(case["query"]["indices"], case["query"]["values"])
        got = ref.search([q], case["top"], ids=case["ids"])[0]
        assert got["idx"].tolist() == [i for i, _ in case["expected"]], case["name"]
        scores = got["score"]
        if weights == SW.U8:      # the reference's round_scores
            scores = SW.round_half_away(scores / np.float32(step)) * np.float32(step)
        assert scores.tolist() == [s for _, s in case["expected"]], case["name"]
        if case["name"] == "search_test" and weights == SW.U8:
            assert scores.tolist() == [90.0, 60.0, 30.0]
            assert got["score"].tolist() != [90.0, 60.0, 30.0]      # 20.0 is not representable: the raw scores do differ


def test_fancy_idf_within_one_ulp_of_float64_and_ln2_at_zero():
    assert SW.fancy_idf(0, 0) == np.float32(math.log(2.0))
    rng = np.random.default_rng(1)
    for _ in range(2000):
        n = int(rng.integers(0, 20_000_000))
        df = int(rng.integers(0, n + 1))
        x = np.float32(np.float32(np.float32(np.float32(n) - np.float32(df)) + np.float32(0.5)) / np.float32(np.float32(df) + np.float32(0.5))) + np.float32(1.0)
        want = np.float32(math.log(float(np.float32(x))))
        got = SW.fancy_idf(n, df)
        assert abs(int(got.view(np.int32)) - int(want.view(np.int32))) <= 1, (n, df, got, want)


def _rows(seed, n, n_dims, nnz):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        k = int(rng.integers(0, nnz + 1))
        ix = rng.choice(n_dims, size=k, replace=False).astype(np.uint32)
        rows.append((ix, rng.lognormal(0.0, 1.0, k).astype(np.float32)))
    return rows


def test_corpus_statistics_mask_equals_sorted_id_list():
    rows = _rows(2, 500, 40, 8)
    dim_map = {d: 39 - d for d in range(40)}
    ref = SW.WeightsRestatement(rows, dim_map=dim_map)
    rng = np.random.default_rng(3)
    member = ref.corpus_members(rng.random(500) < 0.4, point_deleted=rng.random(500) < 0.1, vec_deleted=rng.random(300) < 0.1)
    dims = list(range(40)) + [1000]
    a, b = ref.corpus_statistics_mask(dims, member), ref.corpus_statistics_ids(dims, member)
    assert a[0].tolist() == b[0].tolist() and a[1] == b[1]
    assert a[0][-1] == 0 and 0 < a[1] < 500 and a[0].sum() > 0
    g = ref.global_statistics(dims)
    assert g[1] == sum(1 for ix, _ in rows if len(ix)) and all(x <= y for x, y in zip(a[0], g[0]))


def test_merged_statistics_of_two_half_segments_are_their_sums():
    rows = _rows(4, 400, 30, 6)
    dims = list(range(30))
    whole = SW.WeightsRestatement(rows).global_statistics(dims)
    lo, hi = SW.WeightsRestatement(rows[:200]).global_statistics(dims), SW.WeightsRestatement(rows[200:]).global_statistics(dims)
    merged = SW.merge_statistics(lo, hi)
    assert merged[0].tolist() == whole[0].tolist() and merged[1] == whole[1]
    q_idx, q_val = np.array([3, 7, 500], dtype=np.uint32), np.array([1.0, 2.0, 3.0], dtype=np.float32)
    got = SW.remap_idf_weights(q_idx, q_val, dims, merged[0], merged[1])
    want = [np.float32(v * SW.fancy_idf(whole[1], df)) for v, df in zip(q_val, [whole[0][3], whole[0][7], 0])]
    assert got.tolist() == want
