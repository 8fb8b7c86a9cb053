"""The reference side of the custom queries over sparse vectors (tests/sparse_custom_reference.py), pinned on the CPU before any device result is
believed: the numpy `score_by` against the oracle's, the original-order sums against the per-pair merge loop, and the literal that tells the
two summation orders apart."""
import numpy as np
import pytest

import oracle_ffi as O
import sparse_reference as SR
import sparse_custom_reference as SCR


def _bits(a):
    """uint32 view with every NaN folded to one pattern (a query without examples scores NaN; which NaN is the platform's choice)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _oracle_score_by(kind, n_a, n_b, sims, coefs=None):
    out = np.empty(sims.shape[1], dtype=np.float32)
    col = np.empty(max(sims.shape[0], 1), dtype=np.float32)
    cf = None if coefs is None else np.ascontiguousarray(coefs, dtype=np.float32)
    for j in range(sims.shape[1]):
        col[:sims.shape[0]] = sims[:, j]
        out[j] = (O.lib.qo_custom_feedback(n_b, O._p(col), O._p(cf)) if kind == SCR.FEEDBACK
                  else O.lib.qo_custom_combine(kind, n_a, n_b, O._p(col)))
    return out


def _columns(rng, ne, n):
    """Similarity columns with ties, zeros (both signs), negatives, huge and tiny values."""
    sims = rng.standard_normal((ne, n)).astype(np.float32)
    sims[rng.random((ne, n)) < 0.2] = 0.0
    sims[rng.random((ne, n)) < 0.05] = -0.0
    sims[rng.random((ne, n)) < 0.2] = np.float32(1.5)                  # ties across examples and points
    sims[rng.random((ne, n)) < 0.05] *= np.float32(1e30)
    sims[rng.random((ne, n)) < 0.05] *= np.float32(1e-30)
    if ne:
        sims[:, : n // 8] = rng.integers(-2, 3, (ne, n // 8)).astype(np.float32)    # integer similarities: masses of ties
    return sims


SHAPES = [(SCR.BEST_SCORE, 3, 0), (SCR.BEST_SCORE, 0, 3), (SCR.BEST_SCORE, 4, 3), (SCR.BEST_SCORE, 0, 0), (SCR.BEST_SCORE, 1, 1),
          (SCR.SUM_SCORES, 3, 2), (SCR.SUM_SCORES, 0, 4), (SCR.SUM_SCORES, 0, 0),
          (SCR.DISCOVER, 1, 0), (SCR.DISCOVER, 1, 3), (SCR.DISCOVER, 1, 8),
          (SCR.CONTEXT, 0, 0), (SCR.CONTEXT, 0, 1), (SCR.CONTEXT, 0, 4),
          (SCR.FEEDBACK, 1, 0), (SCR.FEEDBACK, 1, 6)]


@pytest.mark.parametrize("kind,n_a,n_b", SHAPES)
def test_numpy_score_by_is_the_oracles(kind, n_a, n_b):
    rng = np.random.default_rng(100 + 17 * kind + 5 * n_a + n_b)
    ne = SCR.n_examples(kind, n_a, n_b)
    sims = _columns(rng, ne, 4000)
    coefs = rng.standard_normal(1 + n_b).astype(np.float32) if kind == SCR.FEEDBACK else None
    got = SCR.score_by(kind, n_a, n_b, sims, coefs)
    want = _oracle_score_by(kind, n_a, n_b, sims, coefs)
    assert got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want))


def test_total_cmp_orders_signed_zeros_and_nans():
    a = np.array([-0.0, 0.0, 0.0, 1.0, -np.inf, np.nan, -1.0], dtype=np.float32)
    b = np.array([0.0, -0.0, 0.0, -1.0, -np.inf, np.inf, -2.0], dtype=np.float32)
    assert SCR.total_cmp(a, b).tolist() == [-1, 1, 0, 1, 0, 1, 1]


def _rows(seed, n, n_dims, nnz):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        k = int(rng.integers(0, nnz + 1))
        ix = rng.choice(n_dims, size=k, replace=False).astype(np.uint32)
        rows.append((ix, rng.standard_normal(k).astype(np.float32)))
    return rows


def test_original_order_sums_are_score_pair_on_the_unmapped_vectors():
    n_dims = 48
    rows = _rows(1, 300, n_dims, 24)
    examples = _rows(2, 6, n_dims, 24) + [([], []), ([7, 500, 3], [1.0, 2.0, -1.0])]       # dimension 500: no stored point has it
    perm = np.random.default_rng(3).permutation(n_dims)
    dim_map = {int(d): int(perm[d]) for d in range(n_dims)}
    plain, mapped = SR.Restatement(rows), SR.Restatement(rows, dim_map=dim_map)
    sorted_rows = [SR.sort_vector(*r) for r in rows]
    differs = False
    for ex in examples:
        ei, ev = SR.sort_vector(*ex)
        want = np.array([SR.score_pair(ri, rv, ei, ev)[0] for ri, rv in sorted_rows], dtype=np.float32)
        for rest in (plain, mapped):
            got = SCR.original_order_sims(rest, ex)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        ids = np.array([5, 299, 0, 17])
        assert np.array_equal(SCR.original_order_sims(mapped, ex, ids).view(np.uint32), want[ids].view(np.uint32))
        remapped, _ = mapped.score_matrix([mapped.prepare_query(*ex)])
        differs = differs or not np.array_equal(remapped[0].view(np.uint32), want.view(np.uint32))
    assert differs      # the remapped order gives other floats somewhere in this data: the two orders are told apart


def test_the_literal_that_tells_the_two_orders_apart():
    example = ([1, 2, 3], [1.0, 1.0, 1.0])
    rows = [([1, 2, 3], [1e8, 1.0, -1e8])]
    dim_map = {1: 0, 3: 1, 2: 2}
    rest = SR.Restatement(rows, dim_map=dim_map)
    assert SCR.original_order_sims(rest, example).tolist() == [0.0]            # (1e8 + 1) - 1e8 in float32
    remapped, _ = rest.score_matrix([rest.prepare_query(*example)])
    assert remapped.tolist() == [[1.0]]                                         # (1e8 - 1e8) + 1

    class Q:
        kind, n_a, n_b, examples, coefs = SCR.SUM_SCORES, 1, 0, [example], None
    assert SCR.custom_scores(rest, Q).tolist() == [0.0]


def test_search_returns_points_without_overlap_in_offset_order():
    rows = [([9], [1.0])] * 5 + [([1], [2.0]), ([1], [-1.0])]

    class Q:
        kind, n_a, n_b, examples, coefs = SCR.SUM_SCORES, 1, 0, [([1], [1.0])], None
    got = SCR.search(SR.Restatement(rows), Q, 4, live=np.array([1, 0, 1, 1, 1, 1, 1], dtype=bool))
    assert got["idx"].tolist() == [5, 0, 2, 3] and got["score"].tolist() == [2.0, 0.0, 0.0, 0.0]
