"""CPU: what tests/test_gpu_exact_scan_large_blocks.py expects holds before a device is asked (tests/exact_scan_expectations.py): the row counts are
what the kernels' grid caps ask for, the expected lists follow the rule of tests/parity_asserts.py, and for every case of the GPU module - its block,
its checked queries, its deleted rows and id lists - every checked query has a boundary tie group larger than the slots left for it and finds its
planted rows in the expected list."""
import numpy as np
import pytest

import exact_scan_expectations as X
import oracle_ffi as O


def test_row_counts_follow_from_the_grid_caps():
    cus = 256
    assert X.SECOND_PASS_ROW == cus * 8 * 16                          # scan_sq_mfma_kernel at one block per CU: 8 waves x 16 rows
    assert X.N_MFMA > cus * 8 * 8 * 16 and X.N_MFMA >= 2 ** 18 and X.N_MFMA % 16 == 7
    assert X.N_VALU > cus * 4 * 8 * 32 and X.N_VALU % 32 != 0        # scan_kernel: R = 4 x 8 rows per wave, 8 waves, 4 blocks per CU
    assert X.N_BQROWS > cus * 8 * 256 and X.N_BQROWS % 64 != 0       # bq_rows_kernel: 256 rows per block, 8 blocks per CU
    assert X.N_L1[0] // 65536 == 1 and X.N_L1[1] // 65536 == 2 and all(n % 65536 for n in X.N_L1)
    for n in (X.N_MFMA, X.N_VALU, X.N_BQROWS):
        assert X.pre_n(n) == 8192
        for c in range(X.N_CHECKED):
            o = X.planted_offsets(n, c)
            assert o[0] < o[1] < X.pre_n(n) <= o[2] < o[3] < o[4] < o[5] < n and o[3] // 16 == X.SECOND_PASS_ROW // 16
            assert o[4] // 16 == (n - 1) // 16 - 1 and o[5] // 16 == (n - 1) // 16      # the last whole tile of 16, the partial one
    assert X.pre_n(2 ** 24 + 5) == 2 ** 14


def test_expected_list_is_the_rule_of_parity_asserts():
    sc = np.array([1.0, 3.0, 3.0, -0.0, 0.0, 3.0, np.nan, 2.0], dtype=np.float32)
    ids, s = X.expected_list(sc, 4)
    assert ids.tolist() == [6, 1, 2, 5] and np.isnan(s[0])           # NaN greatest, then descending, ascending offsets among ties
    assert X.expected_list(sc, 8)[0].tolist() == [6, 1, 2, 5, 7, 0, 4, 3]      # +0.0 above -0.0: the order of the bits
    live = np.array([1, 0, 1, 1, 1, 1, 0, 1], dtype=bool)
    assert X.expected_list(sc, 3, live=live)[0].tolist() == [2, 5, 7]
    assert X.expected_list(sc, 5, cand=[5, 5, 7, 2, 0, 7])[0].tolist() == [2, 5, 5, 7, 7]      # an id list: one entry per occurrence
    assert X.boundary_group(sc, 3) == (2, 3) and X.boundary_group(sc, 4) == (3, 3)
    with pytest.raises(AssertionError):
        X.check_preconditions(sc[None, :], 4, [[]])                  # the group fits: nothing is tested
    with pytest.raises(AssertionError):
        X.check_preconditions(sc[None, :], 3, [[5]])                 # a planted row that is not in the list
    X.check_preconditions(sc[None, :], 3, [[1]])
    # against the oracle's queue on a list without ties at the boundary, and its scores' bits
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((500, 8)).astype(np.float32)
    st = O.DenseStorage(O.F32, O.DOT, rows)
    q = rng.standard_normal((1, 8)).astype(np.float32)
    want = st.peek_top(q, 10)[0]
    ids, s = X.expected_list(st.score_points(q, np.arange(500))[0], 10)
    assert ids.tolist() == want["idx"].tolist() and np.array_equal(s.view(np.uint32), want["score"].view(np.uint32))


def _sorted(cases):
    return sorted(cases, key=lambda c: (repr(c.spec), c.n, c.nq, c.top))


@pytest.mark.parametrize("case", _sorted(X.CASES), ids=repr)
def test_preconditions_of_every_case(case):
    w = X.world_of(case.spec, case.n)
    k = min(case.nq, X.N_CHECKED)
    assert w.rows.shape[0] == case.n and w.scores.shape == (X.N_CHECKED, case.n)
    X.check_preconditions(w.scores[:k], case.top, w.planted[:k])
    for c in range(k):                                               # the six planted rows head the list
        assert sorted(X.expected_list(w.scores[c], 6)[0].tolist()) == sorted(w.planted[c])
    # every score of the block is the oracle's score of that row's bytes (a sample of rows and the planted ones, scored directly)
    ids = np.concatenate([np.random.default_rng(3).integers(0, case.n, 40), w.planted[0]])
    direct = w.score_rows(w.queries[:2], w.rows[ids])
    assert np.array_equal(direct.view(np.uint32), np.ascontiguousarray(w.scores[:2, ids]).view(np.uint32))


@pytest.mark.parametrize("edge", X.EDGES)
@pytest.mark.parametrize("case", X.EDGE_CASES, ids=repr)
def test_preconditions_of_the_prescan_edges(case, edge):
    w, live, cand = X.edge_setup(case, edge)
    k = min(case.nq, X.N_CHECKED)
    X.check_preconditions(w.scores[:k], X.TOP, w.planted[:k], cand=cand, live=live)
    p = X.pre_n(case.n if cand is None else len(cand))
    prefix = np.arange(p) if cand is None else cand[:p]
    if edge == "prefix_deleted":
        assert not live[:p].any() and live[p:].all()
    elif edge == "prefix_top_minus_1_live":
        assert live[:p].sum() == X.TOP - 1
    else:
        assert len(cand) >= 2 ** 18 and cand[0] > cand[p - 1] > cand[-1] and len(np.unique(cand)) == len(cand)
        in_prefix = np.zeros(case.n, dtype=bool)
        in_prefix[prefix] = True
        for c in range(k):
            ids, sc = X.expected_list(w.scores[c], X.TOP, cand=cand)
            pre_ids, pre_sc = X.expected_list(w.scores[c], X.TOP, cand=prefix)
            assert X.score_ord(pre_sc[-1:])[0] == X.score_ord(sc[-1:])[0]          # the prefix's k-th best score is the final one
            if edge == "prefix_holds_the_result":
                assert pre_ids.tolist() == ids.tolist()                             # ... and so is its key: the bound itself belongs to the result
            else:
                tied = np.flatnonzero(X.score_ord(w.scores[c]) == X.score_ord(sc[-1:])[0])
                behind = tied[~in_prefix[tied] & np.isin(tied, cand)]
                assert (behind < prefix.min()).sum() == 5 and (behind > prefix.max()).sum() == 2
                assert set(behind[behind < prefix.min()].tolist()) < set(ids.tolist())   # rows equal to the bound's score, behind the prefix, in the result


@pytest.mark.parametrize("case", X.ID_LIST_CASES, ids=repr)
def test_preconditions_of_the_id_lists(case):
    w, cand = X.id_list_of(case)
    k = min(case.nq, X.N_CHECKED)
    assert len(cand) == case.n and len(np.unique(cand)) < 0.7 * case.n
    X.check_preconditions(w.scores[:k], X.TOP, w.planted[:k], cand=cand)
    for c in range(k):                                               # the head of the list repeats an id: 8 entries of 6 rows
        ids, _ = X.expected_list(w.scores[c], 8, cand=cand)
        assert sorted(set(ids.tolist())) == sorted(w.planted[c]) and ids.tolist().count(w.planted[c][0]) == 2 and ids.tolist().count(w.planted[c][-1]) == 2


@pytest.mark.parametrize("n", X.N_L1)
def test_preconditions_of_the_l1_blocks(n):
    w, live = X.l1_setup(n)
    X.check_preconditions(w.scores[:X.L1_QUERIES], X.TOP, w.planted[:X.L1_QUERIES], live=live)
    assert abs(live.mean() - 0.8) < 0.01 and all(len(w.planted[c]) >= (3 if n < 131_071 else 4) for c in range(X.L1_QUERIES))
    assert (w.scores <= 0).all()
