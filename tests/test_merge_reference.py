"""tests/merge_reference.py against the oracle's aggregator (`qo_merge_topk` = `SearchResultAggregator::push` per item + the bounded queue)
where the reference's list is fully determined: every score of a query distinct, most items a repeat of an earlier id.  CPU only."""
import numpy as np
import pytest

import merge_reference as M
import oracle_ffi as O

SHAPES = [(2, 3, 10, 15), (8, 4, 64, 100), (5, 3, 65, 120), (3, 2, 130, 200), (16, 2, 129, 300), (4, 2, 1000, 1500), (64, 2, 256, 400)]


def _case(shape):
    n_lists, nq, k, n_ids = shape
    return M.duplicate_heavy_lists(np.random.default_rng(n_lists * 10007 + k), n_lists, nq, k, n_ids)


def test_ord_word_is_the_f32_order_word():
    f = np.float32
    assert M.ord_word(f("nan")) == 0xFFFFFFFF and M.ord_word(np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]) == 0xFFFFFFFF
    assert M.ord_word(f(0.0)) == 0x80000000 and M.ord_word(f(-0.0)) == 0x7FFFFFFF
    assert M.ord_word(f("inf")) == 0xFF800000 and M.ord_word(f("-inf")) == 0x007FFFFF
    vals = [f("-inf"), f(-3.5), f(-1e-45), f(-0.0), f(0.0), f(1e-45), f(1.0), f(np.nextafter(f(1.0), f(2.0))), f("inf"), f("nan")]
    words = [M.ord_word(v) for v in vals]
    assert words == sorted(words) and len(set(words)) == len(words)


@pytest.mark.parametrize("shape", SHAPES)
def test_model_equals_the_aggregator_on_duplicate_heavy_lists(shape):
    n_lists, nq, k, n_ids = shape
    lists, counts = _case(shape)
    assert M.duplicate_share(lists, counts, k) > 0
    for bases in (None, (np.arange(n_lists, dtype=np.uint32) % 2) * 7):       # lists share two id spaces: twins made and unmade by the bases
        want = O.merge_topk(lists, counts, k, bases)
        got = M.merge(lists, counts, k, bases)
        for q in range(nq):
            assert got[q]["idx"].tolist() == want[q]["idx"].tolist()
            assert got[q]["score"].view(np.uint32).tolist() == want[q]["score"].view(np.uint32).tolist()
            scores = [s.tobytes() for _, s in M.live_items(lists, counts, k, bases)[q]]
            assert len(set(scores)) == len(scores)                            # the precondition: no two items of a query tie


def test_the_cases_are_duplicate_heavy():
    """At least half of all live items of the cases above repeat an earlier id: the cases cannot quietly go back to disjoint ids."""
    live = dup = 0
    for shape in SHAPES:
        lists, counts = _case(shape)
        for items in M.live_items(lists, counts, shape[2]):
            live += len(items)
            dup += len(items) - len({idx for idx, _ in items})
    assert dup / live >= 0.5, (dup, live)


def test_sort_scored_orders_without_dedupe():
    f = np.float32
    scores = np.array([1.0, np.nan, 1.0, -0.0, 0.0, 2.0, 9.0], dtype=f)
    ids = np.array([7, 3, 2, 5, 6, 1, 0], dtype=np.uint32)
    got = M.sort_scored(scores, ids, 6, 5)                                     # the seventh pair is past the count
    assert got["idx"].tolist() == [3, 1, 2, 7, 6]
    assert M.sort_scored(scores, ids, 0, 5).shape == (0,)
