"""Dense u8 segments with QMX_SEG_U8_WIDE and rows of 1088 .. 2048 bytes (qdrant_amd/csrc/scan_u8w.hip scan_u8w_staged_kernel): rows and queries staged through
LDS rings, the rows by LDS-DMA straight from the row-major block.  As for the shorter rows the lists must be the oracle's ids and score bits, ties included."""
import numpy as np
import pytest

import oracle_ffi as O
from parity_asserts import assert_reference_lists
from test_gpu_u8_wide import DISTS, N, _queries, _rows, _search, qa  # noqa: F401  (N = 2^18 + 37: the last 256-row tile holds 37 rows)

pytestmark = pytest.mark.gpu

KERNEL = "scan_u8w_staged_kernel"


def _wide_lists(qa, s, nq):
    got = s.peek_top_all()
    assert KERNEL in qa._ffi.last_kernel(s.scorer._h), qa._ffi.last_kernel(s.scorer._h)
    assert s.counters.prefilter_queries == nq
    return got


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("dim,nq,top", [(1088, 130, 64), (1536, 70, 10), (2048, 40, 10)])
def test_staged_pass_returns_the_oracle_lists(qa, dist, dim, nq, top):  # noqa: F811
    """1088: the shortest staged row, its last stage one real chunk and one padded, and a nearly empty second query tile; 1536 with 70 queries: live queries in
    the upper query half beside dead slots; 2048: the limit, three whole ring turns per tile.  Rows uniform over 0..255"""
    rows, queries = _rows(dim), _queries(nq, dim)
    vs, s = _search(qa, rows, dist, queries, top)
    if dim == 1088:
        info = vs.info()
        assert info["derived_copy"] == "u8_wide" and info["derived_copy_bytes"] == (N + 255) // 256 * 256 * (8 if dist == O.COSINE else 4) + (4 * N if dist == O.COSINE else 0)
    assert_reference_lists(_wide_lists(qa, s, nq), O.DenseStorage(O.U8, dist, rows), queries, top, threads=16)


@pytest.mark.parametrize("scalar_order", [False, True])
def test_totals_at_the_edge_of_the_derivation_in_both_orders(qa, scalar_order):
    """rows and queries in 200..255 at dim 2048, row 0 and query 0 all 255: a Dot total of 133 171 200 < 2^27 from lane totals of 16 646 400 < 2^24"""
    dim, nq, top = 2048, 20, 10
    rows, queries = _rows(dim, 200).copy(), _queries(nq, dim, 200)
    rows[0], queries[0] = 255, 255
    _, s = _search(qa, rows, O.DOT, queries, top, flags=qa._ffi.SEG_U8_WIDE | (qa._ffi.SEG_U8_SCALAR_ORDER if scalar_order else 0))
    got = _wide_lists(qa, s, nq)
    assert int(got[0]["idx"][0]) == 0 and float(got[0]["score"][0]) == 133171200.0
    assert_reference_lists(got, O.DenseStorage(O.U8, O.DOT, rows, u8_isa=O.ISA_SCALAR if scalar_order else O.ISA_AUTO), queries, top, threads=16)
    assert s.counters.fallback_queries == 0


@pytest.mark.parametrize("dist", [O.EUCLID, O.COSINE])
def test_winners_in_the_last_rows_of_the_partial_tile(qa, dist):
    """the last three rows as queries 0, 65 and 69 - two of them in the upper query half: each leads its list (a column entry or a row number from the wrong
    slot of the column ring loses it), and is absent once deleted"""
    dim, nq, top = 1088, 70, 10
    rows = _rows(dim)
    queries = _queries(nq, dim)
    at = [0, 65, 69]
    queries[at] = rows[N - 3:]
    vs, s = _search(qa, rows, dist, queries, top)
    got = _wide_lists(qa, s, nq)
    assert [int(got[i]["idx"][0]) for i in at] == [N - 3, N - 2, N - 1]
    assert_reference_lists(got, O.DenseStorage(O.U8, dist, rows), queries, top, threads=16)
    deleted = np.zeros(N, dtype=bool)
    deleted[N - 3:] = True
    vs.set_deleted(deleted, None)
    s = qa.BatchFilteredSearcher(queries, vs, top)
    got = _wide_lists(qa, s, nq)
    assert not any(np.isin(got[i]["idx"], [N - 3, N - 2, N - 1]).any() for i in range(nq))
    assert_reference_lists(got, O.DenseStorage(O.U8, dist, rows, point_deleted=deleted), queries, top, live=~deleted, threads=16)
