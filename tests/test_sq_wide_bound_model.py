"""The integer reject bound of the scalar-int8 128-query pass (qdrant_amd/csrc/scan_sqw.hip), restated in numpy and checked on the CPU against the
oracle's f32 scores: a pair (row, query) whose score reaches a threshold T passes  dot + B[row] >= A[query]  with B[row] = ceil(vector_offset /
multiplier) + 1 (sqw_stats_kernel) and A[query] = floor((T - query_offset) / multiplier - margin) (sqw_pack_kernel) - on centred blocks and on
un-centred ones (dot / cosine: vector_offset / multiplier ~ dim (offset / alpha)^2) up to the gate of segment_sq_stats (api_segment.hip), below which
no column entry reaches the clamp and no bound leaves the int32 range.  The oracle is the reference; the model only restates the inequality.  The device
code follows these formulas line by line; the GPU tests (test_gpu_sq_wide.py) compare its lists with the oracle's."""
import numpy as np
import pytest

import oracle_ffi as O

N_ROWS, N_QUERIES = 4096, 8
CLAMP = 2.0 ** 30


def column(vector_offset, multiplier):
    """sqw_stats_kernel: (entries before the clamp, entries) in f64"""
    b = np.ceil(vector_offset.astype(np.float64) / float(multiplier)) + 1.0
    return b, np.clip(b, -CLAMP, CLAMP)


def bound(t, q_off, multiplier, off_absmax, dim):
    """sqw_pack_kernel: a_thr in f64; the kernel's A[query] is its floor, saturated at the ends of int32"""
    eps, m = 3.8146972656e-6, float(multiplier)
    t, q_off = np.asarray(t, dtype=np.float64), float(q_off)
    sizes = m * 16129.0 * dim + abs(q_off) + float(off_absmax) + np.abs(t)
    return (t - q_off) / m - (sizes * eps / m + 3.0)


def gate(off_absmax, multiplier, dim):
    """segment_sq_stats: the pass serves the block"""
    return float(off_absmax) / float(multiplier) + 16129.0 * dim < CLAMP


def gate_ratio(dim):
    """the offset / alpha at which an all-127 dot row reaches the gate: dim x^2 + 127 dim x + 127^2 dim = 2^30"""
    return (-127.0 + np.sqrt(127.0 ** 2 - 4.0 * (16129.0 - CLAMP / dim))) / 2.0


def make_block(kind, dist, dim, rng, n):
    """centred: Gaussian rows; un-centred: uniform values in [low, 1] with low / (1 - low) * 127 = offset / alpha a given share of the gate's"""
    if kind == "centred":
        x = rng.standard_normal((n, dim)).astype(np.float32)
    else:
        ratio = {"uncentred_half": 0.5, "uncentred_at_gate": 0.97, "uncentred_past_gate": 1.4}[kind] * gate_ratio(dim)
        low = ratio / (ratio + 127.0)
        x = rng.uniform(low, 1.0, (n, dim)).astype(np.float32)
    if dist == O.COSINE:
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def encoded(kind, dist, dim, seed):
    """-> oracle, its rows, vector_offset column, code matrix, queries as stored, their codes and offsets, the oracle's scores [query, row]"""
    rng = np.random.default_rng(seed)
    x = make_block(kind, dist, dim, rng, N_ROWS)
    q = make_block(kind, dist, dim, rng, N_QUERIES)
    q[N_QUERIES // 2:] = O.preprocess(dist, rng.standard_normal((N_QUERIES - N_QUERIES // 2, dim)).astype(np.float32))      # ... and queries unlike the rows
    mn, mx = np.float32(x.min()), np.float32(x.max())
    osq = O.SqOracle(dist, dim, (mx - mn) / np.float32(127.0), mn)
    rows = osq.encode_rows(x)
    v_off = rows[:, :4].copy().view(np.float32)[:, 0]
    codes = rows[:, 4:].astype(np.int64)
    q_enc = [osq.encode_query(qi) for qi in q]
    q_codes = np.stack([c for c, _ in q_enc]).astype(np.int64)
    q_off = np.array([o for _, o in q_enc], dtype=np.float32)
    scores = osq.score_points(q, np.arange(N_ROWS, dtype=np.uint32))
    return osq, v_off, codes, q_codes, q_off, scores


KINDS = ["centred", "uncentred_half", "uncentred_at_gate"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("dist", [O.DOT, O.COSINE, O.EUCLID])
def test_a_pair_that_reaches_the_threshold_passes_the_integer_test(dist, dim, kind):
    """for every query and every threshold t among its scores: every row with oracle score >= t has dot + B[row] >= floor(a_thr(t)) - the smallest
    dot + B[row] over the rows at or above t (a running minimum down the sorted scores) against the bound of t"""
    osq, v_off, codes, q_codes, q_off, scores = encoded(kind, dist, dim, seed=dim + 7 * dist)
    m = osq.sq.multiplier
    assert m > 0.0
    off_absmax = np.abs(v_off).max()
    assert gate(off_absmax, m, dim)
    _, b = column(v_off, m)
    dots = q_codes @ codes.T
    for qi in range(N_QUERIES):
        order = np.argsort(-scores[qi].astype(np.float64), kind="stable")
        lhs = (dots[qi] + b)[order]
        lowest_at_or_above = np.minimum.accumulate(lhs)
        t = scores[qi][order]
        # (equal scores: the minimum has to cover the whole group of ties - take it at the group's last member)
        last_of_group = np.r_[t[1:] != t[:-1], True]
        group_end = np.flatnonzero(last_of_group)[np.cumsum(last_of_group) - last_of_group]
        a = np.floor(bound(t, q_off[qi], m, off_absmax, dim))
        slack = lowest_at_or_above[group_end] - a
        assert (slack >= 0).all(), (qi, float(slack.min()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("dist", [O.DOT, O.COSINE, O.EUCLID])
def test_below_the_gate_nothing_clamps_and_no_bound_saturates(dist, dim, kind):
    osq, v_off, codes, q_codes, q_off, scores = encoded(kind, dist, dim, seed=dim + 7 * dist)
    m = osq.sq.multiplier
    off_absmax = np.abs(v_off).max()
    assert gate(off_absmax, m, dim)
    raw, b = column(v_off, m)
    assert np.array_equal(raw, b) and np.abs(raw).max() < CLAMP
    dots = q_codes @ codes.T
    assert np.abs(dots + b[None, :]).max() < 2.0 ** 31      # the sum the scan forms in int32
    for qi in range(N_QUERIES):
        a = bound(scores[qi], q_off[qi], m, off_absmax, dim)
        assert (a > -2147483647.0).all() and (a < 2147483520.0).all()


@pytest.mark.parametrize("dist", [O.DOT, O.COSINE])
def test_past_the_gate_the_column_would_clamp(dist):
    """the gate is not idle: an un-centred dot / cosine block 1.4 times past its offset / alpha has entries beyond 2^30, and the gate refuses it"""
    dim = 256
    osq, v_off, codes, q_codes, q_off, scores = encoded("uncentred_past_gate", dist, dim, seed=3)
    raw, b = column(v_off, osq.sq.multiplier)
    assert not gate(np.abs(v_off).max(), osq.sq.multiplier, dim)
    assert (raw > CLAMP).all() and (b == CLAMP).all()
