"""The host model of grouped search (tests/group_reference.py): its restatement of GroupsAggregator / GroupByDriver reproduces the literals of the
reference's own unit tests (tests/golden/group_literals.json), and the driver converges to `grouped_exact` - the contract of qmx_group_search - when
its searches are exact and its budget suffices.  CPU only."""
import json
import os

import numpy as np
import pytest

import group_reference as G

HERE = os.path.dirname(os.path.abspath(__file__))
LIT = json.load(open(os.path.join(HERE, "golden", "group_literals.json")))


def _payload(keys):
    return G.NO_PAYLOAD if keys == "__no_payload__" else keys


def _add_all(agg, points):
    for p in points:
        assert agg.add_point(p["id"], p["score"], _payload(p["keys"])) is None


def test_literal_group_with_multiple_payload_values():
    lit = LIT["aggregator"]["test_group_with_multiple_payload_values"]
    agg = G.GroupsAggregator(lit["groups"], lit["group_size"])
    _add_all(agg, lit["points"])
    got = agg.distill()
    assert [[pid for pid, _ in hits] for _, hits in got] == [e["hits"] for e in lit["expected"]]


def test_literal_it_adds_single_points():
    lit = LIT["aggregator"]["it_adds_single_points"]
    agg = G.GroupsAggregator(lit["groups"], lit["group_size"])
    for i, c in enumerate(lit["cases"]):
        p = c["point"]
        res = agg.add_point(p["id"], p["score"], _payload(p["keys"]))
        assert (res or "ok") == c["result"], i
        assert len(agg) == c["groups_count"], i
        if c["group_size"] > 0:
            assert len(agg.groups[c["key"]]) == c["group_size"], i
        else:
            assert c["key"] not in agg.groups, i
    assert len(agg.full_groups) == lit["full_groups_len"]
    assert agg.keys_of_unfilled_best_groups() == lit["keys_of_unfilled_best_groups"]
    assert agg.len_of_filled_best_groups() == lit["len_of_filled_best_groups"]
    assert agg.distill() == [(e["key"], [tuple(h) for h in e["hits"]]) for e in lit["expected"]]


def test_literal_aggregate_less_groups():
    lit = LIT["aggregator"]["test_aggregate_less_groups"]
    agg = G.GroupsAggregator(lit["groups"], lit["group_size"])
    _add_all(agg, lit["points"])
    assert agg.distill() == [(e["key"], [tuple(h) for h in e["hits"]]) for e in lit["expected"]]


@pytest.mark.parametrize("name", ["single_request_budget_yields_one_shaped_request", "stops_early_when_enough_groups_are_filled",
                                  "moves_to_filling_and_finishes_on_empty_responses"])
def test_literal_driver(name):
    lit = LIT["driver"][name]
    d = G.GroupByDriver(LIT["driver"]["groups"], LIT["driver"]["group_size"], *lit["budget"])
    kept = {}
    for step in lit["steps"]:
        if "add_points" in step:
            d.add_points([(p["id"], p["score"], p["keys"]) for p in step["add_points"]])
            continue
        r = d.next_request()
        assert (r is not None) == step["next_request"]
        if "limit" in step:
            assert r["limit"] == step["limit"] and r["not_empty"] == step["not_empty"]
        if "remember" in step:
            kept[step["remember"]] = r
        if "differs_from" in step:
            assert r != kept[step["differs_from"]]
    groups = d.distill()
    assert len(groups) == lit["groups_len"]
    if "keys" in lit:
        assert [k for k, _ in groups] == lit["keys"]
    if "hits_len" in lit:
        assert all(len(h) == lit["hits_len"] for _, h in groups)


def test_literal_driver_zero_groups_or_group_size():
    lit = LIT["driver"]["zero_groups_or_group_size_finishes_immediately"]
    for groups, group_size in lit["shapes"]:
        d = G.GroupByDriver(groups, group_size, *lit["budget"])
        assert d.next_request() is None and d.distill() == []
        assert G.grouped_exact([(0, 1.0)], lambda i: [0], groups, group_size) == []


# ---- the driver converges to the contract ------------------------------------------------------------------------------------------------

LAYOUTS = ["uniform", "multi", "singletons", "dominant", "sparse_keys"]


def _case(seed, layout):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(40, 400))
    scores = rng.permutation(n).astype(np.float32) / np.float32(n)      # distinct
    n_groups = int(rng.integers(2, 40))
    if layout == "uniform":
        keys = [[int(k)] for k in rng.integers(0, n_groups, n)]
    elif layout == "multi":
        keys = [sorted(set(int(k) for k in rng.integers(0, n_groups, int(rng.integers(0, 4))))) for _ in range(n)]
    elif layout == "singletons":
        keys = [[i] for i in range(n)]
    elif layout == "dominant":      # one group owns the best half
        keys = [[int(k)] for k in rng.integers(1, n_groups + 1, n)]
        for i in np.argsort(-scores)[:n // 2]:
            keys[int(i)] = [0]
    else:                           # most points carry no key
        keys = [[int(rng.integers(0, n_groups))] if rng.random() < 0.3 else [] for _ in range(n)]
    limit, group_size = int(rng.integers(1, 8)), int(rng.integers(1, 6))
    thr = float(scores[int(rng.integers(0, n))]) if seed % 3 == 0 else None
    return G.rank(scores), (lambda i: keys[i]), limit, group_size, thr


def _plain(groups):
    return [(k, [pid for pid, _ in hits]) for k, hits in groups]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_unlimited_budget_driver_equals_grouped_exact(layout):
    for seed in range(40):
        ranked, keys_of, limit, group_size, thr = _case(seed, layout)
        got, stopped_by, _ = G.run_driver(ranked, keys_of, limit, group_size, collect=10 ** 9, fill=10 ** 9, score_threshold=thr)
        assert stopped_by in ("enough_groups", "empty"), (seed, stopped_by)
        assert _plain(got) == _plain(G.grouped_exact(ranked, keys_of, limit, group_size, thr)), seed


def test_default_budget_driver_equals_grouped_exact_unless_it_ran_out():
    left_out = total = 0
    for layout in LAYOUTS:
        for seed in range(40):
            ranked, keys_of, limit, group_size, thr = _case(seed, layout)
            got, stopped_by, spent = G.run_driver(ranked, keys_of, limit, group_size, score_threshold=thr)
            total += 1
            assert spent <= G.MAX_GET_GROUPS_REQUESTS + G.MAX_GROUP_FILLING_REQUESTS
            if stopped_by == "budget":      # the reference returns what it has: unfilled groups; qmx_group_search returns the exact answer there
                left_out += 1
                continue
            assert _plain(got) == _plain(G.grouped_exact(ranked, keys_of, limit, group_size, thr)), (layout, seed, stopped_by)
    assert left_out * 10 <= total, (left_out, total)
