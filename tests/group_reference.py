"""Grouped search on the host, for the tests of qmx_group_search (no device, no library):

  GroupsAggregator, GroupByDriver : a Python restatement of lib/shard/src/grouping/aggregator.rs and driver.rs - the budget, the three states,
                                    `shape_candidates_query`'s limit and is-empty restriction, `exclude_aggregated_points`, the `except_on` /
                                    `match_on` key filters - driven by an exact numpy search (`run_driver`);
  grouped_exact                   : the contract of include/qdrant_amd.h in a dozen lines: what that loop converges to.

Where the reference leaves an order unpinned (ScoredPoint::cmp is the score alone, best_group_keys runs sort_unstable over a hash map, hits are
drained from a hash map) the restatement breaks ties the way the contract does: the lower id first, then the lower key."""
import math

MAX_GET_GROUPS_REQUESTS = 5
MAX_GROUP_FILLING_REQUESTS = 5

KEY_NOT_FOUND, BAD_KEY_TYPE = "KeyNotFound", "BadKeyType"
NO_PAYLOAD = object()       # a point without payload: add_point's KeyNotFound


def _key_order(k):
    return (0, k, "") if isinstance(k, int) else (1, 0, k)


def _group_ids(payload):
    """add_point's first half (aggregator.rs:62-85): the values of the field, arrays flattened, every value a GroupId (string or integer), unique."""
    if payload is NO_PAYLOAD:
        return KEY_NOT_FOUND
    values = list(payload) if isinstance(payload, (list, tuple)) else [payload]
    out = []
    for v in values:
        if isinstance(v, bool) or not isinstance(v, (str, int)):
            return BAD_KEY_TYPE
        if v not in out:
            out.append(v)
    return out


class GroupsAggregator:
    def __init__(self, groups, group_size):
        self.max_groups, self.max_group_size = groups, group_size
        self.groups = {}               # key -> {id: score}
        self.full_groups = set()
        self.group_best = {}           # key -> (score, id)
        self.all_ids = set()

    def add_point(self, pid, score, payload):
        keys = _group_ids(payload)
        if isinstance(keys, str):
            return keys
        for key in keys:
            group = self.groups.setdefault(key, {})
            if pid not in group:       # (an occupied entry is replaced only by a newer version: there are none here)
                group[pid] = score
                self.all_ids.add(pid)
            if len(group) == self.max_group_size:
                self.full_groups.add(key)
            best = self.group_best.get(key)
            if best is None or score > best[0]:      # point.cmp(other) == Greater: the score alone
                self.group_best[key] = (score, pid)
        return None

    def add_points(self, points):
        for pid, score, payload in points:
            self.add_point(pid, score, payload)      # KeyNotFound / BadKeyType are ignored

    def __len__(self):
        return len(self.groups)

    def best_group_keys(self):
        pairs = sorted(self.group_best.items(), key=lambda kv: (-kv[1][0], kv[1][1], _key_order(kv[0])))
        return [k for k, _ in pairs[:self.max_groups]]

    def keys_of_unfilled_best_groups(self):
        return [k for k in self.best_group_keys() if k not in self.full_groups]

    def keys_of_filled_groups(self):
        return list(self.full_groups)

    def len_of_filled_best_groups(self):
        return len([k for k in self.best_group_keys() if k in self.full_groups])

    def distill(self):
        out = []
        for key in self.best_group_keys():
            hits = sorted(self.groups[key].items(), key=lambda kv: (-kv[1], kv[0]))[:self.max_group_size]
            out.append((key, [(pid, score) for pid, score in hits]))
        return out


class GroupByDriver:
    """next_request() -> {"limit", "except": full keys, "match": unfilled best keys or None, "exclude_ids", "not_empty": True} or None."""

    def __init__(self, groups, group_size, collect=MAX_GET_GROUPS_REQUESTS, fill=MAX_GROUP_FILLING_REQUESTS):
        self.groups, self.group_size = groups, group_size
        self.candidates_limit = groups * group_size
        self.aggregator = GroupsAggregator(groups, group_size)
        self.state = ("done",) if groups == 0 or group_size == 0 else ("collecting", collect, fill)
        self.stopped_by = "zero" if self.state[0] == "done" else None      # enough_groups | empty | budget | zero
        self.collect_ran_out = False      # Collecting ended because its requests were spent, not on enough groups or an empty page

    def _request(self, except_keys, match_keys):
        return {"limit": self.candidates_limit, "except": list(except_keys), "match": None if match_keys is None else list(match_keys),
                "exclude_ids": set(self.aggregator.all_ids), "not_empty": True}

    def next_request(self):
        while True:
            if self.state[0] == "collecting":
                _, left, fill = self.state
                if left == 0:
                    self.state = ("filling", fill)
                    self.collect_ran_out = True
                    continue
                self.state = ("collecting", left - 1, fill)
                return self._request(self.aggregator.keys_of_filled_groups(), None)
            if self.state[0] == "filling":
                left = self.state[1]
                if left == 0:
                    self.state = ("done",)
                    self.stopped_by = "budget"
                    continue
                self.state = ("filling", left - 1)
                return self._request([], self.aggregator.keys_of_unfilled_best_groups())
            return None

    def add_points(self, points):
        self.aggregator.add_points(points)
        enough = self.aggregator.len_of_filled_best_groups() >= self.groups
        if self.state[0] == "collecting":
            if enough:
                self.state, self.stopped_by = ("done",), "enough_groups"
            elif not points:
                self.state = ("filling", self.state[2])
        elif self.state[0] == "filling":
            if enough or not points:
                self.state, self.stopped_by = ("done",), "enough_groups" if enough else "empty"

    def distill(self):
        return self.aggregator.distill()


def exact_search(ranked, keys_of, request, score_threshold=None):
    """An exact backend: the best `limit` points of the ranked stream [(id, score)] that pass the request's filter.  `except` on an array holds
    when some value is outside the list, `match` when some value is inside (the payload index's any-semantics over arrays)."""
    out = []
    for pid, score in ranked:
        if len(out) >= request["limit"]:
            break
        if score_threshold is not None and score < score_threshold:
            break
        keys = keys_of(pid)
        if not keys or pid in request["exclude_ids"]:
            continue
        if request["except"] and all(k in request["except"] for k in keys):
            continue
        if request["match"] is not None and not any(k in request["match"] for k in keys):
            continue
        out.append((pid, score, list(keys)))
    return out


def run_driver(ranked, keys_of, groups, group_size, collect=MAX_GET_GROUPS_REQUESTS, fill=MAX_GROUP_FILLING_REQUESTS, score_threshold=None):
    """-> (groups as [(key, [(id, score)])], what stopped the driver, requests spent)"""
    d = GroupByDriver(groups, group_size, collect, fill)
    spent = 0
    while True:
        r = d.next_request()
        if r is None:
            break
        spent += 1
        d.add_points(exact_search(ranked, keys_of, r, score_threshold))
    return d.distill(), d.stopped_by, spent


def grouped_exact(ranked, keys_of, limit, group_size, score_threshold=None):
    """The contract: `ranked` = the candidates as [(id, score)], score descending, the lower id first among equal scores."""
    groups = {}      # (insertion order = order of the best hit; a point's keys ascending)
    for pid, score in ranked:
        if score_threshold is not None and score < score_threshold:
            break
        for k in sorted(set(keys_of(pid))):
            hits = groups.setdefault(k, [])
            if len(hits) < group_size:
                hits.append((pid, score))
    return list(groups.items())[:limit] if limit and group_size else []


def rank(scores, ids=None):
    """[(id, score)] of a score row in the project's order."""
    ids = range(len(scores)) if ids is None else ids
    return sorted(((int(i), float(scores[j])) for j, i in enumerate(ids)), key=lambda t: (-t[1] if not math.isnan(t[1]) else -math.inf, t[0]))
