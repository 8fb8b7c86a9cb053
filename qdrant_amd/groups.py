"""Grouped search on the device: `search_groups` / `query_groups` = "the best `limit` groups by a payload key, `group_size` hits each"
(`group_by`, lib/collection/src/grouping/group_by.rs:263-356).  The reference drives up to 5 + 5 whole searches through `GroupByDriver` and feeds
`GroupsAggregator`; qmx_group_search returns in one call what that loop converges to (include/qdrant_amd.h has the contract)."""
import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

from . import _ffi as F
from .scorer import RawScorer, ScoredPointOffset, new_raw_scorer


class GroupKeys:
    """The group key as the device reads it (qmx_group_keys): dense key indices 0..n_distinct-1 over the point offsets 0..n_points, evaluated by the
    caller's payload index.  `keys` [n_points] with F.GROUP_NONE for a point without a usable key; or, with `offsets` [n_points + 1], the CSR values
    of multi-valued keys (the keys of one point are made unique here).  n_distinct None = 1 + the largest key."""

    def __init__(self, n_points: int, keys, offsets=None, n_distinct: Optional[int] = None, device_id: int = 0):
        self.n_points, self.device_id = int(n_points), device_id
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        if offsets is None:
            if len(keys) != self.n_points:
                raise ValueError("one key per point (or CSR offsets)")
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            if len(offsets) != self.n_points + 1 or (len(offsets) and int(offsets[-1]) != len(keys)):
                raise ValueError("offsets: n_points + 1 entries, the last one = len(keys)")
            parts = [np.unique(keys[int(offsets[p]):int(offsets[p + 1])]) for p in range(self.n_points)]
            offsets = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
            keys = np.ascontiguousarray(np.concatenate(parts) if parts else keys[:0], dtype=np.uint32)
        if n_distinct is None:
            real = keys[keys != F.GROUP_NONE]
            n_distinct = int(real.max()) + 1 if len(real) else 0
        self.n_distinct = int(n_distinct)
        self._h = C.c_void_p()
        F.check(F.lib().qmx_group_keys_create(device_id, self.n_points, F.ptr(keys), F.ptr(offsets), self.n_distinct, C.byref(self._h)))

    def close(self):
        if self._h:
            F.lib().qmx_group_keys_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def search_groups(storage_or_scorer, queries, group_keys: GroupKeys, limit: int, group_size: int, ids=None, score_threshold: Optional[float] = None,
                  counters: Optional["F.GroupCounters"] = None) -> List[List[Tuple[int, np.ndarray]]]:
    """Per query the best `limit` groups as (key_index, hits): hits = the group's `group_size` best points (ScoredPointOffset, score descending, the
    lower offset first among equal scores), groups ordered by their best hit.  `storage_or_scorer`: a storage (then `queries` are the Nearest
    vectors) or a RawScorer made over one (`queries` None) - its filter, the storage's deleted flags and `ids` bound the candidates as they bound
    a search.  `counters`: an F.GroupCounters to fill."""
    scorer = storage_or_scorer if isinstance(storage_or_scorer, RawScorer) else new_raw_scorer(queries, storage_or_scorer)
    try:
        nq, limit, group_size = scorer.nq, int(limit), int(group_size)
        out_keys = np.full((nq, max(limit, 1)), F.GROUP_NONE, dtype=np.uint32)
        out_sizes = np.zeros((nq, max(limit, 1)), dtype=np.uint32)
        out_hits = np.zeros((nq, max(limit, 1), max(group_size, 1)), dtype=ScoredPointOffset)
        out_n = np.zeros(nq, dtype=np.uint32)
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint32)
        thr = None if score_threshold is None else C.byref(C.c_float(score_threshold))
        F.check(F.lib().qmx_group_search(scorer._h, group_keys._h, limit, group_size, F.ptr(ids), 0 if ids is None else len(ids), thr, F.ptr(out_keys),
                                         F.ptr(out_sizes), F.ptr(out_hits), F.ptr(out_n), None if counters is None else C.byref(counters)))
        return [[(int(out_keys[q, g]), out_hits[q, g, :out_sizes[q, g]].copy()) for g in range(int(out_n[q]))] for q in range(nq)]
    finally:
        if scorer is not storage_or_scorer:
            scorer.close()
