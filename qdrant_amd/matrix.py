"""The distance matrix API on the device (`/points/search/matrix/pairs` and `/offsets`): `Collection::search_points_matrix`
(lib/collection/src/collection/distance_matrix.rs:141-289) = "sample `sample` points under a filter and return, for each of them, its `limit` nearest
among the other sampled points".  `sample_points` is the reference's `Sample::Random` query made deterministic in a seed, `search_matrix` its batch of
Nearest searches under `HasId(sample)` with the row's own entry dropped; include/qdrant_amd.h has both contracts.  Ids are point offsets of one segment."""
import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

from . import _ffi as F
from .scorer import ScoredPointOffset, _bits_to_words

DEFAULT_SAMPLE = 10               # CollectionSearchMatrixRequest::DEFAULT_SAMPLE (distance_matrix.rs:43)
DEFAULT_LIMIT_PER_SAMPLE = 3      # ... ::DEFAULT_LIMIT_PER_SAMPLE (:42)
MAX_SAMPLE = 65536

SearchMatrixPair = np.dtype([("a", np.uint32), ("b", np.uint32), ("score", np.float32)])      # SearchMatrixPair {a, b, score}


class SearchMatrix:
    """`CollectionSearchMatrixResponse` {sample_ids, nearests} (distance_matrix.rs:28-32): `ids` uint32 [S] ascending, `nearests` one ScoredPointOffset
    array per sampled point (idx = the neighbour's offset), `cols` the neighbours' positions in `ids`."""

    def __init__(self, ids: np.ndarray, nearests: List[np.ndarray], cols: List[np.ndarray]):
        self.ids, self.nearests, self.cols = ids, nearests, cols

    def pairs(self) -> np.ndarray:
        """`SearchMatrixPairsResponse` (distance_matrix.rs:96-118): (a, b, score) row by row, each row's hits in list order."""
        out = np.zeros(sum(len(r) for r in self.nearests), dtype=SearchMatrixPair)
        at = 0
        for a, row in zip(self.ids, self.nearests):
            out["a"][at:at + len(row)] = a
            out["b"][at:at + len(row)] = row["idx"]
            out["score"][at:at + len(row)] = row["score"]
            at += len(row)
        return out

    def offsets(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """`SearchMatrixOffsetsResponse` (distance_matrix.rs:64-94): (offsets_row, offsets_col, scores, ids); the columns are the device's, not a host lookup."""
        rows = np.concatenate([np.full(len(r), i, dtype=np.uint64) for i, r in enumerate(self.nearests)]) if self.nearests else np.zeros(0, np.uint64)
        cols = np.concatenate(self.cols).astype(np.uint64) if self.cols else np.zeros(0, np.uint64)
        scores = np.concatenate([r["score"] for r in self.nearests]) if self.nearests else np.zeros(0, np.float32)
        return rows, cols, scores.astype(np.float32), self.ids


def _sample(storage, n: int, mask, seed: int, out_ids) -> int:
    if mask is not None and len(mask) == 0:      # (a mask without bits allows nothing; its empty word array has no address to hand over)
        return 0
    words = _bits_to_words(mask)
    count = C.c_uint32(0)
    F.check(F.lib().qmx_sample_points(storage._h, F.ptr(words), 0 if mask is None else len(mask), int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, F.ptr(out_ids),
                                      C.cast(C.byref(count), C.c_void_p)))
    return int(count.value)


def sample_points(storage, n: int, mask=None, seed: int = 0) -> np.ndarray:
    """qmx_sample_points: the `n` live points of `storage` (allowed by the bool array `mask`, when given) with the smallest seeded keys, as ascending
    uint32 offsets; fewer when fewer qualify."""
    out = np.zeros(max(int(n), 1), dtype=np.uint32)
    return out[:_sample(storage, n, mask, seed, out)].copy()


def search_matrix(storage, sample_ids, limit: int = DEFAULT_LIMIT_PER_SAMPLE, counters: Optional["F.Counters"] = None) -> SearchMatrix:
    """qmx_search_matrix: for every point of `sample_ids` (strictly ascending offsets; a numpy array or a device tensor of int32 / uint32) its `limit`
    nearest among the others."""
    on_device = hasattr(sample_ids, "data_ptr")
    ids = sample_ids if on_device else np.ascontiguousarray(sample_ids, dtype=np.uint32)
    s, limit = int(ids.shape[0]), int(limit)
    hits = np.zeros((s, max(limit, 1)), dtype=ScoredPointOffset)
    cols = np.zeros((s, max(limit, 1)), dtype=np.uint32)
    counts = np.zeros(max(s, 1), dtype=np.uint32)
    F.check(F.lib().qmx_search_matrix(storage._h, F.ptr(ids), s, limit, F.ptr(hits), F.ptr(cols), F.ptr(counts), None if counters is None else C.byref(counters)))
    host_ids = ids.cpu().numpy().view(np.uint32).copy() if on_device else ids
    return SearchMatrix(host_ids, [hits[i, :counts[i]].copy() for i in range(s)], [cols[i, :counts[i]].copy() for i in range(s)])


def _search_matrix_sampled(storage, sample: int, limit: int, mask, seed: int) -> SearchMatrix:
    import torch
    d_ids = torch.zeros(max(int(sample), 1), dtype=torch.int32, device=torch.device("cuda", getattr(storage, "device_id", 0)))
    count = _sample(storage, sample, mask, seed, d_ids)      # (the ids stay on the device between the two calls)
    return search_matrix(storage, d_ids[:count], limit)


def search_matrix_pairs(storage, sample: int = DEFAULT_SAMPLE, limit: int = DEFAULT_LIMIT_PER_SAMPLE, mask=None, seed: int = 0) -> np.ndarray:
    """`/points/search/matrix/pairs`: sample, search, `SearchMatrix.pairs()`."""
    return _search_matrix_sampled(storage, sample, limit, mask, seed).pairs()


def search_matrix_offsets(storage, sample: int = DEFAULT_SAMPLE, limit: int = DEFAULT_LIMIT_PER_SAMPLE, mask=None, seed: int = 0):
    """`/points/search/matrix/offsets`: sample, search, `SearchMatrix.offsets()`."""
    return _search_matrix_sampled(storage, sample, limit, mask, seed).offsets()
