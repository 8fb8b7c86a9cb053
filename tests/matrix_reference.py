"""The contract of the distance matrix API (qmx_sample_points, qmx_search_matrix; include/qdrant_amd.h) in plain numpy: what the device calls are
tested against.  `Collection::search_points_matrix`, lib/collection/src/collection/distance_matrix.rs."""
import numpy as np

M64 = (1 << 64) - 1
SearchMatrixPair = np.dtype([("a", np.uint32), ("b", np.uint32), ("score", np.float32)])

# (seed, offset) -> key, computed once by both forms below and frozen; (0, 0) is the first output of splitmix64 from state 0
FROZEN_KEYS = [
    (0, 0, 0xE220A8397B1DCDAF),
    (0, 1, 0x6E789E6AA1B965F4),
    (1, 0, 0x910A2DEC89025CC1),
    (0x5EED, 12345, 0xCBC84078A7339C6A),
    (M64, 0xFFFFFFFE, 0xB079DC1E4A436403),
    (42, 199999, 0xB038E54BB6EEE9C6),
]


def sample_key_int(seed: int, offset: int) -> int:
    """The sampler's key with Python ints masked to 64 bits."""
    z = (seed + (offset + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_keys_np(seed: int, offsets) -> np.ndarray:
    """... with numpy uint64 arithmetic, which wraps mod 2^64."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + (np.asarray(offsets, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sample_reference(live, n: int, seed: int) -> np.ndarray:
    """The n live offsets of smallest (key, offset), ascending.  `live`: bool per offset (not deleted, vector present, allowed)."""
    cand = np.flatnonzero(np.asarray(live, dtype=bool)).astype(np.uint64)
    keys = sample_keys_np(seed, cand)
    order = np.lexsort((cand, keys))[:n]
    return np.sort(cand[order]).astype(np.uint32)


def matrix_reference(score_matrix, live, limit: int):
    """score_matrix [S][S]: row i = the scores of sample point i as the query against every sample point; live [S].  Per row the positions of the
    `limit` best live others - score descending (NaN greatest, as OrderedFloat), then position ascending; self dropped by POSITION - as a list of
    (cols, scores)."""
    sc = np.asarray(score_matrix, dtype=np.float32)
    live = np.asarray(live, dtype=bool)
    s = sc.shape[0]
    out = []
    if s < 2 or limit == 0:
        return [(np.zeros(0, np.uint32), np.zeros(0, np.float32)) for _ in range(s)]
    cand = np.flatnonzero(live)
    for i in range(s):
        cols = cand[cand != i]
        row = sc[i, cols]
        rank = np.where(np.isnan(row), np.inf, row.astype(np.float64))
        if len(cols) > 4 * limit + 64:      # (only the rows at or above the limit-th best score can be in the list: sort those)
            keep = rank >= np.partition(rank, len(rank) - limit)[len(rank) - limit]
            cols, row, rank = cols[keep], row[keep], rank[keep]
        order = np.lexsort((cols, -rank))[:limit]
        out.append((cols[order].astype(np.uint32), row[order]))
    return out


def pairs_reference(ids, nearests) -> np.ndarray:
    """SearchMatrixPairsResponse::from (distance_matrix.rs:96-118).  nearests: per row a list of (id, score)."""
    return np.array([(a, b, s) for a, row in zip(ids, nearests) for b, s in row], dtype=SearchMatrixPair)


def offsets_reference(ids, nearests):
    """SearchMatrixOffsetsResponse::from (distance_matrix.rs:64-94): the columns by a lookup of the id, as the reference does it."""
    offset_by_id = {int(x): i for i, x in enumerate(ids)}
    rows = [i for i, row in enumerate(nearests) for _ in row]
    cols = [offset_by_id[int(b)] for row in nearests for b, _ in row]
    scores = [s for row in nearests for _, s in row]
    return (np.array(rows, dtype=np.uint64), np.array(cols, dtype=np.uint64), np.array(scores, dtype=np.float32), np.asarray(ids))
