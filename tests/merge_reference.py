"""A plain model of the cross-segment merge (`SearchResultAggregator::push`, lib/shard/src/search_result_aggregator.rs:28-37, behind
`BatchResultAggregator`) and of the rescoring tail's sort, on Python ints: no float compare decides an order here.

The order is the one include/qdrant_amd.h states for every top-k list: score descending in the f32 order word of csrc/common.hpp
(NaN greatest, -0.0 just below +0.0), the LOWER id first among equal scores.  Where all scores of a merge are distinct this is the
reference's own list (tests/test_merge_reference.py holds the model to the oracle's aggregator there); among equal scores the
reference's order is that of its heap, and the header's rule is the device's contract."""
import struct

import numpy as np

ScoredPointOffset = np.dtype([("idx", np.uint32), ("score", np.float32)])


def ord_word(score):
    """f32 -> u32, monotonic in the score: NaN -> 0xFFFFFFFF, else the bits with the sign flipped (negative: all bits)."""
    b = struct.unpack("<I", struct.pack("<f", score))[0]
    if (b & 0x7F800000) == 0x7F800000 and (b & 0x007FFFFF):
        return 0xFFFFFFFF
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def word_score_bits(word):
    """The inverse of ord_word as f32 bits.  Every NaN shares the word 0xFFFFFFFF, so a NaN score comes back as 0x7FFFFFFF whatever
    its payload was (`ord_to_score` of common.hpp: the device sorts keys, not records); every other score comes back bit for bit."""
    return (word & 0x7FFFFFFF) if word & 0x80000000 else (~word & 0xFFFFFFFF)


def _sorted(items, top):
    """items: (id, np.float32 score) -> ScoredPointOffset array of the best `top`."""
    keys = sorted((-ord_word(score), idx) for idx, score in items)[:top]
    out = np.zeros(len(keys), dtype=ScoredPointOffset)
    out["idx"] = [idx for _, idx in keys]
    out["score"] = np.array([word_score_bits(-w) for w, _ in keys], dtype=np.uint32).view(np.float32)
    return out


def live_items(lists, counts, k, bases=None):
    """Per query the (id, score) items in the aggregator's order: list-major, then position, min(counts[l, q], k) per list."""
    n_lists, nq = lists.shape[0], lists.shape[1]
    per_query = []
    for q in range(nq):
        items = []
        for l in range(n_lists):
            cnt = k if counts is None else min(int(counts[l][q]), k)
            base = 0 if bases is None else int(bases[l])
            row = lists[l, q]
            items += [((int(row["idx"][i]) + base) & 0xFFFFFFFF, row["score"][i]) for i in range(cnt)]
        per_query.append(items)
    return per_query


def merge(lists, counts, k, bases=None):
    """lists [n_lists, nq, k] ScoredPointOffset, counts [n_lists, nq] or None -> one ScoredPointOffset array per query."""
    out = []
    for items in live_items(lists, counts, k, bases):
        seen, kept = set(), []
        for idx, score in items:
            if idx not in seen:          # the first occurrence stays, later ones go whatever their score
                seen.add(idx)
                kept.append((idx, score))
        out.append(_sorted(kept, k))
    return out


def sort_scored(scores, ids, count, top):
    """The first `count` (score, id) pairs, sorted and cut to `top`; no dedupe (ids are distinct by precondition)."""
    return _sorted([(int(ids[i]), scores[i]) for i in range(int(count))], top)


def duplicate_share(lists, counts, k, bases=None):
    """Share of the live items that repeat an earlier item's id (what the merge has to drop)."""
    live = dup = 0
    for items in live_items(lists, counts, k, bases):
        live += len(items)
        dup += len(items) - len({idx for idx, _ in items})
    return dup / max(live, 1)


def distinct_scores(rng, n):
    """n distinct f32 scores in [-1, 1): integers over a power of two, every step exact in f32."""
    half = 1 << int(2 * n).bit_length()
    assert half <= 1 << 22
    return rng.permutation(2 * half)[:n].astype(np.float32) / np.float32(half) - np.float32(1.0)


def duplicate_heavy_lists(rng, n_lists, nq, k, n_ids):
    """Lists as a segment search returns them (scores descending, ids distinct inside a list), ids from a pool of n_ids << n_lists * k,
    every score of a query distinct; counts random, 0 and k among them whenever there is room."""
    lists = np.zeros((n_lists, nq, k), dtype=ScoredPointOffset)
    for q in range(nq):
        pool = distinct_scores(rng, n_lists * k)
        assert len(set(pool.view(np.uint32).tolist())) == n_lists * k
        for l in range(n_lists):
            lists[l, q]["score"] = np.sort(pool[l * k:(l + 1) * k])[::-1]
            lists[l, q]["idx"] = rng.permutation(n_ids)[:k] if n_ids >= k else rng.integers(0, n_ids, k)
    counts = rng.integers(0, k + 1, size=(n_lists, nq)).astype(np.uint32)
    flat = counts.reshape(-1)
    flat[rng.integers(0, flat.size)] = k
    if flat.size > 1:
        flat[(int(np.argmax(flat == k)) + 1) % flat.size] = 0
    return lists, counts
