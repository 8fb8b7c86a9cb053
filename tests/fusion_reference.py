"""numpy restatement (np.float32, one rounded operation per step, the reference's order) of the reference's fusion and MMR code:

  position_score, rrf_scoring                                 lib/segment/src/common/reciprocal_rank_fusion.rs:32-99
  welfords_mean_variance, distr_norm, norm, score_fusion      lib/segment/src/common/score_fusion.rs:46-164
  mmr_from_points_with_vector, maximal_marginal_relevance     lib/shard/src/query/mmr/mod.rs:42-100, 198-279

Lists are numpy arrays of ScoredPointOffset (idx, score).  The reference leaves the order among equal fused scores to its hash map; the final sort
here applies the project's rule instead: score descending in OrderedFloat order, the lower offset first among equal scores.  The MMR part keeps
the reference's own tie behaviour: `max_by_key` returns the last maximal element in the iteration order of an IndexSet that shrinks by swap_remove.
Pair and relevance scores come in as callables.  Checker only: nothing under qdrant_amd/ imports this file."""
import numpy as np

ScoredPointOffset = np.dtype([("idx", np.uint32), ("score", np.float32)])
f32 = np.float32


def _of_key(x):
    """OrderedFloat as a sortable pair: NaN greatest (and equal to itself), -0.0 == 0.0."""
    x = f32(x)
    if np.isnan(x):
        return (1, 0.0)
    return (0, float(x))          # float(-0.0) == float(0.0) compares equal


def position_score(position, k, weight):
    """reciprocal_rank_fusion.rs:32-39"""
    weight = f32(weight)
    if weight <= f32(0.0):
        return f32(0.0)
    with np.errstate(all="ignore"):
        return f32(1.0) / (f32(position + 1) / weight + f32(k) - f32(1.0))


def _sorted(acc, top):
    items = sorted(acc.items(), key=lambda kv: (tuple(-c for c in _of_key(kv[1])), kv[0]))
    if top is not None:
        items = items[:top]
    out = np.zeros(len(items), dtype=ScoredPointOffset)
    for i, (idx, score) in enumerate(items):
        out[i] = (idx, score)
    return out


def rrf_scoring(responses, k=2, weights=None, top=None):
    """reciprocal_rank_fusion.rs:54-99.  A weights list of another length than the responses: ValueError (the reference's validation error)."""
    if weights is not None and len(weights) != len(responses):
        raise ValueError("Number of weights in RRF should match number of pre-fetches: got %d, expected %d" % (len(weights), len(responses)))
    acc = {}
    for s, response in enumerate(responses):
        weight = f32(1.0) if weights is None else f32(weights[s])
        for pos, idx in enumerate(response["idx"].tolist()):
            score = position_score(pos, k, weight)
            if idx in acc:
                with np.errstate(all="ignore"):
                    acc[idx] = f32(acc[idx] + score)
            else:
                acc[idx] = score
    return _sorted(acc, top)


def welfords_mean_variance(scores):
    """score_fusion.rs:126-145"""
    mean, aggregate = f32(0.0), f32(0.0)
    with np.errstate(all="ignore"):
        for k, x in enumerate(np.asarray(scores, dtype=np.float32), start=1):
            old_delta = f32(x - mean)
            mean = f32(mean + f32(old_delta / f32(k)))
            delta = f32(x - mean)
            aggregate = f32(aggregate + f32(old_delta * delta))
        return mean, f32(aggregate / f32(f32(len(scores)) - f32(1.0)))


def norm(scores, lo, hi):
    """score_fusion.rs:97-109"""
    scores = np.asarray(scores, dtype=np.float32)
    if lo == hi:
        return np.full(len(scores), 0.5, dtype=np.float32)
    with np.errstate(all="ignore"):
        span = f32(hi - lo)
        return np.array([f32(f32(s - lo) / span) for s in scores], dtype=np.float32)


def distr_norm(scores):
    """score_fusion.rs:149-164"""
    scores = np.asarray(scores, dtype=np.float32)
    if len(scores) < 2:
        return np.full(len(scores), 0.5, dtype=np.float32)
    mean, variance = welfords_mean_variance(scores)
    with np.errstate(all="ignore"):
        std_dev = f32(np.sqrt(variance))
        lo = f32(mean - f32(f32(3.0) * std_dev))
        hi = f32(mean + f32(f32(3.0) * std_dev))
    return norm(scores, lo, hi)


def score_fusion(responses, weights=(), top=None):
    """score_fusion.rs:46-94 with ScoreFusion::dbsf(): Distr normalisation, Sum, LargeBetter; missing weights are 1.0."""
    acc = {}
    for s, response in enumerate(responses):
        weight = f32(weights[s]) if s < len(weights) else f32(1.0)
        normed = distr_norm(response["score"])
        for idx, x in zip(response["idx"].tolist(), normed):
            with np.errstate(all="ignore"):
                score = f32(x * weight)
                acc[idx] = f32(acc[idx] + score) if idx in acc else score
    return _sorted(acc, top)


def maximal_marginal_relevance(n, relevance, similarity, lambda_, limit):
    """mod.rs:198-279 over candidates 0..n: `relevance(c)` and `similarity(c, s)` (candidate c as the query against selected s) are callables
    returning f32.  Returns the selected candidate indices in selection order."""
    if n == 0 or limit == 0:
        return []
    lambda_ = f32(lambda_)
    rel = [f32(relevance(c)) for c in range(n)]
    remaining = list(range(n))          # IndexSet filled 0..n

    def swap_remove(c):
        p = remaining.index(c)
        remaining[p] = remaining[-1]
        remaining.pop()

    def last_max(items, key):
        best = None
        for it in items:                # max_by_key: the last maximal element
            if best is None or _of_key(key(it)) >= _of_key(key(best)):
                best = it
        return best

    selected = [last_max(remaining, lambda c: rel[c])]
    swap_remove(selected[0])
    cache = {}

    def sim(c, s):
        if (c, s) not in cache:
            cache[(c, s)] = f32(similarity(c, s))
        return cache[(c, s)]

    while len(selected) < limit and remaining:
        scored = []
        for c in remaining:
            max_sim = last_max([sim(c, s) for s in selected], lambda x: x)
            with np.errstate(all="ignore"):
                scored.append((c, f32(f32(lambda_ * rel[c]) - f32(f32(f32(1.0) - lambda_) * max_sim))))
        best = last_max(scored, lambda cs: cs[1])[0]
        swap_remove(best)
        selected.append(best)
    return selected


def mmr_from_points(candidates, relevance_of_id, similarity_of_ids, lambda_, limit):
    """mod.rs:42-100 over one ScoredPointOffset list: unique by id (first occurrence stays), fewer than two candidates returned as they are,
    else the selection in selection order with the INPUT scores.  relevance_of_id(id) / similarity_of_ids(id_c, id_s) return f32."""
    candidates = np.asarray(candidates, dtype=ScoredPointOffset)
    seen, keep = set(), []
    for j, idx in enumerate(candidates["idx"].tolist()):
        if idx not in seen:
            seen.add(idx)
            keep.append(j)
    uniq = candidates[keep] if keep else np.zeros(0, dtype=ScoredPointOffset)
    if len(uniq) < 2:
        return uniq
    ids = uniq["idx"].tolist()
    picked = maximal_marginal_relevance(len(uniq), lambda c: relevance_of_id(ids[c]), lambda c, s: similarity_of_ids(ids[c], ids[s]), lambda_, limit)
    return uniq[picked] if picked else np.zeros(0, dtype=ScoredPointOffset)
