"""merge_points_kernel (csrc/topk_merge.hip) where it can go wrong: ids that repeat across and inside lists, twins placed against
the 64-entry pass structure, twins made and unmade by id bases, ties across pass boundaries, and the documented size cap.

Every case is a hand-built set of lists run through qmx_merge_topk (host arrays), qmx_merge_topk_async (device arrays, ids globalised by the
caller and by `list_idx_base_dev`) and qmx_merge_topk_packed_async (records with rubbish in the padding), each held to the plain model of
tests/merge_reference.py: ids, score bits, counts, and (0, 0.0f) in every slot past the count.  Where the kept items' scores are all
distinct the reference's order is determined and the oracle's aggregator (`SearchResultAggregator::push`,
lib/shard/src/search_result_aggregator.rs:28-37) is asserted too; among equal scores the rule is the header's: the lower id first."""
import ctypes as C

import numpy as np
import pytest

import merge_reference as M
import oracle_ffi as O

pytestmark = pytest.mark.gpu

NAN_OUT = 0x7FFFFFFF         # what the order word of a NaN decodes to (merge_reference.word_score_bits)
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    import torch
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return torch.device("cuda", 0)


def _build(per_list, k, nq=1, dead=None):
    """per_list[l] = [(idx, score), ...] for one query (repeated for every query) -> lists, counts.  The slots past a list's count hold
    `dead[l]` where given, else a live id with the best score there is: an entry past the count is not an item."""
    n_lists = len(per_list)
    lists = np.zeros((n_lists, nq, k), dtype=O.ScoredPointOffset)
    counts = np.zeros((n_lists, nq), dtype=np.uint32)
    some_id = next((it[0] for items in per_list for it in items), 0)
    for l, items in enumerate(per_list):
        assert len(items) <= k
        pad = list(dead[l]) if dead and dead.get(l) else []
        row = list(items) + pad + [(some_id, np.inf)] * (k - len(items) - len(pad))
        for q in range(nq):
            lists[l, q]["idx"] = [it[0] for it in row]
            lists[l, q]["score"] = np.array([it[1] for it in row], dtype=np.float32)
            counts[l, q] = len(items)
    return lists, counts


def _oracle_determined(items):
    """The reference's list is determined when no two KEPT items compare equal (OrderedFloat: -0.0 == 0.0, all NaN equal)."""
    seen, keys = set(), []
    for idx, score in items:
        if idx not in seen:
            seen.add(idx)
            keys.append("nan" if score != score else float(score))
    return len(set(keys)) == len(keys)


def _check_rows(tag, idx, bits, cnt, want, k):
    """idx / bits [nq, k] uint32, cnt [nq] against the model's lists."""
    for q, w in enumerate(want):
        assert cnt[q] == len(w), (tag, q, int(cnt[q]), len(w))
        assert idx[q, :len(w)].tolist() == w["idx"].tolist(), (tag, q)
        assert bits[q, :len(w)].tolist() == w["score"].view(np.uint32).tolist(), (tag, q)
        assert not idx[q, len(w):].any() and not bits[q, len(w):].any(), (tag, q, "slots past the count are (0, 0.0f)")


def _run_all(dev, lists, counts, k, bases=None, check_oracle=True):
    """All entry points against the model; returns the model's lists."""
    import torch
    from qdrant_amd import _ffi as F, sharded
    lib = F.lib()
    n_lists, nq = lists.shape[0], lists.shape[1]
    want = M.merge(lists, counts, k, bases)
    if check_oracle:
        ref = O.merge_topk(lists, counts, k, bases)
        for q, items in enumerate(M.live_items(lists, counts, k, bases)):
            if _oracle_determined(items):
                bits = ref[q]["score"].view(np.uint32).copy()
                bits[np.isnan(ref[q]["score"])] = NAN_OUT
                assert ref[q]["idx"].tolist() == want[q]["idx"].tolist() and bits.tolist() == want[q]["score"].view(np.uint32).tolist(), ("oracle", q)
    # the two spellings of the same ids: globalised by the caller / idx + base on the device (a base of the test's own where the case has none)
    b = np.ascontiguousarray(bases, dtype=np.uint32) if bases is not None else (np.arange(n_lists, dtype=np.uint32) * np.uint32(1000003) + np.uint32(0xFFFF0000))
    glob = lists.copy()
    glob["idx"] = lists["idx"] + (b[:, None, None] if bases is not None else np.uint32(0))
    local = glob.copy()
    local["idx"] = glob["idx"] - b[:, None, None]                                # wraps: idx + base is the id again mod 2^32
    rubbish = 0x7F7F7F7F
    # 1. host arrays
    out = np.full((nq, k, 2), rubbish, dtype=np.uint32)
    oc = np.full(nq, rubbish, dtype=np.uint32)
    F.check(lib.qmx_merge_topk(0, F.ptr(glob), F.ptr(counts), n_lists, nq, k, F.ptr(out), F.ptr(oc)))
    _check_rows("host", out[:, :, 0], out[:, :, 1], oc, want, k)
    # 2. device arrays, without and with bases
    st = torch.cuda.Stream(dev)
    d_cnt = None if counts is None else torch.from_numpy(counts.view(np.int32)).to(dev)
    d_base = torch.from_numpy(b.view(np.int32)).to(dev)
    for tag, src, base in (("async", glob, None), ("async+bases", local, d_base)):
        d_l = torch.from_numpy(np.ascontiguousarray(src).view(np.int32).reshape(n_lists, nq, k, 2)).to(dev)
        d_out = torch.full((nq, k, 2), rubbish, dtype=torch.int32, device=dev)
        d_oc = torch.full((nq,), rubbish, dtype=torch.int32, device=dev)
        F.check(lib.qmx_merge_topk_async(0, C.c_void_p(st.cuda_stream), F.ptr(d_l), F.ptr(d_cnt), F.ptr(base), n_lists, nq, k, F.ptr(d_out), F.ptr(d_oc)))
        st.synchronize()
        got = d_out.cpu().numpy().view(np.uint32)
        _check_rows(tag, got[:, :, 0], got[:, :, 1], d_oc.cpu().numpy().view(np.uint32), want, k)
    # 3. packed records, bases on the device
    words = sharded.record_words(nq, k)
    rec = np.full((n_lists, words), rubbish, dtype=np.int32)
    for l in range(n_lists):
        rec[l, :nq * k * 2] = np.ascontiguousarray(local[l]).view(np.int32).reshape(-1)
        rec[l, nq * k * 2:nq * k * 2 + nq] = (np.full(nq, k, dtype=np.uint32) if counts is None else counts[l]).view(np.int32)
    d_rec = torch.from_numpy(rec).to(dev)
    d_out = torch.full((nq, k, 2), rubbish, dtype=torch.int32, device=dev)
    d_oc = torch.full((nq,), rubbish, dtype=torch.int32, device=dev)
    F.check(lib.qmx_merge_topk_packed_async(0, C.c_void_p(st.cuda_stream), F.ptr(d_rec), F.ptr(d_base), n_lists, nq, k, F.ptr(d_out), F.ptr(d_oc)))
    st.synchronize()
    got = d_out.cpu().numpy().view(np.uint32)
    _check_rows("packed", got[:, :, 0], got[:, :, 1], d_oc.cpu().numpy().view(np.uint32), want, k)
    return want


# ---- duplicate-heavy random lists ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_lists,nq,k", [(2, 3, 10), (8, 4, 64), (5, 3, 65), (3, 2, 128), (16, 2, 129), (4, 2, 1000), (64, 2, 256)])
def test_duplicate_heavy_lists(dev, n_lists, nq, k):
    rng = np.random.default_rng(n_lists * 10007 + k)
    lists, counts = M.duplicate_heavy_lists(rng, n_lists, nq, k, n_ids=k + k // 2)
    assert counts.min() == 0 and counts.max() == k
    share = M.duplicate_share(lists, counts, k)
    assert share > (0.25 if n_lists >= 4 else 0.0), share         # (the share of items DROPPED; two lists of distinct ids cannot reach one half)
    for items in M.live_items(lists, counts, k):
        assert _oracle_determined(items)
    _run_all(dev, lists, counts, k)


# ---- twins against the pass structure --------------------------------------------------------------------------------------------------

def _ranked(k, n_lists, total, rng):
    """`total` items with the scores total .. 1 (the item of final rank r scores total - r: a score of total - r + 0.5 slots in AT rank r), ids
    in random order, dealt to the lists round-robin."""
    ids = 10_000 + rng.permutation(total)
    per_list = [[] for _ in range(n_lists)]
    for r in range(total):
        per_list[r % n_lists].append((int(ids[r]), f32(total - r)))
    return per_list


X = 77


def _at_rank(total, r):
    return f32(total - r + 0.5)


def _twin_cases(k):
    """name -> (per_list, dead, expected rank of X or None)"""
    total, n_lists = 2 * k + 20, 3         # k slots per list hold total / 3 ranked items and the injected ones
    cases = {}

    def base(seed):
        return _ranked(k, n_lists, total, np.random.default_rng(seed + k))

    p = base(1)
    p[0].append((X, f32(-5.0)))             # the first occurrence is the worst item of all: it misses the top k
    p[2].insert(0, (X, f32(9999.0)))        # the twin would be the best
    cases["first_misses_the_top_twin_is_best"] = (p, None, None)
    p = base(2)
    p[0].insert(2, (X, _at_rank(total, 5)))
    p[1].append((X, _at_rank(total, 70)))
    cases["first_in_pass0_twin_in_pass1"] = (p, None, 5)
    p = base(3)
    p[0].append((X, _at_rank(total, 70)))
    p[1].insert(2, (X, _at_rank(total, 5)))
    cases["first_in_pass1_twin_in_pass0"] = (p, None, 70)
    for r in (63, 64):
        for twin_rank in (3, 100):
            p = base(4 + r + twin_rank)
            p[1].append((X, _at_rank(total, r)))
            p[2].append((X, _at_rank(total, twin_rank)))
            cases["kept_at_rank_%d_twin_at_%d" % (r, twin_rank)] = (p, None, r)
    p = base(5)
    p[1].insert(3, (X, _at_rank(total, 66)))
    p[1].insert(1, (X + 1, _at_rank(total, 30)))
    p[1].append((X, _at_rank(total, 2)))    # the same list again: dropped too
    p[1].append((X + 1, _at_rank(total, 1)))
    cases["twin_inside_one_list"] = (p, None, 66 + 1)       # X + 1 at rank 30 pushes X to 67
    p = base(6)
    p[2].append((X, _at_rank(total, 64)))
    cases["twin_past_the_count_is_no_item"] = (p, {0: [(X, f32(9999.0))], 1: [(X, _at_rank(total, 1))]}, 64)
    return cases


@pytest.mark.parametrize("k", [65, 130])
@pytest.mark.parametrize("name", ["first_misses_the_top_twin_is_best", "first_in_pass0_twin_in_pass1", "first_in_pass1_twin_in_pass0",
                                  "kept_at_rank_63_twin_at_3", "kept_at_rank_63_twin_at_100", "kept_at_rank_64_twin_at_3", "kept_at_rank_64_twin_at_100",
                                  "twin_inside_one_list", "twin_past_the_count_is_no_item"])
def test_twin_placement_against_the_passes(dev, k, name):
    per_list, dead, rank = _twin_cases(k)[name]
    lists, counts = _build(per_list, k, nq=2, dead=dead)
    want = _run_all(dev, lists, counts, k)
    ids = want[0]["idx"].tolist()
    assert len(ids) == k and ids.count(X) == (0 if rank is None or rank >= k else 1)
    if rank is not None and rank < k:
        assert ids.index(X) == rank                           # the case is what its name says


# ---- twins made by bases ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [10, 130])
def test_twins_made_and_unmade_by_bases(dev, k):
    rng = np.random.default_rng(k)
    n_lists = 4
    bases = np.array([100, 50, 1000, 0xFFFFFF00], dtype=np.uint32)
    per_list = [[(int(i), f32(s)) for i, s in zip(rng.permutation(5000)[:k - 4] + 20_000 * (l + 1), -np.sort(-rng.permutation(100_000)[:k - 4]) + f32(0.25) * l)]
                for l in range(n_lists)]
    per_list[0].append((5, f32(-1.0)))                  # id 105
    per_list[1].append((55, f32(200_000.0)))            # 55 + 50 = 105 again: dropped, best score or not
    per_list[0].append((7, f32(-2.0)))                  # id 107
    per_list[2].append((7, f32(-3.0)))                  # the same idx under another base: id 1007, stays
    per_list[3].append((0x105 + 0x100, f32(300_000.0)))    # 0x205 + 0xFFFFFF00 wraps to 0x105 = 261 ...
    per_list[1].append((261 - 50, f32(-4.0)))           # ... which list 1 pushed first
    lists, counts = _build(per_list, k, nq=2)
    want = _run_all(dev, lists, counts, k, bases)
    every = M.merge(lists, counts, n_lists * k, bases)[0]      # (a model call with room for every item: who survives the dedupe)
    kept = dict(zip(every["idx"].tolist(), every["score"].tolist()))
    assert kept[105] == -1.0 and kept[107] == -2.0 and kept[1007] == -3.0 and kept[261] == -4.0
    assert 200_000.0 not in want[0]["score"].tolist() and 300_000.0 not in want[0]["score"].tolist()


# ---- a replicated segment --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_lists,k,count0", [(2, 64, 64), (4, 130, 130), (4, 130, 70), (7, 65, 1)])
def test_replicated_segment_gives_list_zero(dev, n_lists, k, count0):
    rng = np.random.default_rng(k + count0)
    first = [(int(i), f32(s)) for i, s in zip(rng.permutation(100_000)[:count0], -np.sort(-rng.permutation(1_000_000)[:count0]))]
    lists, counts = _build([first] * n_lists, k, nq=3)
    want = _run_all(dev, lists, counts, k)
    for q in range(3):
        assert want[q]["idx"].tolist() == [i for i, _ in first] and want[q]["score"].tolist() == [float(s) for _, s in first]


# ---- ties ------------------------------------------------------------------------------------------------------------------------------

def _deal(items, n_lists, k, rng):
    """items in any order -> n_lists lists (random owner, random position)."""
    per_list = [[] for _ in range(n_lists)]
    for it in [items[i] for i in rng.permutation(len(items))]:
        free = [l for l in range(n_lists) if len(per_list[l]) < k]
        per_list[free[int(rng.integers(0, len(free)))]].append(it)
    return per_list


def test_equal_scores_straddle_the_pass_boundaries(dev):
    """Ranks 60..67 share one score and so do ranks 125..131: the lower id first, across 63|64 and 127|128, and the cut at 130 inside a run."""
    rng = np.random.default_rng(11)
    k, total = 130, 200
    ids = rng.permutation(50_000)[:total]
    scores = [f32(total - r) for r in range(total)]
    for lo, hi in ((60, 67), (125, 131)):
        for r in range(lo, hi + 1):
            scores[r] = scores[lo]
    lists, counts = _build(_deal(list(zip(ids.tolist(), scores)), 3, k, rng), k, nq=2)
    want = _run_all(dev, lists, counts, k)[0]
    assert want["idx"][60:68].tolist() == sorted(ids[60:68].tolist()) and len(set(want["score"][60:68].tolist())) == 1
    assert want["idx"][125:130].tolist() == sorted(ids[125:132].tolist())[:5]


@pytest.mark.parametrize("k,better", [(65, 0), (130, 61), (130, 64), (200, 30)])
def test_a_whole_pass_of_one_score(dev, k, better):
    """70 equal scores behind `better` distinct ones: a 64-entry pass filled with one value (and for k = 65 / 130 the cut inside the run)."""
    rng = np.random.default_rng(k + better)
    ids = rng.permutation(50_000)[:better + 70 + 5]
    items = [(int(ids[i]), f32(1000 - i)) for i in range(better)] + [(int(i), f32(1.0)) for i in ids[better:better + 70]] + \
            [(int(i), f32(-7.0 - j)) for j, i in enumerate(ids[better + 70:])]
    lists, counts = _build(_deal(items, 4, k, rng), k, nq=2)
    want = _run_all(dev, lists, counts, k)[0]
    run = sorted(ids[better:better + 70].tolist())
    assert want["idx"][better:better + 70].tolist() == run[:k - better]


def test_zeros_infinities_and_nan_on_both_sides_of_a_pass_boundary(dev):
    rng = np.random.default_rng(12)
    k = 130
    nan2 = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]       # a negative NaN with a payload: the same order word
    ids = iter(rng.permutation(50_000).tolist())
    items = [(next(ids), f32(np.nan)), (next(ids), nan2), (next(ids), f32(np.inf)), (next(ids), f32(np.inf))]         # ranks 0..3
    items += [(next(ids), f32(100 - i)) for i in range(59)]                                                          # ranks 4..62
    zeros = [(next(ids), f32(0.0)), (next(ids), f32(-0.0))]                                                           # rank 63 | rank 64
    items += zeros
    items += [(next(ids), f32(-1 - i)) for i in range(62)]                                                           # ranks 65..126
    infs = [(next(ids), f32(-np.inf)), (next(ids), f32(-np.inf))]                                                     # rank 127 | rank 128
    items += infs
    twin = items[0][0]
    lists, counts = _build(_deal(items, 3, k, rng), k, nq=2)
    assert counts[2, 0] + 2 <= k
    # NaN-scored twins: one id twice under NaN, and a finite first occurrence whose twin is NaN
    lists[2, :, counts[2, 0]] = (twin, np.nan)
    lists[2, :, counts[2, 0] + 1] = (items[70][0], np.nan)
    counts[2, :] += 2
    want = _run_all(dev, lists, counts, k)[0]
    bits = want["score"].view(np.uint32).tolist()
    assert bits[:4] == [NAN_OUT, NAN_OUT, 0x7F800000, 0x7F800000] and bits[63:65] == [0x00000000, 0x80000000]
    assert want["idx"][63:65].tolist() == [zeros[0][0], zeros[1][0]] and bits[127:129] == [0xFF800000, 0xFF800000]
    assert want["idx"][127:129].tolist() == sorted(i for i, _ in infs) and len(want) == len(items) == k - 1 and want["idx"].tolist().count(twin) == 1


def test_nan_scores_straddle_a_pass_boundary(dev):
    """66 NaN scores (mixed payloads) with distinct ids, then +inf: all NaN first by ascending id, across 63|64."""
    rng = np.random.default_rng(13)
    k = 65 + 5
    ids = rng.permutation(50_000)[:80].tolist()
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    items = [(ids[i], nans[i % 4]) for i in range(66)] + [(ids[66 + i], f32(np.inf) if i < 2 else f32(5 - i)) for i in range(14)]
    lists, counts = _build(_deal(items, 2, k, rng), k, nq=1)
    want = _run_all(dev, lists, counts, k)[0]
    assert want["idx"][:66].tolist() == sorted(ids[:66]) and want["score"].view(np.uint32)[:66].tolist() == [NAN_OUT] * 66


# ---- degenerate shapes -----------------------------------------------------------------------------------------------------------------

def test_one_list(dev):
    rng = np.random.default_rng(14)
    k = 130
    items = [(int(i), f32(s)) for i, s in zip(rng.integers(0, 80, 100), rng.permutation(1000)[:100])]      # ids repeat inside the list
    lists, counts = _build([items], k, nq=2)
    want = _run_all(dev, lists, counts, k)
    assert len(want[0]) == len({i for i, _ in items}) < 100


@pytest.mark.parametrize("k", [1, 64, 130])
def test_all_counts_zero(dev, k):
    lists, counts = _build([[], [], []], k, nq=3)
    want = _run_all(dev, lists, counts, k)
    assert all(len(w) == 0 for w in want)


def test_fewer_distinct_ids_than_k(dev):
    """At most 70 ids in 4 x 300 slots: the count is the number of distinct ids, reached in the second pass, and the row is cleared behind it."""
    rng = np.random.default_rng(15)
    k = 300
    lists, counts = M.duplicate_heavy_lists(rng, 4, 2, k, n_ids=70)
    counts[:] = [[300, 17], [250, 300], [0, 64], [300, 65]]
    want = _run_all(dev, lists, counts, k)
    for q in range(2):
        assert len(want[q]) == len({i for i, _ in M.live_items(lists, counts, k)[q]}) and 64 < len(want[q]) <= 70


def test_no_counts_means_full_lists(dev):
    rng = np.random.default_rng(16)
    lists, _ = M.duplicate_heavy_lists(rng, 3, 2, 70, n_ids=100)
    _run_all(dev, lists, None, 70)


def test_k_of_one(dev):
    lists, counts = _build([[(4, f32(1.0))], [(9, f32(3.0))], [(4, f32(5.0))], [], [(2, f32(3.0))]], 1, nq=2)
    want = _run_all(dev, lists, counts, 1)
    assert want[0]["idx"].tolist() == [2]          # 4 keeps its first score, 1.0; 9 and 2 tie at 3.0: the lower id


# ---- the size cap ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_lists,k", [(16, 1024), (256, 64)])
def test_merge_at_the_cap(dev, n_lists, k):
    """n_lists * k = 16384, the documented limit: a 64 KiB seen-id table in LDS beside the pass's 2 KiB of static arrays.  The launch is
    accepted as it stands (no hipFuncSetAttribute) and the lists are the model's.  Measured on an MI355X, four launches of nq = 2 each:
    (256, 64) 0.2 s, (16, 1024) 3.6 s.  (1, 16384) gives the model's lists too, but its 256 passes re-run the quadratic twin scan in one
    wavefront: 96 s for the four launches, so it is not part of the suite."""
    rng = np.random.default_rng(n_lists + k)
    nq, total = 2, n_lists * k
    lists = np.zeros((n_lists, nq, k), dtype=O.ScoredPointOffset)
    for q in range(nq):
        ids = np.repeat(rng.permutation(1 << 17)[:total // 2], 2)[rng.permutation(total)].reshape(n_lists, k)      # every id twice, anywhere
        scores = M.distinct_scores(rng, total).reshape(n_lists, k)
        lists[:, q]["idx"] = ids
        lists[:, q]["score"] = scores
    counts = np.full((n_lists, nq), k, dtype=np.uint32)
    if n_lists > 1:
        counts[n_lists // 2, 0] = k // 3
    assert abs(M.duplicate_share(lists, counts, k) - 0.5) < 0.02
    _run_all(dev, lists, counts, k, check_oracle=False)


@pytest.mark.parametrize("n_lists,k", [(17, 1024), (1, 16385)])
def test_merge_past_the_cap_is_refused(dev, n_lists, k):
    import torch
    from qdrant_amd import _ffi as F, sharded
    lib = F.lib()
    nq = 2
    lists = np.zeros((n_lists, nq, k), dtype=O.ScoredPointOffset)
    counts = np.zeros((n_lists, nq), dtype=np.uint32)
    out = np.zeros((nq, k), dtype=O.ScoredPointOffset)
    oc = np.zeros(nq, dtype=np.uint32)
    text = "merge of %d lists x %d entries exceeds the 64 KiB seen-id table" % (n_lists, k)
    assert lib.qmx_merge_topk(0, F.ptr(lists), F.ptr(counts), n_lists, nq, k, F.ptr(out), F.ptr(oc)) == F.ERR_NOT_SUPPORTED
    assert F.last_error() == text
    d_l = torch.zeros((n_lists, sharded.record_words(nq, k)), dtype=torch.int32, device=dev)       # large enough for either layout
    d_c = torch.zeros((n_lists, nq), dtype=torch.int32, device=dev)
    d_out, d_oc = torch.zeros((nq, k, 2), dtype=torch.int32, device=dev), torch.zeros((nq,), dtype=torch.int32, device=dev)
    assert lib.qmx_merge_topk_async(0, None, F.ptr(d_l), F.ptr(d_c), None, n_lists, nq, k, F.ptr(d_out), F.ptr(d_oc)) == F.ERR_NOT_SUPPORTED
    assert F.last_error() == text
    assert lib.qmx_merge_topk_packed_async(0, None, F.ptr(d_l), None, n_lists, nq, k, F.ptr(d_out), F.ptr(d_oc)) == F.ERR_NOT_SUPPORTED
    assert F.last_error() == text
    torch.cuda.synchronize()
    assert not d_out.any() and not d_oc.any()
