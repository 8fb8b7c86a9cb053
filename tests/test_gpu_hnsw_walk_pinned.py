"""The device walk (hnsw.hpp: hnsw_search_kernel), pinned: searches over small graphs from the CPU oracle's builder - never the batched device build -
hashed over everything the API hands back (ids, score bits, counts, the vectors_scored counter; pop traces and the hop prefilter's counters where a call
has them) and compared with tests/golden/hnsw_walk_digests.json, recorded on the device at the commit the file names.  The oracle comparisons of
test_gpu_hnsw*.py leave a walk free wherever scores tie or a storage's scores are not the oracle's to the bit; a search is one wave with a visited set
of its own, so every one of these walks is deterministic, and a refactor of the walk must leave every digest - and the kernel each case launched - as
it is.

Every case walks about 2 000 points with 48 different queries, repeated six times: 288 searches on at most one slot per compute unit (option
hnsw_per_cu = 1: the option cannot cap below that, so 48 searches alone would each have a slot of their own), so that slots draw a second search from
the counter and meet the visited set the first one gave back - the fixture checks that the device has fewer compute units than a case has searches.
A few points are deleted, the first entry point among them.  The kernel's name is pinned with every digest (multi-vector storages make their scorer
inside the call: it is caught there).  The ACORN case over m0 = 96 walks seeded plain arrays made for it (_two_class_plain): the 96 links of every popped candidate fail the
filter and each leads to 96 points that pass, so that the first candidate of every search collects more ids (the test counts them: over 6 000) than the
hop buffer of 4 160 holds, and the walk has to score a prefix early.

Recording (only when the walk's behaviour is meant to change): run this module with QMX_HNSW_WALK_DIGESTS_RECORD=<path of a JSON file>; the digests
are written there and nothing is compared.  Without the variable the module only compares."""
import functools
import hashlib
import json
import os
import types

import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnsw_walk_digests.json")
RECORD = os.environ.get("QMX_HNSW_WALK_DIGESTS_RECORD")

N, N_BIG, NQ, REPEAT, TOP = 2000, 16000, 48, 6, 10


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count < NQ * REPEAT      # one slot per compute unit: slots take a second search
    qdrant_amd.set_option("hnsw_per_cu", 1)
    yield qdrant_amd
    qdrant_amd.set_option("hnsw_per_cu", -1)


@functools.lru_cache(maxsize=None)
def _rows(n, dim, seed=1):
    """A mixture of gaussians, seeded; the rows of a narrower storage are the leading coordinates of the widest."""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((16, 96)).astype(np.float32) * 2.0
    wide = (centers[rng.integers(0, 16, n)] + rng.standard_normal((n, 96)).astype(np.float32) * 0.6).astype(np.float32)
    return np.ascontiguousarray(wide[:, :dim])


def _unit(rows):
    return (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)


def _queries(dim, nq=NQ):
    return np.tile(_rows(nq, dim, seed=2), (REPEAT, 1))


@functools.lru_cache(maxsize=None)
def _plain(n, m):
    """The oracle's graph over the first 64 coordinates (Dot), as plain arrays."""
    st = O.DenseStorage(O.F32, O.DOT, _rows(n, 64))
    return O.Hnsw(st, m=m, ef_construct=64, seed=7, threads=0).export_plain()


@functools.lru_cache(maxsize=None)
def _two_class_plain(n):
    """Seeded plain arrays, level 0 alone, 96 links a point (m = 48, m0 = 96): a point whose id is a multiple of 8 links to 96 points whose ids are not,
    every other point to 96 multiples of 8.  Under the filter "id % 8 != 0" ACORN explores all 96 links of a popped candidate (they fail the filter) and
    collects what they link to (it passes)."""
    rng = np.random.default_rng(17)
    ids = np.arange(n, dtype=np.uint32)
    failing, passing = ids[ids % 8 == 0], ids[ids % 8 != 0]
    neighbors = np.stack([rng.choice(passing if i % 8 == 0 else failing, 96, replace=False) for i in range(n)]).astype(np.uint32)
    return types.SimpleNamespace(m=48, m0=96, reindex=np.zeros(n, dtype=np.uint32), level_offsets=np.array([0, n], dtype=np.uint64),
                                 offsets=np.arange(n + 1, dtype=np.uint64) * 96, neighbors=neighbors.ravel(), ep_ids=np.array([5, 9], dtype=np.uint32),
                                 ep_levels=np.zeros(2, dtype=np.uint32), xp_ids=np.zeros(0, dtype=np.uint32), xp_levels=np.zeros(0, dtype=np.uint32))


def _with(plain, **changes):
    fields = {k: getattr(plain, k) for k in ("m", "m0", "reindex", "level_offsets", "offsets", "neighbors", "ep_ids", "ep_levels")}
    fields["xp_ids"], fields["xp_levels"] = getattr(plain, "xp_ids", ()), getattr(plain, "xp_levels", ())
    fields.update(changes)
    return types.SimpleNamespace(**fields)


def _deleted(plain, n=N, all_entry_points=False):
    d = np.zeros(n, dtype=bool)
    d[[i for i in (3, 77, n - 1) if i < n]] = True
    eps = np.asarray(plain.ep_ids, dtype=np.int64)
    d[eps if all_entry_points else eps[:1]] = True
    return d


class _Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def array(self, a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        self.h.update(np.uint64(a.size).tobytes())
        self.h.update(a.astype(a.dtype.newbyteorder("<")).tobytes())

    def lists(self, res):
        self.array([len(r) for r in res], np.uint32)
        for r in res:
            self.array(r["idx"], np.uint32)
            self.array(np.ascontiguousarray(r["score"]).view(np.uint32), np.uint32)

    def number(self, v):
        self.array([int(v)], np.uint64)


def _check(name, digest, kernel=""):
    got = {"digest": digest.h.hexdigest(), "kernel": kernel}
    if RECORD:
        doc = {"cases": {}}
        if os.path.exists(RECORD):
            with open(RECORD) as f:
                doc = json.load(f)
        doc["cases"][name] = got
        with open(RECORD, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
        return
    with open(GOLDEN) as f:
        want = json.load(f)["cases"]
    assert name in want, "no recorded digest for %s" % name
    assert got == want[name], (name, got, want[name])


def _storage(qa, kind, dim, rows=None, n=N):
    D = qa.Distance
    raw = _rows(n, dim) if rows is None else rows
    if kind == "f32_dot":
        return qa.VectorStorage(raw, D.Dot)
    if kind == "f16_dot":
        return qa.VectorStorage(raw.astype(np.float16), D.Dot, qa.VectorStorageDatatype.Float16)
    if kind == "u8_cosine":
        return qa.VectorStorage(np.clip(raw * 20.0 + 128.0, 0, 255).astype(np.uint8), D.Cosine, qa.VectorStorageDatatype.Uint8)
    if kind == "sq_euclid":
        quant = qa.ScalarQuantizer.from_min_max(raw, dim, D.Euclid)
        return qa.EncodedVectorsU8(quant.encode(raw), quant)
    if kind == "bq":
        quant = qa.BinaryQuantizer(dim, D.Dot)
        return qa.EncodedVectorsBin(quant.encode(raw), quant)
    if kind.startswith("pq"):           # pq<chunk>: 256 centroids, dim / chunk LUT rows of 1 KiB per search
        rng = np.random.default_rng(dim)
        cen = (raw[rng.choice(len(raw), 256, replace=False)] + rng.standard_normal((256, dim)).astype(np.float32) * 0.1).astype(np.float32)
        quant = qa.ProductQuantizer(dim, D.Dot, int(kind[2:]), cen)
        return qa.EncodedVectorsPQ(quant.encode(raw), quant)
    dist, bits = {"tq4_dot": (D.Dot, 0), "tq2_dot": (D.Dot, 1), "tq1_dot": (D.Dot, 3), "tq4_manhattan": (D.Manhattan, 0)}[kind]
    quant = qa.TurboQuantizer(dim, dist, bits)
    return qa.EncodedVectorsTQ(quant.encode(raw), quant)


WALK_CASES = [
    # name, storage kind, dim, m of the graph, ef, options, how
    ("f32_d33_ef64", "f32_dot", 33, 16, 64, {}, "search"),
    ("f16_d40_ef64", "f16_dot", 40, 16, 64, {}, "search"),
    ("u8_d96_ef64", "u8_cosine", 96, 16, 64, {}, "search"),
    ("sq_d48_ef64_aux_links", "sq_euclid", 48, 16, 64, {}, "search"),          # the packed level 0 with the rows' offsets beside the links
    ("bq_d64_ef64", "bq", 64, 16, 64, {}, "search"),
    ("tq4_d64_ef64", "tq4_dot", 64, 16, 64, {}, "search"),
    ("tq2_d64_ef64", "tq2_dot", 64, 16, 64, {}, "search"),
    ("tq1_d64_ef64", "tq1_dot", 64, 16, 64, {}, "search"),
    ("tq4_manhattan_d48_ef64", "tq4_manhattan", 48, 16, 64, {}, "search"),
    ("pq_d64_staged_lut", "pq4", 64, 16, 64, {}, "search"),                       # 16 KiB of LUT: staged in LDS
    ("pq_d64_global_lut_prefilter", "pq2", 64, 16, 64, {}, "search"),            # 32 KiB: read from global memory, the hop prefilter on ...
    ("pq_d64_global_lut_no_prefilter", "pq2", 64, 16, 64, {"hnsw_no_pq_prefilter": 1}, "search"),      # ... and off
    ("pq_d64_lut_free", "pq4", 64, 16, 64, {"hnsw_pq_direct_walk": 1}, "search"),
    ("f32_d33_ef200", "f32_dot", 33, 16, 200, {}, "search"),                      # the 512-entry register beam
    ("f32_d33_ef600", "f32_dot", 33, 16, 600, {}, "search"),                      # the LDS beam
    ("sq_d48_ef600", "sq_euclid", 48, 16, 600, {}, "search"),
    ("f32_d33_m48_long_lists", "f32_dot", 33, 48, 64, {}, "search"),              # level-0 lists of up to 96 links: CSR, two lane passes
    ("bq_d64_traced", "bq", 64, 16, 64, {}, "traced"),
    ("pq_d64_global_lut_traced", "pq2", 64, 16, 64, {}, "traced"),
    ("sq_d48_reference_heaps", "sq_euclid", 48, 16, 64, {"hnsw_reference_heap_order": 1}, "traced"),
    ("bq_d64_reference_heaps_ef200", "bq", 64, 16, 200, {"hnsw_reference_heap_order": 1}, "traced"),
    ("f32_d33_whole_bitmap_clear", "f32_dot", 33, 16, 64, {"hnsw_log_cap": 1, "hnsw_no_lds_visited": 1}, "search"),
    ("f32_d33_log_cap_1", "f32_dot", 33, 16, 64, {"hnsw_log_cap": 1}, "search"),
    ("bq_d64_no_lds_visited", "bq", 64, 16, 64, {"hnsw_no_lds_visited": 1}, "search"),
    ("f32_d33_acorn_m16", "f32_dot", 33, 16, 64, {}, "acorn"),
    ("sq_d48_acorn_m16", "sq_euclid", 48, 16, 64, {}, "acorn"),
    ("f32_d33_acorn_m48_early_flush", "f32_dot", 33, 48, 64, {}, "acorn_big"),
    ("f32_d33_acorn_ef600", "f32_dot", 33, 16, 600, {}, "acorn"),
    ("f32_d33_per_request_filters", "f32_dot", 33, 16, 64, {}, "filters"),
    ("sq_d48_per_request_filters", "sq_euclid", 48, 16, 64, {}, "filters"),
    ("f32_d33_extra_entry_point", "f32_dot", 33, 16, 64, {}, "extra_ep"),
]


@pytest.mark.parametrize("name,kind,dim,m,ef,options,how", WALK_CASES, ids=[c[0] for c in WALK_CASES])
def test_walk_digest(qa, name, kind, dim, m, ef, options, how):
    n = N_BIG if how == "acorn_big" else N
    plain = _two_class_plain(n) if how == "acorn_big" else _plain(n, m)
    if m == 48:      # lists past one 64-lane pass (and past the 63 links a packed level-0 row holds): the CSR arrays, two passes
        assert int(np.max(np.diff(np.asarray(plain.offsets, dtype=np.int64)[:n + 1]))) > 64
    st = _storage(qa, kind, dim, n=n)
    if how == "extra_ep":           # every entry point is deleted: the live extra entry point of the highest level, the last of them
        plain = _with(plain, xp_ids=np.array([5, 9, 1500], dtype=np.uint32), xp_levels=np.array([0, 0, 0], dtype=np.uint32))
        assert not np.isin([5, 9, 1500], plain.ep_ids).any()
    st.set_deleted(point_deleted=_deleted(plain, n, all_entry_points=how == "extra_ep"))
    graph = qa.GraphLayers.from_plain(plain)
    scorer = qa.new_raw_scorer(_queries(dim), st)
    rng = np.random.default_rng(11)
    if how == "acorn":
        scorer.set_filter(rng.random(N) < 0.3)
    if how == "acorn_big":
        # the entry point of every search is point 9 (point 5 is deleted): what its 96 links link to is what its expansion collects, less the deleted
        assert len(np.unique(plain.neighbors.reshape(n, 96)[plain.neighbors.reshape(n, 96)[9]])) > 6000 > 4160
        scorer.set_filter(np.arange(n) % 8 != 0)
    if how == "filters":
        masks = np.stack([rng.random(N) < p for p in (0.7, 0.4, 0.9)])
        scorer.set_filters(masks, [None if i % 4 == 3 else i % 4 for i in range(scorer.nq)])
    d = _Digest()
    for opt, v in options.items():
        qa.set_option(opt, v)
    try:
        if how == "traced":
            res, pops = graph.search_traced(TOP, ef, scorer)
            d.lists(res)
            d.lists(pops)
        else:
            res, scored = graph.search(TOP, ef, scorer, with_scored=True, acorn=how in ("acorn", "acorn_big"))
            d.lists(res)
            d.number(scored)
            d.number(graph.counters.prefilter_candidates)
            d.number(graph.counters.verified_rows)
    finally:
        for opt in options:
            qa.set_option(opt, -1)
    assert any(len(r) for r in res)
    _check(name, d, qa._ffi.last_kernel(scorer._h))


@pytest.mark.parametrize("ef", [64, 200])
def test_search_with_vectors_digest(qa, ef):
    """Steered by binary codes, whose scores tie by the dozen: the stack of evicted candidates that tie with the bound."""
    plain = _plain(N, 16)
    links, base = _storage(qa, "bq", 64), _storage(qa, "f32_dot", 64)
    for st in (links, base):
        st.set_deleted(point_deleted=_deleted(plain))
    graph = qa.GraphLayers.from_plain(plain)
    links_scorer, base_scorer = qa.new_raw_scorer(_queries(64), links), qa.new_raw_scorer(_queries(64), base)
    res, scored = graph.search_with_vectors(TOP, ef, links_scorer, base_scorer, with_scored=True)
    d = _Digest()
    d.lists(res)
    d.number(scored)
    _check("with_vectors_bq_d64_ef%d" % ef, d, qa._ffi.last_kernel(links_scorer._h))


def test_one_point_digest(qa):
    rows = _rows(1, 33, seed=5)
    plain = O.Hnsw(O.DenseStorage(O.F32, O.DOT, rows), m=16, ef_construct=64, seed=7, threads=0).export_plain()
    graph = qa.GraphLayers.from_plain(plain)
    scorer = qa.new_raw_scorer(_queries(33), qa.VectorStorage(rows, qa.Distance.Dot))
    d = _Digest()
    for ef in (64, 600):
        res, scored = graph.search(TOP, ef, scorer, with_scored=True)
        assert all(len(r) == 1 for r in res)
        d.lists(res)
        d.number(scored)
    _check("one_point", d, qa._ffi.last_kernel(scorer._h))


def _custom_queries(qa, dim, multi):
    rng = np.random.default_rng(23)

    def V(k):
        if multi:
            return [rng.standard_normal((int(rng.integers(1, 5)), dim)).astype(np.float32) * 2.0 for _ in range(k)]
        return [rng.standard_normal(dim).astype(np.float32) * 2.0 for _ in range(k)]
    out = []
    for _ in range(NQ // 4):
        out += [qa.CustomQuery.recommend_best_score(V(3), V(2)), qa.CustomQuery.recommend_sum_scores(V(2), V(1)),
                qa.CustomQuery.discover(V(1)[0], [tuple(V(2)) for _ in range(2)]),
                qa.CustomQuery.feedback_naive(V(1)[0], list(zip(V(3), [0.9, 0.2, 0.6])), a=0.7, b=1.2, c=0.5)]
    if multi:
        for q in out:
            q.examples = [np.atleast_2d(e) for e in q.examples]
    return out * REPEAT


@pytest.mark.parametrize("kind,dim,ef", [("f32_dot", 33, 64), ("sq_euclid", 48, 64), ("pq2", 64, 64), ("tq4_manhattan", 48, 64), ("f32_dot", 33, 600)])
def test_custom_walk_digest(qa, kind, dim, ef):
    plain = _plain(N, 16)
    st = _storage(qa, kind, dim)
    st.set_deleted(point_deleted=_deleted(plain))
    graph = qa.GraphLayers.from_plain(plain)
    scorer = qa.CustomRawScorer(_custom_queries(qa, dim, False), st)
    res, scored = scorer.search_hnsw(graph, TOP, ef, with_scored=True)
    d = _Digest()
    d.lists(res)
    d.number(scored)
    _check("custom_%s_d%d_ef%d" % (kind, dim, ef), d, qa._ffi.last_kernel(scorer.examples._h))


def _catch_scorer(st):
    """A multi-vector storage makes the scorer of a search inside the call: keep it, for the name of the kernel it launched."""
    made, make = [], st._queries

    def keeping(queries):
        made.append(make(queries))
        return made[-1]
    st._queries = keeping
    return made


def _multi_storage(qa, kind, dim, n_points):
    """-> (storage of n_points points of 1 to 4 inner rows, the graph of the oracle over every point's first inner row)."""
    rng = np.random.default_rng(9)
    offsets = np.zeros(n_points + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(rng.integers(1, 5, n_points))
    inner = _rows(int(offsets[-1]), dim, seed=3)
    first = np.ascontiguousarray(inner[offsets[:-1].astype(np.int64)])
    plain = O.Hnsw(O.DenseStorage(O.F32, O.DOT, first), m=16, ef_construct=64, seed=7, threads=0).export_plain()
    if kind == "f32_dot":
        st = qa.MultiDenseVectorStorage(inner, offsets, qa.Distance.Dot)
    else:
        st = qa.QuantizedMultivectorStorage(_storage(qa, kind, dim, rows=inner), offsets)
    st.set_deleted(_deleted(plain, n_points))
    return st, plain


@pytest.mark.parametrize("kind,dim,ef", [("f32_dot", 33, 64), ("sq_euclid", 48, 64), ("pq4", 64, 64), ("f32_dot", 33, 200)])
def test_maxsim_walk_digest(qa, kind, dim, ef):
    st, plain = _multi_storage(qa, kind, dim, 800)
    graph = qa.GraphLayers.from_plain(plain)
    rng = np.random.default_rng(29)
    queries = [rng.standard_normal((int(rng.integers(1, 6)), dim)).astype(np.float32) * 2.0 for _ in range(NQ)] * REPEAT
    made = _catch_scorer(st)
    res, ctr = st.search_hnsw(graph, queries, TOP, ef, with_counters=True)
    d = _Digest()
    d.lists(res)
    d.number(ctr.vectors_scored)
    _check("maxsim_%s_d%d_ef%d" % (kind, dim, ef), d, qa._ffi.last_kernel(made[-1][0]._h))


@pytest.mark.parametrize("kind,dim", [("f32_dot", 33), ("sq_euclid", 48)])
def test_multivector_custom_walk_digest(qa, kind, dim):
    st, plain = _multi_storage(qa, kind, dim, 800)
    graph = qa.GraphLayers.from_plain(plain)
    made = _catch_scorer(st)
    res, ctr = st.custom_search_hnsw(graph, _custom_queries(qa, dim, True), TOP, 64, with_counters=True)
    d = _Digest()
    d.lists(res)
    d.number(ctr.vectors_scored)
    _check("custom_multi_%s_d%d" % (kind, dim), d, qa._ffi.last_kernel(made[-1][0]._h))
