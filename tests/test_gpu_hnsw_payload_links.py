"""Payload-block sub-graphs merged into the graph (`qmx_hnsw_build_payload_links`, hnsw_build_payload.hpp) against the Python model of the reference's
flat additional graphs and `merge_from_other` (payload_links_reference.py), and the walks of the merged graph against the model walk with the per-hop limit and, like for like, the CPU oracle's."""
import numpy as np
import pytest

import oracle_ffi as O
import payload_links_reference as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


def _dist(qa, d):
    return {O.COSINE: qa.Distance.Cosine, O.DOT: qa.Distance.Dot, O.EUCLID: qa.Distance.Euclid}[d]


def _clustered(n, dim, seed, k=64):
    """The generator of test_gpu_hnsw_build.py: a mixture of gaussians, no tied scores."""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((k, dim)).astype(np.float32) * 2.0
    return (centers[rng.integers(0, k, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.6).astype(np.float32)


def _tenant_of(n, tenants):
    return ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(tenants)


def _rows0(plain, n):
    off = plain.offsets[:n + 1].astype(np.int64)
    return [plain.neighbors[off[i]:off[i + 1]].tolist() for i in range(n)]


def _recall(got, want):
    return sum(len(set(g["idx"].tolist()) & set(w["idx"].tolist())) for g, w in zip(got, want)) / float(max(1, sum(len(w) for w in want)))


class _Setup:
    """Rows, their device storage and the pairwise score of stored rows as the build sees it, f32 or SQ."""

    def __init__(self, qa, kind, distance, n, dim, seed, deleted=None, k=32):
        self.n, self.distance = n, distance
        self.rows = O.preprocess(distance, _clustered(n, dim, seed, k=k))
        self.ost = O.DenseStorage(O.F32, distance, self.rows, point_deleted=deleted)
        self.vs = qa.VectorStorage(self.rows, _dist(qa, distance))
        self.storage, self.osq = self.vs, None
        if kind == "sq":
            self.quant = qa.ScalarQuantizer.from_min_max(self.rows, dim, _dist(qa, distance))
            self.osq = O.SqOracle(distance, dim, self.quant.alpha, self.quant.offset)
            self.osq.encode_rows(self.rows)
            self.storage = qa.EncodedVectorsU8(self.quant.encode(self.rows), self.quant)
        if deleted is not None:
            self.storage.set_deleted(point_deleted=deleted)

    def table(self, ids):
        ids = np.asarray(ids, dtype=np.uint32)
        if self.osq is None:
            return self.ost.score_points(self.rows[ids], ids, encoded=True)
        a, b = np.repeat(ids, len(ids)), np.tile(ids, len(ids))
        return self.osq.score_internal(a, b).reshape(len(ids), len(ids))


def _case_blocks(n, deleted_point):
    """150 points, 65 points (one past a wave) and 2 points, none in id order; one point sits in two blocks, one deleted point inside the first."""
    rng = np.random.default_rng(5)
    perm = rng.permutation(n)
    perm = perm[perm != deleted_point]
    a = perm[:149].tolist()
    a.insert(40, deleted_point)
    b = perm[149:213].tolist() + [a[10]]
    c = perm[213:215].tolist()
    return [np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32), np.array(c, dtype=np.uint32)]


@pytest.mark.parametrize("kind,distance,efc", [("f32", O.DOT, 16), ("f32", O.EUCLID, 16), ("sq", O.DOT, 16), ("sq", O.EUCLID, 16), ("f32", O.DOT, 600)])
def test_one_point_per_launch_builds_the_models_graphs_link_for_link(qa, kind, distance, efc):
    """max_batch = 1: every block graph is the model's sequential flat graph, and the merged rows and entry points are the model's merge_from_other over
    a main graph built with m = 4.  efc = 600: the insertion beam in LDS (above the register beam of 512)."""
    n, dim, pm0, dead = 600, 24, 8, 77
    deleted = np.zeros(n, dtype=bool)
    deleted[dead] = True
    s = _Setup(qa, kind, distance, n, dim, 11, deleted)
    blocks = _case_blocks(n, dead)
    assert dead in blocks[0] and len(blocks[1]) == 65 and len(blocks[2]) == 2 and set(blocks[0]) & set(blocks[1])
    live = [b[~deleted[b]] for b in blocks]
    model_rows = [M.build_flat_graph(s.table(ids), pm0, efc) for ids in live]
    for ids, rows in zip(live, model_rows):
        g = qa.GraphLayers.build_payload_links(s.storage, [ids], payload_m0=pm0, ef_construct=efc, max_batch=1)
        p = g.export_plain()
        assert (p.m, p.m0) == (0, pm0) and len(p.level_offsets) == 2
        got = _rows0(p, n)
        for pos, row in enumerate(rows):
            assert got[ids[pos]] == [int(ids[x]) for x in row], (pos, got[ids[pos]], row)
        assert sum(len(r) for r in got) == sum(len(r) for r in rows)          # nothing outside the block
        assert p.ep_ids.tolist() == [int(ids[0])] and p.ep_levels.tolist() == [0] and len(p.xp_ids) == 0
        assert g.payload_info.blocks_built == 1 and g.payload_info.links_added == sum(len(r) for r in rows)
    main = qa.GraphLayers.build(s.storage, m=4, ef_construct=32, seed=1, max_batch=1)
    mp = main.export_plain()
    model = M.Graph.from_plain(mp, n)
    for ids, rows in zip(live, model_rows):
        model.merge_from_other(M.block_graph(n, ids, rows))
    merged = qa.GraphLayers.build_payload_links(s.storage, blocks, payload_m0=pm0, ef_construct=efc, max_batch=1, main=main)
    p = merged.export_plain()
    assert (p.m, p.m0) == (mp.m, mp.m0)
    assert np.array_equal(p.reindex, mp.reindex) and np.array_equal(p.level_offsets, mp.level_offsets)
    assert _rows0(p, n) == [model.links[i][0] for i in range(n)]
    got = M.Graph.from_plain(p, n)
    assert [l[1:] for l in got.links] == [l[1:] for l in M.Graph.from_plain(mp, n).links]          # levels >= 1 are the main graph's
    assert got.entry_points == model.entry_points and got.extra_entry_points == model.extra_entry_points
    assert got.entry_points[1:] == [(int(ids[0]), 0) for ids in live]
    assert np.array_equal(main.export_plain().neighbors, mp.neighbors)          # the main graph is untouched
    both = int(blocks[0][10])
    assert len(model.links[both][0]) > len(mp.neighbors[int(mp.offsets[both]):int(mp.offsets[both + 1])])
    assert merged.payload_info.longest_row == max(len(l[0]) for l in model.links)


def test_edges_and_argument_errors(qa):
    n, dim, pm0 = 300, 24, 8
    deleted = np.zeros(n, dtype=bool)
    deleted[[20, 21, 22]] = True
    s = _Setup(qa, "f32", O.COSINE, n, dim, 3, deleted)
    main = qa.GraphLayers.build(s.storage, m=4, ef_construct=32, seed=2)
    mp = main.export_plain()
    build = qa.GraphLayers.build_payload_links
    # no block: the main graph's arrays
    p = build(s.storage, [], payload_m0=pm0, ef_construct=16, main=main).export_plain()
    for f in ("reindex", "level_offsets", "offsets", "neighbors", "ep_ids", "ep_levels", "xp_ids", "xp_levels"):
        assert np.array_equal(getattr(p, f), getattr(mp, f)), f
    p = build(s.storage, (np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32)), payload_m0=pm0, ef_construct=16).export_plain()
    assert len(p.neighbors) == 0 and len(p.ep_ids) == 0 and p.offsets.tolist() == [0] * (n + 1)
    # an empty block, a one-point block, an all-deleted block, then a block of three
    g = build(s.storage, [[], [5], [20, 21, 22], [7, 8, 21, 9]], payload_m0=pm0, ef_construct=16, main=main)
    p = g.export_plain()
    assert p.ep_ids.tolist() == mp.ep_ids.tolist() + [5, 7] and p.ep_levels.tolist() == mp.ep_levels.tolist() + [0, 0]
    assert g.payload_info.blocks_built == 2
    base, got = _rows0(mp, n), _rows0(p, n)
    for i in range(n):
        if i in (7, 8, 9):
            assert got[i][:len(base[i])] == base[i] and set(got[i]) - set(base[i]) <= {7, 8, 9} - {i}
            assert set(got[i]) & ({7, 8, 9} - {i}) or set(base[i]) & ({7, 8, 9} - {i})          # no point of the block is left without a link into it
        else:
            assert got[i] == base[i]
    # main_graph = NULL works and is searchable at once
    flat = build(s.storage, [np.arange(100, 200)], payload_m0=pm0, ef_construct=16)
    allowed = np.zeros(n, dtype=bool)
    allowed[100:200] = True
    scorer = qa.new_raw_scorer(s.rows[150:153], s.vs)
    scorer.set_filter(allowed)
    res = flat.search(5, 32, scorer)
    assert all(len(r) == 5 and allowed[r["idx"]].all() for r in res)          # the walk starts at the block's entry point and stays inside the block
    scorer.set_filter(~allowed)
    assert all(len(r) == 0 for r in flat.search(5, 32, scorer))               # no entry point passes: nothing to walk
    # argument errors: the status, and no graph
    E = qa._ffi
    bad = [([[1, 2, n]], dict(), E.ERR_BAD_ARG), ([[1, 2, 1]], dict(), E.ERR_BAD_ARG), ([[1, 2]], dict(payload_m0=0), E.ERR_BAD_ARG),
           ([[1, 2]], dict(payload_m0=129), E.ERR_BAD_ARG), ([[1, 2]], dict(ef_construct=0), E.ERR_BAD_ARG), ([[1, 2]], dict(ef_construct=4097), E.ERR_BAD_ARG),
           ((np.array([1, 2], dtype=np.uint64), np.array([1, 2], dtype=np.uint32)), dict(), E.ERR_BAD_ARG),
           ((np.array([0, 2, 1], dtype=np.uint64), np.array([1, 2], dtype=np.uint32)), dict(), E.ERR_BAD_ARG)]
    for blocks, kw, status in bad:
        args = dict(payload_m0=pm0, ef_construct=16)
        args.update(kw)
        with pytest.raises(qa.QmxError) as e:
            build(s.storage, blocks, **args)
        assert e.value.status == status, (blocks, kw)
    assert build(s.storage, [[1, 2], [2, 1]], payload_m0=pm0, ef_construct=16).payload_info.blocks_built == 2      # the same point in DIFFERENT blocks is fine
    # *out stays NULL on an error; a main graph without its host arrays is refused
    import ctypes as C
    b = E.HnswPayloadBlocks()
    off, pts = np.array([0, 2], dtype=np.uint64), np.array([1, n], dtype=np.uint32)
    b.offsets, b.points, b.n_blocks, b.payload_m0, b.ef_construct = E.ptr(off).value, E.ptr(pts).value, 1, pm0, 16
    out = C.c_void_p(1234)
    assert E.lib().qmx_hnsw_build_payload_links(s.storage._h, None, None, C.byref(b), C.byref(out), None) == E.ERR_BAD_ARG and not out.value
    loaded = qa.GraphLayers.from_plain(mp)
    with pytest.raises(qa.QmxError) as e:
        build(s.storage, [[1, 2]], payload_m0=pm0, ef_construct=16, main=loaded)
    assert e.value.status == E.ERR_NOT_SUPPORTED
    # a product-quantized segment needs the original vectors; a sparse segment is not served; the lists are host arrays
    cen = O.PqOracle.train(s.rows, dim, 4, 16, iters=1)
    codes = O.PqOracle(O.COSINE, dim, 4, cen).encode(s.rows)
    pq = qa.EncodedVectorsPQ(codes, qa.ProductQuantizer(dim, qa.Distance.Cosine, 4, cen))
    with pytest.raises(qa.QmxError) as e:
        build(pq, [[1, 2]], payload_m0=pm0, ef_construct=16)
    assert e.value.status == E.ERR_NOT_SUPPORTED
    sparse = qa.SparseVectorStorage([([1, 2], [1.0, 2.0]), ([2, 3], [1.0, 1.0]), ([1], [3.0])])
    out = C.c_void_p(1234)
    b.points = E.ptr(np.array([0, 1], dtype=np.uint32)).value
    keep = np.array([0, 1], dtype=np.uint32)
    b.points = E.ptr(keep).value
    assert E.lib().qmx_hnsw_build_payload_links(sparse._h, None, None, C.byref(b), C.byref(out), None) == E.ERR_NOT_SUPPORTED and not out.value
    import torch
    d_off, d_pts = torch.tensor([0, 2], dtype=torch.int64, device="cuda"), torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    for o_, p_ in ((E.ptr(d_off), E.ptr(keep)), (E.ptr(off), E.ptr(d_pts))):
        b.offsets, b.points = (o_.value if hasattr(o_, "value") else o_), (p_.value if hasattr(p_, "value") else p_)
        out = C.c_void_p(1234)
        assert E.lib().qmx_hnsw_build_payload_links(s.storage._h, None, None, C.byref(b), C.byref(out), None) == E.ERR_BAD_ARG and not out.value
    # the exported m = 0 graph loads again through qmx_hnsw_create and walks the same
    fp = flat.export_plain()
    assert (fp.m, fp.m0) == (0, pm0)
    again = qa.GraphLayers.from_plain(fp)
    scorer.set_filter(allowed)
    for a_, b_ in zip(flat.search(5, 32, scorer), again.search(5, 32, scorer)):
        assert a_["idx"].tolist() == b_["idx"].tolist()


@pytest.mark.parametrize("kind", ["pq", "tq4", "tq1"])
def test_pq_and_turboquant_segments_build_through_the_original_vectors(qa, kind):
    """PQ / TurboQuant segments: the insertion searches of a block graph score through the query of the point's ORIGINAL vector (the round's items are
    gathered by id), the heuristic and the back links through score_internal - as qmx_hnsw_build_quantized.  Bars, those of the existing PQ / TQ build
    tests: the invariants, and the filtered recall of the graph walked by the quantized scorer within 0.05 of the graph built over the f32 rows and
    walked by the same scorer."""
    n, dim, tenants, pm0, efc, top, ef = 4096, 64, 8, 16, 64, 10, 64
    rows = O.preprocess(O.DOT, _clustered(n, dim, 41, k=48))
    vs = qa.VectorStorage(rows, qa.Distance.Dot)
    if kind == "pq":
        cen = O.PqOracle.train(rows[:2000], dim, 4, 256, iters=4)
        enc = qa.EncodedVectorsPQ(O.PqOracle(O.DOT, dim, 4, cen).encode(rows), qa.ProductQuantizer(dim, qa.Distance.Dot, 4, cen))
    else:
        bits = O.TQ_BITS4 if kind == "tq4" else O.TQ_BITS1
        enc = qa.EncodedVectorsTQ(O.TqOracle(O.DOT, dim, bits).encode_rows(rows), qa.TurboQuantizer(dim, qa.Distance.Dot, bits))
    tenant = _tenant_of(n, tenants)
    blocks = [np.flatnonzero(tenant == t).astype(np.uint32)[::-1].copy() for t in range(tenants)]          # (descending ids: gathered, not a range)
    with pytest.raises(qa.QmxError) as e:
        qa.GraphLayers.build_payload_links(enc, blocks, payload_m0=pm0, ef_construct=efc)
    assert e.value.status == qa._ffi.ERR_NOT_SUPPORTED
    g_q = qa.GraphLayers.build_payload_links(enc, blocks, payload_m0=pm0, ef_construct=efc, original=vs)
    g_f = qa.GraphLayers.build_payload_links(vs, blocks, payload_m0=pm0, ef_construct=efc)
    p = g_q.export_plain()
    for i, row in enumerate(_rows0(p, n)):
        assert 1 <= len(row) <= pm0 and len(set(row)) == len(row) and i not in row and all(tenant[x] == tenant[i] for x in row)
    assert p.ep_ids.tolist() == [int(b[0]) for b in blocks]
    nq = 64
    queries = _clustered(nq, dim, 42, k=48)
    q_tenant = np.arange(nq) % tenants
    masks = np.stack([tenant == t for t in range(tenants)])
    exact = [O.DenseStorage(O.F32, O.DOT, rows, point_deleted=~masks[q_tenant[qi]]).peek_top(queries[qi:qi + 1], top)[0] for qi in range(nq)]
    scorer = qa.new_raw_scorer(queries, enc)
    scorer.set_filters(masks, q_tenant.astype(np.uint32))
    r_q, r_f = _recall(g_q.search(top, ef, scorer), exact), _recall(g_f.search(top, ef, scorer), exact)
    print("%s: filtered recall@10 through the quantized scorer, graph built through it %.3f, graph built over the f32 rows %.3f" % (kind, r_q, r_f))
    assert r_q > r_f - 0.05, (r_q, r_f)


def test_concurrent_blocks_invariants_and_launch_count(qa):
    """40 blocks of about 300 points by a hash, the default batches: one launch pair inserts the next batch of EVERY block."""
    n, dim, tenants, pm0, efc = 12000, 24, 40, 16, 48
    s = _Setup(qa, "f32", O.DOT, n, dim, 19, k=64)
    tenant = _tenant_of(n, tenants)
    blocks = [np.flatnonzero(tenant == t).astype(np.uint32) for t in range(tenants)]
    main = qa.GraphLayers.build(s.storage, m=8, ef_construct=48, seed=4)
    mp = main.export_plain()
    merged = qa.GraphLayers.build_payload_links(s.storage, blocks, payload_m0=pm0, ef_construct=efc, main=main)
    flat = qa.GraphLayers.build_payload_links(s.storage, blocks, payload_m0=pm0, ef_construct=efc)
    base, got, own = _rows0(mp, n), _rows0(merged.export_plain(), n), _rows0(flat.export_plain(), n)
    for i in range(n):
        row = own[i]
        assert len(row) <= pm0 and len(set(row)) == len(row) and i not in row
        assert all(tenant[x] == tenant[i] for x in row)                      # block links stay inside the block
        assert len(row) >= 1
        assert got[i][:len(base[i])] == base[i] and len(set(got[i])) == len(got[i])
        assert len(got[i]) <= len(base[i]) + pm0 * 1                         # main + payload_m0 x memberships (one field: one membership)
        added = got[i][len(base[i]):]          # (two concurrent builds need not agree link for link: the merged graph is held to the same invariants)
        assert all(tenant[x] == tenant[i] for x in added) and i not in added and not set(added) & set(base[i])
        assert len(added) + sum(1 for x in base[i] if tenant[x] == tenant[i]) >= 1
    p = merged.export_plain()
    assert p.ep_ids.tolist() == mp.ep_ids.tolist() + [int(b[0]) for b in blocks] and p.ep_levels.tolist()[len(mp.ep_ids):] == [0] * tenants
    assert np.array_equal(p.xp_ids, mp.xp_ids)
    # Block concurrency, derived: the batches of a block depend on its size alone (<= max(1, inserted / 32) per round), and a round takes the next batch of
    # every block - so all the blocks need exactly the rounds of the largest one built alone, two launches each: the constant is 0
    largest = max(blocks, key=len)
    alone = qa.GraphLayers.build_payload_links(s.storage, [largest], payload_m0=pm0, ef_construct=efc)
    assert merged.payload_info.launches <= alone.payload_info.launches + 0
    assert alone.payload_info.launches > 40 and merged.payload_info.blocks_built == tenants


def _oracle_walk(plain, n, m0, s, queries, top, ef, allowed, acorn):
    """The oracle's walk of exported arrays.  The oracle's import cuts every row to m0 links, so it is given the arrays under an m0 that holds the
    longest row (the device graph beside it is created from the same arrays with the same m0: the comparison is like for like)."""
    w = O.PlainLinks(plain.m, m0, plain.reindex, plain.level_offsets, plain.offsets, plain.neighbors, plain.ep_ids, plain.ep_levels, plain.xp_ids, plain.xp_levels)
    g = O.Hnsw.from_plain(w, n)
    g.algorithm = 1 if acorn else 0
    ost = O.DenseStorage(O.F32, s.distance, s.rows, point_deleted=None if allowed is None else ~allowed)
    if s.osq is None:
        return g.search_dense(ost, queries, top, ef)
    return g.search_sq(ost, s.osq, O.preprocess(s.distance, queries), top, ef)


@pytest.mark.parametrize("kind", ["f32", "sq"])
def test_long_rows_walk_like_the_oracle(qa, kind):
    """m0 = 32, payload_m0 = 32, two fields: rows pass 63 links (no packed level 0) and 2 m0 (the SQ offset table is not made).  The device walks of the
    merged graph - plain and ACORN, filtered and not - are the oracle's walks of the exported arrays, ids and score bits."""
    n, dim, top, ef = 3000, 24, 10, 48
    s = _Setup(qa, kind, O.DOT, n, dim, 23, k=16)
    t1, t2 = _tenant_of(n, 6), (np.arange(n) // 7) % 5
    blocks = [np.flatnonzero(t1 == t).astype(np.uint32) for t in range(6)] + [np.flatnonzero(t2 == t).astype(np.uint32) for t in range(5)]
    main = qa.GraphLayers.build(s.storage, m=16, m0=32, ef_construct=64, seed=6)
    merged = qa.GraphLayers.build_payload_links(s.storage, blocks, payload_m0=32, ef_construct=64, main=main)
    p = merged.export_plain()
    longest = int(np.diff(p.offsets[:n + 1].astype(np.int64)).max())
    assert longest > 64 and longest == merged.payload_info.longest_row and p.m0 == 32          # the case is what it says
    queries = _clustered(24, dim, 24, k=16)
    allowed = (t1 == 2)
    # the oracle cannot hold a row longer than its m0: both sides walk the exported arrays under m0 = 128
    wide = qa.GraphLayers(p.m, 128, p.reindex, p.level_offsets, p.offsets, p.neighbors, p.ep_ids, p.ep_levels, p.xp_ids, p.xp_levels)
    for acorn in (False, True):
        for mask in (None, allowed):
            scorer = qa.new_raw_scorer(queries, s.storage)
            if mask is not None:
                scorer.set_filter(mask)
            want = _oracle_walk(p, n, 128, s, queries, top, ef, mask, acorn)
            got = wide.search(top, ef, scorer, acorn=acorn)
            for a, b in zip(got, want):
                assert a["idx"].tolist() == b["idx"].tolist() and np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32)), (acorn, mask is not None)
    # The merged graph itself: m0 = 32 is its per-hop limit and its rows are up to three times as long - the regime this build creates.  The reference there:
    # the Python restatement of search_on_level / search_on_level_acorn with `limit` (payload_links_reference.walk), ids and score bits.
    model = M.Graph.from_plain(p, n)
    if s.osq is None:
        scores = s.ost.score_points(queries, np.arange(n))
    else:
        scores = s.osq.score_points(O.preprocess(s.distance, queries), np.arange(n))
    cut = 0
    for acorn in (False, True):
        for mask in (None, allowed):
            scorer = qa.new_raw_scorer(queries, s.storage)
            if mask is not None:
                scorer.set_filter(mask)
            mine = merged.search(top, ef, scorer, acorn=acorn)
            for qi, a in enumerate(mine):
                ids, sc = M.walk(model, p.m, p.m0, scores[qi], mask, top, ef, acorn=acorn)
                assert a["idx"].tolist() == ids, (kind, acorn, mask is not None, qi)
                assert np.array_equal(a["score"].view(np.uint32), np.array(sc, dtype=np.float32).view(np.uint32)), (kind, acorn, mask is not None, qi)
            # ... and the limit is met: the same walk without it (m0 = 128) gives other lists for some queries
            other = wide.search(top, ef, scorer, acorn=acorn)
            cut += sum(int(a["idx"].tolist() != b["idx"].tolist()) for a, b in zip(mine, other))
    assert cut > 0


@pytest.fixture(scope="module")
def tenants_8k(qa):
    n, dim, tenants = 8192, 32, 16
    s = _Setup(qa, "f32", O.DOT, n, dim, 31, k=64)
    tenant = _tenant_of(n, tenants)
    blocks = [np.flatnonzero(tenant == t).astype(np.uint32) for t in range(tenants)]
    main = qa.GraphLayers.build(s.storage, m=8, ef_construct=64, seed=9)
    merged = qa.GraphLayers.build_payload_links(s.storage, blocks, payload_m=8, ef_construct=64, main=main)
    return s, tenant, blocks, main, merged


def test_payload_links_pay_under_a_tenant_filter(qa, tenants_8k):
    """8 192 points, 16 tenants, main m = 8, payload_m = 8, ef 64, 64 filtered queries: recall@10 against the exact filtered search."""
    s, tenant, blocks, main, merged = tenants_8k
    n, nq, top, ef = s.n, 64, 10, 64
    queries = _clustered(nq, s.rows.shape[1], 32, k=64)
    q_tenant = np.arange(nq) % 16
    masks = np.stack([tenant == t for t in range(16)])
    sequential = qa.GraphLayers.build_payload_links(s.storage, blocks, payload_m=8, ef_construct=64, max_batch=1, main=main)
    flat = qa.GraphLayers.build_payload_links(s.storage, blocks, payload_m=8, ef_construct=64)
    exact, r_alone = [], []
    for qi in range(nq):
        ost = O.DenseStorage(O.F32, O.DOT, s.rows, point_deleted=~masks[q_tenant[qi]])
        exact.append(ost.peek_top(queries[qi:qi + 1], top)[0])

    def filtered(graph):
        scorer = qa.new_raw_scorer(queries, s.storage)
        scorer.set_filters(masks, q_tenant.astype(np.uint32))
        return graph.search(top, ef, scorer)
    r_main, r_merged, r_seq, r_flat = (_recall(filtered(g), exact) for g in (main, merged, sequential, flat))
    # (d): the tenant's rows alone under an ordinary hierarchical graph, searched unfiltered
    alone = []
    for t in range(16):
        ids = blocks[t]
        sub = qa.VectorStorage(s.rows[ids], qa.Distance.Dot)
        g = qa.GraphLayers.build(sub, m=8, m0=16, ef_construct=64, seed=9)
        sel = np.flatnonzero(q_tenant == t)
        for qi, r in zip(sel, g.search(top, ef, qa.new_raw_scorer(queries[sel], sub))):
            alone.append((qi, ids[r["idx"]]))
    r_alone = sum(len(set(ids.tolist()) & set(exact[qi]["idx"].tolist())) for qi, ids in alone) / float(sum(len(e) for e in exact))
    print("recall@10 under a 1/16 tenant filter: main only %.3f, merged %.3f, merged sequential %.3f, m = 0 graph %.3f, stand-alone per-tenant graph %.3f"
          % (r_main, r_merged, r_seq, r_flat, r_alone))
    assert r_merged >= r_seq - 0.03, (r_merged, r_seq)
    assert r_flat >= r_alone - 0.05, (r_flat, r_alone)


def test_128_requests_of_many_tenants_in_one_batch(qa, tenants_8k):
    """qmx_query_set_filters over the merged graph: the lists of a batch of 128 requests, each under its tenant's filter, are those of each request alone."""
    s, tenant, blocks, main, merged = tenants_8k
    nq, top, ef = 128, 10, 64
    queries = _clustered(nq, s.rows.shape[1], 33, k=64)
    q_tenant = (np.arange(nq) * 5) % 16
    masks = np.stack([tenant == t for t in range(16)])
    scorer = qa.new_raw_scorer(queries, s.storage)
    scorer.set_filters(masks, q_tenant.astype(np.uint32))
    batch = merged.search(top, ef, scorer)
    for qi in range(nq):
        one = qa.new_raw_scorer(queries[qi:qi + 1], s.storage)
        one.set_filter(masks[q_tenant[qi]])
        want = merged.search(top, ef, one)[0]
        assert batch[qi]["idx"].tolist() == want["idx"].tolist() and np.array_equal(batch[qi]["score"].view(np.uint32), want["score"].view(np.uint32))
        assert len(want) == top and masks[q_tenant[qi]][want["idx"]].all()
