"""The model of the payload-block build (payload_links_reference.py) and the block selection (qdrant_amd.hnsw.select_payload_blocks), without a device."""
import numpy as np

import oracle_ffi as O
import payload_links_reference as M


def _clustered(n, dim, seed, k=16):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((k, dim)).astype(np.float32) * 2.0
    return (centers[rng.integers(0, k, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.6).astype(np.float32)


def test_merge_dedups_keeps_order_pushes_missing_levels_and_appends_entry_points():
    """merge_from_other on the reference's own shapes (graph_layers_builder.rs:346-381, entry_points.rs:41-44)."""
    g = M.Graph(4)
    g.links = [[[1, 2], [3]], [[0]], [[0, 3]], [[2], [0]]]
    g.max_level = 1
    g.entry_points, g.extra_entry_points = [(0, 1)], [(3, 1)]
    other = M.Graph(5)                      # one point more than the main graph: its layers are appended
    other.links = [[[2, 3, 1]], [[3, 0]], [[]], [[1], [2], [1]], [[0]]]
    other.max_level = 2
    other.entry_points, other.extra_entry_points = [(1, 0)], [(2, 0)]
    g.merge_from_other(other)
    assert g.links[0] == [[1, 2, 3], [3]]            # 2 and 1 were there: only 3 is appended, the current row stays in front
    assert g.links[1] == [[0, 3]]                    # the other row's order among the new links
    assert g.links[2] == [[0, 3]]                    # an empty other row changes nothing
    assert g.links[3] == [[2, 1], [0, 2], [1]]       # level 1 merged, level 2 was missing: pushed as it is
    assert g.links[4] == [[0]]
    assert g.max_level == 2
    assert g.entry_points == [(0, 1), (1, 0)]        # appended ...
    assert g.extra_entry_points == [(3, 1)]          # ... the extra entry points are not
    # merging the same graph again adds no link
    before = [[list(l) for l in p] for p in g.links]
    g.merge_from_other(other)
    assert g.links == before and g.entry_points == [(0, 1), (1, 0), (1, 0)]


def test_select_payload_blocks_on_both_sides_of_each_threshold():
    from qdrant_amd.hnsw import select_payload_blocks
    total, avg, fst = 10000, 16, 400
    max_block = total // avg * 4            # 2500
    blocks = [np.arange(max_block), np.arange(max_block + 1), np.arange(fst // 4), np.arange(fst // 4 + 1), np.arange(0)]
    assert select_payload_blocks(blocks, total, avg, fst) == [0, 3]
    # integer division first, as the reference: 10000 / 17 = 588 -> 2352
    assert select_payload_blocks([np.arange(2352), np.arange(2353)], total, 17, fst) == [0]
    # no main graph (m = 0): no upper bound
    assert select_payload_blocks(blocks, total, 0, fst) == [0, 1, 3]


def test_flat_build_invariants_on_200_points():
    n, dim, m0, efc = 200, 16, 8, 16
    rows = O.preprocess(O.DOT, _clustered(n, dim, 3))
    st = O.DenseStorage(O.F32, O.DOT, rows)
    score = st.score_points(rows, np.arange(n), encoded=True)
    links = M.build_flat_graph(score, m0, efc)
    assert len(links) == n
    for p, row in enumerate(links):
        assert len(row) <= m0 and len(set(row)) == len(row) and p not in row
        assert all(0 <= x < n for x in row)
    # every point found the graph, and a re-selection keeps its best candidate at least: no row is empty
    assert all(len(links[p]) >= 1 for p in range(n))
    # (links are directed and the heuristic prunes: not every point need be reachable from the entry point, most are)
    seen, todo = {0}, [0]
    while todo:
        for x in links[todo.pop()]:
            if x not in seen:
                seen.add(x)
                todo.append(x)
    assert len(seen) > 0.9 * n
    # search_on_level with a list as long as the graph: what is reachable, in the exact order
    got = M.search_on_level(links, 0, score[7], n)
    order = sorted(seen, key=lambda x: (-float(score[7][x]), x))
    assert [x for x, _ in got] == order
    # the block graph over a larger id space, and its merge into an empty graph
    ids = np.arange(1000, 1000 + n)[::-1]
    g = M.block_graph(1300, ids, links)
    assert g.entry_points == [(int(ids[0]), 0)] and g.links[int(ids[5])][0] == [int(ids[x]) for x in links[5]]
    base = M.Graph(1300)
    base.merge_from_other(g)
    assert base.links[int(ids[5])][0] == g.links[int(ids[5])][0] and base.entry_points == g.entry_points
