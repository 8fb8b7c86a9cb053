"""The model of the payload-block sub-graphs (hnsw/build.rs:408-531, build_filtered_graph :631-716) the device build is held against.

The CPU oracle's builder draws its levels from a seed, so it cannot make the FLAT additional graph of a block
(`GraphLayersBuilder::new_with_params(total, payload_m, ef_construct, 1, ..)`: every point on level 0).  This module restates that build in
Python: a sequential `link_new_point` over a level-0-only graph - `search_on_level(ef_construct)` with the point itself excluded by
construction (it is not in the graph yet), the oracle's own `qo_links_heuristic` / `qo_links_connect_heuristic` for the selection - over an
injected table of pairwise scores, plus `merge_from_other` (graph_layers_builder.rs:346-381) and the entry-point merge (entry_points.rs:41-44).

Everything works on POSITIONS within a block (0 .. k); `score[a][b]` is the score of point b for the stored row a as the query.  Among equal
scores the queues prefer the lower position (the device's keys do; the reference's order there is its binary heaps').
"""
import numpy as np

import oracle_ffi as O


def search_on_level(links, entry, score_row, ef):
    """GraphLayersBase::search_on_level (graph_layers.rs:108-149) on one level: `links[c]` the list of c, `score_row[x]` the query's score of x.
    Returns the `nearest` queue, best first, as (position, score) pairs."""
    visited = {entry}
    beam = [[float(score_row[entry]), entry, False]]      # descending (score, then lower position first), at most ef entries

    def offer(s, x):
        if len(beam) >= ef:
            ws, wx = beam[-1][0], beam[-1][1]
            if not (s > ws or (s == ws and x < wx)):
                return
        at = 0
        while at < len(beam) and (beam[at][0] > s or (beam[at][0] == s and beam[at][1] < x)):
            at += 1
        beam.insert(at, [s, x, False])
        del beam[ef:]

    while True:
        cand = next((e for e in beam if not e[2]), None)      # the best candidate not yet expanded; one below a full queue's worst is not in it
        if cand is None:
            break
        cand[2] = True
        for x in links[cand[1]]:
            if x in visited:
                continue
            visited.add(x)
            offer(float(score_row[x]), x)
    return [(e[1], np.float32(e[0])) for e in beam]


def _beam_search(entry, score_row, ef, expand):
    """The loop of search_on_level / search_on_level_acorn: `expand(candidate)` returns the points to score, in order (and does the visited bookkeeping)."""
    beam = [[float(score_row[entry]), entry, False]]

    def offer(s, x):
        if len(beam) >= ef:
            ws, wx = beam[-1][0], beam[-1][1]
            if not (s > ws or (s == ws and x < wx)):
                return
        at = 0
        while at < len(beam) and (beam[at][0] > s or (beam[at][0] == s and beam[at][1] < x)):
            at += 1
        beam.insert(at, [s, x, False])
        del beam[ef:]

    while True:
        cand = next((e for e in beam if not e[2]), None)
        if cand is None:
            break
        cand[2] = True
        for x in expand(cand[1]):
            offer(float(score_row[x]), x)
    return [(e[1], np.float32(e[0])) for e in beam]


def walk(graph, m, m0, score_row, allowed, top, ef, acorn=False):
    """GraphLayers::search (graph_layers.rs:530-562) of one query over a Graph whose rows may be LONGER than m0: `score_row[x]` the query's score of point
    x, `allowed` the filter (None: every point passes).  m / m0 are the reference's per-hop limits (`score_points(ids, limit = get_m(level))`: the
    unvisited links are filtered, then cut to `limit`, point_scorer.rs:265-277), not capacities.  Returns (ids, scores), best first, at most top."""
    def check(x):
        return allowed is None or bool(allowed[x])

    # EntryPoints::get_entry_point (entry_points.rs:96-112)
    entry = next(((i, l) for i, l in graph.entry_points if check(i)), None)
    if entry is None:
        for i, l in graph.extra_entry_points:          # max_by_key(level): the last maximal element wins
            if check(i) and (entry is None or l >= entry[1]):
                entry = (i, l)
    if entry is None:
        return [], []
    cur, top_level = entry
    # search_entry (graph_layers.rs:247-317): greedy on the levels above 0
    for level in range(top_level, 0, -1):
        cur_score, changed = score_row[cur], True
        while changed:
            changed = False
            for x in [y for y in graph.links[cur][level] if check(y)][:m]:
                if score_row[x] > cur_score:
                    cur, cur_score, changed = x, score_row[x], True
    ef = max(ef, top)
    hop1, hop2 = {cur}, set()

    def expand_plain(c):          # search_on_level (graph_layers.rs:108-149)
        kept = [x for x in graph.links[c][0] if x not in hop1 and check(x)][:m0]
        hop1.update(kept)
        return kept

    def expand_acorn(c):          # search_on_level_acorn (graph_layers.rs:154-243)
        to_score, to_explore = [], []
        for x in graph.links[c][0]:
            if x in hop1:
                continue
            hop1.add(x)
            if check(x):
                to_score.append(x)
                if len(to_score) >= m0:
                    break
            else:
                to_explore.append(x)
        for e in to_explore:
            total_limit = len(to_score) + m0
            for x in graph.links[e][0]:
                if x in hop1 or x in hop2:
                    continue
                hop2.add(x)
                if check(x):
                    hop1.add(x)
                    to_score.append(x)
                    if len(to_score) >= total_limit:
                        break
        return to_score
    nearest = _beam_search(cur, score_row, ef, expand_acorn if acorn else expand_plain)[:top]
    return [x for x, _ in nearest], [s for _, s in nearest]


def build_flat_graph(score, m0, ef_construct):
    """The additional graph of one block of k = len(score) live points, inserted in position order: position 0 is the entry point.
    Returns the k link rows (positions)."""
    k = len(score)
    table = np.ascontiguousarray(score, dtype=np.float32)
    links = [[] for _ in range(k)]
    for p in range(1, k):
        nearest = search_on_level(links, 0, table[p], ef_construct)
        cand = np.zeros(len(nearest), dtype=O.ScoredPointOffset)
        cand["idx"] = [x for x, _ in nearest]
        cand["score"] = [s for _, s in nearest]
        sel = O.links_heuristic(cand, m0, table)
        links[p] = list(sel)
        for q in sel:
            if len(links[q]) < m0:
                links[q].append(p)
            else:
                links[q] = O.links_connect_heuristic(links[q], p, q, m0, table)
    return links


class Graph:
    """links[p][level] = the list; entry_points / extra_entry_points = [(id, level)]"""

    def __init__(self, n):
        self.links = [[[]] for _ in range(n)]
        self.entry_points, self.extra_entry_points, self.max_level = [], [], 0

    @classmethod
    def from_plain(cls, p, n):
        g = cls(n)
        L = len(p.level_offsets) - 1
        for i in range(n):
            g.links[i] = []
            for l in range(L):
                if l and int(p.reindex[i]) >= int(p.level_offsets[l + 1] - p.level_offsets[l]):
                    break
                slot = i if l == 0 else int(p.level_offsets[l]) + int(p.reindex[i])
                g.links[i].append(p.neighbors[int(p.offsets[slot]):int(p.offsets[slot + 1])].tolist())
        g.max_level = max(L - 1, 0)
        g.entry_points = list(zip(np.asarray(p.ep_ids).tolist(), np.asarray(p.ep_levels).tolist()))
        g.extra_entry_points = list(zip(np.asarray(p.xp_ids).tolist(), np.asarray(p.xp_levels).tolist()))
        return g

    def merge_from_other(self, other):
        """GraphLayersBuilder::merge_from_other + EntryPoints::merge_from_other."""
        self.max_level = max(self.max_level, other.max_level)
        while len(self.links) < len(other.links):
            self.links.append([])
        for p, layers in enumerate(other.links):
            cur = self.links[p]
            for level, other_links in enumerate(layers):
                if len(cur) <= level:
                    cur.append(list(other_links))
                else:
                    seen = set(cur[level])
                    for x in other_links:
                        if x not in seen:
                            seen.add(x)
                            cur[level].append(x)
        self.entry_points += other.entry_points      # (the extra entry points are not merged)


def block_graph(n, ids, rows):
    """The additional graph of a block as a Graph over all n points: `ids` the block's LIVE points in insertion order, `rows` its link rows in positions."""
    g = Graph(n)
    for pos, row in enumerate(rows):
        g.links[ids[pos]][0] = [int(ids[x]) for x in row]
    if len(ids):
        g.entry_points = [(int(ids[0]), 0)]
    return g


def row0(plain, p):
    return plain.neighbors[int(plain.offsets[p]):int(plain.offsets[p + 1])].tolist()
