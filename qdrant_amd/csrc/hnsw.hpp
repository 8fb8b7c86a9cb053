// hnsw.hpp — device-resident HNSW search: one wavefront walks the graph for one query.
//
// Replaces, for a graph whose links sit in HBM next to the stored block,
//   GraphLayers::search                    lib/segment/src/index/hnsw_index/graph_layers.rs:530-562
//   GraphLayersBase::search_on_level       graph_layers.rs:108-149   (ef-bounded beam, level 0)
//   GraphLayersBase::search_entry_on_level graph_layers.rs:279-317   (greedy descent, levels > 0)
//   GraphLayersBase::search_entry          graph_layers.rs:247-277
//   GraphLayers::get_entry_point           graph_layers.rs:505-528 + entry_points.rs:96-112
//   SearchContext::process_candidate       search_context.rs:32-40
//   FilteredScorer::score_points           point_scorer.rs:265-304   (deleted filter + limit, then score)
//   VisitedListHandle                      index/visited_pool.rs:18-80
// The per-hop `RawScorer::score_points` call of the reference (<= m0 ids per hop) becomes an
// in-kernel gather with the lane policies of the brute-force scan, so a hop never leaves the GPU
// and every score carries the same bits as the scan / the x86 reference.
//
// Mapping
//   * block = 1 wavefront = 1 search at a time; grid = "slots" (CUs x occupancy), each slot loops
//     over queries slot, slot + grid, ...  Many independent searches per CU hide the latency of the
//     dependent loads of a hop (offsets -> links -> visited word -> rows).
//   * the query (tile entry / SQ codes / PQ LUT) is staged in LDS once per search.
//   * `nearest` and `candidates` of SearchContext are ONE sorted register list of 64*E keys
//     (entry e*64+lane) with an "expanded" flag per entry: every candidate the reference can still
//     pop with score >= lower_bound is an element of `nearest` (an evicted candidate is below the
//     bound and ends the loop), so "pop the best candidate" = "best unexpanded entry" and the loop
//     ends when the first ef entries are all expanded.  Identical results whenever scores are
//     distinct; among equal scores the reference's order is BinaryHeap-dependent (unpinned).
//   * visited set = one bit per point in a per-slot HBM bitmap, test-and-set with an L2 atomic;
//     the words a search touched are logged and cleared afterwards (whole-bitmap clear if the
//     log overflows).
//   * links = the plain GraphLinks arrays (graph_links/view.rs: reindex, level_offsets, offsets,
//     neighbors) as serialised by graph_links/serializer.rs:52-176.
//
// Files: hnsw_hop.hpp (the hop scorers and hop_score), hnsw_sets.hpp (beam, visited table, reference heaps), hnsw_layout.hpp (the dynamic LDS of a
// launch), and here the walk: hnsw_search_one, the staging of a search's query entry, the kernel and its launchers.
#pragma once
#include "hnsw_hop.hpp"
#include "hnsw_layout.hpp"
#include "hnsw_sets.hpp"

namespace qmx {

// One search.  `qp` = the query entry (LDS or global).
template <class H, int E>
__device__ __forceinline__ void hnsw_search_one(const ScanArgs &a, const HnswArgs &h, const unsigned char *qp,
                                                uint32_t *hop_ids, float *hop_scores, uint32_t *vis, uint32_t *vlog,
                                                uint32_t qi, int lane, unsigned char *beam_lds = nullptr, uint32_t *vtab = nullptr, const unsigned char *pq8 = nullptr) {
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    uint32_t n_scored = 0;

    // ---- get_entry_point: first live entry point, else the live extra point of the highest level ----
    bool have_ep = false;
    uint32_t ep_id = 0, ep_level = 0;
    for (uint32_t base = 0; base < h.n_ep && !have_ep; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        const bool ok = i < h.n_ep && walk_live<H>(a.del, h.ep_ids[i < h.n_ep ? i : 0], qi);
        const uint64_t m = __ballot(ok);
        if (m) {
            const uint32_t first = base + (uint32_t)__builtin_ctzll(m);
            ep_id = h.ep_ids[first];
            ep_level = h.ep_levels[first];
            have_ep = true;
        }
    }
    if (!have_ep) {
        for (uint32_t i = 0; i < h.n_xp; ++i) {   // max_by_key(level): the last maximal element wins
            const uint32_t id = h.xp_ids[i], lv = h.xp_levels[i];
            if (walk_live<H>(a.del, id, qi) && (!have_ep || lv >= ep_level)) { ep_id = id; ep_level = lv; have_ep = true; }
        }
    }
    if (!have_ep) {
        if (lane == 0) {
            h.out_counts[qi] = 0;
            if (h.out_scored) h.out_scored[qi] = 0;
            if (h.expanded) h.expanded_cnt[qi] = 0;
        }
        return;
    }
    if (ep_level >= h.n_levels) ep_level = h.n_levels - 1;

    // ---- search_entry: greedy descent over levels ep_level .. 1 ----
    uint32_t cur_id = ep_id;
    float cur_score;
    {
        if (lane == 0) hop_ids[0] = cur_id;
        hop_score<H>(a, qp, hop_ids, hop_scores, 1, lane);
        cur_score = hop_scores[0];
        n_scored += 1;
    }
    for (uint32_t level = ep_level; level > 0; --level) {
        if (level != ep_level) n_scored += 1;   // search_entry_on_level re-scores its entry (same value)
        bool changed = true;
        while (changed) {
            changed = false;
            // a node that has no slot on this level (an inconsistent links file: the host validates what it can see) has no links here
            const uint64_t slot = h.level_offsets[level] + h.reindex[cur_id];
            const bool slot_ok = slot < h.level_offsets[level + 1] && slot + 1 < h.n_offsets;
            uint64_t o0 = slot_ok ? h.offsets[slot] : 0, o1 = slot_ok ? h.offsets[slot + 1] : 0;
            if (o1 > h.n_neighbors) o1 = h.n_neighbors;
            if (o0 > o1) o0 = o1;
            uint32_t remaining = h.m;   // filter_truncate limit = level_m
            for (uint64_t base = o0; base < o1 && remaining > 0; base += 64) {
                const uint64_t i = base + (uint64_t)lane;
                const bool on = i < o1;
                const uint32_t id = on ? h.neighbors[i] : 0;
                bool keep = on && id < h.n_points && walk_live<H>(a.del, id, qi);
                const uint64_t mask = __ballot(keep);
                const uint32_t rank = (uint32_t)__popcll(mask & lt_mask);
                keep = keep && rank < remaining;
                uint32_t k = (uint32_t)__popcll(mask);
                if (k > remaining) k = remaining;
                remaining -= k;
                __syncthreads();
                if (keep) hop_ids[rank] = id;
                hop_score<H>(a, qp, hop_ids, hop_scores, k, lane);
                // sequential `if score > current.score` over the batch == first maximum above current
                uint64_t mk = 0;
                if ((uint32_t)lane < k && hop_scores[lane] > cur_score)
                    mk = ((uint64_t)score_to_ord(hop_scores[lane]) << 32) | (uint32_t)(~(uint32_t)lane);
                const uint64_t best = wave_max_u64(mk);
                if (best) {
                    const uint32_t bl = ~(uint32_t)best;
                    cur_id = hop_ids[bl];
                    cur_score = hop_scores[bl];
                    changed = true;
                }
                n_scored += k;
            }
        }
    }

    // ---- search_on_level(level 0, ef) ----
    const uint32_t ef = h.ef > h.top ? h.ef : h.top;
    if constexpr (E == HNSW_E_REF) {
        // ---- option hnsw_reference_heap_order: search_on_level with the reference's own heaps (plain walk only) ----
        __syncthreads();                    // (the previous search of this block is done with the LDS heap)
        RefHeaps rh;
        rh.init(beam_lds, ef, h.ref_cands + (uint64_t)blockIdx.x * h.ref_cap, h.ref_cap, beam_lds + hnsw_beam_lds(ef), HNSW_REF_CAND_LDS);
        uint32_t log_cnt = 0, n_pop = 0;
        const LdsVisited lv{vtab};             // (round 6: the visited set in LDS here too - an exact set either way, hnsw.hpp LdsVisited)
        if (lv.tab) {
            if (lane == 0) { bool in_bm; lv.test_and_set(cur_id, vis, &in_bm); }
        } else {
            if (lane == 0) {
                atomicOr(&vis[cur_id >> 5], 1u << (cur_id & 31));
                vlog[0] = cur_id >> 5;
            }
            log_cnt = 1;
        }
        if (lane == 0) rh.process_candidate(cur_id, cur_score);
        while (true) {
            uint32_t ok = 0, c_idx = 0, c_bits = 0;
            if (lane == 0) {
                uint2 c;
                if (rh.c_pop(&c)) {
                    const float lower_bound = rh.n_len ? RefHeaps::sc(rh.nd[0]) : -3.40282347e+38f;     // ScoreType::min_value()
                    if (!(RefHeaps::sc(c) < lower_bound)) { ok = 1; c_idx = c.x; c_bits = c.y; }
                }
            }
            ok = (uint32_t)__builtin_amdgcn_readfirstlane((int)ok);
            if (!ok) break;
            const uint32_t cand = (uint32_t)__builtin_amdgcn_readfirstlane((int)c_idx);
            if (h.pops) {
                if (lane == 0 && n_pop < h.pop_cap) {
                    qmx_scored_point p;
                    p.idx = cand;
                    p.score = __uint_as_float(c_bits);
                    h.pops[(uint64_t)qi * h.pop_cap + n_pop] = p;
                }
                ++n_pop;
            }
            uint64_t o0 = 0, o1 = 0;
            uint32_t packed_id = 0;
            if (h.l0) {
                const uint32_t *rowp = h.l0 + (uint64_t)cand * h.l0_stride;
                packed_id = (uint32_t)lane + 1 < h.l0_stride ? rowp[lane + 1] : 0;
                o1 = rowp[0];
            } else {
                o0 = h.offsets[cand];
                o1 = h.offsets[(uint64_t)cand + 1];
            }
            uint32_t remaining = h.m0;
            for (uint64_t base = o0; base < o1 && remaining > 0; base += 64) {
                const uint64_t i = base + (uint64_t)lane;
                const bool on = i < o1;
                const uint32_t id = h.l0 ? (on ? packed_id : 0) : (on ? h.neighbors[i] : 0);
                const bool live = on && id < h.n_points && walk_live<H>(a.del, id, qi);
                const uint32_t bit = 1u << (id & 31);
                bool in_bm = true, was_visited = true;
                if (lv.tab) {
                    if (live) was_visited = lv.test_and_set(id, vis, &in_bm);
                } else {
                    const uint32_t old = live ? atomicOr(&vis[id >> 5], bit) : bit;
                    was_visited = (old & bit) != 0;
                }
                bool keep = live && !was_visited;
                const uint64_t mask = __ballot(keep);
                const uint32_t rank = (uint32_t)__popcll(mask & lt_mask);
                uint32_t k = (uint32_t)__popcll(mask);
                if (k > remaining) {
                    if (keep && rank >= remaining) { lv.unset(id, vis, in_bm); keep = false; }
                    k = remaining;
                }
                remaining -= k;
                __syncthreads();
                if (keep) hop_ids[rank] = id;
                {   // the bitmap words this search dirtied (with the LDS table: only the ids of full buckets)
                    const uint64_t bm = __ballot(keep && in_bm);
                    const uint32_t brank = (uint32_t)__popcll(bm & lt_mask);
                    if (keep && in_bm && log_cnt + brank < h.log_cap) vlog[log_cnt + brank] = id >> 5;
                    log_cnt += (uint32_t)__popcll(bm);
                }
                hop_score<H>(a, qp, hop_ids, hop_scores, k, lane);
                {
                    // process_candidate in link order (graph_layers.rs:139-143), by one lane.  A candidate that does not beat the root of a FULL `nearest` at
                    // the start of the hop cannot beat it later in the hop either (the root only rises): push would hand it back (`Some(value)`,
                    // fixed_length_priority_queue.rs:47-59) and nothing changes - those are told apart by all lanes at once, the one lane walks the others
                    const bool full = __builtin_amdgcn_readfirstlane((int)(rh.n_len >= rh.n_cap)) != 0;
                    const uint32_t root_bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)(full ? rh.nd[0].y : 0u));
                    const bool mine = (uint32_t)lane < k;
                    const bool may_enter = mine && (!full || RefHeaps::of_cmp(__uint_as_float(root_bits), hop_scores[mine ? lane : 0]) < 0);
                    uint64_t todo = __ballot(may_enter);
                    if (lane == 0) {
                        while (todo) {
                            const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                            todo &= todo - 1;
                            rh.process_candidate(hop_ids[j], hop_scores[j]);
                        }
                    }
                }
                n_scored += k;
                __syncthreads();
            }
        }
        if (lane == 0) {
            const uint32_t n = rh.n_into_sorted();
            const uint32_t cnt = n < h.top ? n : h.top;
            for (uint32_t i = 0; i < cnt; ++i) {
                qmx_scored_point p;
                p.idx = rh.nd[i].x;
                p.score = RefHeaps::sc(rh.nd[i]);
                h.out[(uint64_t)qi * h.top + i] = p;
            }
            h.out_counts[qi] = cnt;
            if (h.out_scored) h.out_scored[qi] = n_scored;
            if (h.pops) h.pop_cnt[qi] = n_pop;
            if (rh.overflow) *a.err_flag = 2;
        }
        __syncthreads();
        lv.clear(lane);
        if (log_cnt <= h.log_cap) {
            for (uint32_t i = (uint32_t)lane; i < log_cnt; i += 64) vis[vlog[i]] = 0;
        } else {
            for (uint64_t w = (uint64_t)lane; w < h.vis_words; w += 64) vis[w] = 0;
        }
        __threadfence();
        return;
    } else {
    Beam<E> beam;
    if constexpr (E == 0) {
        __syncthreads();                    // (the previous search of this block is done with the LDS list)
        beam.init(beam_lds, ef);
    }
    beam.clear();
    uint32_t log_cnt = 0;
    const LdsVisited lv{h.acorn ? nullptr : vtab};      // (ACORN keeps its two bitmaps)
    {
        if (lv.tab) {
            if (lane == 0) { bool in_bm; lv.test_and_set(cur_id, vis, &in_bm); }       // (an empty table: the entry goes in)
        } else {
            if (lane == 0) {
                atomicOr(&vis[cur_id >> 5], 1u << (cur_id & 31));
                vlog[0] = cur_id >> 5;
            }
            log_cnt = 1;
        }
        beam.insert(make_key(cur_score, cur_id), ef, lane);
    }
    if (h.acorn) {
        // ---- search_on_level_acorn (graph_layers.rs:154-243): links that fail the filters are explored instead of scored ----
        const uint32_t half = (uint32_t)(h.vis_words / 2);           // vis = hop1_visited_list, vis + half = hop2_visited_list
        uint32_t *to_explore = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(hop_ids) + hnsw_hop_lds(h.hop_cap));
        const uint32_t hop_limit = h.m0;                                // hop1_limit = hop2_limit = get_m(0)
        auto mask_le = [](int l) -> uint64_t { return l >= 63 ? ~0ull : ((2ull << l) - 1ull); };
        auto nth_set = [](uint64_t m, uint32_t nth) -> int {            // lane of the nth (1-based) set bit
            for (uint32_t i = 1; i < nth; ++i) m &= m - 1;
            return __builtin_ctzll(m);
        };
        // the links of `node` on level 0, 64 per call: (id, in range)
        auto link_of = [&](uint32_t node, uint64_t base, uint64_t o1, bool *on) -> uint32_t {
            const uint64_t i = base + (uint64_t)lane;
            *on = i < o1;
            if (h.l0) return *on ? h.l0[(uint64_t)node * h.l0_stride + 1 + i] : 0;
            return *on ? h.neighbors[i] : 0;
        };
        auto log_words = [&](bool mine, uint32_t word) {                 // remember the bitmap words this search dirtied
            const uint64_t m = __ballot(mine);
            const uint32_t r = (uint32_t)__popcll(m & lt_mask);
            if (mine && log_cnt + r < h.log_cap) vlog[log_cnt + r] = word;
            log_cnt += (uint32_t)__popcll(m);
        };
        uint32_t n_score = 0;
        // the points collected so far are scored and offered to the beam, in order: once per popped candidate - or earlier, when the next explored node's
        // links might not fit the hop buffer (m0 > 64: up to m0 (m0 + 1) points per candidate; process_candidate touches the beam only, so scoring a
        // prefix early changes nothing)
        auto flush_scores = [&]() {
            hop_score<H>(a, qp, hop_ids, hop_scores, n_score, lane);
            for (uint32_t base = 0; base < n_score; base += 64) {
                const uint32_t j = base + (uint32_t)lane;
                const uint64_t mykey = j < n_score ? make_key(hop_scores[j], hop_ids[j]) : 0;
                uint64_t mm = __ballot(mykey > beam.at(ef - 1));
                while (mm) {
                    const int src = __builtin_ctzll(mm);
                    mm &= mm - 1;
                    const uint64_t nk = readlane_u64(mykey, src);
                    if (nk > beam.at(ef - 1)) beam.insert(nk, ef, lane);
                }
            }
            n_scored += n_score;
            n_score = 0;
            __syncthreads();
        };
        while (true) {
            const uint64_t ck = beam.pop_best(lane);
            if (ck == 0) break;
            const uint32_t cand = key_idx(ck);
            uint32_t n_explore = 0;
            __syncthreads();
            {   // 1-hop neighbours (:196-211): every unvisited link is marked; passing ones are scored (at most hop_limit), the others explored
                uint64_t o0, o1;
                if (h.l0) { o0 = 0; o1 = h.l0[(uint64_t)cand * h.l0_stride]; } else { o0 = h.offsets[cand]; o1 = h.offsets[(uint64_t)cand + 1]; }
                bool broke = false;
                for (uint64_t base = o0; base < o1 && !broke; base += 64) {
                    bool on;
                    const uint32_t id = link_of(cand, base, o1, &on);
                    const bool valid = on && id < h.n_points;
                    const uint32_t bit = 1u << (id & 31);
                    const uint32_t old = valid ? atomicOr(&vis[id >> 5], bit) : bit;      // check_and_update_visited
                    const bool lv = valid ? walk_live<H>(a.del, id, qi) : false;           // filters().check_vector(hop1), in flight with it
                    const bool fresh = valid && !(old & bit);
                    const bool ok = fresh && lv;
                    const uint64_t okm = __ballot(ok), frm = __ballot(fresh);
                    int brk = 64;
                    const uint32_t need = hop_limit - n_score;
                    if ((uint32_t)__popcll(okm) >= need) { brk = nth_set(okm, need); broke = true; }
                    const bool processed = lane <= brk;
                    if (fresh && !processed) atomicAnd(&vis[id >> 5], ~bit);              // links behind the break were never looked at
                    log_words(fresh && processed, id >> 5);
                    const uint64_t keep = mask_le(brk);
                    if (ok && processed) hop_ids[n_score + (uint32_t)__popcll(okm & lt_mask)] = id;
                    const uint64_t exm = frm & ~okm & keep;
                    if (fresh && !ok && processed) to_explore[n_explore + (uint32_t)__popcll(exm & lt_mask)] = id;
                    n_score += (uint32_t)__popcll(okm & keep);
                    n_explore += (uint32_t)__popcll(exm);
                }
            }
            __syncthreads();
            // 2-hop neighbours (:213-235): the links of every explored node, at most hop_limit scored per node.  The walk is a chain of
            // dependent memory round trips, so per node they are cut to two: the links of node e + 1 are fetched while node e is
            // resolved, and the three lookups of a link (hop-1 bit, hop-2 test-and-set, filter bits) go out together - a hop-2 bit
            // set for a link that turns out to sit in the hop-1 list is taken back, as the reference never sets it.
            uint32_t nx_id = 0;
            uint64_t nx_o1 = 0;
            bool nx_on = false;
            auto fetch_links = [&](uint32_t node) {
                if (h.l0) { nx_o1 = h.l0[(uint64_t)node * h.l0_stride]; } else { nx_o1 = h.offsets[(uint64_t)node + 1] - h.offsets[node]; }
                const uint64_t o0 = h.l0 ? 0 : h.offsets[node];
                // validity against the real count is applied when the node is resolved; the load itself stays inside the table
                const uint64_t lim = h.l0 ? (uint64_t)(h.l0_stride - 1) : (h.n_neighbors > o0 ? h.n_neighbors - o0 : 0);
                nx_id = link_of(node, o0, o0 + (lim < 64 ? lim : 64), &nx_on);
            };
            if (n_explore) fetch_links(to_explore[0]);
            for (uint32_t e = 0; e < n_explore; ++e) {
                if (n_score + hop_limit > h.hop_cap) flush_scores();
                const uint32_t node = to_explore[e];
                const uint64_t cnt = nx_o1;
                uint32_t id0 = nx_id;
                if (e + 1 < n_explore) fetch_links(to_explore[e + 1]);
                const uint64_t o0 = h.l0 ? 0 : h.offsets[node];
                const uint64_t o1 = o0 + cnt;
                uint32_t added = 0;
                bool broke = false;
                for (uint64_t base = o0; base < o1 && !broke; base += 64) {
                    bool on = base + (uint64_t)lane < o1;
                    uint32_t id = id0;
                    if (base != o0) id = link_of(node, base, o1, &on);     // (more than 64 links: not reached with m0 <= 64)
                    const bool valid = on && id < h.n_points;
                    const uint32_t bit = 1u << (id & 31);
                    const uint32_t r1 = valid ? atomicOr(&vis[id >> 5], 0u) : bit;                        // hop1_visited_list.check(hop2)
                    const uint32_t old2 = valid ? atomicOr(&vis[half + (id >> 5)], bit) : bit;            // hop2_visited_list.check_and_update_visited(hop2)
                    const bool lv = valid ? walk_live<H>(a.del, id, qi) : false;                          // filters().check_vector(hop2)
                    const bool s1 = (r1 & bit) != 0;
                    const bool set2 = valid && !(old2 & bit);            // this lane set the hop-2 bit
                    if (s1 && set2) atomicAnd(&vis[half + (id >> 5)], ~bit);
                    const bool fresh = valid && !s1 && set2;
                    const bool ok = fresh && lv;
                    const uint64_t okm = __ballot(ok);
                    int brk = 64;
                    const uint32_t need = hop_limit - added;
                    if ((uint32_t)__popcll(okm) >= need) { brk = nth_set(okm, need); broke = true; }
                    const bool processed = lane <= brk;
                    if (fresh && !processed) atomicAnd(&vis[half + (id >> 5)], ~bit);
                    log_words(fresh && processed, half + (id >> 5));
                    if (ok && processed) {
                        atomicOr(&vis[id >> 5], bit);                                                     // hop1_visited_list.check_and_update_visited(hop2)
                        hop_ids[n_score + added + (uint32_t)__popcll(okm & lt_mask)] = id;
                    }
                    log_words(ok && processed, id >> 5);
                    added += (uint32_t)__popcll(okm & mask_le(brk));
                }
                n_score += added;
            }
            // score_points_unfiltered + process_candidate, in order (:237-239)
            flush_scores();
        }
    } else {
    // search_on_level_with_vectors: `candidates` also holds what `nearest` evicted before it was expanded; when every entry of the beam is
    // expanded the reference pops the best of those: one whose score EQUALS the lower bound is expanded like any other (the loop breaks on strict
    // `candidate.score < lower_bound` only, graph_layers.rs:354-365), the first one below it has its base vector scored and ends the loop.
    // Every evicted-unexpanded candidate that can still be popped is kept.  Evictions arrive in strictly increasing key order (the entry that leaves is the
    // beam's worst, and whatever left before was worse still), and the bound never falls - so only the evictions of the LATEST score can ever tie with
    // the bound, and an eviction of a higher score retires all earlier ones: they can no longer tie, and only the best of them (ev_old: the last to leave)
    // can still be popped - as the candidate that ends the loop, once the latest group has been popped whole.  The
    // latest-score group lives in ev[0..3] (best first) with its older members on a per-slot stack in global memory (h.ev_spill: ascending keys, so the top of
    // the stack is the next best) - integer link scores (BQ, 1-bit TurboQuant) evict dozens of equal scores.  Among equal scores the pop order is the key's
    // (lower id first) where the reference's is its heap's.
    uint64_t ev[4] = {0, 0, 0, 0}, ev_old = 0;
    uint32_t n_spill = 0, n_offered = 0, n_exact = 0;
    uint64_t *const spill = h.ev_spill ? h.ev_spill + (uint64_t)blockIdx.x * h.ev_cap : nullptr;
    uint32_t n_exp = 0;
    while (true) {
        uint64_t ck = beam.pop_best(lane);
        if (ck == 0) {
            if (h.expanded && ev[0] && key_score(ev[0]) == key_score(beam.at(ef - 1))) {
                ck = ev[0];
                ev[0] = ev[1]; ev[1] = ev[2]; ev[2] = ev[3]; ev[3] = 0;
                if (n_spill) {      // (wave-uniform; agent-scope accesses: the stack is written and read back by this wave through L2)
                    --n_spill;
                    ev[3] = __hip_atomic_load(&spill[n_spill], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else break;
        }
        const uint32_t cand = key_idx(ck);
        if (h.expanded) {
            if (lane == 0 && n_exp < h.xcap) h.expanded[(uint64_t)qi * h.xcap + n_exp] = cand;
            ++n_exp;
        }
        if (h.pops) {     // qmx_hnsw_search_traced: the pop sequence (n_exp doubles as its counter: `expanded` and `pops` are never both set)
            if (lane == 0 && n_exp < h.pop_cap) {
                qmx_scored_point p;
                p.idx = cand;
                p.score = key_score(ck);
                h.pops[(uint64_t)qi * h.pop_cap + n_exp] = p;
            }
            ++n_exp;
        }
        // links of `cand` on level 0: the packed table needs ONE round trip (count and links are independent loads of the
        // same row), the CSR arrays two (offsets, then neighbors)
        uint64_t o0 = 0, o1 = 0;
        uint32_t packed_id = 0, packed_off = 0;
        if (h.l0) {
            const uint32_t *rowp = h.l0 + (uint64_t)cand * h.l0_stride;
            if (h.l0_aux_off) {
                // an SQ graph's wider table (hnsw_pack_level0_aux_kernel): [m0 link slots, 0xFFFFFFFF behind the last link][the vector_offset of every linked
                // row] - no count word, so that m0 = 32 makes a row of 256 bytes: two whole lines
                const uint32_t link_slots = h.l0_aux_off;
                packed_id = (uint32_t)lane < link_slots ? rowp[lane] : 0xFFFFFFFFu;
                if constexpr (hop_adds_offset<H>::value) packed_off = (uint32_t)lane < link_slots ? rowp[link_slots + (uint32_t)lane] : 0u;
                o1 = (uint64_t)__popcll(__ballot(packed_id != 0xFFFFFFFFu));
            } else {
                packed_id = (uint32_t)lane + 1 < h.l0_stride ? rowp[lane + 1] : 0;
                o1 = rowp[0];
            }
        } else {
            o0 = h.offsets[cand];
            o1 = h.offsets[(uint64_t)cand + 1];
        }
        uint32_t remaining = h.m0;
        for (uint64_t base = o0; base < o1 && remaining > 0; base += 64) {
            const uint64_t i = base + (uint64_t)lane;
            const bool on = i < o1;
            const uint32_t id = h.l0 ? (on ? packed_id : 0) : (on ? h.neighbors[i] : 0);
            const bool live = on && id < h.n_points && walk_live<H>(a.del, id, qi);
            const uint32_t bit = 1u << (id & 31);
            bool in_bm = true, was_visited = true;
            if (lv.tab) {
                if (live) was_visited = lv.test_and_set(id, vis, &in_bm);
            } else {
                const uint32_t old = live ? atomicOr(&vis[id >> 5], bit) : bit;
                was_visited = (old & bit) != 0;
            }
            bool keep = live && !was_visited;
            const uint64_t mask = __ballot(keep);
            const uint32_t rank = (uint32_t)__popcll(mask & lt_mask);
            uint32_t k = (uint32_t)__popcll(mask);
            if (k > remaining) {   // more links than level_m: the reference scores only the first `limit`
                if (keep && rank >= remaining) { lv.unset(id, vis, in_bm); keep = false; }
                k = remaining;
            }
            remaining -= k;
            __syncthreads();
            if (keep) {
                hop_ids[rank] = id;
                if constexpr (hop_adds_offset<H>::value) hop_scores[rank] = __uint_as_float(packed_off);      // (read only when the row carried it: below)
            }
            {   // the bitmap words this search dirtied (with the LDS table: only the ids of full buckets)
                const uint64_t bm = __ballot(keep && in_bm);
                const uint32_t brank = (uint32_t)__popcll(bm & lt_mask);
                if (keep && in_bm && log_cnt + brank < h.log_cap) vlog[log_cnt + brank] = id >> 5;
                log_cnt += (uint32_t)__popcll(bm);
            }
            n_scored += k;
            if constexpr (has_hop_prefilter<H>::value) {      // candidates that cannot beat the beam's worst entry leave here, unscored (the same walk: see H::prefilter)
                if (pq8) {
                    n_offered += k;
                    k = H::prefilter(a, pq8, hop_ids, k, beam.at(ef - 1), lane);
                    n_exact += k;
                }
            }
            hop_score<H>(a, qp, hop_ids, hop_scores, k, lane, h.l0 != nullptr && h.l0_aux_off != 0);
            const uint64_t mykey = (uint32_t)lane < k ? make_key(hop_scores[lane], hop_ids[lane]) : 0;
            uint64_t mm = __ballot(mykey > beam.at(ef - 1));
            while (mm) {
                const int src = __builtin_ctzll(mm);
                mm &= mm - 1;
                const uint64_t nk = readlane_u64(mykey, src);
                const uint64_t last = beam.at(ef - 1);
                if (nk > last) {
                    if (h.expanded && last != 0 && !beam.done_at(ef - 1)) {      // an unexpanded entry leaves `nearest`: it stays in `candidates`
                        if (ev[0] && (last >> 32) != (ev[0] >> 32)) {             // a higher score: the earlier evictions are retired
                            ev_old = ev[0];
                            ev[0] = ev[1] = ev[2] = ev[3] = 0;
                            n_spill = 0;
                        }
                        if (ev[3]) {                                              // the group's oldest member of the four makes room
                            if (spill && n_spill < h.ev_cap) {
                                if (lane == 0) __hip_atomic_store(&spill[n_spill], ev[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                ++n_spill;
                            } else if (lane == 0) *a.err_flag = 2;                // (more equal scores than the stack holds: reported, never silently dropped)
                        }
                        ev[3] = ev[2]; ev[2] = ev[1]; ev[1] = ev[0]; ev[0] = last;
                    }
                    beam.insert(nk, ef, lane);
                }
            }
        }
    }
    if (h.expanded) {
        const uint64_t last_pop = ev[0] ? ev[0] : ev_old;
        if (last_pop) {   // the pop that ends the loop: the best evicted candidate below the bound
            if (lane == 0 && n_exp < h.xcap) h.expanded[(uint64_t)qi * h.xcap + n_exp] = key_idx(last_pop);
            ++n_exp;
        }
        if (lane == 0) h.expanded_cnt[qi] = n_exp;
    }
    if (h.pops && lane == 0) h.pop_cnt[qi] = n_exp;
    if (h.pq_stats && lane == 0 && n_offered) {
        atomicAdd(&h.pq_stats[0], (unsigned long long)n_offered);
        atomicAdd(&h.pq_stats[1], (unsigned long long)n_exact);
    }
    }

    // ---- nearest.into_iter_sorted().take(top) ----
    {
        uint32_t count = 0;
        if constexpr (E == 0) {
            for (uint32_t base = 0; base < h.top; base += 64) {
                const uint32_t idx = base + (uint32_t)lane;
                const uint64_t k = idx < h.top ? beam.at(idx) : 0ull;
                const bool ok = k != 0;
                if (ok) {
                    qmx_scored_point p;
                    p.idx = key_idx(k);
                    p.score = key_score(k);
                    h.out[(uint64_t)qi * h.top + idx] = p;
                }
                count += (uint32_t)__popcll(__ballot(ok));
            }
        } else {
#pragma unroll
        for (int e = 0; e < (E ? E : 1); ++e) {
            const uint32_t idx = (uint32_t)e * 64 + (uint32_t)lane;
            const bool ok = beam.key[e] != 0 && idx < h.top;
            if (ok) {
                qmx_scored_point p;
                p.idx = key_idx(beam.key[e]);
                p.score = key_score(beam.key[e]);
                h.out[(uint64_t)qi * h.top + idx] = p;
            }
            count += (uint32_t)__popcll(__ballot(ok));
        }
        }
        if (lane == 0) {
            h.out_counts[qi] = count;
            if (h.out_scored) h.out_scored[qi] = n_scored;
        }
    }

    // ---- give the visited bitmap (and the LDS table) back all-zero ----
    __syncthreads();
    lv.clear(lane);
    if (log_cnt <= h.log_cap) {
        for (uint32_t i = (uint32_t)lane; i < log_cnt; i += 64) vis[vlog[i]] = 0;
    } else {
        for (uint64_t w = (uint64_t)lane; w < h.vis_words; w += 64) vis[w] = 0;
    }
    __threadfence();
    }   // E != HNSW_E_REF
}

// the dynamic LDS of the instantiation <E, QLDS> for a launch with arguments h
template <int E, bool QLDS>
__host__ __device__ __forceinline__ HnswLds hnsw_lds_layout(const HnswArgs &h) {
    return hnsw_lds_layout(E, QLDS, h.hop_cap, h.acorn, h.explore_cap, h.lds_query_bytes, h.ef > h.top ? h.ef : h.top, h.vis_lds, h.pq8 != nullptr, h.pq8_stride);
}

// ---- the query entry of a search, staged ------------------------------------------------------------------------------------------------------
// the wave copies n16 pieces of 16 bytes from global memory into LDS
__device__ __forceinline__ void stage_copy(unsigned char *dst, const unsigned char *src, uint32_t n16, int lane) {
    const uint4 *s = reinterpret_cast<const uint4 *>(src);
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    for (uint32_t i = (uint32_t)lane; i < n16; i += 64) d[i] = s[i];
}
// the 16-byte header in front of a multi-query's tokens (HopMaxSim); one lane writes it
__device__ __forceinline__ void write_maxsim_header(unsigned char *at, uint32_t n_tokens, const unsigned char *tokens) {
    *reinterpret_cast<uint32_t *>(at) = n_tokens;
    *reinterpret_cast<const unsigned char **>(at + 8) = tokens;
}
// the header in front of a custom query's examples (HopCustom); one lane writes it
__device__ __forceinline__ void write_custom_header(unsigned char *at, const qmx_custom_query &cq, const unsigned char *entries, const uint32_t *ex_off) {
    CustomHeader *hd = reinterpret_cast<CustomHeader *>(at);
    hd->kind = cq.kind; hd->n_a = cq.n_a; hd->n_b = cq.n_b; hd->coef_first = cq.coef_first;
    hd->entries = entries;
    hd->ex_off = ex_off;
}

// Stages the query entry of search qi in q_lds (QLDS; a header always sits there) -> where the entry lies: behind the header in LDS, or in global memory.
template <class H, bool QLDS>
__device__ __forceinline__ const unsigned char *stage_search_entry(const ScanArgs &a, const HnswArgs &h, unsigned char *q_lds, uint32_t qi, int lane) {
    const unsigned char *queries = reinterpret_cast<const unsigned char *>(a.queries);
    if constexpr (is_maxsim<H>::value) {
        // (the header always sits in LDS; the entries follow when the launch's budget holds them, else they are read where they lie)
        const uint32_t t0 = a.mv_qfirst[qi], n_tokens = a.mv_qfirst[qi + 1] - t0;
        const unsigned char *qg = queries + (uint64_t)t0 * a.q_stride;
        const bool fits = 16 + (uint64_t)n_tokens * a.q_stride <= h.lds_query_bytes;
        __syncthreads();
        if (fits) stage_copy(q_lds + 16, qg, n_tokens * (a.q_stride / 16), lane);
        if (lane == 0) write_maxsim_header(q_lds, n_tokens, fits ? q_lds + 16 : qg);
        __syncthreads();
        return q_lds + 16;
    } else if constexpr (is_custom<H>::value) {
        // (the header always sits in LDS: launch_hnsw_hop grants at least its 32 bytes; the examples follow when the launch's budget holds them)
        const qmx_custom_query cq = a.cq_desc[qi];
        const uint32_t ne = cq.kind <= QMX_CUSTOM_RECO_SUM_SCORES ? cq.n_a + cq.n_b : cq.n_a + 2 * cq.n_b;
        unsigned char *base = q_lds + sizeof(CustomHeader);
        if constexpr (H::MULTI_EXAMPLES) {
            // [header][offset table, 16-byte padded][per example: 16-byte MaxSim header (its token count) + its tokens]; the API sized the launch for it
            uint32_t *tab = reinterpret_cast<uint32_t *>(base);
            uint32_t off = (4 * ne + 15u) & ~15u;
            __syncthreads();
            for (uint32_t e = 0; e < ne; ++e) {
                const uint32_t t0 = a.mv_qfirst[cq.first + e], nt = a.mv_qfirst[cq.first + e + 1] - t0;
                // (the visited table and the PQ image sit right behind the query entry: an example that did not fit the launch's entry must not be
                // staged over them - the search is refused instead)
                if (sizeof(CustomHeader) + (uint64_t)off + 16 + (uint64_t)nt * a.q_stride > h.lds_query_bytes) {
                    if (lane == 0) *a.err_flag = 1;
                    break;
                }
                if (lane == 0) {
                    tab[e] = off + 16;
                    write_maxsim_header(base + off, nt, base + off + 16);
                }
                stage_copy(base + off + 16, queries + (uint64_t)t0 * a.q_stride, nt * (a.q_stride / 16), lane);
                off += 16 + nt * a.q_stride;
            }
            if (lane == 0) write_custom_header(q_lds, cq, base, tab);
        } else {
            const unsigned char *qg = queries + (uint64_t)cq.first * a.q_stride;
            const bool fits = sizeof(CustomHeader) + (uint64_t)ne * a.q_stride <= h.lds_query_bytes;
            __syncthreads();
            if (fits) stage_copy(base, qg, ne * (a.q_stride / 16), lane);
            if (lane == 0) write_custom_header(q_lds, cq, fits ? base : qg, nullptr);
        }
        __syncthreads();
        return base;
    } else {
        const unsigned char *qg = queries + (uint64_t)qi * a.q_stride;
        if constexpr (QLDS) {
            __syncthreads();
            stage_copy(q_lds, qg, (h.lds_query_bytes < a.q_stride ? h.lds_query_bytes : a.q_stride) / 16, lane);     // (a policy may own scratch behind its entry)
            __syncthreads();
            return q_lds;
        } else {
            return qg;
        }
    }
}

#ifndef QMX_WALK_KERNEL_ATTR
#define QMX_WALK_KERNEL_ATTR
#endif
template <class H, int E, bool QLDS>
__global__ __launch_bounds__(64) QMX_WALK_KERNEL_ATTR void hnsw_search_kernel(const ScanArgs a, const HnswArgs h) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const HnswLds at = hnsw_lds_layout<E, QLDS>(h);
    uint32_t *hop_ids = reinterpret_cast<uint32_t *>(smem + at.hop_ids);
    float *hop_scores = reinterpret_cast<float *>(smem + at.hop_scores);
    // every region by the layout: the query entry and the beam found from the region in front of them, the two regions behind the beam looked up
    // where the launch has them
    unsigned char *q_lds = smem + at.explore + (at.query - at.explore);
    uint32_t *vis = h.visited + (uint64_t)blockIdx.x * h.vis_words;
    uint32_t *vlog = h.vis_log + (uint64_t)blockIdx.x * h.log_cap;
    unsigned char *beam_lds = q_lds + (at.beam - at.query);      // E == 0: the LDS beam behind the query entry (E == HNSW_E_REF: `nearest`)
    // the search's visited table (LdsVisited): zero once here, every search leaves it zero
    uint32_t *vtab = nullptr;
    if (h.vis_lds) vtab = reinterpret_cast<uint32_t *>(smem + hnsw_lds_layout<E, QLDS>(h).visited);
    if (vtab) {
        LdsVisited{vtab}.clear(lane);
        __syncthreads();
    }
    // Searches are handed out one at a time (h.next_query, set to gridDim.x by the host): a slot that finishes takes the next unstarted search.  With the
    // static stride qi += gridDim.x the launch lasted ceil(nq / slots) searches of the slowest slot - 8 192 searches on 2 304 slots paid for 4 rounds while
    // doing 3.56 (profiles/r5_sq_walk_visited.md).
    auto next_search = [&](uint32_t qi) -> uint32_t {
        if (!h.next_query) return qi + gridDim.x;
        uint32_t v = 0;
        if (lane == 0) v = atomicAdd(h.next_query, 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    };
    // HopPQ's 8-bit LUT image of the search (HnswArgs::pq8)
    unsigned char *pq8_lds = nullptr;
    if constexpr (has_hop_prefilter<H>::value) {
        if (h.pq8) pq8_lds = smem + hnsw_lds_layout<E, QLDS>(h).pq8;
    }
    for (uint32_t qi = blockIdx.x; qi < h.nq; qi = next_search(qi)) {
        if constexpr (has_hop_prefilter<H>::value) {
            if (pq8_lds) {
                __syncthreads();
                stage_copy(pq8_lds, h.pq8 + (uint64_t)qi * h.pq8_stride, h.pq8_stride / 16, lane);
                __syncthreads();
            }
        }
        const unsigned char *qp = stage_search_entry<H, QLDS>(a, h, q_lds, qi, lane);
        hnsw_search_one<H, E>(a, h, qp, hop_ids, hop_scores, vis, vlog, qi, lane, beam_lds, vtab, pq8_lds);
    }
}

// occupancy of an instantiation (blocks of one wave per CU) for a launch with arguments h — used by the API to size the scratch
template <class H, int E, bool QLDS>
int32_t hnsw_occupancy_inst(const HnswArgs &h, int *per_cu) {
    auto kfn = hnsw_search_kernel<H, E, QLDS>;
    static thread_local DeviceOnce attr_once;
    if (attr_once.need()) {
        QMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_once.mark();
    }
    int n = 0;
    QMX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kfn, 64, hnsw_lds_layout<E, QLDS>(h).total));
    *per_cu = n < 1 ? 1 : n;
    return QMX_OK;
}

template <class H, int E, bool QLDS>
int32_t launch_hnsw_inst(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid) {
    const uint32_t ef = h.ef > h.top ? h.ef : h.top;
    const size_t lds = hnsw_lds_layout<E, QLDS>(h).total;
    QMX_REQUIRE(lds <= 160 * 1024, QMX_ERR_NOT_SUPPORTED, "hnsw walk: %zu bytes of LDS (query entry + a list of %u)", lds, ef);
    ::qmx::clear_stale_error();
    QMX_NOTE_KERNEL((hnsw_search_kernel<H, E, QLDS>));
    hipLaunchKernelGGL((hnsw_search_kernel<H, E, QLDS>), dim3(grid), dim3(64), lds, st, a, h);
    QMX_HIP(hipGetLastError());
    return QMX_OK;
}

// the policies option hnsw_reference_heap_order is instantiated for: the plain single-vector walks (dense, SQ, PQ, BQ, TurboQuant)
template <class H>
struct ref_heaps_built {
    static constexpr bool value = !is_custom<H>::value && !is_maxsim<H>::value && !is_maxsim_q<H>::value && !is_maxsim_internal<H>::value && !is_tql1<H>::value;
};

// the instantiation <H, E, QLDS> that serves a launch, handed to `with` as a tag
template <int E, bool QLDS>
struct WalkInst {
    static constexpr int e = E;
    static constexpr bool qlds = QLDS;
};
template <class H, class With>
int32_t choose_hnsw_inst(const HnswArgs &h, uint32_t ef, With &&with) {
    const bool qlds = h.lds_query_bytes > 0;
    if (h.ref_heaps) {      // option hnsw_reference_heap_order: the plain walk of the policies a stored graph is walked with
        if constexpr (ref_heaps_built<H>::value) {
            QMX_REQUIRE(!h.acorn && !h.expanded, QMX_ERR_NOT_SUPPORTED, "hnsw_reference_heap_order: the plain walk only (not ACORN, not search_with_vectors)");
            return qlds ? with(WalkInst<HNSW_E_REF, true>{}) : with(WalkInst<HNSW_E_REF, false>{});
        } else {
            set_error("hnsw_reference_heap_order: not built for this scorer (custom queries, multi-vector points, TurboQuant over Manhattan)");
            return QMX_ERR_NOT_SUPPORTED;
        }
    }
    if (ef > HNSW_MAX_EF_REG) {        // the LDS beam: one instantiation per policy, the query entry staged
        QMX_REQUIRE(qlds, QMX_ERR_NOT_SUPPORTED, "hnsw ef %u > %u needs the query entry in LDS (it does not fit)", ef, HNSW_MAX_EF_REG);
        return with(WalkInst<0, true>{});
    }
    if constexpr (is_custom<H>::value || is_maxsim<H>::value) {      // (always staged: no instantiation that reads the entry from global memory)
        return ef <= 128 ? with(WalkInst<2, true>{}) : with(WalkInst<8, true>{});
    } else {
        if (ef <= 128) return qlds ? with(WalkInst<2, true>{}) : with(WalkInst<2, false>{});
        return qlds ? with(WalkInst<8, true>{}) : with(WalkInst<8, false>{});
    }
}

// grid == 0: only report the occupancy in *per_cu (no launch)
template <class H>
int32_t launch_hnsw_hop(hipStream_t st, const ScanArgs &a, const HnswArgs &h, uint32_t grid, int *per_cu) {
    const uint32_t ef = h.ef > h.top ? h.ef : h.top;
    QMX_REQUIRE(ef >= 1 && ef <= HNSW_MAX_EF, QMX_ERR_NOT_SUPPORTED, "hnsw ef %u not in 1..%u", ef, HNSW_MAX_EF);
    if constexpr (!per_query_filter<H>::value && !is_custom<H>::value && !is_maxsim<H>::value && !is_maxsim_q<H>::value && !is_maxsim_internal<H>::value) {
        if (a.del.filter_of) return launch_hnsw_hop<HopPerQuery<H>>(st, a, h, grid, per_cu);      // (also for the occupancy query: the scratch is sized for the kernel that runs)
    } else if constexpr (!per_query_filter<H>::value) {
        QMX_REQUIRE(!a.del.filter_of, QMX_ERR_NOT_SUPPORTED, "this walk does not serve per-request filters (qmx_query_set_filters)");
    }
    if constexpr (is_maxsim<H>::value) QMX_REQUIRE(h.lds_query_bytes > 0, QMX_ERR_NOT_SUPPORTED, "the inner vectors of a multi-query must fit the LDS");
    if constexpr (is_custom<H>::value) QMX_REQUIRE(h.lds_query_bytes >= sizeof(CustomHeader), QMX_ERR_OTHER, "the custom walk keeps its header in LDS");
    return choose_hnsw_inst<H>(h, ef, [&](auto inst) -> int32_t {
        constexpr int E = decltype(inst)::e;
        constexpr bool QLDS = decltype(inst)::qlds;
        if (grid == 0) return hnsw_occupancy_inst<H, E, QLDS>(h, per_cu);
        return launch_hnsw_inst<H, E, QLDS>(st, a, h, grid);
    });
}

// launch functors for the per-dtype dispatchers (dispatch_dense / dispatch_sq): the storage's hop policy under the wrapper of the walk's scorer
template <template <class> class Wrap>
struct HnswLauncherOf {
    hipStream_t st;
    const HnswArgs *h;
    uint32_t grid;
    int *per_cu;
    template <class P> int32_t row(const ScanArgs &a) const { return launch_hnsw_hop<Wrap<HopRow<P>>>(st, a, *h, grid, per_cu); }
    template <class S> int32_t small(const ScanArgs &a) const { return launch_hnsw_hop<Wrap<HopSmall<S>>>(st, a, *h, grid, per_cu); }
};
template <class H> using HopPlain = H;
template <class H> using HopCustomMaxSim = HopCustom<HopMaxSim<H>>;
using HnswLauncher = HnswLauncherOf<HopPlain>;
using HnswCustomLauncher = HnswLauncherOf<HopCustom>;
using HnswCustomMaxSimLauncher = HnswLauncherOf<HopCustomMaxSim>;
using HnswMaxSimLauncher = HnswLauncherOf<HopMaxSim>;

}  // namespace qmx
