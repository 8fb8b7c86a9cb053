// hnsw_sets.hpp — what a search of the walk (hnsw.hpp) keeps: the beam (registers or LDS), the visited set in LDS, and the two binary heaps of option
// hnsw_reference_heap_order.
#pragma once
#include "hnsw_layout.hpp"
#include "scan_common.hpp"

namespace qmx {

// ---- the beam: sorted descending, entry index = e * 64 + lane ------------------------------------
template <int E>
struct Beam {
    uint64_t key[E];
    uint32_t done[E];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int e = 0; e < E; ++e) { key[e] = 0; done[e] = 0; }
    }
    __device__ __forceinline__ uint64_t at(uint32_t idx) const {   // idx uniform
        uint64_t r = 0;
#pragma unroll
        for (int e = 0; e < E; ++e)
            if ((idx >> 6) == (uint32_t)e) r = readlane_u64(key[e], (int)(idx & 63));
        return r;
    }
    // insert nk (uniform, non-zero), keep the first `cap` entries
    __device__ __forceinline__ void insert(uint64_t nk, uint32_t cap, int lane) {
        uint32_t p = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) p += (uint32_t)__popcll(__ballot(key[e] > nk));
        uint64_t carry_k = 0;
        uint32_t carry_d = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            uint64_t up = shfl_up1_u64(key[e]);
            uint32_t upd = (uint32_t)__shfl_up((int)done[e], 1, 64);
            const uint64_t last_k = readlane_u64(key[e], 63);
            const uint32_t last_d = (uint32_t)__builtin_amdgcn_readlane((int)done[e], 63);
            if (lane == 0) { up = carry_k; upd = carry_d; }
            const uint32_t idx = (uint32_t)e * 64 + (uint32_t)lane;
            if (idx == p) { key[e] = nk; done[e] = 0; }
            else if (idx > p) { key[e] = up; done[e] = upd; }
            if (idx >= cap) { key[e] = 0; done[e] = 0; }
            carry_k = last_k;
            carry_d = last_d;
        }
    }
    __device__ __forceinline__ bool done_at(uint32_t idx) const {   // idx uniform
        uint32_t r = 0;
#pragma unroll
        for (int e = 0; e < E; ++e)
            if ((idx >> 6) == (uint32_t)e) r = (uint32_t)__builtin_amdgcn_readlane((int)done[e], (int)(idx & 63));
        return r != 0;
    }
    // best unexpanded entry -> its key (0 if none); marks it expanded
    __device__ __forceinline__ uint64_t pop_best(int lane) {
        uint64_t ck = 0;
        bool found = false;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint64_t m = __ballot(key[e] != 0 && done[e] == 0);
            if (!found && m) {
                const int l = __builtin_ctzll(m);
                ck = readlane_u64(key[e], l);
                if (lane == l) done[e] = 1;
                found = true;
            }
        }
        return ck;
    }};

// The same list for ef > 512, kept in LDS (the walk kernel appends `cap` keys + `cap` flag bytes to its dynamic LDS): the same interface, every
// operation wave-cooperative.  insert: the position by a two-level search (64 block ends, then the block), then the tail moves up one entry, 64
// at a time from the end; pop_best scans from a hint below which every entry is expanded.  Slower per operation than the register beam, and meant
// to be: searches this wide are rare.
template <>
struct Beam<0> {
    uint64_t *key;
    unsigned char *done;
    uint32_t len, hint;
    __device__ __forceinline__ void init(unsigned char *lds, uint32_t cap) {
        key = reinterpret_cast<uint64_t *>(lds);
        done = lds + 8 * (size_t)cap;
    }
    __device__ __forceinline__ void clear() { len = 0; hint = 0; }
    __device__ __forceinline__ uint64_t at(uint32_t idx) const { return idx < len ? key[idx] : 0ull; }        // idx uniform
    __device__ __forceinline__ bool done_at(uint32_t idx) const { return idx < len && done[idx] != 0; }
    __device__ __forceinline__ void insert(uint64_t nk, uint32_t cap, int lane) {
        // p = number of keys above nk (descending, distinct keys)
        uint32_t p = 0;
        if (len) {
            const uint32_t stride = (len + 63) / 64;                       // <= 64 while cap <= 4096
            const uint32_t last = (uint32_t)lane * stride + stride - 1;     // the end of the lane's block
            const bool whole = last < len && key[last] > nk;                // the block lies above nk as a whole
            const uint32_t b = (uint32_t)__popcll(__ballot(whole));         // (monotone: the first b blocks)
            const uint32_t i = b * stride + (uint32_t)lane;
            const bool above = (uint32_t)lane < stride && i < len && key[i] > nk;
            p = b * stride + (uint32_t)__popcll(__ballot(above));
        }
        const uint32_t new_len = len < cap ? len + 1 : cap;
        if (p >= new_len) return;                                           // (below a full list: the callers test against at(cap - 1) first)
        for (uint32_t hi = new_len - 1; hi > p;) {                          // entries [p, new_len - 1) move up by one, the last of a full list drops out
            const uint32_t lo = hi - p > 64 ? hi - 63 : p + 1;
            const uint32_t i = lo + (uint32_t)lane;
            uint64_t k = 0;
            unsigned char d = 0;
            if (i <= hi) { k = key[i - 1]; d = done[i - 1]; }
            if (i <= hi) { key[i] = k; done[i] = d; }
            hi = lo - 1;
        }
        if (lane == 0) { key[p] = nk; done[p] = 0; }
        len = new_len;
        if (p < hint) hint = p;
    }
    __device__ __forceinline__ uint64_t pop_best(int lane) {
        for (uint32_t base = hint; base < len; base += 64) {
            const uint32_t i = base + (uint32_t)lane;
            const uint64_t m = __ballot(i < len && done[i] == 0);
            if (m) {
                const uint32_t at = base + (uint32_t)__builtin_ctzll(m);
                if (i == at) done[i] = 1;
                hint = at + 1;
                return key[at];
            }
        }
        hint = len;
        return 0ull;
    }
};

// ---- the visited set of a search, in LDS ----------------------------------------------------------------------------------------------
// One bit per point in a per-slot HBM bitmap costs the walk a third of its time at 10 M points: every test-and-set is an L2 atomic on a random word of a
// 1.25 MB bitmap (5 GB over the slots in flight), i.e. an HBM read-modify-write per link - tools/micro/gather_roof measures the row gathers of a hop at
// 6.2 TB/s alone and at 3.4 TB/s with those atomics beside them, which is where the walk sat (profiles/r5_sq_walk_visited.md).  A search inserts a few
// thousand ids, so its set fits the LDS: 1024 buckets (id & 1023) of eight 16-bit tags ((id >> 10) + 1; 0 = empty, 0xFFFF = taken back) = 16 KiB per search.  test_and_set looks
// the tag up in its bucket (one ds_read_b128), claims the first empty half-word with a compare-and-swap on the word that holds it (lanes of the wave insert
// side by side; a lost race re-reads), and when the bucket is full - about 1 % of the inserts of an ef = 128 search, more for wide ones - falls back to the
// HBM bitmap for that id.  An id is recorded in exactly one of the two places (the bucket is consulted first, and a full bucket never frees a slot while the
// search runs: unset() marks the slot instead of emptying it), so the set is exact: same fresh / visited answers as the bitmap alone, hence the same
// walk.  Graphs of more than 65534 x 1024 points (tags would not fit), ACORN and the reference-heap mode keep the bitmap.
// (One search = one wave = one work-group of 64 threads - `__launch_bounds__(64)` on the walk kernels: the plain 16-byte read of a bucket below races with
// nobody but the lanes of its own wave, whose LDS operations execute in order.  A launch with more than one wave per group would need atomic bucket reads.)
struct LdsVisited {
    uint32_t *tab;      // LDS, 4096 words; nullptr: the bitmap only
    // -> true when `id` was visited before; *in_bitmap: the id lives (now or already) in the HBM bitmap, not in the table
    __device__ __forceinline__ bool test_and_set(uint32_t id, uint32_t *vis, bool *in_bitmap) const {
        const uint32_t bit = 1u << (id & 31);
        *in_bitmap = false;
        if (tab) {
            uint32_t *b = tab + (id & 1023u) * 4u;
            const uint32_t tag = (id >> 10) + 1u;
            for (;;) {
                const uint4 w4 = *reinterpret_cast<const uint4 *>(b);
                const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
                int empty = -1;
                bool found = false;
#pragma unroll
                for (int d = 3; d >= 0; --d) {
                    const uint32_t lo = w[d] & 0xFFFFu, hi = w[d] >> 16;
                    found = found || lo == tag || hi == tag;
                    if (hi == 0) empty = 2 * d + 1;
                    if (lo == 0) empty = 2 * d;
                }
                if (found) return true;
                if (empty < 0) break;                                    // the bucket is full: this id is the bitmap's
                const int d = empty >> 1;
                const uint32_t expected = w[d], desired = expected | (tag << (16 * (empty & 1)));
                if (atomicCAS(&b[d], expected, desired) == expected) return false;
            }
        }
        *in_bitmap = true;
        return (atomicOr(&vis[id >> 5], bit) & bit) != 0;
    }
    // takes back an insert this search made (a link behind the level's limit: the reference never looked at it)
    __device__ __forceinline__ void unset(uint32_t id, uint32_t *vis, bool in_bitmap) const {
        if (in_bitmap || !tab) { atomicAnd(&vis[id >> 5], ~(1u << (id & 31))); return; }
        // The slot is not freed but marked (tag 0xFFFF: no id of a graph this table serves has it): a bucket that was ever full stays full, so an id that
        // went to the bitmap because its bucket was full can never be mistaken for a fresh one by a later lookup that finds room in that bucket.
        uint32_t *b = tab + (id & 1023u) * 4u;
        const uint32_t tag = (id >> 10) + 1u;
        for (int d = 0; d < 4; ++d) {
            for (;;) {
                const uint32_t w = b[d];
                uint32_t nw = w;
                if ((w & 0xFFFFu) == tag) nw = w | 0xFFFFu;
                else if ((w >> 16) == tag) nw = w | 0xFFFF0000u;
                else break;
                if (atomicCAS(&b[d], w, nw) == w) return;
            }
        }
    }
    __device__ __forceinline__ void clear(int lane) const {               // wave-cooperative; the caller barriers
        if (!tab) return;
        uint4 *t = reinterpret_cast<uint4 *>(tab);
        for (uint32_t i = (uint32_t)lane; i < HNSW_VIS_LDS_BYTES / 16; i += 64) t[i] = make_uint4(0, 0, 0, 0);
    }
};

// ---- option hnsw_reference_heap_order: the reference's two binary heaps, worked by ONE lane in std's exact sift order ---------------------
// `nearest` = FixedLengthPriorityQueue<ScoredPointOffset> = BinaryHeap<Reverse<T>> of at most ef entries (lib/common/common/src/
// fixed_length_priority_queue.rs:20-65; push :47-59 replaces the root only on strict root < value, through PeekMut = sift_down(0));
// `candidates` = BinaryHeap<ScoredPointOffset> (search_context.rs:8-40; pop = swap with the last + sift_down_to_bottom(0) + sift_up).
// ScoredPointOffset orders by OrderedFloat(score) alone, so which of two equal scores a sift moves depends on where they sit in the array:
// reproducing the arrays is the only way to reproduce the reference's lists among equal scores (integer scorers: SQ, u8, BQ, 1-bit TQ).
// Every heap operation is a chain of dependent loads of one lane; `nearest` sits in LDS, and so do the first HNSW_REF_CAND_LDS entries of
// `candidates` (round 6: the levels every sift touches; rounds 5's heap lived in HBM whole: a pop was a dozen dependent trips to memory); the rest of
// the array (unbounded in the reference) is a per-slot HBM scratch of ref_cap entries.
struct RefHeaps {
    uint2 *nd;                 // nearest: x = idx, y = score bits
    uint2 *cd;                 // candidates: entries [c_lds, c_cap) live here ...
    uint2 *cl;                 // ... entries [0, c_lds) in LDS
    uint32_t n_len, n_cap, c_len, c_cap, c_lds;
    bool overflow;
    __device__ __forceinline__ uint2 cget(uint32_t i) const { return i < c_lds ? cl[i] : cd[i]; }
    __device__ __forceinline__ void cset(uint32_t i, uint2 v) { if (i < c_lds) cl[i] = v; else cd[i] = v; }
    // OrderedFloat::cmp: NaN is the greatest value and equal to itself
    static __device__ __forceinline__ int of_cmp(float a, float b) {
        if (a < b) return -1;
        if (a > b) return 1;
        if (a == b) return 0;
        const bool an = a != a, bn = b != b;
        if (an && bn) return 0;
        return an ? 1 : -1;
    }
    static __device__ __forceinline__ float sc(uint2 v) { return __uint_as_float(v.y); }
    static __device__ __forceinline__ int rev_cmp(uint2 a, uint2 b) { return of_cmp(sc(b), sc(a)); }      // Reverse<T>
    __device__ __forceinline__ void init(unsigned char *lds, uint32_t ef, uint2 *scratch, uint32_t cap, unsigned char *cand_lds, uint32_t cand_lds_entries) {
        nd = reinterpret_cast<uint2 *>(lds);
        cd = scratch;
        cl = reinterpret_cast<uint2 *>(cand_lds);
        c_lds = cand_lds_entries;
        n_len = 0; n_cap = ef ? ef : 1; c_len = 0; c_cap = cap;
        overflow = false;
    }
    // BinaryHeap::sift_up(0, pos) under Reverse
    __device__ void n_sift_up(uint32_t pos) {
        const uint2 elt = nd[pos];
        while (pos > 0) {
            const uint32_t parent = (pos - 1) / 2;
            if (rev_cmp(elt, nd[parent]) <= 0) break;
            nd[pos] = nd[parent];
            pos = parent;
        }
        nd[pos] = elt;
    }
    // BinaryHeap::sift_down_range(pos, end) under Reverse
    __device__ void n_sift_down_range(uint32_t pos, uint32_t end) {
        const uint2 elt = nd[pos];
        uint32_t child = 2 * pos + 1;
        while (end >= 2 && child <= end - 2) {
            child += rev_cmp(nd[child], nd[child + 1]) <= 0 ? 1u : 0u;
            if (rev_cmp(elt, nd[child]) >= 0) { nd[pos] = elt; return; }
            nd[pos] = nd[child];
            pos = child;
            child = 2 * pos + 1;
        }
        if (end >= 1 && child == end - 1 && rev_cmp(elt, nd[child]) < 0) {
            nd[pos] = nd[child];
            pos = child;
        }
        nd[pos] = elt;
    }
    // FixedLengthPriorityQueue::push -> was the value kept (SearchContext::process_candidate's `was_added`)
    __device__ bool n_push(uint2 v) {
        if (n_len < n_cap) {
            nd[n_len] = v;
            n_sift_up(n_len);
            ++n_len;
            return true;                                   // None
        }
        if (of_cmp(sc(nd[0]), sc(v)) < 0) {
            const uint2 removed = nd[0];
            nd[0] = v;
            n_sift_down_range(0, n_len);
            return removed.x != v.x;                       // Some(removed): removed.idx != score_point.idx
        }
        return false;                                      // Some(value): rejected
    }
    __device__ void c_push(uint2 v) {
        if (c_len == c_cap) { overflow = true; return; }
        uint32_t pos = c_len++;
        while (pos > 0) {                                  // sift_up(0, pos)
            const uint32_t parent = (pos - 1) / 2;
            const uint2 pv = cget(parent);
            if (of_cmp(sc(v), sc(pv)) <= 0) break;
            cset(pos, pv);
            pos = parent;
        }
        cset(pos, v);
    }
    __device__ bool c_pop(uint2 *out) {
        if (c_len == 0) return false;
        uint2 item = cget(--c_len);
        if (c_len > 0) {
            const uint2 root = cget(0);
            // sift_down_to_bottom(0) of `item`, then sift_up from where it landed
            const uint32_t end = c_len;
            uint32_t pos = 0, child = 1;
            while (end >= 2 && child <= end - 2) {
                const uint2 l = cget(child), r = cget(child + 1);
                const bool right = of_cmp(sc(l), sc(r)) <= 0;
                cset(pos, right ? r : l);
                pos = child + (right ? 1u : 0u);
                child = 2 * pos + 1;
            }
            if (child == end - 1) { cset(pos, cget(child)); pos = child; }
            while (pos > 0) {
                const uint32_t parent = (pos - 1) / 2;
                const uint2 pv = cget(parent);
                if (of_cmp(sc(item), sc(pv)) <= 0) break;
                cset(pos, pv);
                pos = parent;
            }
            cset(pos, item);
            item = root;
        }
        *out = item;
        return true;
    }
    // SearchContext::process_candidate (search_context.rs:32-40)
    __device__ void process_candidate(uint32_t idx, float score) {
        const uint2 v = make_uint2(idx, __float_as_uint(score));
        if (n_push(v)) c_push(v);
    }
    // into_iter_sorted(): BinaryHeap::into_sorted_vec under Reverse = descending score, in place
    __device__ uint32_t n_into_sorted() {
        uint32_t end = n_len;
        while (end > 1) {
            --end;
            const uint2 t = nd[0]; nd[0] = nd[end]; nd[end] = t;
            n_sift_down_range(0, end);
        }
        return n_len;
    }
};

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace qmx
