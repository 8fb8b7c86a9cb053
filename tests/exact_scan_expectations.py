"""What tests/test_gpu_exact_scan_large_blocks.py expects, worked out on the CPU alone (imports the oracle, never the device): the row counts, the blocks,
the planted rows, the expected lists and the preconditions that make a case worth running.  tests/test_exact_scan_expectations.py checks all of it for
every case without a GPU.  Test infrastructure.

Row counts.  Every exact scan kernel is persistent: its grid is capped and a wave loops `tile += tw` over what the cap leaves.  On 256 CUs

  * scan_sq_mfma_kernel: 16 rows per wave, 8 waves per block, at least one block per CU -> one grid pass covers at least 256 * 8 * 16 = 32 768 rows (row
    SECOND_PASS_ROW is the first row of the second pass then) and, at 8 blocks per CU, at most 2^18.  N_MFMA = 2^18 + 87: every wave takes at least two
    tiles under any occupancy, the pre-scan is on (n >= 2^18), and n % 16 = 7: the last tile is partial.
  * the generic scan_kernel (behind it launch_scan_sq and launch_scan_tq): at most R = 4 groups of 8 rows per wave, 8 waves per block, 4 blocks per CU
    -> up to 256 * 4 * 8 * 32 = 262 144 rows per pass.  N_VALU = 3 * 2^17 + 87 is above that.
  * bq_rows_kernel: 256 rows per block, 8 blocks per CU -> 2 048 * 256 = 524 288 rows per pass.  N_BQROWS = 2^19 + 2^17 + 87.
  * tq_l1_scores_device works in batches of 65 536 rows: N_L1 = one batch + 37 rows, two batches + 5 rows.

From 2^18 candidates on, pass 0 of an exact tile scores a prefix of pre_n(n) rows first; the k-th best key of the prefix is the scan's starting bound.

Blocks.  BQ rows are random code bytes (under scalar-encoded queries, whose scores are 15 or 255 times as many: drawn from a base as below).  Every other
storage encodes a base of N_BASE vectors once and gathers the block from it, block[i] =
base[draw[i]]: every score then occurs n / N_BASE (8 to 20) times at scattered offsets, so every boundary at top = 10 is a tie group, and the oracle's
score of block row i is its score of base row draw[i] (a score is a function of the query and the row's bytes; the oracle scores the base only).
For each of the N_CHECKED queries the oracle checks, the row that scores best is planted at planted_offsets(n, c): offsets 0, pre_n - 1, pre_n,
SECOND_PASS_ROW, n - 16 and n - 1 for query 0, moved by c rows towards the inside of their tile for query c.  The draw avoids the best and the second
best base row of every checked query, so the planted copies are all there are: they head the expected list, whatever their offset."""
import numpy as np

import oracle_ffi as O

N_MFMA = 2 ** 18 + 87
N_VALU = 3 * 2 ** 17 + 87
N_BQROWS = 2 ** 19 + 2 ** 17 + 87
N_L1 = (65_536 + 37, 2 * 65_536 + 5)
N_BASE = 2 ** 15
SECOND_PASS_ROW = 32_768
N_CHECKED = 4
TOP = 10
L1_PLANTED = (65_535, 65_536, 131_071, 131_072)      # ... and n - 1: the batch edges of the TurboQuant-L1 route


def pre_n(n):
    """rows of the prefix an exact tile scans first (api_search.hip exact_tile, prescan_shift = 10)"""
    return max(n >> 10, 1 << 13) & ~15


def planted_offsets(n, c):
    p = pre_n(n)
    return [c, p - 1 - c, p + c, SECOND_PASS_ROW + c, n - 16 + c, n - 1 - c]


def score_ord(scores):
    """the device's order of f32 scores as integers (common.hpp score_to_ord): bigger = better, NaN greatest"""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    b = s.view(np.uint32).astype(np.int64)
    o = np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)
    return np.where(s != s, 0xFFFFFFFF, o)


def expected_list(scores, top, cand=None, live=None):
    """tests/parity_asserts.py's rule over the live candidates: descending score (its bits), ascending offset, the lowest offsets fill a tied boundary.
    scores: one query's score of every row of the block; cand: the id list (repeats allowed: one entry per occurrence), None = every row; live: bool mask
    of the rows.  Returns (ids, scores) of the list."""
    ids = np.arange(len(scores), dtype=np.int64) if cand is None else np.asarray(cand, dtype=np.int64)
    if live is not None:
        ids = ids[live[ids]]
    sc = np.asarray(scores, dtype=np.float32)[ids]
    o = score_ord(sc)
    if len(o) > top:                                         # (np.lexsort((ids, -o))[:top], without sorting what cannot be in it)
        keep = np.flatnonzero(o >= np.partition(o, len(o) - top)[len(o) - top])
        ids, sc, o = ids[keep], sc[keep], o[keep]
    order = np.lexsort((ids, -o))[:top]
    return ids[order], sc[order]


def boundary_group(scores, top, cand=None, live=None):
    """(slots, members): the entries of the expected list that carry its last score, and the live candidates that carry it"""
    ids, sc = expected_list(scores, top, cand, live)
    if len(ids) < top:
        return 0, 0
    every = np.arange(len(scores), dtype=np.int64) if cand is None else np.asarray(cand, dtype=np.int64)
    if live is not None:
        every = every[live[every]]
    last = score_ord(sc[-1:])[0]
    return int((score_ord(sc) == last).sum()), int((score_ord(np.asarray(scores, dtype=np.float32)[every]) == last).sum())


def check_preconditions(scores, top, planted, cand=None, live=None):
    """A case is worth running if, for every checked query, some tied rows do not fit (the boundary group is larger than the slots left for it) and
    the planted rows a search may return are in the expected list.  scores: [checked queries, n]; planted: per query the offsets."""
    in_list = None if cand is None else set(np.asarray(cand).tolist())
    for c in range(scores.shape[0]):
        slots, members = boundary_group(scores[c], top, cand, live)
        assert members > slots >= 1, (c, slots, members)
        ids, _ = expected_list(scores[c], top, cand, live)
        may = [p for p in planted[c] if (live is None or live[p]) and (in_list is None or p in in_list)]
        assert set(may) <= set(ids.tolist()), (c, may, ids.tolist())


# ---- the storages ---------------------------------------------------------------------------------------------------------------------------------
class Spec:
    """kind: bq | tq | sq | u8 | f16; dist: oracle_ffi distance; dim; bits: BQ query bits (1, 4, 8) or the TQBits code; plus: TurboQuant+ (TQMode::Plus)"""

    def __init__(self, kind, dist, dim, bits=0, plus=False):
        self.kind, self.dist, self.dim, self.bits, self.plus = kind, dist, dim, bits, plus

    def key(self):
        return (self.kind, self.dist, self.dim, self.bits, self.plus)

    def __repr__(self):
        return "%s-%s-%d-%s%s" % (self.kind, {O.DOT: "dot", O.EUCLID: "euclid", O.MANHATTAN: "l1", O.COSINE: "cos"}[self.dist], self.dim, self.bits,
                                   "+" if self.plus else "")


def _seed(spec, n):
    return ({"bq": 1, "tq": 2, "sq": 3, "u8": 4, "f16": 5}[spec.kind] * 1_000_003 + spec.dist * 10_007 + spec.dim * 101 + spec.bits * 13 + (7 if spec.plus else 0)
            + n)


class Base:
    """the N_BASE encoded rows of a storage, its N_CHECKED queries and the oracle's scores of the base"""

    def __init__(self, spec):
        self.spec = spec
        rng = np.random.default_rng(_seed(spec, 0))
        dim, dist = spec.dim, spec.dist
        self.sq_params = self.tq_plus = None
        if spec.kind == "u8":
            self.rows = rng.integers(0, 256, (N_BASE, dim), dtype=np.uint8)
            self.queries = (rng.uniform(0, 255, (N_CHECKED, dim)) * (rng.random((N_CHECKED, dim)) < 0.5)).astype(np.float32)      # (half the coordinates each)
            self.oracle = O.DenseStorage(O.U8, dist, self.rows)
            self.scores = self.oracle.score_points(self.queries, np.arange(N_BASE, dtype=np.uint32))
            return
        if spec.kind == "bq":      # scalar-encoded queries: 15 (255) times as many distinct scores as bits - the block needs the base to tie
            self.rows = rng.integers(0, 256, (N_BASE, dim // 8), dtype=np.uint8)
            self.queries = rng.standard_normal((N_CHECKED, dim)).astype(np.float32)
            self.oracle = O.BqOracle(dist, dim)
            self.oracle.rows = self.rows
            self.scores = self.oracle.score_points_scalar(self.queries, np.arange(N_BASE, dtype=np.uint32), spec.bits)
            return
        vecs = O.preprocess(dist, rng.standard_normal((N_BASE, dim)).astype(np.float32))
        self.queries = rng.standard_normal((N_CHECKED, dim)).astype(np.float32)
        qpre = O.preprocess(dist, self.queries)
        ids = np.arange(N_BASE, dtype=np.uint32)
        if spec.kind == "f16":
            self.rows = O.to_f16(vecs)
            self.oracle = O.DenseStorage(O.F16, dist, self.rows)
            self.scores = self.oracle.score_points(self.queries, ids)
        elif spec.kind == "sq":
            mn, mx = np.float32(vecs.min()), np.float32(vecs.max())                # alpha_offset_from_min_max (ScalarQuantizer.from_min_max)
            self.sq_params = ((mx - mn) / np.float32(127.0), mn)
            self.oracle = O.SqOracle(dist, dim, *self.sq_params)
            self.rows = self.oracle.encode_rows(vecs)
            self.scores = self.oracle.score_points(qpre, ids)
        else:
            assert spec.kind == "tq"
            if spec.plus:
                self.tq_plus = O.tq_plus_fit(dist, dim, spec.bits, vecs[:2048])
                self.oracle = O.TqOracle(dist, dim, spec.bits, shift=self.tq_plus[0], scale=self.tq_plus[1])
            else:
                self.oracle = O.TqOracle(dist, dim, spec.bits)
            self.rows = self.oracle.encode_rows(vecs)
            self.scores = self.oracle.score_points(qpre, ids)
        self.rows = np.ascontiguousarray(self.rows)


_BASES = {}


def base_of(spec):
    if spec.key() not in _BASES:
        _BASES[spec.key()] = Base(spec)
    return _BASES[spec.key()]


class World:
    """One block: rows [n, row bytes], queries [N_CHECKED, dim] (raw f32), scores [N_CHECKED, n] (the oracle's), planted[c] (offsets), and what
    `replant` needs to put copies of a query's best (rank 0) or second best (rank 1) row at further offsets."""

    def __init__(self, spec, n, plant=True):
        self.spec, self.n = spec, n
        rng = np.random.default_rng(_seed(spec, n))
        self.planted = [planted_offsets(n, c) if plant else [] for c in range(N_CHECKED)]
        assert len({p for pl in self.planted for p in pl}) == sum(len(pl) for pl in self.planted)
        if spec.kind == "bq" and spec.bits == 1:
            dim = spec.dim
            self.base = None
            self.oracle = O.BqOracle(spec.dist, dim)
            self.queries = rng.standard_normal((N_CHECKED, dim)).astype(np.float32)
            self.rows = rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)
            code = self.oracle.encode(self.queries)                                 # a query's own one-bit code: no row scores better
            near = code.copy()
            near[:, 0] ^= 1                                                         # ... and one bit away from it: the second best score there is
            self.best = [code, near]
            self.oracle.rows = self.rows
            self.scores = self.oracle.score_points(self.queries, np.arange(n, dtype=np.uint32))
        else:
            self.base = b = base_of(spec)
            self.oracle, self.queries = b.oracle, b.queries
            # per checked query the base rows that carry its two best score VALUES: the lowest of each is what gets planted, none of them is drawn
            best, second, taken = [], [], []
            for c in range(N_CHECKED):
                o = score_ord(b.scores[c])
                v = np.unique(o)[-2:]
                best.append(int(np.flatnonzero(o == v[1])[0]))
                second.append(int(np.flatnonzero(o == v[0])[0]))
                taken.append(np.flatnonzero(o >= v[0]))
            self.best = [np.array(best), np.array(second)]
            assert len(set(best + second)) == 2 * N_CHECKED, "the checked queries' best rows must differ"
            taken = np.unique(np.concatenate(taken))
            self.draw = rng.integers(0, N_BASE, n)
            while True:
                bad = np.isin(self.draw, taken)
                if not bad.any():
                    break
                self.draw[bad] = rng.integers(0, N_BASE, int(bad.sum()))
            self.rows = b.rows[self.draw]
            self.scores = np.ascontiguousarray(b.scores[:, self.draw])
        self._plant([(p, c, 0) for c in range(N_CHECKED) for p in self.planted[c]])
        if plant:
            self.tie_up(TOP)

    def score_rows(self, queries_raw, rows):
        """the oracle's scores of row bytes that need not be in the block (what the block's scores are gathered from)"""
        k, keep = self.spec.kind, getattr(self.oracle, "rows", None)
        if k in ("u8", "f16"):
            return O.DenseStorage(O.U8 if k == "u8" else O.F16, self.spec.dist, rows).score_points(queries_raw, np.arange(len(rows), dtype=np.uint32))
        try:
            self.oracle.rows = np.ascontiguousarray(rows)
            ids = np.arange(len(rows), dtype=np.uint32)
            if k == "bq":
                return self.oracle.score_points(queries_raw, ids) if self.spec.bits == 1 else self.oracle.score_points_scalar(queries_raw, ids, self.spec.bits)
            return self.oracle.score_points(O.preprocess(self.spec.dist, queries_raw), ids)
        finally:
            self.oracle.rows = keep

    def _plant(self, items):
        """items: (offset, checked query, rank)"""
        if not items:
            return
        at = np.array([p for p, _, _ in items])
        if self.base is None:
            new = np.stack([self.best[rank][c] for _, c, rank in items])
            self.rows[at] = new
            self.scores[:, at] = self.score_rows(self.queries, new)
        else:
            src = np.array([self.best[rank][c] for _, c, rank in items])
            self.draw[at] = src
            self.rows[at] = self.base.rows[src]
            self.scores[:, at] = self.base.scores[:, src]

    def _copy(self):
        w = World.__new__(World)
        w.__dict__.update(self.__dict__)
        w.rows, w.scores = self.rows.copy(), self.scores.copy()
        if self.base is not None:
            w.draw = self.draw.copy()
        if self.base is None:
            w.oracle = O.BqOracle(self.spec.dist, self.spec.dim)
            w.oracle.rows = w.rows
        return w

    def replant(self, items):
        """a copy of the world with further planted rows; planted[c] then lists the rank-0 copies"""
        w = self._copy()
        w.planted = [list(pl) + [p for p, c2, rank in items if c2 == c and rank == 0] for c, pl in enumerate(self.planted)]
        w._plant(items)
        return w

    def tie_up(self, top, cand=None, live=None, queries=N_CHECKED):
        """Where a checked query's boundary group happens to fit the slots left for it (a base row drawn less often than the average), copies of the
        group's last row go to further offsets - live ones of the candidate list, behind the prefix, not planted - until the group is 3 larger."""
        rng = np.random.default_rng(self.n + top)
        used = {p for pl in self.planted for p in pl}
        pool = np.arange(self.n) if cand is None else np.unique(cand)
        pool = pool[(pool >= pre_n(self.n) + 64) & (pool < self.n - 64)]
        if live is not None:
            pool = pool[live[pool]]
        for _ in range(2):                                   # (a copy made for one query scores somewhere for the others: look twice)
            for c in range(queries):
                slots, members = boundary_group(self.scores[c], top, cand, live)
                if members > slots or slots == 0:
                    continue
                src = int(expected_list(self.scores[c], top, cand, live)[0][-1])
                for dst in rng.permutation(pool)[:64]:
                    if members >= slots + 3:
                        break
                    dst = int(dst)
                    if dst in used or score_ord(self.scores[c][dst:dst + 1])[0] >= score_ord(self.scores[c][src:src + 1])[0]:
                        continue
                    used.add(dst)
                    self.rows[dst] = self.rows[src]
                    self.scores[:, dst] = self.scores[:, src]
                    if self.base is not None:
                        self.draw[dst] = self.draw[src]
                    members += 1
        return self


_WORLD = {}


def world_of(spec, n):
    """one block at a time is kept (the bases stay)"""
    key = (spec.key(), n)
    if key not in _WORLD:
        _WORLD.clear()
        _WORLD[key] = World(spec, n)
    return _WORLD[key]


# ---- the cases of the GPU module ------------------------------------------------------------------------------------------------------------------
class Case:
    """nq queries (the checked ones, repeated through the batch), the kernel the last scan of the search must be, options to set around the search"""

    def __init__(self, spec, n, nq, kernel, top=TOP, options=()):
        self.spec, self.n, self.nq, self.kernel, self.top, self.options = spec, n, nq, kernel, top, tuple(options)

    def __repr__(self):
        return "%r-n%d-q%d-top%d" % (self.spec, self.n, self.nq, self.top)


def _cases():
    out = []
    D, E, M = O.DOT, O.EUCLID, O.MANHATTAN
    # BQ, SameAsStorage: 2 queries on the generic kernel (no pre-scan), 4 / 16 / 19 on bq_rows_kernel with it (19 = a tile of 16 + a remainder of 3 at qt = 4)
    out += [Case(Spec("bq", D, 128, 1), N_VALU, 2, "scan_kernel<qmx::RowBQ,"), Case(Spec("bq", E, 384, 1), N_VALU, 2, "scan_kernel<qmx::RowBQ,")]
    for dist in (D, E):
        for dim in (128, 384):
            out += [Case(Spec("bq", dist, dim, 1), N_BQROWS, nq, "bq_rows_kernel<%d," % qt) for nq, qt in ((4, 4), (16, 16), (19, 4))]
    out += [Case(Spec("bq", D, 128, 1), N_BQROWS, 16, "bq_rows_kernel<16,", top=64),          # every lane of the wave list in use
            Case(Spec("bq", E, 128, 1), N_BQROWS, 4, "bq_rows_kernel<4,", top=65)]            # two passes: key_bound on pass 1, the pre-scan on pass 0 only
    # BQ, Scalar4bits / Scalar8bits: 2 queries on the bit-plane instantiations of bq_rows_kernel, 5 on the matrix cores with the pre-scan
    for dist, dim, bits in ((D, 128, 4), (E, 384, 8)):
        out += [Case(Spec("bq", dist, dim, bits), N_BQROWS, 2, "bq_rows_kernel<2,"),
                Case(Spec("bq", dist, dim, bits), N_MFMA, 5, "scan_sq_mfma_kernel<qmx::BqOps<%d>" % bits)]
    # TurboQuant: 2 queries launch_scan_tq, 9 the matrix cores at qt = 16 with the pre-scan; 4 bits: 2 queries, and 33 = 32 + a remainder tile of 1
    for dist in (D, E):
        for bits, plus, valu, mfma in ((O.TQ_BITS2, False, "RowTQ2", "TqOps<2,"), (O.TQ_BITS1_5, False, "RowTQ1", "Tq1Ops<1,"),
                                       (O.TQ_BITS1, False, "RowTQ1", "Tq1Ops<1,"), (O.TQ_BITS1, True, "RowTQ1", "Tq1Ops<2,")):
            out += [Case(Spec("tq", dist, 128, bits, plus), N_VALU, 2, "scan_kernel<qmx::" + valu),
                    Case(Spec("tq", dist, 128, bits, plus), N_MFMA, 9, "scan_sq_mfma_kernel<qmx::" + mfma)]
        out += [Case(Spec("tq", dist, 128, O.TQ_BITS4), N_VALU, 2, "scan_kernel<qmx::RowTQ4"),
                Case(Spec("tq", dist, 128, O.TQ_BITS4), N_MFMA, 33, "scan_kernel<qmx::RowTQ4", options=(("tq_wide_min_queries", 0),))]
    # SQ: 9 queries on the matrix cores at qt = 16 (Dot), on launch_scan_sq (Manhattan)
    out += [Case(Spec("sq", D, 64), N_MFMA, 9, "scan_sq_mfma_kernel<qmx::SqOps, 16,"), Case(Spec("sq", M, 64), N_VALU, 9, "scan_kernel<qmx::RowSQ<true,")]
    # u8 and f16 on the generic kernel, f16 Dot from 8 queries on the matrix cores with the pre-scan
    for dist in (D, M):
        out += [Case(Spec("u8", dist, 32), N_VALU, nq, "scan_kernel<qmx::RowU8<") for nq in (3, 16)]
    out += [Case(Spec("f16", D, 64), N_VALU, 3, "scan_kernel<qmx::RowF16<"), Case(Spec("f16", D, 64), N_MFMA, 9, "scan_sq_mfma_kernel<qmx::F16Ops,"),
            Case(Spec("f16", E, 64), N_VALU, 9, "scan_kernel<qmx::RowF16<")]
    return out


CASES = _cases()

# the pre-scan's edge cases and the id lists run on one case per kernel family
EDGE_CASES = [Case(Spec("bq", O.DOT, 128, 1), N_BQROWS, 16, "bq_rows_kernel<16,"),
              Case(Spec("tq", O.DOT, 128, O.TQ_BITS1), N_MFMA, 9, "scan_sq_mfma_kernel<qmx::Tq1Ops<1,"),
              Case(Spec("f16", O.DOT, 64), N_MFMA, 9, "scan_sq_mfma_kernel<qmx::F16Ops,")]
ID_LIST_CASES = EDGE_CASES + [Case(Spec("bq", O.DOT, 128, 1), N_VALU, 2, "scan_kernel<qmx::RowBQ,"), Case(Spec("u8", O.DOT, 32), N_VALU, 3, "scan_kernel<qmx::RowU8<")]
EDGES = ("prefix_deleted", "prefix_top_minus_1_live", "prefix_kth_is_final_kth", "prefix_holds_the_result")


def edge_setup(case, edge):
    """(world, live mask or None, id list or None) of a pre-scan edge case at top = TOP:
    prefix_deleted            every row of the prefix is deleted: the pre-scan finds nothing, there is no bound
    prefix_top_minus_1_live   TOP - 1 rows of the prefix are live: its list does not fill, there is still no bound
    prefix_kth_is_final_kth   an id list, high ids first.  For every checked query the prefix holds 3 copies of its best row and 7 of its second best:
                              the prefix's k-th best score is the second best score.  Behind the prefix: one more copy of the best row, and copies of
                              the second best at higher ids (2, they lose) and at lower ids (5, they belong to the result): the final k-th best score is
                              the prefix's, and rows that tie with the bound must enter
    prefix_holds_the_result   an id list that starts with the expected list of every checked query, the rest in descending order: the prefix's k-th
                              best KEY is the final one - the row that equals the bound must stay"""
    w = world_of(case.spec, case.n)
    n, p = case.n, pre_n(case.n)
    if edge == "prefix_deleted" or edge == "prefix_top_minus_1_live":
        live = np.ones(n, dtype=bool)
        live[:p] = False
        if edge == "prefix_top_minus_1_live":
            keep = [c for c in range(N_CHECKED)] + [p - 1 - c for c in range(N_CHECKED)] + [p // 2]
            assert len(keep) == TOP - 1
            live[keep] = True
        return w._copy().tie_up(TOP, live=live), live, None
    if edge == "prefix_kth_is_final_kth":
        # the list: ids n - 200 - p .. n - 201 descending (the prefix), then n - 200 .. n - 1, then the rest descending
        hi0 = n - 200 - p
        cand = np.concatenate([np.arange(n - 201, hi0 - 1, -1), np.arange(n - 200, n), np.arange(hi0 - 1, -1, -1)])
        assert len(cand) == n and np.array_equal(np.sort(cand), np.arange(n))
        used = {x for pl in w.planted for x in pl}
        items = []
        for c in range(N_CHECKED):
            inside = [hi0 + 100 + 40 * c + j for j in range(10)]                     # ids of the prefix
            higher = [n - 150 + 10 * c + j for j in range(2)]                        # behind it in the list, higher ids
            lower = [100_000 + 40 * c + j for j in range(5)]                         # behind it, lower ids
            assert not (set(inside + higher + lower) & used)
            items += [(x, c, 0) for x in inside[:3]] + [(x, c, 1) for x in inside[3:] + higher + lower]
        # (the block's own planted copies of the best row are taken out of the list: one more copy stays behind the prefix, at offset c)
        drop = {x for c in range(N_CHECKED) for x in w.planted[c] if x != c}
        w2 = w.replant(items)
        cand = cand[~np.isin(cand, list(drop))]
        return w2, None, cand
    assert edge == "prefix_holds_the_result"
    head = np.unique(np.concatenate([expected_list(w.scores[c], TOP)[0] for c in range(N_CHECKED)]))[::-1]
    rest = np.arange(n - 1, -1, -1)
    cand = np.concatenate([head, rest[~np.isin(rest, head)]])
    return w, None, cand


def id_list_of(case):
    """a shuffled list of n ids drawn with repeats (a third of the rows never occur, another third more than once), with every planted row in it and
    the first and the last planted row of every checked query twice"""
    w = world_of(case.spec, case.n)
    rng = np.random.default_rng(case.n + case.nq)
    cand = rng.integers(0, case.n, case.n)
    every = [p for c in range(N_CHECKED) for p in w.planted[c]]
    cand[np.isin(cand, every)] = 5_000                       # (no chance occurrences of the planted rows: the head of the list is what is stated here)
    must = every + [w.planted[c][i] for c in range(N_CHECKED) for i in (0, -1)]
    cand[rng.permutation(case.n)[:len(must)]] = must
    return w._copy().tie_up(TOP, cand=cand), cand


# ---- TurboQuant over Manhattan (tq_l1_scores_device: batches of 65 536 rows) ----------------------------------------------------------------------
L1_SPEC = Spec("tq", O.MANHATTAN, 64, O.TQ_BITS4)
L1_QUERIES = 3


def l1_setup(n):
    """(world, live): query c's best row at the batch edges (moved c rows away from them for c > 0) and at the end of the block, 20 % of the other
    rows deleted"""
    items = [(p, c, 0) for c in range(L1_QUERIES) for p in sorted({65_535 - c, 65_536 + c, 131_071 - c, 131_072 + c, n - 1 - c}) if 0 <= p < n]
    assert len({p for p, _, _ in items}) == len(items)
    w = World(L1_SPEC, n, plant=False).replant(items)
    live = np.random.default_rng(n).random(n) >= 0.2
    live[[p for p, _, _ in items]] = True
    return w.tie_up(TOP, live=live, queries=L1_QUERIES), live
