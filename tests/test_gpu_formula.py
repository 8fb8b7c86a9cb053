"""Formula rescoring on the device (qmx_formula_rescore*, qmx_formula_eval; formula.hip) against the float64 restatement of FormulaScorer and
do_rescore_with_formula in tests/formula_reference.py, over the fixed inputs of tests/formula_cases.py.  Arithmetic-only formulas are compared bit
for bit (f64 on the uint64 view, f32 on the uint32 view, lists id for id).  Formulas with libm nodes too: tests/test_formula_reference.py proves
that none of their reference values lies within 2^-40 relative of an f32 rounding midpoint, and the per-node-kind test below bounds the device's
f64 functions against glibc's by 2^-45, the figure that guard was derived under."""
import ctypes as C

import numpy as np
import pytest

import qdrant_amd as qa
from qdrant_amd import _ffi as F
import formula_reference as FR
import formula_cases as FC

pytestmark = pytest.mark.gpu
SPO = FR.ScoredPointOffset


@pytest.fixture(scope="module")
def cols():
    host = FC.payload()
    dev = FC.device_columns(host)
    yield host, dev
    dev.close()


def _same(got, want, what):
    assert got["idx"].tolist() == want["idx"].tolist(), what
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32)), what


def _check(cols, lists, formula, defaults, limit, threshold=None):
    host, dev = cols
    got = qa.formula_rescore(lists, formula, dev, limit, threshold, defaults)
    assert len(got) == len(lists[0])
    for qi in range(len(got)):
        want = FR.rescore(formula, [src[qi] for src in lists], host, defaults or {}, limit, threshold)
        _same(got[qi], want, qi)
    return got


@pytest.mark.parametrize("n_sources,nq", [(1, 1), (2, 33), (3, 33)])
def test_arithmetic_ragged_counts_heavy_overlap(cols, n_sources, nq):
    lists = FC.lists(n_sources * 131 + nq, n_sources, nq, 60, [FC.POOL])
    assert any(len(l) == 0 for src in lists for l in src) or nq == 1
    for limit in (10, 400):      # below and above the number of distinct ids
        _check(cols, lists, FC.ARITH, FC.ARITH_DEFAULTS, limit)


def test_arithmetic_disjoint_pools_duplicates_and_a_threshold_mid_list(cols):
    pools = [np.arange(s * 400, s * 400 + 300) for s in range(3)]      # disjoint id ranges
    lists = FC.lists(7, 3, 33, 80, pools)
    full = _check(cols, lists, FC.ARITH, FC.ARITH_DEFAULTS, 300)
    _check(cols, lists, FC.ARITH, FC.ARITH_DEFAULTS, 64)
    longest = max(full, key=len)
    threshold = float(longest["score"][len(longest) // 2])             # a score of the list itself: `>=` keeps it
    cut = _check(cols, lists, FC.ARITH, FC.ARITH_DEFAULTS, 300, threshold)
    assert any(0 < len(c) < len(f) for c, f in zip(cut, full))
    dup = FC.lists(8, 3, 33, 50, [np.arange(1000, 1040)], duplicates=True)      # 50 draws of 40 ids: ids repeat inside a list
    assert any(len(set(l["idx"].tolist())) < len(l) for l in dup[0])
    _check(cols, dup, FC.ARITH, FC.ARITH_DEFAULTS, 30)                  # $score[s] is the LAST duplicate's


def test_formula_eval_every_point_bit_for_bit_with_all_presence_states(cols):
    host, dev = cols
    rng = np.random.default_rng(21)
    ids = np.arange(FC.N_POINTS, dtype=np.uint32)
    scores = rng.standard_normal((3, FC.N_POINTS)).astype(np.float32)
    missing = rng.random((3, FC.N_POINTS)) < 0.3
    precise, got, status = qa.formula_eval(FC.ARITH, dev, ids, scores, missing, FC.ARITH_DEFAULTS)
    seen = set()
    for p in ids.tolist():
        maps = [{p: scores[s, p]} if not missing[s, p] else {} for s in range(3)]
        v, st = FR.precise_and_status(FC.ARITH, p, maps, host, FC.ARITH_DEFAULTS)
        assert status[p] == st, p
        seen.add((host["price"].state(p), st))
        if st == 0:
            assert precise[p].view(np.uint64) == np.float64(v).view(np.uint64), p
            assert got[p].view(np.uint32) == np.float32(v).view(np.uint32), p
    assert seen == {(0, 0), (1, 0), (2, FR.BAD_VALUE)}      # absent (the default), present, invalid
    # without a default the absent value is an error of its own, and `scores` may be left out altogether
    _, _, status = qa.formula_eval(qa.payload("price"), dev, ids)
    assert status.tolist() == [[FR.NO_VALUE, 0, FR.BAD_VALUE][host["price"].state(p)] for p in ids.tolist()]
    # past the columns' points: no value, no condition
    _, got, status = qa.formula_eval(qa.sum_(qa.payload("price"), qa.condition("promo")), dev, [FC.N_POINTS, 4_000_000_000], defaults={"price": 3.0})
    assert status.tolist() == [0, 0] and got.tolist() == [3.0, 3.0]


def _error_lists():
    rng = np.random.default_rng(31)
    nq = 33
    planted = {1: FC.NO_GAP[:2], 2: FC.BAD_STRICT, 3: FC.ZERO_A[:1], 4: FC.NEG_B, 5: FC.ZERO_C, 6: FC.HUGE_D, 7: (750, 710)}
    lists = [[], []]
    for qi in range(nq):
        pool = np.arange((qi % 10) * 100, (qi % 10) * 100 + 90)
        for s in range(2):
            l = FC.one_list(rng, 60, pool)
            if s == 1:
                for k, at in enumerate(planted.get(qi % 10, ())):
                    if at not in l["idx"]:
                        l["idx"][len(l) - 1 - k] = at
            lists[s].append(l)
    return lists


def test_error_requests_report_the_lowest_failing_offset_and_leave_the_neighbours_intact(cols):
    host, dev = cols
    lists = _error_lists()
    nq, limit = len(lists[0]), 20
    packed, counts, _, stride = qa.query._pack(lists)
    out = np.zeros((nq, limit), dtype=SPO)
    oc, status, points = (np.full(nq, 77, dtype=np.uint32) for _ in range(3))
    f = qa.CompiledFormula(FC.ERRORS, dev)
    F.check(F.lib().qmx_formula_rescore(f._h, dev._h, F.ptr(packed), F.ptr(counts), 2, nq, stride, limit, None, F.ptr(out), F.ptr(oc), F.ptr(status),
                                        F.ptr(points)))      # the call itself succeeds
    f.close()
    want_codes = {1: (130, FR.NO_VALUE), 2: (250, FR.BAD_VALUE), 3: (333, FR.NON_FINITE), 4: (444, FR.NON_FINITE), 5: (555, FR.NON_FINITE),
                  6: (620, FR.NON_FINITE), 7: (710, FR.NO_VALUE)}      # 710: its missing value comes before its ln(0)
    for qi in range(nq):
        responses = [src[qi] for src in lists]
        if qi % 10 in want_codes:
            with pytest.raises(FR.RequestError) as e:
                FR.rescore(FC.ERRORS, responses, host, {}, limit)
            assert (e.value.point, e.value.code) == want_codes[qi % 10]
            assert (int(points[qi]), int(status[qi]), int(oc[qi])) == (e.value.point, e.value.code, 0), qi
        else:
            assert (int(status[qi]), int(points[qi])) == (0, 0), qi
            _same(out[qi, :oc[qi]], FR.rescore(FC.ERRORS, responses, host, {}, limit), qi)
    with pytest.raises(qa.FormulaError) as e:
        qa.formula_rescore(lists, FC.ERRORS, dev, limit)
    assert (e.value.request, e.value.point, e.value.code) == (1, 130, F.FORMULA_NO_VALUE)
    # the short circuits keep a failing operand from being evaluated: a zero `a` ends the product before ln(a), a zero numerator the quotient
    guarded = qa.sum_(qa.mult(qa.payload("a"), qa.ln(qa.payload("a"))), qa.div(qa.payload("c"), qa.payload("c")), qa.div(qa.const(3.0), qa.payload("c"), 7.5))
    precise, _, st = qa.formula_eval(guarded, dev, [333, 555, 5])
    assert st.tolist() == [0, 0, 0] and precise.tolist() == [0.0 + 1.0 + 1.5, 0.0 + 0.0 + 7.5, 0.0 + 1.0 + 1.5]


@pytest.mark.parametrize("case", FC.LIBM_CASES, ids=lambda c: c[0])
def test_formulas_with_libm_nodes(cols, case):
    name, formula, defaults, seed, n_sources, nq = case
    lists = FC.libm_lists(seed, n_sources, nq)
    for limit in (10, 400):
        _check(cols, lists, formula, defaults, limit)
    cut = _check(cols, lists, formula, defaults, 400, FC.LIBM_THRESHOLD)
    if name == "mix":
        assert any(0 < len(c) < len(set(np.concatenate([src[qi]["idx"] for src in lists]).tolist())) for qi, c in enumerate(cut))


def test_device_f64_functions_against_glibc_per_node_kind(cols, capsys):
    """The guard of the libm comparisons (2^-40) was derived for functions within 2^-45 relative of the host's; this is where that is measured:
    the largest relative difference between qmx_formula_eval's f64 and the restatement's over 2 000 points, per node kind."""
    host, dev = cols
    ids = np.arange(FC.N_POINTS, dtype=np.uint32)
    worst = {}
    for name, formula in FC.NODE_KINDS.items():
        precise, _, status = qa.formula_eval(formula, dev, ids, defaults=FC.LIBM_GEO_DEFAULTS)
        assert not status.any(), name
        want = np.array([FR.eval_expression(formula, p, [], host, FC.LIBM_GEO_DEFAULTS) for p in ids.tolist()])
        worst[name] = float(np.max(np.abs(precise - want) / np.abs(want)))
    with capsys.disabled():
        for name, w in worst.items():
            print("\n  formula f64 vs glibc, %-13s max relative difference %.3e (2^%.1f)" % (name, w, np.log2(w) if w else -np.inf), end="")
        print()
    for name, w in worst.items():
        assert w <= 2.0 ** -45, (name, w)


def test_negative_zero_ties_with_zero_and_keeps_its_bits():
    z = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -0.0, 0.0, 0.0])
    dev = qa.PayloadColumns(len(z), numbers={"z": z})
    ids = np.array([(i, 1.0) for i in (5, 3, 0, 4, 6, 1)], dtype=SPO)
    got = qa.formula_rescore([[ids]], qa.neg(qa.payload("z")), dev, 8)[0]      # OrderedFloat holds -0.0 == 0.0: the offset decides
    assert got["idx"].tolist() == [0, 1, 3, 5, 6, 4]
    assert got["score"].view(np.uint32).tolist() == [0x80000000, 0, 0, 0, 0x80000000, np.float32(-1.0).view(np.uint32)]
    assert [len(l) for l in qa.formula_rescore([[ids]], qa.neg(qa.payload("z")), dev, 8, score_threshold=-0.0)] == [5]
    dev.close()


def test_caps_and_malformed_formulas_are_refused(cols):
    host, dev = cols
    one = np.array([(1, 1.0)], dtype=SPO)
    simple = qa.sum_(qa.score(0), qa.mult(qa.const(0.5), qa.score(1)), qa.payload("rating"))
    for lists, limit in (([[one]] * (F.FUSE_MAX_SOURCES + 1), 10), ([[one]], 65537)):
        with pytest.raises(qa.QmxError) as e:
            qa.formula_rescore(lists, simple, dev, limit, defaults={"rating": 1.0})
        assert e.value.status == F.ERR_NOT_SUPPORTED
    big = np.zeros(F.FUSE_MAX_ENTRIES // 2 + 1, dtype=SPO)
    big["idx"] = np.arange(len(big))
    with pytest.raises(qa.QmxError) as e:
        qa.formula_rescore([[big], [big]], simple, dev, 10, defaults={"rating": 1.0})
    assert e.value.status == F.ERR_NOT_SUPPORTED
    full = big[:F.FUSE_MAX_ENTRIES // 2]      # exactly the cap: 2 x 4096 entries, half of them past the columns' points
    full["score"] = -np.arange(len(full), dtype=np.float32)
    lists = [[full], [full[::-1].copy()]]
    for limit in (100, 5000):
        _check(cols, lists, simple, {"rating": 1.0}, limit)
    # the deepest stack the library takes, and one value more
    def nested(levels):
        e = qa.score(0)
        for _ in range(levels):
            e = qa.div(qa.const(1.0), e)
        return e
    _check(cols, FC.lists(3, 1, 2, 20, [FC.POOL], positive=True), nested(F.FORMULA_MAX_DEPTH - 1), None, 50)
    with pytest.raises(qa.QmxError) as e:
        qa.CompiledFormula(nested(F.FORMULA_MAX_DEPTH), dev)
    assert e.value.status == F.ERR_NOT_SUPPORTED
    with pytest.raises(qa.QmxError) as e:
        qa.formula_rescore([[one]], qa.payload("loc"), dev, 10)      # a geo column read as a number
    assert e.value.status == F.ERR_BAD_ARG
    qa.CompiledFormula(qa.geo_distance((0.0, 0.0), "loc"), dev, defaults={"loc": (1.0, 2.0)}).close()
    bad = F.FormulaDefault()
    bad.is_column, bad.index, bad.kind, bad.value = 1, dev.index["loc"], F.PAYLOAD_NUMBER, 1.0      # a number as the default of a geo column
    n = F.FormulaNode()
    n.op, n.var = F.FORMULA_GEO_DISTANCE, dev.index["loc"]
    assert F.lib().qmx_formula_create(C.byref(n), 1, 0, C.byref(bad), 1, C.byref(C.c_void_p())) == F.ERR_BAD_ARG
    kids = np.array([1, 0], dtype=np.uint32)      # node 0 = sum(node 1), node 1 = neg(node 0): a cycle
    nodes = (F.FormulaNode * 2)()
    nodes[0].op, nodes[0].n_children, nodes[0].children = F.FORMULA_SUM, 1, kids.ctypes.data
    nodes[1].op, nodes[1].n_children, nodes[1].children = F.FORMULA_NEG, 1, kids.ctypes.data + 4
    for root, n_nodes in ((0, 2), (5, 2)):      # ... and a root out of range
        h = C.c_void_p()
        assert F.lib().qmx_formula_create(nodes, n_nodes, root, None, 0, C.byref(h)) == F.ERR_BAD_ARG
        assert "cycle" in F.last_error() or "out of range" in F.last_error()


def _sparse_rows(rng, n, n_dims, nnz):
    rows = []
    for _ in range(n):
        k = int(rng.integers(1, nnz + 1))
        rows.append((rng.choice(n_dims, size=k, replace=False).astype(np.uint32), rng.lognormal(0.0, 1.0, k).astype(np.float32)))
    return rows


def test_hybrid_search_with_a_formula_stage_equals_the_staged_calls(cols):
    import oracle_ffi as O
    host, dev = cols
    rng = np.random.default_rng(77)
    n, dim, nq, top = FC.N_POINTS, 48, 5, 30
    rows = O.preprocess(O.COSINE, O.synth(0xF0, 0, n, dim))
    st = qa.VectorStorage(rows, qa.Distance.Cosine)
    sparse = qa.SparseVectorStorage(_sparse_rows(rng, n, 300, 12))
    queries = O.synth(0xF1, 0, nq, dim)
    sparse_queries = _sparse_rows(rng, nq, 300, 8)
    limits = (60, 100)
    formula = qa.sum_(qa.score(0), qa.mult(qa.const(0.3), qa.score(1), qa.lin_decay(qa.payload("rating"), scale=4.0)), qa.condition("promo"))
    stage = qa.Formula(formula, dev, score_threshold=0.2)
    sources = [(qa.new_raw_scorer(queries, st), limits[0]), (qa.new_raw_scorer(sparse_queries, sparse), limits[1])]
    rescored = qa.hybrid_search(sources, stage, top)
    reranked = qa.hybrid_search(sources, stage, top, mmr=qa.Mmr(qa.new_raw_scorer(queries, st), 0.5, 10))
    # staged: the two searches, then formula_rescore over their lists, then mmr over its lists
    dense_lists = qa.BatchFilteredSearcher(queries, st, limits[0]).peek_top_all()
    sparse_lists = sparse.search(sparse_queries, limits[1])
    staged = qa.formula_rescore([dense_lists, sparse_lists], formula, dev, top, 0.2)
    staged_mmr = qa.mmr(st, queries, staged, 0.5, 10)
    for qi in range(nq):
        assert 0 < len(staged[qi]) <= top
        _same(rescored[qi], staged[qi], qi)
        _same(rescored[qi], FR.rescore(formula, [dense_lists[qi], sparse_lists[qi]], host, {}, top, 0.2), qi)
        _same(reranked[qi], staged_mmr[qi], qi)
    with pytest.raises(qa.FormulaError) as e:      # every point of request 0 fails: the lowest offset of its lists is reported
        qa.hybrid_search(sources, qa.Formula(qa.sqrt(qa.const(-3.0))), top)
    lowest = min(int(dense_lists[0]["idx"].min()), int(sparse_lists[0]["idx"].min()))
    assert (e.value.request, e.value.point, e.value.code) == (0, lowest, F.FORMULA_NON_FINITE)
