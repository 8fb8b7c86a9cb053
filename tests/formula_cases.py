"""The fixed inputs the formula tests share (tests/test_formula_reference.py on the CPU, tests/test_gpu_formula.py on the device): payload columns
over 2 000 points with all three presence states, ragged prefetch lists as the fusion tests draw them, and the formulas.  Every seed is fixed: the
CPU test proves on the reference alone that the formulas with libm nodes produce no fragile value (formula_reference.is_fragile) for these inputs."""
import numpy as np

import qdrant_amd as qa
import formula_reference as FR

SPO = FR.ScoredPointOffset
N_POINTS = 2000
EPOCH = 1_700_000_000_000_000      # datetime micros the `ts` column lies behind

# where the error formula fails: offset -> what is planted there
NO_GAP = (130, 150, 710)           # `gap` has no value (and no default)
BAD_STRICT = (250,)                # `strict` holds an array
ZERO_A = (333, 710, 750)           # ln(0)
NEG_B = (444,)                     # sqrt(-3)
ZERO_C = (555,)                    # 1 / 0
HUGE_D = (620,)                    # 1e45 * 1e-3: a finite f64 beyond f32


def payload():
    """name -> formula_reference.Column"""
    rng = np.random.default_rng(11)
    ids = np.arange(N_POINTS)
    rating = rng.uniform(-3.0, 3.0, N_POINTS)
    rating[ids % 13 == 0] = 0.0
    price_present = np.where(ids < 1500, ids % 4 != 3, ids % 5 >= 2)
    price_invalid = (ids >= 1500) & (ids % 5 == 0)
    cols = {
        "rating": FR.Column("number", rating),
        "pos": FR.Column("number", rng.uniform(0.01, 1000.0, N_POINTS)),
        "price": FR.Column("number", rng.uniform(1.0, 500.0, N_POINTS), present=price_present, invalid=price_invalid),
        "loc": FR.Column("geo", rng.uniform(-60.0, 60.0, N_POINTS), rng.uniform(-170.0, 170.0, N_POINTS), present=ids % 6 != 5),
        "ts": FR.Column("datetime", EPOCH + rng.integers(0, 30_000_000_000_000, N_POINTS), present=ids % 7 != 6),
        "promo": FR.Column("condition", rng.random(N_POINTS) < 0.3),
    }

    def planted(base, at, value):
        v = np.full(N_POINTS, base)
        v[list(at)] = value
        return v
    gap_present = np.ones(N_POINTS, dtype=bool)
    gap_present[list(NO_GAP)] = False
    strict_invalid = np.zeros(N_POINTS, dtype=bool)
    strict_invalid[list(BAD_STRICT)] = True
    cols["gap"] = FR.Column("number", rng.integers(-50, 50, N_POINTS).astype(np.float64), present=gap_present)
    cols["strict"] = FR.Column("number", np.full(N_POINTS, 2.0), invalid=strict_invalid)
    cols["a"] = FR.Column("number", planted(1.0, ZERO_A, 0.0))
    cols["b"] = FR.Column("number", planted(4.0, NEG_B, -3.0))
    cols["c"] = FR.Column("number", planted(2.0, ZERO_C, 0.0))
    cols["d"] = FR.Column("number", planted(1.0, HUGE_D, 1e45))
    return cols


def device_columns(cols):
    """The same columns as a qdrant_amd.PayloadColumns."""
    by_kind = {"number": {}, "geo": {}, "datetime": {}, "condition": {}}
    for name, c in cols.items():
        if c.kind == "condition":
            by_kind["condition"][name] = c.values
        else:
            values = (c.values, c.values2) if c.kind == "geo" else (c.values,)
            by_kind[c.kind][name] = values + (c.present, c.invalid)
    return qa.PayloadColumns(N_POINTS, numbers=by_kind["number"], geo=by_kind["geo"], datetimes=by_kind["datetime"], conditions=by_kind["condition"])


def one_list(rng, count, pool, duplicates=False, positive=False):
    """A list as a search returns it: ids of `pool`, scores descending."""
    ids = rng.choice(pool, size=count, replace=duplicates) if count else np.zeros(0, dtype=np.int64)
    scores = rng.standard_normal(count)
    if positive:
        scores = np.abs(scores) + 0.1
    out = np.zeros(count, dtype=SPO)
    out["idx"], out["score"] = ids, np.sort(scores.astype(np.float32))[::-1]
    return out


def lists(seed, n_sources, nq, stride, pools, duplicates=False, positive=False):
    """Ragged lists [n_sources][nq]: every count in 0..stride, with an empty list, a one-entry list and a full list planted."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n_sources):
        src = []
        for qi in range(nq):
            pool = pools[s % len(pools)]
            count = int(rng.integers(0, min(stride, len(pool)) + 1))
            if (qi + s) % 7 == 3:
                count = 0
            elif (qi + s) % 7 == 1:
                count = 1
            elif (qi + s) % 7 == 2:
                count = min(stride, len(pool))
            src.append(one_list(rng, count, pool, duplicates, positive))
        out.append(src)
    return out


POOL = np.arange(1000, 1090)      # 90 ids for up to 3 x 60 entries: nearly every id in several lists; `price` is present or absent here, never invalid

# arithmetic only: every step is one correctly rounded IEEE operation on both sides
ARITH = qa.sum_(
    qa.score(0),
    qa.mult(qa.const(0.3), qa.score(1), qa.payload("rating")),                     # a zero rating ends the product at once
    qa.condition("promo"),
    qa.div(qa.payload("price"), qa.const(7.0)),
    qa.neg(qa.abs_(qa.payload("rating"))),
    qa.sqrt(qa.abs_(qa.score(2))),
    qa.lin_decay(qa.payload("price"), target=qa.const(100.0), midpoint=0.5, scale=200.0),
    qa.div(qa.sum_(qa.datetime("ts"), qa.neg(qa.datetime(EPOCH))), qa.const(86400.0)),
    qa.div(qa.score(0), qa.payload("rating"), by_zero_default=2.5),
)
ARITH_DEFAULTS = {"price": 10.0, "ts": EPOCH + 123_456_789, ("score", 1): -0.25}

# the six planted failures; clean points score gap + 2 + 0 + 2 + 0.5 + 0.001 + $score[0], exactly on both sides (ln(1.0) is 0.0 in any libm)
ERRORS = qa.sum_(qa.payload("gap"), qa.payload("strict"), qa.ln(qa.payload("a")), qa.sqrt(qa.payload("b")), qa.div(qa.const(1.0), qa.payload("c")),
                 qa.mult(qa.payload("d"), qa.const(1e-3)), qa.score(0))

# libm nodes; scores are drawn positive and every term is positive, so nothing cancels
LIBM_GEO = qa.sum_(qa.score(0), qa.mult(qa.const(0.3), qa.score(1), qa.gauss_decay(qa.geo_distance((48.1, 11.5), "loc"), scale=5e6)),
                   qa.condition("promo"))
LIBM_GEO_DEFAULTS = {"loc": (40.0, -3.0), ("score", 1): 0.75}      # (without it a point outside list 1 scores $score[0] + 0 or 1 exactly: often an exact f32 tie)
LIBM_MIX = qa.sum_(
    qa.exp(qa.div(qa.score(0), qa.const(4.0))),
    qa.ln(qa.sum_(qa.const(1.5), qa.abs_(qa.score(1)))),
    qa.log10(qa.sum_(qa.const(2.0), qa.payload("price"))),
    qa.pow_(qa.sum_(qa.const(1.1), qa.abs_(qa.payload("rating"))), qa.const(1.7)),
    qa.exp_decay(qa.payload("price"), target=qa.const(50.0), midpoint=0.3, scale=120.0),
)
LIBM_MIX_DEFAULTS = {"price": 10.0}
LIBM_THRESHOLD = 5.0

# (name, formula, defaults, seed, n_sources, nq): the requests of the libm comparisons
LIBM_CASES = [
    ("geo", LIBM_GEO, LIBM_GEO_DEFAULTS, 501, 2, 33),
    ("mix", LIBM_MIX, LIBM_MIX_DEFAULTS, 502, 2, 33),
    ("mix-one", LIBM_MIX, LIBM_MIX_DEFAULTS, 503, 1, 1),
]


def libm_lists(seed, n_sources, nq):
    return lists(seed, n_sources, nq, 60, [POOL], positive=True)


# one node kind each, evaluated over every point: where the device's f64 functions are measured against glibc's
NODE_KINDS = {
    "exp": qa.exp(qa.payload("rating")),
    "ln": qa.ln(qa.payload("pos")),
    "log10": qa.log10(qa.payload("pos")),
    "pow": qa.pow_(qa.payload("pos"), qa.payload("rating")),
    "gauss_decay": qa.gauss_decay(qa.payload("rating"), scale=1.5),
    "exp_decay": qa.exp_decay(qa.payload("rating"), midpoint=0.3, scale=2.0),
    "geo_distance": qa.geo_distance((48.1, 11.5), "loc"),
}
