"""Pure-Python float64 restatement of the reference's formula rescoring:

  FormulaScorer::score, eval_expression, the three decay bodies    lib/segment/src/index/query_optimization/rescore_formula/formula_scorer.rs:76-343
  decay_params_to_lambda                                           .../rescore_formula/parsed_formula.rs:186-224
  do_rescore_with_formula                                          lib/segment/src/segment/read_view/formula_rescore.rs:29-104
  Haversine.distance                                               the geo crate, as formula_scorer.rs:130 calls it

A Python float IS an IEEE f64 and every +, *, / and math.sqrt one correctly rounded operation; math.exp / log / log10 / pow / sin / cos / asin are
glibc's, the libm the reference's f64 methods reach on Linux.  Results are cast with np.float32.

An expression is a tree of tuples, (op, ...), the form qdrant_amd's builders produce:
  ("const", c) ("score", i) ("payload", name) ("condition", name) ("geo_distance", (lat, lon), name) ("datetime", micros) ("datetime_key", name)
  ("sum", [..]) ("mult", [..]) ("div", left, right, by_zero_default | None) ("neg", x) ("sqrt", x) ("pow", base, exponent) ("exp", x) ("log10", x)
  ("ln", x) ("abs", x) ("decay", "lin" | "gauss" | "exp", x, target | None, lambda)

Payload is a dict name -> Column; a point's value in a column is absent, one value, or `invalid` (a value of the wrong type, or several values:
what `get_payload_value` hands on as something `from_value` rejects).  Defaults: {("score", i) | name: number | (lat, lon) | datetime micros}.
The reference reports "whichever point's error the hash order met last"; the rule restated here is the project's: the first error in evaluation
order of the LOWEST failing offset.  Checker only: nothing under qdrant_amd/ imports this file."""
import math

import numpy as np

ScoredPointOffset = np.dtype([("idx", np.uint32), ("score", np.float32)])
NON_FINITE, NO_VALUE, BAD_VALUE = 1, 2, 3      # qmx_formula_status
MEAN_EARTH_RADIUS = 6371008.8


class EvalError(Exception):
    """OperationError::NonFiniteNumber (NON_FINITE) or VariableTypeError (NO_VALUE: nothing in payload nor defaults; BAD_VALUE: wrong type)."""

    def __init__(self, code):
        super().__init__(code)
        self.code = code


class RequestError(Exception):
    def __init__(self, point, code):
        super().__init__(point, code)
        self.point, self.code = point, code


class Column:
    """kind "number" (values), "geo" (values = lat, values2 = lon), "datetime" (values = int micros) or "condition" (values = bool per point);
    present (None = all) / invalid (None = none): bool per point."""

    def __init__(self, kind, values, values2=None, present=None, invalid=None):
        self.kind, self.values, self.values2, self.present, self.invalid = kind, values, values2, present, invalid

    def state(self, point):
        """0 = no value, 1 = one value, 2 = invalid"""
        if point >= len(self.values):
            return 0
        if self.invalid is not None and self.invalid[point]:
            return 2
        return 1 if self.present is None or self.present[point] else 0


def _libm(fn, *args):
    try:
        return fn(*args)
    except ValueError:          # a domain error: NaN or an infinity, either way not finite
        return math.nan
    except OverflowError:
        return math.inf


def _checked(v):
    if not math.isfinite(v):
        raise EvalError(NON_FINITE)
    return v


def haversine(lat1, lon1, lat2, lon2):
    """geo's Haversine.distance over f64: to_radians is x * (PI / 180.0), powi(2) a product."""
    to_rad = math.pi / 180.0
    theta1, theta2 = lat1 * to_rad, lat2 * to_rad
    delta_theta, delta_lambda = (lat2 - lat1) * to_rad, (lon2 - lon1) * to_rad
    st, sl = math.sin(delta_theta / 2.0), math.sin(delta_lambda / 2.0)
    a = st * st + math.cos(theta1) * math.cos(theta2) * (sl * sl)
    return MEAN_EARTH_RADIUS * (2.0 * math.asin(math.sqrt(a)))


def decay_params_to_lambda(kind, midpoint=None, scale=None):
    """parsed_formula.rs:186-224: midpoint / scale are f32 (DEFAULT_DECAY_MIDPOINT 0.5, DEFAULT_DECAY_SCALE 1.0) widened to f64."""
    midpoint = float(np.float32(0.5 if midpoint is None else midpoint))
    scale = float(np.float32(1.0 if scale is None else scale))
    if kind == "lin":
        if not (0.0 <= midpoint <= 1.0):
            raise ValueError("Linear decay midpoint should be in the range [0.0, 1.0]")
    elif not (midpoint > 0.0 and midpoint < 1.0):
        raise ValueError("Decay midpoint should be in the range (0.0, 1.0)")
    if scale <= 0.0:
        raise ValueError("Decay scale should be non-zero positive")
    if kind == "lin":
        return (1.0 - midpoint) / scale
    if kind == "exp":
        return math.log(midpoint) / scale
    return math.log(midpoint) / (scale * scale)


def _payload_value(name, point, payload, defaults, kind):
    """get_parsed_payload_value: the point's value, else the default, else NO_VALUE; a value `from_value` rejects: BAD_VALUE."""
    col = payload.get(name)
    state = col.state(point) if col is not None else 0
    if state == 2 or (state == 1 and col.kind != kind):
        raise EvalError(BAD_VALUE)
    if state == 1:
        return (col.values[point], col.values2[point]) if kind == "geo" else col.values[point]
    if name not in defaults:
        raise EvalError(NO_VALUE)
    return defaults[name]


def eval_expression(e, point, scores, payload, defaults):
    """formula_scorer.rs:92-282.  scores: one {offset: f32 score} dict per prefetch."""
    op = e[0]
    ev = lambda x: eval_expression(x, point, scores, payload, defaults)      # noqa: E731
    if op == "const":
        return float(e[1])
    if op == "score":
        if e[1] < len(scores) and point in scores[e[1]]:
            return float(scores[e[1]][point])
        return float(defaults.get(("score", e[1]), 0.0))
    if op == "payload":
        return float(_payload_value(e[1], point, payload, defaults, "number"))
    if op == "condition":
        col = payload[e[1]]
        return 1.0 if point < len(col.values) and col.values[point] else 0.0
    if op == "geo_distance":
        lat, lon = _payload_value(e[2], point, payload, defaults, "geo")
        return haversine(e[1][0], e[1][1], float(lat), float(lon))
    if op in ("datetime", "datetime_key"):
        micros = e[1] if op == "datetime" else _payload_value(e[1], point, payload, defaults, "datetime")
        return float(int(micros)) / 1_000_000.0
    if op == "mult":
        product = 1.0
        for x in e[1]:
            value = ev(x)
            if value == 0.0:
                return 0.0
            product *= value
        return product
    if op == "sum":
        acc = 0.0
        for x in e[1]:
            acc = acc + ev(x)
        return acc
    if op == "div":
        left = ev(e[1])
        if left == 0.0:
            return 0.0
        right = ev(e[2])
        if right == 0.0 and e[3] is not None:
            return float(e[3])
        if right == 0.0:
            raise EvalError(NON_FINITE)          # left / 0.0 with left != 0.0: an infinity, or NaN
        return _checked(left / right)
    if op == "neg":
        return -ev(e[1])
    if op == "abs":
        return abs(ev(e[1]))
    if op == "sqrt":
        return _checked(_libm(math.sqrt, ev(e[1])))
    if op == "pow":
        base = ev(e[1])
        return _checked(_libm(math.pow, base, ev(e[2])))
    if op == "exp":
        return _checked(_libm(math.exp, ev(e[1])))
    if op == "log10":
        return _checked(_libm(math.log10, ev(e[1])))
    if op == "ln":
        return _checked(_libm(math.log, ev(e[1])))
    if op == "decay":
        kind, lam = e[1], e[4]
        x = ev(e[2])
        target = ev(e[3]) if e[3] is not None else 0.0
        if kind == "exp":
            return _libm(math.exp, lam * abs(x - target))
        if kind == "gauss":
            diff = x - target
            return _libm(math.exp, lam * diff * diff)
        value = -lam * abs(x - target) + 1.0
        return value if value > 0.0 else 0.0          # f64::max(0.0): NaN gives 0.0 as well
    raise ValueError("unknown op %r" % (op,))


def cast(v):
    """FormulaScorer::score's `as f32`, which must be finite."""
    with np.errstate(all="ignore"):
        s = np.float32(v)
    if not np.isfinite(s):
        raise EvalError(NON_FINITE)
    return s


def score(e, point, scores, payload, defaults):
    return cast(eval_expression(e, point, scores, payload, defaults))


def precise_and_status(e, point, scores, payload, defaults):
    """(f64 value or None, status) of one point - what qmx_formula_eval reports."""
    try:
        v = eval_expression(e, point, scores, payload, defaults)
    except EvalError as err:
        return None, err.code
    try:
        cast(v)
    except EvalError as err:
        return v, err.code
    return v, 0


def prefetch_maps(responses):
    """`collect::<AHashMap>`: one map per prefetch, a repeated id keeps its LAST score."""
    return [{int(i): np.float32(s) for i, s in zip(r["idx"].tolist(), r["score"])} for r in responses]


def _of_key(x):
    return (1, 0.0) if np.isnan(x) else (0, float(x))


def rescore(e, responses, payload, defaults, limit, score_threshold=None):
    """formula_rescore.rs:29-104 for one request; RequestError(lowest failing offset, its first error) where the reference returns Err."""
    scores = prefetch_maps(responses)
    points = sorted(set().union(*[set(m) for m in scores])) if scores else []
    kept = []
    for p in points:
        try:
            s = score(e, p, scores, payload, defaults)
        except EvalError as err:
            raise RequestError(p, err.code)
        if score_threshold is None or s >= np.float32(score_threshold):
            kept.append((p, s))
    kept.sort(key=lambda ps: (tuple(-c for c in _of_key(ps[1])), ps[0]))
    out = np.zeros(min(limit, len(kept)), dtype=ScoredPointOffset)
    for i, (p, s) in enumerate(kept[:limit]):
        out[i] = (p, s)
    return out


def is_fragile(v, guard=2.0 ** -40):
    """Whether the f64 value v lies within |v| * guard of an f32 rounding midpoint: there a last-bits difference in v can change its f32 cast."""
    with np.errstate(all="ignore"):
        f = np.float32(v)
    if not np.isfinite(f):
        return True
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    dist = min(abs(v - (float(f) + float(lo)) / 2.0), abs(v - (float(f) + float(hi)) / 2.0))
    return dist <= abs(v) * guard
