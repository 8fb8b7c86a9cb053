"""The graphs of the device build, pinned: tiny graphs built one point per launch (max_batch = 1: one wavefront per launch, so the build is
deterministic) hashed over their exported plain arrays and compared with tests/golden/hnsw_build_digests.json, recorded on the device at the
commit the file names.  The main build (every storage, the three beams, lists past one 64-lane pass), the multi-vector build and the payload-block
build (with and without a main graph) each have their cases; a refactor of the insertion kernels or of the host code around them must leave every
digest as it is.

Recording (only when the build's behaviour is meant to change): run this module with QMX_HNSW_DIGESTS_RECORD=<path of a JSON file>; the digests are
written there and nothing is compared.  Without the variable the module only compares."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnsw_build_digests.json")
RECORD = os.environ.get("QMX_HNSW_DIGESTS_RECORD")

N, DELETED = 300, (0, 7, 299)


@pytest.fixture(scope="module")
def qa():
    import qdrant_amd
    assert qdrant_amd.device_count() >= 1
    return qdrant_amd


@functools.lru_cache(maxsize=None)
def _rows(n, dim, seed=1):
    """A mixture of gaussians (no tied f32 scores), seeded."""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((16, dim)).astype(np.float32) * 2.0
    return (centers[rng.integers(0, 16, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.6).astype(np.float32)


def _unit(rows):
    return (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)


def _digest(plain):
    h = hashlib.sha256()
    for arr, dt in ((plain.reindex, np.uint32), (plain.level_offsets, np.uint64), (plain.offsets, np.uint64), (plain.neighbors, np.uint32),
                    (plain.ep_ids, np.uint32), (plain.ep_levels, np.uint32), (plain.xp_ids, np.uint32), (plain.xp_levels, np.uint32)):
        a = np.ascontiguousarray(arr, dtype=dt)
        h.update(np.uint64(len(a)).tobytes())
        h.update(a.astype(a.dtype.newbyteorder("<")).tobytes())
    return h.hexdigest()


def _check(name, plain):
    got = _digest(plain)
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
    """-> (storage, original or None) over n seeded rows of `dim` coordinates."""
    D = qa.Distance
    raw = _rows(n, dim) if rows is None else rows
    if kind == "f32_cosine":
        return qa.VectorStorage(_unit(raw), D.Cosine), None
    if kind == "f32_dot":
        return qa.VectorStorage(raw, D.Dot), None
    if kind == "f16_dot":
        return qa.VectorStorage(raw.astype(np.float16), D.Dot, qa.VectorStorageDatatype.Float16), None
    if kind == "u8_cosine":
        return qa.VectorStorage(np.clip(raw * 20.0 + 128.0, 0, 255).astype(np.uint8), D.Cosine, qa.VectorStorageDatatype.Uint8), None
    if kind == "sq_euclid":
        quant = qa.ScalarQuantizer.from_min_max(raw, dim, D.Euclid)
        return qa.EncodedVectorsU8(quant.encode(raw), quant), None
    if kind == "bq":
        quant = qa.BinaryQuantizer(dim, D.Dot)
        return qa.EncodedVectorsBin(quant.encode(raw), quant), None
    if kind == "pq_dot":
        rng = np.random.default_rng(dim)
        cen = (raw[rng.choice(len(raw), 256, replace=False)] + rng.standard_normal((256, dim)).astype(np.float32) * 0.1).astype(np.float32)
        quant = qa.ProductQuantizer(dim, D.Dot, 4, cen)
        return qa.EncodedVectorsPQ(quant.encode(raw), quant), qa.VectorStorage(raw, D.Dot)
    tq = {"tq4_cosine": (D.Cosine, 0), "tq4_dot": (D.Dot, 0), "tq1_dot": (D.Dot, 3), "tq4_manhattan": (D.Manhattan, 0)}[kind]
    stored = _unit(raw) if tq[0] == D.Cosine else raw
    quant = qa.TurboQuantizer(dim, tq[0], tq[1])
    return qa.EncodedVectorsTQ(quant.encode(stored), quant), qa.VectorStorage(stored, tq[0])


def _deleted(n=N):
    d = np.zeros(n, dtype=bool)
    d[[i for i in DELETED if i < n]] = True
    return d


MAIN_CASES = [
    # name, storage kind, dim, m, m0, ef_construct, option
    ("main_f32_cosine_d33", "f32_cosine", 33, 8, 16, 16, None),              # a row whose last 16-byte piece is partial
    ("main_f16_dot_d40_ef200", "f16_dot", 40, 8, 16, 200, None),             # the 512-entry register beam
    ("main_u8_cosine_d100", "u8_cosine", 100, 8, 16, 16, None),              # the row-norm path
    ("main_sq_euclid_d48", "sq_euclid", 48, 8, 16, 16, None),
    ("main_bq_d128", "bq", 128, 8, 16, 16, None),
    ("main_pq_dot_d64_table_free", "pq_dot", 64, 8, 16, 16, 0),
    ("main_pq_dot_d64_tables", "pq_dot", 64, 8, 16, 16, 1),
    ("main_tq4_cosine_d64", "tq4_cosine", 64, 8, 16, 16, None),
    ("main_tq1_dot_d64", "tq1_dot", 64, 8, 16, 16, None),
    # (48, not 40, coordinates: over Manhattan the build takes rotations over a multiple of 16 coordinates and refuses the others)
    ("main_tq4_manhattan_d48", "tq4_manhattan", 48, 8, 16, 16, None),
    ("main_f32_ef600", "f32_dot", 33, 8, 16, 600, None),                     # the LDS beam
    ("main_f32_m40", "f32_dot", 33, 40, 80, 16, None),                       # lists longer than one 64-lane pass
]


@pytest.mark.parametrize("name,kind,dim,m,m0,efc,pq_tables", MAIN_CASES, ids=[c[0] for c in MAIN_CASES])
def test_main_build_digest(qa, name, kind, dim, m, m0, efc, pq_tables):
    st, original = _storage(qa, kind, dim)
    st.set_deleted(point_deleted=_deleted())
    if pq_tables is not None:
        qa.set_option("hnsw_pq_table_build", pq_tables)
    try:
        g = qa.GraphLayers.build(st, m=m, m0=m0, ef_construct=efc, seed=3, max_batch=1, original=original)
    finally:
        if pq_tables is not None:
            qa.set_option("hnsw_pq_table_build", -1)
    _check(name, g.export_plain())


@pytest.mark.parametrize("kind", ["f32", "pq"])
def test_multivector_build_digest(qa, kind):
    """120 points of 1 to 4 inner rows."""
    n, dim = 120, 64
    rng = np.random.default_rng(9)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(rng.integers(1, 5, n))
    inner = _rows(int(offsets[-1]), dim, seed=2)
    original = None
    if kind == "f32":
        st = qa.MultiDenseVectorStorage(inner, offsets, qa.Distance.Dot)
    else:
        enc, original = _storage(qa, "pq_dot", dim, rows=inner)
        st = qa.QuantizedMultivectorStorage(enc, offsets)
    st.set_deleted(_deleted(n))
    g = qa.GraphLayers.build_multi(st, m=8, m0=16, ef_construct=16, seed=3, max_batch=1, original=original)
    _check("multi_%s" % kind, g.export_plain())


def _blocks(big):
    """Blocks of 1, 2 and `big` points, none in id order; the small ones lie inside the big one, which also lists a deleted point."""
    perm = np.random.default_rng(5).permutation(N)
    perm = perm[~np.isin(perm, DELETED)]
    large = perm[:big - 1].tolist()
    large.insert(40, 7)
    return [np.array([large[3]], dtype=np.uint32), np.array([large[90], large[12]], dtype=np.uint32), np.array(large, dtype=np.uint32)]


PAYLOAD_CASES = [
    # name, storage kind, dim, largest block, payload_m0, ef_construct
    ("payload_f32_dot_d33", "f32_dot", 33, 150, 16, 16),
    ("payload_sq", "sq_euclid", 48, 150, 16, 16),
    ("payload_bq", "bq", 128, 150, 16, 16),
    ("payload_pq", "pq_dot", 64, 150, 16, 16),
    ("payload_tq4", "tq4_dot", 64, 150, 16, 16),
    ("payload_f32_ef600", "f32_dot", 33, 150, 16, 600),
    ("payload_f32_block200_pm80", "f32_dot", 33, 200, 80, 100),            # full rows re-selected across two lane passes
]


@pytest.mark.parametrize("with_main", [False, True], ids=["flat", "merged"])
@pytest.mark.parametrize("name,kind,dim,big,pm0,efc", PAYLOAD_CASES, ids=[c[0] for c in PAYLOAD_CASES])
def test_payload_links_digest(qa, name, kind, dim, big, pm0, efc, with_main):
    st, original = _storage(qa, kind, dim)
    st.set_deleted(point_deleted=_deleted())
    main = qa.GraphLayers.build(st, m=8, m0=16, ef_construct=16, seed=3, max_batch=1, original=original) if with_main else None
    g = qa.GraphLayers.build_payload_links(st, _blocks(big), payload_m0=pm0, ef_construct=efc, max_batch=1, main=main, original=original)
    assert g.payload_info.blocks_built == 3
    _check("%s_%s" % (name, "merged" if with_main else "flat"), g.export_plain())
