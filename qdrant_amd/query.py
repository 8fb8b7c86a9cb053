"""Hybrid queries on the device: fusion of prefetch lists (RRF, DBSF) and MMR re-ranking - the last steps of the reference's Query API
(`rrf_scoring`, `score_fusion`, `mmr_from_points_with_vector`) over lists the dense and sparse searches of this package return.

A list is a numpy array of ScoredPointOffset as the searches return it; `lists[s][qi]` is the list of source s for query qi.  Offsets are point
offsets of one shared id space (the named vectors of a segment share the id tracker)."""
import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _ffi as F
from .scorer import RawScorer, ScoredPointOffset, SparseVectorStorage, VectorStorage, new_raw_scorer


def _pack(lists):
    """[n_sources][nq] lists -> ([n_sources][nq][stride] entries, [n_sources][nq] counts)"""
    n_sources = len(lists)
    nq = len(lists[0]) if n_sources else 0
    if any(len(src) != nq for src in lists):
        raise ValueError("every source needs one list per query")
    stride = max([len(l) for src in lists for l in src] + [1])
    packed = np.zeros((n_sources, nq, stride), dtype=ScoredPointOffset)
    counts = np.zeros((n_sources, nq), dtype=np.uint32)
    for s, src in enumerate(lists):
        for qi, l in enumerate(src):
            packed[s, qi, :len(l)] = l
            counts[s, qi] = len(l)
    return packed, counts, nq, stride


def _fusion_params(kind: int, top: int, k: int, weights):
    p = F.FusionParams()
    p.kind, p.rrf_k, p.top = kind, int(k), int(top)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    p.weights, p.n_weights = (None, 0) if w is None else (w.ctypes.data, len(w))
    return p, w      # (w is kept alive by the caller)


def _fuse(lists, kind, top, k, weights, device_id) -> List[np.ndarray]:
    packed, counts, nq, stride = _pack(lists)
    params, keep = _fusion_params(kind, top, k, weights)
    out = np.zeros((nq, top), dtype=ScoredPointOffset)
    oc = np.zeros(nq, dtype=np.uint32)
    F.check(F.lib().qmx_fuse_topk(device_id, F.ptr(packed), F.ptr(counts), len(lists), nq, stride, C.byref(params), F.ptr(out), F.ptr(oc)))
    del keep
    return [out[i, :oc[i]].copy() for i in range(nq)]


def rrf(lists, top: int, k: int = 2, weights: Optional[Sequence[float]] = None, device_id: int = 0) -> List[np.ndarray]:
    """`rrf_scoring(responses, k, weights)` (reciprocal_rank_fusion.rs:54-99) per query, the best `top` kept: score descending, the lower offset
    first among equal scores.  `weights`: None or one per source (another length raises, as the reference rejects it)."""
    return _fuse(lists, F.FUSION_RRF, top, k, weights, device_id)


def dbsf(lists, top: int, weights: Optional[Sequence[float]] = None, device_id: int = 0) -> List[np.ndarray]:
    """`score_fusion(responses, ScoreFusion::dbsf())` (score_fusion.rs:46-94) per query; missing weights are 1.0."""
    return _fuse(lists, F.FUSION_DBSF, top, 0, weights, device_id)


def _mmr(select, scorer, candidates, lambda_, limit):
    if len(candidates) != scorer.nq:
        raise ValueError("one candidate list per request")
    packed, counts, nq, stride = _pack([candidates])
    out = np.zeros((nq, limit), dtype=ScoredPointOffset)
    oc = np.zeros(nq, dtype=np.uint32)
    F.check(select(scorer._h, F.ptr(packed), F.ptr(counts), stride, float(lambda_), int(limit), F.ptr(out), F.ptr(oc)))
    return [out[i, :oc[i]].copy() for i in range(nq)]


def mmr(storage: VectorStorage, vectors, candidates, lambda_: float, limit: int) -> List[np.ndarray]:
    """`mmr_from_points_with_vector` (shard/src/query/mmr/mod.rs:42-100): request qi re-ranks candidates[qi] (a ScoredPointOffset list over
    `storage`, a dense f32 / f16 / u8 storage) for diversity against `vectors[qi]`; the picked candidates in selection order, input scores kept.
    (Sparse storages: `sparse_mmr`.)"""
    scorer = vectors if isinstance(vectors, RawScorer) else new_raw_scorer(vectors, storage)
    try:
        return _mmr(F.lib().qmx_mmr_select, scorer, candidates, lambda_, limit)
    finally:
        if scorer is not vectors:
            scorer.close()


def sparse_mmr(storage: SparseVectorStorage, vectors, candidates, lambda_: float, limit: int, idf=None) -> List[np.ndarray]:
    """`mmr` over a SparseVectorStorage: `vectors` are the requests' sparse mmr vectors, (indices, values) pairs (or CSR arrays), or a RawScorer
    made over `storage`; `idf` as new_raw_scorer takes it.  Relevance and similarity are `score_vectors` sums in ascending ORIGINAL index order
    (0.0 without a shared dimension), over the stored f32 rows whatever the index weights are."""
    if not isinstance(storage, SparseVectorStorage):
        raise ValueError("sparse_mmr needs a SparseVectorStorage (dense storages: mmr)")
    scorer = vectors if isinstance(vectors, RawScorer) else new_raw_scorer(vectors, storage, idf=idf)
    try:
        return _mmr(F.lib().qmx_sparse_mmr_select, scorer, candidates, lambda_, limit)
    finally:
        if scorer is not vectors:
            scorer.close()


class Rrf:
    """Fusion::Rrf of hybrid_search: `k` and optional per-source weights."""

    def __init__(self, k: int = 2, weights: Optional[Sequence[float]] = None):
        self.kind, self.k, self.weights = F.FUSION_RRF, k, weights


class Dbsf:
    """Fusion::Dbsf of hybrid_search: optional per-source weights."""

    def __init__(self, weights: Optional[Sequence[float]] = None):
        self.kind, self.k, self.weights = F.FUSION_DBSF, 0, weights


class Mmr:
    """The MMR stage of hybrid_search: `scorer` = the Nearest batch of the requests' mmr vectors (new_raw_scorer) over the dense storage, or over
    the SparseVectorStorage when `mmr.using` names the sparse vector."""

    def __init__(self, scorer: RawScorer, lambda_: float, limit: int):
        self.scorer, self.lambda_, self.limit = scorer, float(lambda_), int(limit)


def hybrid_search(sources, fusion, top: int, mmr: Optional[Mmr] = None, device_id: int = 0, sparse_idf=None) -> List[np.ndarray]:
    """One hybrid request batch without a host round trip between its stages.  `sources`: (scorer, prefetch limit) pairs - query batches of the
    same size made by new_raw_scorer over a dense VectorStorage or a SparseVectorStorage on one device; `fusion`: Rrf(...) or Dbsf(...); `mmr`:
    an optional Mmr stage over the fused list.  Every search, the fusion and the MMR selection are enqueued on one stream, which is synchronised
    once.  (All sources search the largest prefetch limit; a source with a smaller one has its counts clamped - a top list's head is the shorter
    top list.)  A sparse source may be given as ((SparseVectorStorage, queries), prefetch limit): its query batch is then made here, with
    `sparse_idf` as the IDF modifier (True, a corpus mask or merged statistics, as SparseVectorStorage.search takes them)."""
    import torch
    if not sources:
        raise ValueError("no sources")
    made = []
    for i, (s, limit) in enumerate(sources):
        if isinstance(s, tuple):
            storage, queries = s
            made.append(new_raw_scorer(queries, storage, idf=sparse_idf))
            sources = list(sources)
            sources[i] = (made[-1], limit)
    if sparse_idf is not None and not made:
        raise ValueError("sparse_idf needs a sparse source given as ((storage, queries), limit)")
    nq = sources[0][0].nq
    if any(s.nq != nq for s, _ in sources) or (mmr is not None and mmr.scorer.nq != nq):
        raise ValueError("every stage needs the same number of queries")
    limits = [int(l) for _, l in sources]
    stride = max(limits)
    dev = torch.device("cuda", device_id)
    stream = torch.cuda.Stream(dev)
    lib = F.lib()
    params, keep = _fusion_params(fusion.kind, top, fusion.k, fusion.weights)
    scorers = [s for s, _ in sources] + ([mmr.scorer] if mmr is not None else [])
    with torch.cuda.stream(stream):
        lists = torch.empty((len(sources), nq, stride), dtype=torch.int64, device=dev)      # ScoredPointOffset entries (8 bytes)
        counts = torch.zeros((len(sources), nq), dtype=torch.int32, device=dev)
        fused = torch.empty((nq, top), dtype=torch.int64, device=dev)
        fcounts = torch.zeros(nq, dtype=torch.int32, device=dev)
        result, rcounts = fused, fcounts
        try:
            for s in scorers:
                F.check(lib.qmx_query_set_stream(s._h, C.c_void_p(stream.cuda_stream)))
            for i, (s, limit) in enumerate(sources):
                F.check(lib.qmx_search_topk_async(s._h, stride, None, 0, F.ptr(lists[i]), F.ptr(counts[i])))
                if limit < stride:
                    counts[i].clamp_(max=limit)
            F.check(lib.qmx_fuse_topk_async(device_id, C.c_void_p(stream.cuda_stream), F.ptr(lists), F.ptr(counts), len(sources), nq, stride,
                                            C.byref(params), F.ptr(fused), F.ptr(fcounts)))
            if mmr is not None:
                result = torch.empty((nq, mmr.limit), dtype=torch.int64, device=dev)
                rcounts = torch.zeros(nq, dtype=torch.int32, device=dev)
                select = lib.qmx_sparse_mmr_select_async if isinstance(mmr.scorer.storage, SparseVectorStorage) else lib.qmx_mmr_select_async
                F.check(select(mmr.scorer._h, F.ptr(fused), F.ptr(fcounts), top, mmr.lambda_, mmr.limit, F.ptr(result), F.ptr(rcounts)))
            out = torch.empty(result.shape, dtype=result.dtype, pin_memory=True)
            oc = torch.empty(rcounts.shape, dtype=rcounts.dtype, pin_memory=True)
            out.copy_(result, non_blocking=True)
            oc.copy_(rcounts, non_blocking=True)
        finally:
            stream.synchronize()      # the one synchronisation of the request batch
            for s in scorers:
                lib.qmx_query_set_stream(s._h, None)
            for s in made:
                s.close()
    del keep
    # (a fused id past the MMR storage's rows empties that request's MMR list; the next synchronous call on mmr.scorer reports it)
    out = out.numpy().view(ScoredPointOffset).reshape(nq, -1)
    oc = oc.numpy()
    return [out[i, :oc[i]].copy() for i in range(nq)]
