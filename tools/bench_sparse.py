#!/usr/bin/env python3
"""Sparse-vector Nearest search on the device (qmx_search_topk over a QMX_DTYPE_SPARSE segment) on deterministic SPLADE-like data.

Data (generated on the device with torch, seeded): `--points` rows of about `--nnz` non-zeros over `--dims` dimensions, dimensions drawn from
a Zipf law (p(rank k) ~ 1 / k), duplicates per row dropped, positive log-normal weights; queries of about `--qnnz` non-zeros from the same law.
Reports, per batch size Q: ms per batch and QPS; the posting bytes the batch touches (sum over the queries of len(d) x 8 B for each of their
dimensions d) with their GB/s and the fraction of 8 TB/s; the CSR block size; the segment create time (row checks + the posting transpose).
One JSON line per run on stdout; `--out` also writes it to a file.

`--custom KIND:EXAMPLES` (reco_best, reco_sum, discover, context, feedback; for instance `reco_best:7`, `discover:7`): per batch size Q, Q custom
queries of that many examples each through qmx_sparse_custom_search_topk over the same segment - ms per batch, QPS, the posting bytes of all
examples with their GB/s and fraction of 8 TB/s - and beside them the Nearest search of the same Q x EXAMPLES example vectors as plain queries
(same process, same segment): a custom query of E examples reads the postings E plain queries read.

`--weights f32|f16|u8`: the index weights' datatype (`SparseIndexConfig.datatype`); the record carries the posting layout's bytes (8 / 6 / 5 B per
entry) and the device memory the segment took at create.  Over f16 / u8 weights `--custom` measures the row scan that serves the full scan there.
`--idf`: the queries are created with the IDF modifier (global statistics of the segment), and per batch size the record also times
`qmx_sparse_idf_statistics` for the batch's dimensions under a 50 % corpus mask (the mask resident on the device)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime for both)

import qdrant_amd as qa  # noqa: E402
from qdrant_amd import _ffi as F  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def zipf_cdf(n_dims, dev):
    p = 1.0 / torch.arange(1, n_dims + 1, dtype=torch.float64, device=dev)
    c = torch.cumsum(p, 0)
    return (c / c[-1]).to(torch.float64)


def sample_rows(gen, cdf, perm, n_rows, nnz, dev):
    """CSR (lengths, dims, weights) of n_rows rows: ~nnz Zipf draws each, repeats within a row dropped, dims ascending."""
    n_dims = len(perm)
    lens = torch.randint(nnz - nnz // 4, nnz + nnz // 4 + 1, (n_rows,), generator=gen, device=dev)
    total = int(lens.sum())
    u = torch.rand(total, generator=gen, device=dev, dtype=torch.float64)
    dims = perm[torch.searchsorted(cdf, u).clamp_(max=n_dims - 1)]
    row = torch.repeat_interleave(torch.arange(n_rows, device=dev, dtype=torch.int64), lens)
    key = torch.unique(row * n_dims + dims)      # sorted: by row, then dimension
    row, dims = key // n_dims, (key % n_dims).to(torch.int32)
    lens = torch.bincount(row, minlength=n_rows)
    w = torch.exp(torch.randn(len(dims), generator=gen, device=dev) * 0.75 - 0.5).to(torch.float32)
    return lens, dims, w


CUSTOM_KINDS = {"reco_best": F.CUSTOM_RECO_BEST_SCORE, "reco_sum": F.CUSTOM_RECO_SUM_SCORES, "discover": F.CUSTOM_DISCOVER,
                "context": F.CUSTOM_CONTEXT, "feedback": F.CUSTOM_FEEDBACK}


def custom_descriptors(spec, nq):
    """`KIND:EXAMPLES` -> (descriptors of nq queries over nq x EXAMPLES examples back to back, EXAMPLES, feedback coefficients or None)."""
    name, _, count = spec.partition(":")
    if name not in CUSTOM_KINDS or not count.isdigit() or int(count) < 1:
        raise SystemExit("--custom wants KIND:EXAMPLES with KIND one of %s" % ", ".join(CUSTOM_KINDS))
    kind, ne = CUSTOM_KINDS[name], int(count)
    if kind <= F.CUSTOM_RECO_SUM_SCORES:
        n_a, n_b = (ne + 1) // 2, ne // 2
    elif kind == F.CUSTOM_CONTEXT:
        if ne % 2:
            raise SystemExit("a context query has pairs only: an even number of examples")
        n_a, n_b = 0, ne // 2
    else:
        if ne % 2 == 0:
            raise SystemExit("a %s query has a target and pairs: an odd number of examples" % name)
        n_a, n_b = 1, ne // 2
    descs = (F.CustomQuery * nq)()
    for i in range(nq):
        descs[i].kind, descs[i].first, descs[i].n_a, descs[i].n_b, descs[i].coef_first = kind, i * ne, n_a, n_b, i * (1 + n_b)
    coefs = np.tile(np.array([0.5] + [0.1] * n_b, dtype=np.float32), nq) if kind == F.CUSTOM_FEEDBACK else None
    return descs, ne, coefs


def timed(call, warmup, steps):
    for _ in range(warmup):
        call()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(times))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--dims", type=int, default=30522)
    ap.add_argument("--nnz", type=int, default=120)
    ap.add_argument("--qnnz", type=int, default=25)
    ap.add_argument("--batches", default="1,8,32,128")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20241016)
    ap.add_argument("--custom", default=None, metavar="KIND:EXAMPLES", help="custom queries instead of Nearest, e.g. reco_best:7, discover:7")
    ap.add_argument("--weights", default="f32", choices=["f32", "f16", "u8"], help="datatype of the index weights")
    ap.add_argument("--idf", action="store_true", help="IDF-scaled queries, and time the corpus statistics of each batch's dimensions")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    cdf = zipf_cdf(args.dims, dev)
    perm = torch.randperm(args.dims, generator=gen, device=dev).to(torch.int64)     # Zipf rank -> dimension id
    chunk = 1_000_000
    lens_l, dims_l, w_l = [], [], []
    for r0 in range(0, args.points, chunk):
        lens, dims, w = sample_rows(gen, cdf, perm, min(chunk, args.points - r0), args.nnz, dev)
        lens_l.append(lens)
        dims_l.append(dims)
        w_l.append(w)
    lens = torch.cat(lens_l)
    offsets = torch.zeros(args.points + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    indices = torch.cat(dims_l)
    values = torch.cat(w_l)
    del lens_l, dims_l, w_l
    nnz = int(offsets[-1])
    torch.cuda.synchronize()
    datatype = {"f32": qa.VectorStorageDatatype.Float32, "f16": qa.VectorStorageDatatype.Float16, "u8": qa.VectorStorageDatatype.Uint8}[args.weights]
    entry_bytes = {"f32": 8, "f16": 6, "u8": 5}[args.weights]
    free_before = torch.cuda.mem_get_info(dev)[0]
    t0 = time.perf_counter()
    st = qa.SparseVectorStorage(offsets, indices, values, index_datatype=datatype)
    create_s = time.perf_counter() - t0
    segment_bytes = free_before - torch.cuda.mem_get_info(dev)[0]
    corpus_words = None
    if args.idf:
        mgen = torch.Generator(device=dev)
        mgen.manual_seed(args.seed + 2)
        corpus_words = torch.randint(-2**63, 2**63 - 1, ((args.points + 63) // 64,), generator=mgen, device=dev, dtype=torch.int64)      # ~50 % of the points
    del indices, values
    torch.cuda.empty_cache()
    csr_bytes = nnz * 8 + (args.points + 1) * 8
    qgen = torch.Generator(device=dev)
    qgen.manual_seed(args.seed + 1)
    results = []
    for nq in [int(x) for x in args.batches.split(",")]:
        if args.custom:
            descs, ne, coefs = custom_descriptors(args.custom, nq)
            ql, qd, qw = sample_rows(qgen, cdf, perm, nq * ne, args.qnnz, dev)
            qoff = np.zeros(nq * ne + 1, dtype=np.uint64)
            qoff[1:] = np.cumsum(ql.cpu().numpy())
            qidx = qd.cpu().numpy().astype(np.uint32)
            qval = qw.cpu().numpy()
            h = C.c_void_p()
            F.check(F.lib().qmx_sparse_query_create(st._h, F.ptr(qoff), F.ptr(qidx), F.ptr(qval), nq * ne, C.byref(h)))
            if coefs is not None:
                F.check(F.lib().qmx_custom_set_coefficients(h, F.ptr(coefs), len(coefs)))
            out = np.zeros((nq, args.top), dtype=qa.ScoredPointOffset)
            counts = np.zeros(nq, dtype=np.uint32)
            ctr = F.Counters()
            ms = timed(lambda: F.check(F.lib().qmx_sparse_custom_search_topk(h, descs, nq, args.top, None, 0, F.ptr(out), F.ptr(counts), None,
                                                                             C.byref(ctr))), args.warmup, args.steps)
            # the same example vectors as plain queries: what the fusion is measured against
            nout = np.zeros((nq * ne, args.top), dtype=qa.ScoredPointOffset)
            ncounts = np.zeros(nq * ne, dtype=np.uint32)
            nctr = F.Counters()
            nms = timed(lambda: F.check(F.lib().qmx_search_topk(h, args.top, None, 0, F.ptr(nout), F.ptr(ncounts), None, C.byref(nctr))),
                        args.warmup, args.steps)
            F.lib().qmx_query_destroy(h)
            post_bytes = int(ctr.bytes_read)
            gbs = post_bytes / (ms * 1e-3) / 1e9
            results.append({"queries": nq, "examples_per_query": ne, "ms_per_batch": round(ms, 3), "qps": round(nq / (ms * 1e-3), 1),
                            "posting_bytes": post_bytes, "posting_gb_per_s": round(gbs, 1), "hbm_fraction": round(gbs * 1e9 / HBM_BYTES_PER_S, 4),
                            "mean_results": float(counts.mean()), "nearest_queries": nq * ne, "nearest_ms_per_batch": round(nms, 3),
                            "nearest_posting_bytes": int(nctr.bytes_read), "custom_over_nearest": round(ms / nms, 3)})
            continue
        ql, qd, qw = sample_rows(qgen, cdf, perm, nq, args.qnnz, dev)
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum(ql.cpu().numpy())
        qidx = qd.cpu().numpy().astype(np.uint32)
        qval = qw.cpu().numpy()
        h = C.c_void_p()
        idf_rec = {}
        if args.idf:
            qdims = np.unique(qidx)
            df = np.zeros(len(qdims), dtype=np.uint64)
            n_docs = C.c_uint64(0)
            stat_ms = timed(lambda: F.check(F.lib().qmx_sparse_idf_statistics(st._h, F.ptr(qdims), len(qdims), F.ptr(corpus_words), args.points, F.ptr(df),
                                                                              C.byref(n_docs))), args.warmup, args.steps)
            idf_rec = {"idf_corpus_statistics_ms": round(stat_ms, 3), "idf_dims": len(qdims), "idf_corpus_docs": int(n_docs.value),
                       "idf_corpus_posting_entries": int(df.sum())}
            df, n_docs = st.idf_statistics(qdims)
            F.check(F.lib().qmx_sparse_query_create_idf(st._h, F.ptr(qoff), F.ptr(qidx), F.ptr(qval), nq, F.ptr(qdims), F.ptr(df), len(qdims), n_docs,
                                                        C.byref(h)))
        else:
            F.check(F.lib().qmx_sparse_query_create(st._h, F.ptr(qoff), F.ptr(qidx), F.ptr(qval), nq, C.byref(h)))
        out = np.zeros((nq, args.top), dtype=qa.ScoredPointOffset)
        counts = np.zeros(nq, dtype=np.uint32)
        ctr = F.Counters()
        for _ in range(args.warmup):
            F.check(F.lib().qmx_search_topk(h, args.top, None, 0, F.ptr(out), F.ptr(counts), None, C.byref(ctr)))
        times = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            F.check(F.lib().qmx_search_topk(h, args.top, None, 0, F.ptr(out), F.ptr(counts), None, C.byref(ctr)))
            times.append(time.perf_counter() - t0)
        F.lib().qmx_query_destroy(h)
        ms = 1e3 * float(np.median(times))
        idf_rec["ms_runs"] = [round(1e3 * t, 3) for t in times]
        post_bytes = int(ctr.bytes_read)
        gbs = post_bytes / (ms * 1e-3) / 1e9
        results.append({"queries": nq, "ms_per_batch": round(ms, 3), "qps": round(nq / (ms * 1e-3), 1), "posting_bytes": post_bytes,
                        "posting_gb_per_s": round(gbs, 1), "hbm_fraction": round(gbs * 1e9 / HBM_BYTES_PER_S, 4),
                        "mean_results": float(counts.mean()), **idf_rec})
    rec = {"tool": "bench_sparse", "points": args.points, "dims": args.dims, "nnz": nnz, "mean_row_nnz": round(nnz / args.points, 2),
           "qnnz": args.qnnz, "top": args.top, "csr_bytes": csr_bytes, "weights": args.weights, "idf": bool(args.idf), "posting_layout_bytes": nnz * entry_bytes,
           "segment_device_bytes": int(segment_bytes), "create_s": round(create_s, 3),
           "device": torch.cuda.get_device_name(0), "batches": results}
    if args.custom:
        rec["custom"] = args.custom
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
