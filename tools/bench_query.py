#!/usr/bin/env python3
"""Hybrid queries on the device against what a caller of the previous C-ABI had to do on the host.

Data: `--points` x `--dim` f32 cosine rows (the generator of bench.py) and the SPLADE-like sparse segment of tools/bench_sparse.py over the same
points.  Per batch size Q:

 (a) fused pipeline: dense search + sparse search (prefetch `--prefetch` each) + fusion to `--top`, all enqueued on one stream and synchronised
     once (qdrant_amd.hybrid_search), against the same two searches returning their lists to the host and the numpy restatement of the fusion
     (tests/fusion_reference.py) there.  `host_search_ms` is the host path's share spent in the two searches and their copies.
 (b) MMR over the dense top-`--mmr-candidates` list, `limit` in `--mmr-limits`: qmx_mmr_select (one launch) against the same selection driven from
     the host, one round per pick: new_raw_scorer_internal over the picks of all requests, score_points_ragged of the remaining candidates, the
     arg-max in numpy.  `model_bytes` = rows the selection has to read (per request and step: the remaining candidates' rows), `effective_gb_per_s`
     = that over the device time.

 (c) `--sparse-mmr` (instead of (a) and (b), on the sparse segment alone): MMR over the sparse top-`--mmr-candidates` list, qmx_sparse_mmr_select
     against the same host-driven selection over the sparse batch (the segment has no dimension map, so new_raw_scorer_internal +
     score_points_ragged give the kernel's bits; the leg asserts the same picks).  `--sparse-mmr-mapped` adds the device time of the same
     selection on the same rows under a random permutation map (the kernel's other instantiation).

 (d) `--formula` (instead of (a) and (b)): the formula stage `$score[0] + 0.3 * $score[1] * gauss_decay(geo_distance) + condition` over the two
     prefetch lists (a geo column and a condition bitmap over the same points) against the RRF fusion of the same lists, in the same process:
     each stage alone on device lists (`stage_ms`: enqueue + one synchronisation, the lists already on the device) and inside the whole pipeline
     (qdrant_amd.hybrid_search: both searches + the stage, `pipeline_ms`).  `formula_over_rrf` = the formula stage as a multiple of the fusion stage.

One JSON line on stdout; `--out` also writes it to a file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime for both)

import qdrant_amd as qa  # noqa: E402
from qdrant_amd import _ffi as F  # noqa: E402
import bench_sparse as BS  # noqa: E402
import fusion_reference as FR  # noqa: E402  (the host side of comparison (a))


def timed(call, warmup, steps):
    for _ in range(warmup):
        call()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(times))


def sparse_queries(gen, cdf, perm, nq, qnnz, dev):
    ql, qd, qw = BS.sample_rows(gen, cdf, perm, nq, qnnz, dev)
    off = np.zeros(nq + 1, dtype=np.uint64)
    off[1:] = np.cumsum(ql.cpu().numpy())
    return off, qd.cpu().numpy().astype(np.uint32), qw.cpu().numpy()


def host_mmr(storage, scorer, cand, lambda_, limit):
    """The selection of maximal_marginal_relevance driven from the host with the entry points the library had before qmx_mmr_select: per pick one
    batch of internal queries (the picks of all requests) and one ragged score_points over every request's remaining candidates.  Candidate
    lists hold distinct ids (a search result)."""
    nq, c = cand.shape
    ids = np.ascontiguousarray(cand["idx"])
    rel = np.stack(scorer.score_points_ragged(list(ids)))
    order = np.tile(np.arange(c), (nq, 1))
    remaining = c
    max_sim = np.zeros((nq, c), dtype=np.float32)
    picks = np.zeros((nq, limit), dtype=np.int64)
    rows = np.arange(nq)
    lam, one_minus = np.float32(lambda_), np.float32(1.0) - np.float32(lambda_)

    def take(scores):      # the last maximal element in the current order, then swap_remove
        pos = remaining - 1 - np.argmax(scores[:, ::-1], axis=1)
        chosen = order[rows, pos]
        order[rows, pos] = order[rows, remaining - 1]
        return chosen

    picks[:, 0] = take(rel[rows[:, None], order[:, :remaining]])
    remaining -= 1
    for step in range(1, min(limit, c)):
        internal = qa.new_raw_scorer_internal(ids[rows, picks[:, step - 1]], storage)
        live = order[:, :remaining]
        sims = np.stack(internal.score_points_ragged(list(ids[rows[:, None], live])))
        internal.close()
        cur = max_sim[rows[:, None], live]
        cur = sims if step == 1 else np.where(sims >= cur, sims, cur)
        max_sim[rows[:, None], live] = cur
        picks[:, step] = take(lam * rel[rows[:, None], live] - one_minus * cur)
        remaining -= 1
    return cand[rows[:, None], picks[:, :min(limit, c)]]


def sparse_segment(args, dev, gen, cdf, perm, dim_map=None):
    n = args.points
    parts = [BS.sample_rows(gen, cdf, perm, min(1_000_000, n - r0), args.nnz, dev) for r0 in range(0, n, 1_000_000)]
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(torch.cat([p[0] for p in parts]), 0)
    sparse = qa.SparseVectorStorage(offsets, torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]), dim_map=dim_map)
    del parts
    torch.cuda.empty_cache()
    return sparse


def sparse_mmr_leg(args, dev):
    """(c): see the module text."""
    lib = F.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    cdf = BS.zipf_cdf(args.sparse_dims, dev)
    perm = torch.randperm(args.sparse_dims, generator=gen, device=dev).to(torch.int64)
    state = gen.get_state()
    sparse = sparse_segment(args, dev, gen, cdf, perm)
    mapped = None
    if args.sparse_mmr_mapped:      # the same rows (the generator rewound) under a random permutation of the dimensions
        gen.set_state(state)
        keys = np.arange(args.sparse_dims, dtype=np.uint32)
        mapped = sparse_segment(args, dev, gen, cdf, perm, dim_map=(keys, np.random.default_rng(args.seed).permutation(keys)))
    qgen = torch.Generator(device=dev)
    qgen.manual_seed(args.seed + 1)
    c = args.mmr_candidates
    results = []
    for nq in [int(x) for x in args.batches.split(",")]:
        queries = sparse_queries(qgen, cdf, perm, nq, args.qnnz, dev)
        sq = qa.new_raw_scorer(queries, sparse)
        mq = qa.new_raw_scorer(queries, mapped) if mapped is not None else None
        cand = np.zeros((nq, c), dtype=qa.ScoredPointOffset)
        ccnt = np.zeros(nq, dtype=np.uint32)
        F.check(lib.qmx_search_topk(sq._h, c, None, 0, F.ptr(cand), F.ptr(ccnt), None, None))
        assert ccnt.min() == c, "a query overlaps fewer than --mmr-candidates points"
        rec = {"queries": nq, "mmr": []}
        for limit in [int(x) for x in args.mmr_limits.split(",")]:
            out = np.zeros((nq, limit), dtype=qa.ScoredPointOffset)
            oc = np.zeros(nq, dtype=np.uint32)

            def device(scorer=sq):
                F.check(lib.qmx_sparse_mmr_select(scorer._h, F.ptr(cand), F.ptr(ccnt), c, args.mmr_lambda, limit, F.ptr(out), F.ptr(oc)))

            dms = timed(device, args.warmup, args.steps)
            kernel = F.last_kernel(sq._h)
            picks = out["idx"].copy()
            want = []

            def host():
                want[:] = [host_mmr(sparse, sq, cand, args.mmr_lambda, limit)]

            hms = timed(host, 0, max(1, args.steps // 2))
            assert np.array_equal(picks, want[0]["idx"]), "device and host-driven selections differ"
            r = {"candidates": c, "limit": limit, "device_ms": round(dms, 3), "host_ms": round(hms, 3), "host_over_device": round(hms / dms, 2),
                 "same_selection": True, "us_per_step": round(1e3 * dms / limit, 1), "kernel": kernel.split("(")[0]}
            if mq is not None:
                r["mapped_device_ms"] = round(timed(lambda: device(mq), args.warmup, args.steps), 3)
                r["mapped_us_per_step"] = round(1e3 * r["mapped_device_ms"] / limit, 1)
                r["mapped_kernel"] = F.last_kernel(mq._h).split("(")[0]
            rec["mmr"].append(r)
        sq.close()
        if mq is not None:
            mq.close()
        results.append(rec)
    return {"tool": "bench_query", "leg": "sparse_mmr", "points": args.points, "sparse_dims": args.sparse_dims, "nnz": args.nnz, "qnnz": args.qnnz,
            "mmr_lambda": args.mmr_lambda, "device": torch.cuda.get_device_name(0), "batches": results}


def formula_leg(args, dev, dense, sparse, qgen, cdf, perm):
    """(d): see the module text."""
    import ctypes as C
    lib = F.lib()
    n = args.points
    rng = np.random.default_rng(args.seed)
    columns = qa.PayloadColumns(n, geo={"location": (rng.uniform(-60.0, 60.0, n), rng.uniform(-170.0, 170.0, n))}, conditions={"promoted": rng.random(n) < 0.2})
    expr = qa.sum_(qa.score(0), qa.mult(qa.const(0.3), qa.score(1), qa.gauss_decay(qa.geo_distance((48.1, 11.5), "location"), scale=5e6)),
                   qa.condition("promoted"))
    stage = qa.Formula(expr, columns)
    stream = torch.cuda.Stream(dev)
    results = []
    for nq in [int(x) for x in args.batches.split(",")]:
        queries = torch.empty((nq, args.dim), dtype=torch.float32, device=dev)
        F.check(lib.qmx_synth_fill_f32(0, args.seed + 2, 0, nq, args.dim, F.ptr(queries)))
        dq = qa.new_raw_scorer(queries.cpu().numpy(), dense)
        sq = qa.new_raw_scorer(sparse_queries(qgen, cdf, perm, nq, args.qnnz, dev), sparse)
        sources = [(dq, args.prefetch), (sq, args.prefetch)]
        rec = {"queries": nq}
        # the two prefetch lists, once, on the device
        lists = torch.zeros((2, nq, args.prefetch), dtype=torch.int64, device=dev)
        counts = torch.zeros((2, nq), dtype=torch.int32, device=dev)
        out = torch.zeros((nq, args.top), dtype=torch.int64, device=dev)
        oc = torch.zeros((3, nq), dtype=torch.int32, device=dev)
        for i, s in enumerate((dq, sq)):
            F.check(lib.qmx_search_topk_async(s._h, args.prefetch, None, 0, F.ptr(lists[i]), F.ptr(counts[i])))
            F.check(lib.qmx_query_synchronize(s._h))
        params, keep = qa.query._fusion_params(F.FUSION_RRF, args.top, 2, None)
        st = C.c_void_p(stream.cuda_stream)

        def rrf_stage():
            F.check(lib.qmx_fuse_topk_async(0, st, F.ptr(lists), F.ptr(counts), 2, nq, args.prefetch, C.byref(params), F.ptr(out), F.ptr(oc[0])))
            stream.synchronize()

        def formula_stage():
            F.check(lib.qmx_formula_rescore_async(stage.compiled._h, columns._h, st, F.ptr(lists), F.ptr(counts), 2, nq, args.prefetch, args.top, None,
                                                  F.ptr(out), F.ptr(oc[0]), F.ptr(oc[1]), F.ptr(oc[2])))
            stream.synchronize()

        reps = max(20, args.steps)
        rrf_ms = timed(rrf_stage, 3, reps)
        formula_ms = timed(formula_stage, 3, reps)
        assert int(oc[1].max()) == 0, "a formula request failed"
        rec["distinct_ids_per_request"] = round(float(np.mean([len(np.unique(lists[:, i].cpu().numpy().view(qa.ScoredPointOffset)["idx"])) for i in range(nq)])), 1)
        rec["rrf"] = {"stage_ms": round(rrf_ms, 4), "pipeline_ms": round(timed(lambda: qa.hybrid_search(sources, qa.Rrf(), args.top), args.warmup, args.steps), 3)}
        rec["formula"] = {"stage_ms": round(formula_ms, 4),
                          "pipeline_ms": round(timed(lambda: qa.hybrid_search(sources, stage, args.top), args.warmup, args.steps), 3)}
        rec["formula_over_rrf"] = round(formula_ms / rrf_ms, 2)
        del keep
        dq.close()
        sq.close()
        results.append(rec)
    return {"tool": "bench_query", "leg": "formula", "points": n, "dim": args.dim, "sparse_dims": args.sparse_dims, "nnz": args.nnz, "qnnz": args.qnnz,
            "prefetch": args.prefetch, "top": args.top, "formula": "$score[0] + 0.3 * $score[1] * gauss_decay(geo_distance, scale 5e6 m) + condition",
            "device": torch.cuda.get_device_name(0), "batches": results}


def emit(record, out):
    line = json.dumps(record)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--sparse-dims", type=int, default=30522)
    ap.add_argument("--nnz", type=int, default=120)
    ap.add_argument("--qnnz", type=int, default=25)
    ap.add_argument("--batches", default="1,32,128")
    ap.add_argument("--prefetch", type=int, default=1000)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--mmr-candidates", type=int, default=1000)
    ap.add_argument("--mmr-limits", default="10,100")
    ap.add_argument("--mmr-lambda", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20241016)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sparse-mmr", action="store_true", help="leg (c) alone: MMR over the sparse top list")
    ap.add_argument("--formula", action="store_true", help="leg (d) alone: the formula stage against the RRF fusion of the same lists")
    ap.add_argument("--sparse-mmr-mapped", action="store_true", help="with --sparse-mmr: also time the same rows under a permutation map (device only)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.sparse_mmr:
        emit(sparse_mmr_leg(args, dev), args.out)
        return
    lib = F.lib()
    n, dim = args.points, args.dim
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    F.check(lib.qmx_synth_fill_f32(0, args.seed, 0, n, dim, F.ptr(rows)))
    F.check(lib.qmx_preprocess_f32(0, int(qa.Distance.Cosine), F.ptr(rows), n, dim, F.ptr(rows)))
    dense = qa.VectorStorage(rows, qa.Distance.Cosine)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    cdf = BS.zipf_cdf(args.sparse_dims, dev)
    perm = torch.randperm(args.sparse_dims, generator=gen, device=dev).to(torch.int64)
    sparse = sparse_segment(args, dev, gen, cdf, perm)
    qgen = torch.Generator(device=dev)
    qgen.manual_seed(args.seed + 1)
    if args.formula:
        emit(formula_leg(args, dev, dense, sparse, qgen, cdf, perm), args.out)
        return
    row_bytes = dim * 4
    results = []
    for nq in [int(x) for x in args.batches.split(",")]:
        queries = torch.empty((nq, dim), dtype=torch.float32, device=dev)
        F.check(lib.qmx_synth_fill_f32(0, args.seed + 2, 0, nq, dim, F.ptr(queries)))
        queries = queries.cpu().numpy()
        dq = qa.new_raw_scorer(queries, dense)
        sq = qa.new_raw_scorer(sparse_queries(qgen, cdf, perm, nq, args.qnnz, dev), sparse)
        rec = {"queries": nq}
        # ---- (a) search + search + fuse ----
        sources = [(dq, args.prefetch), (sq, args.prefetch)]
        d_out = np.zeros((nq, args.prefetch), dtype=qa.ScoredPointOffset)
        s_out = np.zeros((nq, args.prefetch), dtype=qa.ScoredPointOffset)
        d_cnt, s_cnt = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)

        def host_searches():
            F.check(lib.qmx_search_topk(dq._h, args.prefetch, None, 0, F.ptr(d_out), F.ptr(d_cnt), None, None))
            F.check(lib.qmx_search_topk(sq._h, args.prefetch, None, 0, F.ptr(s_out), F.ptr(s_cnt), None, None))
            return [[d_out[i, :d_cnt[i]] for i in range(nq)], [s_out[i, :s_cnt[i]] for i in range(nq)]]

        rec["host_search_ms"] = round(timed(host_searches, args.warmup, args.steps), 3)
        for name, fusion, host_fuse in (("rrf", qa.Rrf(), lambda r: FR.rrf_scoring(r, 2, None, args.top)),
                                        ("dbsf", qa.Dbsf(), lambda r: FR.score_fusion(r, (), args.top))):
            got = []

            def device():
                got[:] = qa.hybrid_search(sources, fusion, args.top)

            def host():
                lists = host_searches()
                return [host_fuse([lists[0][i], lists[1][i]]) for i in range(nq)]

            dms = timed(device, args.warmup, args.steps)
            hms = timed(host, 0, max(1, args.steps // 2))
            want = host()
            same = all(g["idx"].tolist() == w["idx"].tolist() and np.array_equal(g["score"].view(np.uint32), w["score"].view(np.uint32))
                       for g, w in zip(got, want))
            rec[name] = {"device_ms": round(dms, 3), "host_ms": round(hms, 3), "host_over_device": round(hms / dms, 2), "same_lists": bool(same)}
        # ---- (b) MMR over the dense top list ----
        c = args.mmr_candidates
        cand = np.zeros((nq, c), dtype=qa.ScoredPointOffset)
        ccnt = np.zeros(nq, dtype=np.uint32)
        F.check(lib.qmx_search_topk(dq._h, c, None, 0, F.ptr(cand), F.ptr(ccnt), None, None))
        assert ccnt.min() == c
        rec["mmr"] = []
        for limit in [int(x) for x in args.mmr_limits.split(",")]:
            out = np.zeros((nq, limit), dtype=qa.ScoredPointOffset)
            oc = np.zeros(nq, dtype=np.uint32)
            dms = timed(lambda: F.check(lib.qmx_mmr_select(dq._h, F.ptr(cand), F.ptr(ccnt), c, args.mmr_lambda, limit, F.ptr(out), F.ptr(oc))),
                        args.warmup, args.steps)
            kernel = F.last_kernel(dq._h)
            want = []

            def host():
                want[:] = [host_mmr(dense, dq, cand, args.mmr_lambda, limit)]

            hms = timed(host, 0, max(1, args.steps // 2))
            same = bool(np.array_equal(out["idx"], want[0]["idx"]))
            model = nq * sum(c - i for i in range(1, limit)) * row_bytes
            rec["mmr"].append({"candidates": c, "limit": limit, "device_ms": round(dms, 3), "host_ms": round(hms, 3), "host_over_device": round(hms / dms, 2),
                               "same_selection": same, "model_bytes": model, "model_bytes_per_step": nq * c * row_bytes,
                               "effective_gb_per_s": round(model / (dms * 1e-3) / 1e9, 1), "us_per_step": round(1e3 * dms / limit, 1),
                               "kernel": kernel.split("(")[0]})
        dq.close()
        sq.close()
        results.append(rec)
    emit({"tool": "bench_query", "points": n, "dim": dim, "sparse_dims": args.sparse_dims, "nnz": args.nnz, "qnnz": args.qnnz,
          "prefetch": args.prefetch, "top": args.top, "mmr_lambda": args.mmr_lambda, "device": torch.cuda.get_device_name(0),
          "batches": results}, args.out)


if __name__ == "__main__":
    main()
