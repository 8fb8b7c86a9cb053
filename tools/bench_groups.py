#!/usr/bin/env python3
"""Grouped search (qmx_group_search) against its floor: qmx_search_topk(top = 64) of the same batch, which is exactly its stage 0.

Data: `--points` x `--dim` f32 cosine rows (the generator of bench.py), `--queries` queries, `limit` groups of `group_size` hits.  Three key layouts:

  singletons : every point its own group.  With group_size 1 (`singletons_size1`) stage 0 finishes every query and the overhead over the floor is the
               aggregate and the final kernel; with a larger group_size no group can ever fill - only the end of the stream says so - and every
               query takes the fallback, where one selection page (no row carries an open group's key) ends it;
  chunks     : `--chunk` consecutive points per document - the 64 best hits open the groups but do not fill them: every query takes the fallback
               (score rows, then selection pages over the rows that still carry an unfilled group's key);
  dominant   : as chunks, and one document owns 1 % of the points, seeded near the queries (its rows are noisy copies of them): stage 0 sees one
               group.

Per layout: wall time per batch (median, min, max over `--steps` timed calls after `--warmup`), the counters of the last call (pages,
fallback_queries, score_passes, kernel_launches) and the ratio to the floor measured in the same process on the same rows.  One JSON line on
stdout; `--out` also writes it to a file."""
import argparse
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


def timed(call, warmup, steps):
    for _ in range(warmup):
        call()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        times.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=128)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--group-size", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dim, nq = args.points, args.dim, args.queries
    lib, dev = F.lib(), torch.device("cuda:0")
    seed = 0x5EED0012
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    F.check(lib.qmx_synth_fill_f32(0, seed, 0, n, dim, F.ptr(rows)))
    queries = torch.empty((nq, dim), dtype=torch.float32, device=dev)
    F.check(lib.qmx_synth_fill_f32(0, seed + 1, 0, nq, dim, F.ptr(queries)))
    # the dominant document: the first 1 % of the points are noisy copies of the queries
    dom = max(n // 100, 1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for r0 in range(0, dom, 1 << 16):
        r1 = min(dom, r0 + (1 << 16))
        src = queries[torch.arange(r0, r1, device=dev) % nq]
        rows[r0:r1] = src + 0.3 * src.norm(dim=1, keepdim=True) / dim ** 0.5 * torch.randn((r1 - r0, dim), device=dev, generator=gen)
    F.check(lib.qmx_preprocess_f32(0, int(qa.Distance.Cosine), F.ptr(rows), n, dim, F.ptr(rows)))
    torch.cuda.synchronize(dev)
    storage = qa.VectorStorage(rows, qa.Distance.Cosine)
    scorer = qa.new_raw_scorer(queries.cpu().numpy(), storage)

    out64 = np.zeros((nq, 64), dtype=qa.ScoredPointOffset)
    cnt64 = np.zeros(nq, dtype=np.uint32)

    def floor():
        F.check(lib.qmx_search_topk(scorer._h, 64, None, 0, F.ptr(out64), F.ptr(cnt64), None, None))

    result = {"tool": "bench_groups", "points": n, "dim": dim, "queries": nq, "limit": args.limit, "group_size": args.group_size, "chunk": args.chunk,
              "dtype": "f32", "distance": "cosine", "device": torch.cuda.get_device_name(0),
              "floor_search_topk_64": timed(floor, args.warmup, args.steps), "layouts": {}}
    floor_ms = result["floor_search_topk_64"]["median_ms"]
    ids = np.arange(n, dtype=np.int64)
    chunks = (ids // args.chunk).astype(np.uint32)
    dominant = chunks.copy()
    dominant[:dom] = 0
    single = ids.astype(np.uint32)
    for name, keys, group_size in (("singletons_size1", single, 1), ("singletons", single, args.group_size), ("chunks", chunks, args.group_size),
                                   ("dominant", dominant, args.group_size)):
        gk = qa.GroupKeys(n, keys)
        counters = F.GroupCounters()
        got = [None]

        def grouped():
            got[0] = qa.search_groups(scorer, None, gk, args.limit, group_size, counters=counters)

        t = timed(grouped, args.warmup, args.steps)
        t.update({"pages": int(counters.pages), "fallback_queries": int(counters.fallback_queries), "score_passes": int(counters.score_passes),
                  "kernel_launches": int(counters.kernel_launches), "fallback_share": round(counters.fallback_queries / nq, 3),
                  "over_floor": round(t["median_ms"] / floor_ms, 3), "overhead_ms": round(t["median_ms"] - floor_ms, 3),
                  "group_size": group_size, "groups_first_query": len(got[0][0]), "hits_first_query": int(sum(len(h) for _, h in got[0][0]))})
        result["layouts"][name] = t
        gk.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
