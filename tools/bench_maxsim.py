#!/usr/bin/env python3
"""Brute-force MaxSim over dense f32 multi-vector points: the fused route (qdrant_amd/csrc/maxsim_fused.hip) against the two-step route (the
[tokens][rows] similarity matrix + maxsim_kernel) in ONE process over the SAME storage, option no_maxsim_fused alternating 0 / 1 call by call.

Data: `--rows` x `--dim` standard normal f32 rows (seeded), cut into points of 50 .. 150 rows.  Multi-queries of `--tokens` tokens, batches of
`--queries`.  Two shapes per batch: "rerank" - qmx_multi_search_topk over `--candidates` random points - and "block" - the same call without a
candidate list.  The call is synchronous (it ends with a stream synchronise), so the wall time of a call is device-synchronised; per leg the median,
min and max over `--steps` timed calls after `--warmup` of both legs.  "lists_equal": ids and score bits of the two legs' lists.  One JSON line on
stdout; `--out` also writes it to a file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import qdrant_amd as qa  # noqa: E402
from qdrant_amd import _ffi as F  # noqa: E402
from qdrant_amd.scorer import ScoredPointOffset  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--queries", default="1,16")
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED3A51)
    lens = rng.integers(50, 151, args.rows // 50)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    offsets = offsets[offsets <= args.rows].astype(np.uint64)
    n_points = len(offsets) - 1
    rows = rng.standard_normal((args.rows, args.dim), dtype=np.float32)
    st = qa.MultiDenseVectorStorage(rows, offsets, qa.Distance.Dot)
    ids = np.ascontiguousarray(rng.permutation(n_points)[:args.candidates], dtype=np.uint32)
    lib = F.lib()
    result = {"tool": "bench_maxsim", "rows": args.rows, "dim": args.dim, "points": n_points, "tokens": args.tokens, "candidates": len(ids),
              "candidate_rows": int((offsets[ids.astype(np.int64) + 1] - offsets[ids]).sum()), "top": args.top, "cells": {}}
    for nq in [int(x) for x in args.queries.split(",") if x]:
        scorer, first = st._queries([rng.standard_normal((args.tokens, args.dim), dtype=np.float32) for _ in range(nq)])
        for shape, cand in (("rerank", ids), ("block", None)):
            out = {k: np.zeros((nq, args.top), dtype=ScoredPointOffset) for k in ("fused", "two_step")}
            counts = np.zeros(nq, dtype=np.uint32)
            times = {k: [] for k in out}
            kernels = {}
            for step in range(args.warmup + args.steps):
                for name, off in (("fused", 0), ("two_step", 1)):
                    qa.set_option("no_maxsim_fused", off)
                    t0 = time.perf_counter()
                    F.check(lib.qmx_multi_search_topk(scorer._h, F.ptr(first), nq, F.ptr(offsets), n_points, None, 0, args.top, F.ptr(cand),
                                                      0 if cand is None else len(cand), F.ptr(out[name]), F.ptr(counts)))
                    if step >= args.warmup:
                        times[name].append(1e3 * (time.perf_counter() - t0))
                    kernels[name] = F.last_kernel(scorer._h).split("(")[0]
            qa.set_option("no_maxsim_fused", -1)
            cell = {k: {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "kernel": kernels[k]}
                    for k, t in times.items()}
            cell["lists_equal"] = bool(np.array_equal(out["fused"]["idx"], out["two_step"]["idx"]) and
                                       np.array_equal(out["fused"]["score"].copy().view(np.uint32), out["two_step"]["score"].copy().view(np.uint32)))
            cell["two_step_over_fused"] = round(cell["two_step"]["median_ms"] / cell["fused"]["median_ms"], 3)
            result["cells"]["%s_q%d" % (shape, nq)] = cell
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
