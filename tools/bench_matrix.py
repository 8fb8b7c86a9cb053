#!/usr/bin/env python3
"""The distance matrix API (qmx_sample_points + qmx_search_matrix) against the hand-made path a caller had before it.

Data: `--points` x `--dim` f32 cosine rows (the generator of bench.py).  For every S in `--samples` and limit in `--limits`:

  matrix    : qmx_sample_points(S) with the ids left on the device, then qmx_search_matrix(ids, limit) - the wall time of each call.  The sampler is a
              stage of its own; gather, score and finish run inside the second call and are NOT timed one by one: beside the whole call the tool
              reports the device search of the hand-made path over the same ids, which runs the same scans;
  hand-made : qmx_query_create_internal(ids) + qmx_search_topk(top = limit + 1, ids) + the drop of each row's own entry on the host, each part timed.

The two paths alternate call by call; per path the median of `--steps` timed calls after `--warmup`, with min and max as the spread.  The lists of
both paths are compared (ids and score bits) on the last call.  One JSON line on stdout; `--out` also writes it to a file.  Every number in it is
measured on the device the tool ran on."""
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


def stats(times):
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "steps": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--samples", type=int, nargs="+", default=[1000, 8192, 65536])
    ap.add_argument("--limits", type=int, nargs="+", default=[3, 100])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dim = args.points, args.dim
    lib, dev = F.lib(), torch.device("cuda:0")
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    F.check(lib.qmx_synth_fill_f32(0, 0x5EED0019, 0, n, dim, F.ptr(rows)))
    F.check(lib.qmx_preprocess_f32(0, int(qa.Distance.Cosine), F.ptr(rows), n, dim, F.ptr(rows)))
    torch.cuda.synchronize(dev)
    storage = qa.VectorStorage(rows, qa.Distance.Cosine)
    mask = np.arange(n) % 2 == 0      # "under a filter": every second point
    words = qa.scorer._bits_to_words(mask)
    d_words = torch.from_numpy(words.view(np.int64)).to(dev)
    result = {"tool": "bench_matrix", "points": n, "dim": dim, "dtype": "f32", "distance": "cosine", "device": torch.cuda.get_device_name(0),
              "filter": "every second point", "steps": args.steps, "warmup": args.warmup, "cases": []}
    for s in args.samples:
        d_ids = torch.zeros(s, dtype=torch.int32, device=dev)
        count = C.c_uint32(0)

        def sample():
            F.check(lib.qmx_sample_points(storage._h, F.ptr(d_words), n, s, 19, F.ptr(d_ids), C.cast(C.byref(count), C.c_void_p)))

        sample()
        assert count.value == min(s, int(mask.sum()))
        ids = d_ids.cpu().numpy().view(np.uint32).copy()
        for limit in args.limits:
            top = min(limit + 1, s)
            hits = np.zeros((s, limit), dtype=qa.ScoredPointOffset)
            cols = np.zeros((s, limit), dtype=np.uint32)
            counts = np.zeros(s, dtype=np.uint32)
            hand = np.zeros((s, top), dtype=qa.ScoredPointOffset)
            hand_counts = np.zeros(s, dtype=np.uint32)
            hand_lists = [None]
            parts = {}

            def matrix():
                F.check(lib.qmx_search_matrix(storage._h, F.ptr(d_ids), s, limit, F.ptr(hits), F.ptr(cols), F.ptr(counts), None))

            def hand_made():
                t0 = time.perf_counter()
                h = C.c_void_p()
                F.check(lib.qmx_query_create_internal(storage._h, F.ptr(d_ids), s, C.byref(h)))
                t1 = time.perf_counter()
                F.check(lib.qmx_search_topk(h, top, F.ptr(d_ids), s, F.ptr(hand), F.ptr(hand_counts), None, None))
                t2 = time.perf_counter()
                keep = hand["idx"] != ids[:, None]      # the host-side drop: the row's own entry, then the cut
                hand_lists[0] = [hand[i, :hand_counts[i]][keep[i, :hand_counts[i]]][:limit] for i in range(s)]
                t3 = time.perf_counter()
                lib.qmx_query_destroy(h)
                parts.setdefault("create_ms", []).append(1e3 * (t1 - t0))
                parts.setdefault("search_ms", []).append(1e3 * (t2 - t1))
                parts.setdefault("host_drop_ms", []).append(1e3 * (t3 - t2))

            t = {"sample": [], "matrix": [], "hand_made": []}
            for step in range(args.warmup + args.steps):      # the paths alternate call by call
                for name, call in (("sample", sample), ("matrix", matrix), ("hand_made", hand_made)):
                    t0 = time.perf_counter()
                    call()
                    if step >= args.warmup:
                        t[name].append(1e3 * (time.perf_counter() - t0))
            same = all(np.array_equal(hits[i, :counts[i]]["idx"], hand_lists[0][i]["idx"]) and
                       np.array_equal(hits[i, :counts[i]]["score"].view(np.uint32), hand_lists[0][i]["score"].view(np.uint32)) for i in range(s))
            case = {"sample_size": s, "limit": limit, "sample": stats(t["sample"]), "matrix": stats(t["matrix"]), "hand_made": stats(t["hand_made"]),
                    "hand_made_parts_median_ms": {k: round(float(np.median(v[args.warmup:])), 3) for k, v in parts.items()},
                    "matrix_over_hand_made": round(float(np.median(t["matrix"]) / np.median(t["hand_made"])), 3), "same_lists": bool(same)}
            # the stages of the matrix call: `score` is what the scans of the hand-made path took over the same ids (the same kernels; the matrix call
            # scans the gathered block instead of gathering per query tile), `gather_finish_staging` the rest of the call
            case["matrix_stages_ms"] = {"sample": case["sample"]["median_ms"], "whole_call": case["matrix"]["median_ms"],
                                        "hand_made_search_beside_it": case["hand_made_parts_median_ms"]["search_ms"]}
            result["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
