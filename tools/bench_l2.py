#!/usr/bin/env python3
"""The Euclid int8 prefilter (QMX_SEG_L2_I8_COPY, qdrant_amd/csrc/scan_l2i8.hip) against the route the same segment takes without it.

Data: `--points` x `--dim` f32 rows (bench.py's generator) as a Euclid segment with the centred int8 copy; queries: stored rows (strided over the block)
plus a tenth of a generated vector - queries distributed like the points, as a Euclid collection's are.  Top `--top`, batch sizes `--queries`.
Per batch size, on one stream with device-resident outputs (qmx_search_topk_async, then one synchronise), ALTERNATING call by call:
  l2_i8 : the new route;
  exact : the same tree with option no_l2_prefilter = 1 - the exact Euclid tiles, which is the route without this copy.
Reported per leg: wall time per batch (median, min, max over `--steps` timed calls after `--warmup`), the counters of the last call, the kernel the
search reports; the lists of the two legs are compared (ids and score bits); and for the new route the scan kernel's own time (event pairs around the
scan launches, qmx_query_set_timing, a separate run) as a fraction of `--hbm-gbs` on the bytes the scan streams (copy + norm column, once per 128 queries).
One JSON line on stdout; `--out` also writes it to a file."""
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


def leg(times, scorer):
    c = scorer.last_counters()
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "steps": len(times),
            "prefilter_queries": int(c.prefilter_queries), "prefilter_candidates": int(c.prefilter_candidates), "verified_rows": int(c.verified_rows),
            "fallback_queries": int(c.fallback_queries), "bytes_read": int(c.bytes_read), "kernel": F.last_kernel(scorer._h).split("(")[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", default="16,64,128,512")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the device's peak HBM rate the scan's fraction is taken of")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dim, top = args.points, args.dim, args.top
    lib, dev = F.lib(), torch.device("cuda:0")
    seed = 0x5EED0021
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    F.check(lib.qmx_synth_fill_f32(0, seed, 0, n, dim, F.ptr(rows)))
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    storage = qa.VectorStorage(rows, qa.Distance.Euclid, flags=F.SEG_L2_I8_COPY)
    info = storage.info()
    result = {"tool": "bench_l2", "points": n, "dim": dim, "top": top, "dtype": "f32", "distance": "euclid", "device": torch.cuda.get_device_name(0),
              "derived_copy": info["derived_copy"], "derived_copy_bytes": info["derived_copy_bytes"], "create_s": round(time.perf_counter() - t0, 3),
              "hbm_gbs": args.hbm_gbs, "batches": {}}
    stream = torch.cuda.Stream(device=dev)
    for nq in [int(x) for x in args.queries.split(",") if x]:
        noise = torch.empty((nq, dim), dtype=torch.float32, device=dev)
        F.check(lib.qmx_synth_fill_f32(0, seed + 1 + nq, 0, nq, dim, F.ptr(noise)))
        queries = (rows[torch.arange(nq, device=dev) * (n // nq) + n // (2 * nq)] + 0.1 * noise).cpu().numpy()
        scorer = qa.new_raw_scorer(queries, storage)
        F.check(lib.qmx_query_set_stream(scorer._h, F.ptr(int(stream.cuda_stream))))
        out = {k: torch.zeros((nq, top, 2), dtype=torch.int32, device=dev) for k in ("l2_i8", "exact")}
        counts = {k: torch.zeros(nq, dtype=torch.int32, device=dev) for k in out}
        times = {k: [] for k in out}
        legs = {}
        for step in range(args.warmup + args.steps):
            for name, off in (("l2_i8", 0), ("exact", 1)):
                qa.set_option("no_l2_prefilter", off)
                t1 = time.perf_counter()
                F.check(lib.qmx_search_topk_async(scorer._h, top, None, 0, F.ptr(out[name]), F.ptr(counts[name])))
                stream.synchronize()
                if step >= args.warmup:
                    times[name].append(1e3 * (time.perf_counter() - t1))
                if step == args.warmup + args.steps - 1:
                    legs[name] = leg(times[name], scorer)
        qa.set_option("no_l2_prefilter", -1)
        same = bool(torch.equal(counts["l2_i8"], counts["exact"]) and torch.equal(out["l2_i8"], out["exact"]))
        # the scan kernel alone: event pairs around the scan launches of three more calls
        F.check(lib.qmx_query_set_timing(scorer._h, 1))
        for _ in range(3):
            F.check(lib.qmx_search_topk_async(scorer._h, top, None, 0, F.ptr(out["l2_i8"]), F.ptr(counts["l2_i8"])))
            stream.synchronize()
        ms, launches = C.c_float(), C.c_uint32()
        F.check(lib.qmx_query_timing(scorer._h, C.byref(ms), C.byref(launches)))
        F.check(lib.qmx_query_set_timing(scorer._h, 0))
        scan_ms = ms.value / max(launches.value, 1)
        scan_bytes = (n + 255) // 256 * 256 * (dim + 4)
        result["batches"][str(nq)] = {"l2_i8": legs["l2_i8"], "exact": legs["exact"], "lists_equal": same,
                                      "exact_over_l2_i8": round(legs["exact"]["median_ms"] / legs["l2_i8"]["median_ms"], 3),
                                      "scan_ms_per_launch": round(scan_ms, 4), "scan_launches_timed": int(launches.value),
                                      "scan_fraction_of_hbm": round(scan_bytes / (scan_ms * 1e-3) / (args.hbm_gbs * 1e9), 3) if scan_ms > 0 else None}
        del scorer
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
