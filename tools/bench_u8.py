#!/usr/bin/env python3
"""The 128-query pass over dense u8 rows (QMX_SEG_U8_WIDE, qdrant_amd/csrc/scan_u8w.hip) against the route the same segment takes without it.

Data: `--points` x `--dim` u8 rows, uniform over 0..255 (torch's generator, seeded), as a segment of each of `--distances` with the per-row columns;
queries: uniform bytes.  Top `--top`, batch sizes `--queries`.  Option u8_wide_min_queries is 1 while measuring, so the wide leg is the wide route at
every batch size.  Per batch size, on one stream with device-resident outputs (qmx_search_topk_async, then one synchronise), ALTERNATING call by call:
  u8_wide : the new route;
  exact   : the same tree with option no_u8_wide = 1 - the exact u8 tiles, 16 queries per pass, which is the route without the flag.
Reported per leg: wall time per batch (median, min, max over `--steps` timed calls after `--warmup`), the counters of the last call, the kernel the
search reports; the lists of the two legs are compared (ids and score bits); and for the new route the scan's own time (event pairs around the scan
launch and the finish of its lists, qmx_query_set_timing, a separate run) as a fraction of `--hbm-gbs` on the bytes the scan streams (rows + streamed
column bytes, once per 128 queries).  One JSON line on stdout; `--out` also writes it to a file."""
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
    ap.add_argument("--queries", default="1,8,16,17,32,64,128,512")
    ap.add_argument("--distances", default="dot,euclid,cosine")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the device's peak HBM rate the scan's fraction is taken of")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dim, top = args.points, args.dim, args.top
    lib, dev = F.lib(), torch.device("cuda:0")
    torch.manual_seed(0x5EED0B21)
    rows = torch.randint(0, 256, (n, dim), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    result = {"tool": "bench_u8", "points": n, "dim": dim, "top": top, "dtype": "u8", "device": torch.cuda.get_device_name(0), "hbm_gbs": args.hbm_gbs,
              "distances": {}}
    stream = torch.cuda.Stream(device=dev)
    qa.set_option("u8_wide_min_queries", 1)
    for dname in [d for d in args.distances.split(",") if d]:
        dist = {"dot": qa.Distance.Dot, "euclid": qa.Distance.Euclid, "cosine": qa.Distance.Cosine}[dname]
        t0 = time.perf_counter()
        storage = qa.VectorStorage(rows, dist, qa.VectorStorageDatatype.Uint8, flags=F.SEG_U8_WIDE)
        info = storage.info()
        col_bytes = 8 if dname == "cosine" else 4
        res = {"derived_copy": info["derived_copy"], "derived_copy_bytes": info["derived_copy_bytes"], "create_s": round(time.perf_counter() - t0, 3), "batches": {}}
        for nq in [int(x) for x in args.queries.split(",") if x]:
            queries = torch.randint(0, 256, (nq, dim), device=dev).float().cpu().numpy()
            scorer = qa.new_raw_scorer(queries, storage)
            F.check(lib.qmx_query_set_stream(scorer._h, F.ptr(int(stream.cuda_stream))))
            out = {k: torch.zeros((nq, top, 2), dtype=torch.int32, device=dev) for k in ("u8_wide", "exact")}
            counts = {k: torch.zeros(nq, dtype=torch.int32, device=dev) for k in out}
            times = {k: [] for k in out}
            legs = {}
            for step in range(args.warmup + args.steps):
                for name, off in (("u8_wide", 0), ("exact", 1)):
                    qa.set_option("no_u8_wide", off)
                    t1 = time.perf_counter()
                    F.check(lib.qmx_search_topk_async(scorer._h, top, None, 0, F.ptr(out[name]), F.ptr(counts[name])))
                    stream.synchronize()
                    if step >= args.warmup:
                        times[name].append(1e3 * (time.perf_counter() - t1))
                    if step == args.warmup + args.steps - 1:
                        legs[name] = leg(times[name], scorer)
            qa.set_option("no_u8_wide", -1)
            same = bool(torch.equal(counts["u8_wide"], counts["exact"]) and torch.equal(out["u8_wide"], out["exact"]))
            # the scan (and the finish of its lists) alone: event pairs around the scan launches of three more calls
            F.check(lib.qmx_query_set_timing(scorer._h, 1))
            for _ in range(3):
                F.check(lib.qmx_search_topk_async(scorer._h, top, None, 0, F.ptr(out["u8_wide"]), F.ptr(counts["u8_wide"])))
                stream.synchronize()
            ms, launches = C.c_float(), C.c_uint32()
            F.check(lib.qmx_query_timing(scorer._h, C.byref(ms), C.byref(launches)))
            F.check(lib.qmx_query_set_timing(scorer._h, 0))
            scan_ms = ms.value / max(launches.value, 1)
            scan_bytes = n * (dim + col_bytes)
            res["batches"][str(nq)] = {"u8_wide": legs["u8_wide"], "exact": legs["exact"], "lists_equal": same,
                                       "exact_over_u8_wide": round(legs["exact"]["median_ms"] / legs["u8_wide"]["median_ms"], 3),
                                       "scan_ms_per_launch": round(scan_ms, 4), "scan_launches_timed": int(launches.value),
                                       "scan_fraction_of_hbm": round(scan_bytes / (scan_ms * 1e-3) / (args.hbm_gbs * 1e9), 3) if scan_ms > 0 else None}
            del scorer
        result["distances"][dname] = res
        del storage
    qa.set_option("u8_wide_min_queries", -1)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
