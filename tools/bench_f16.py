#!/usr/bin/env python3
"""The 128-query pass over dense f16 rows (QMX_SEG_F16_WIDE, qdrant_amd/csrc/scan_f16w.hip) against the same rows in a segment without the flag.

Data: `--points` x `--dim` f16 rows, standard normal (torch's generator, seeded; normalised in f32 before the cast for Cosine), as two segments of each
of `--distances`: one with the flag, one without.  Queries: standard normal.  Top `--top`, batch sizes `--queries`.  Option f16_wide_min_queries is 1
while measuring, so the flagged leg is the wide route at every batch size.  Per batch size, on one stream with device-resident outputs
(qmx_search_topk_async, then one synchronise), ALTERNATING call by call after a warm-up of both:
  f16_wide : the flagged segment;
  exact    : the unflagged one - the exact f16 scans in the device's order.
Reported per leg: wall time per batch (median, min, max over `--steps` timed calls after `--warmup`), the counters of the last call, the kernel the
search reports.  The lists are compared: "ids_equal", or - the exact scans sum in another order - "within_tolerance": every id of one leg that the other
lacks has a score within 1e-5 (relative) of the other leg's last score.  For the flagged leg the scan's own time (event pairs around the scan launch,
qmx_query_set_timing, a separate run of three calls) as a fraction of `--hbm-gbs` on the bytes the scan streams (rows + the column, once per 128
queries).  One JSON line on stdout; `--out` also writes it to a file."""
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

REL = 1e-5


def leg(times, scorer):
    c = scorer.last_counters()
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "steps": len(times),
            "prefilter_queries": int(c.prefilter_queries), "prefilter_candidates": int(c.prefilter_candidates), "verified_rows": int(c.verified_rows),
            "fallback_queries": int(c.fallback_queries), "bytes_read": int(c.bytes_read), "kernel": F.last_kernel(scorer._h).split("(")[0]}


def compare(a, b):
    """(nq, top, 2) int32 lists of (id, score bits) -> "ids_equal" | "within_tolerance" | "differ" """
    a, b = a.cpu().numpy(), b.cpu().numpy()
    if np.array_equal(a[:, :, 0], b[:, :, 0]):
        return "ids_equal"
    for la, lb in zip(a, b):
        sa, sb = la[:, 1].copy().view(np.float32), lb[:, 1].copy().view(np.float32)
        for ids, sc, other_ids, other_last in ((la[:, 0], sa, lb[:, 0], sb[-1]), (lb[:, 0], sb, la[:, 0], sa[-1])):
            odd = ~np.isin(ids, other_ids)
            if np.any(np.abs(sc[odd] - other_last) > REL * abs(other_last)):
                return "differ"
    return "within_tolerance"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", default="1,8,16,32,128")
    ap.add_argument("--distances", default="dot,euclid,cosine")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the device's peak HBM rate the scan's fraction is taken of")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dim, top = args.points, args.dim, args.top
    lib, dev = F.lib(), torch.device("cuda:0")
    torch.manual_seed(0x5EEDF160)
    rows = torch.randn((n, dim), dtype=torch.float16, device=dev)
    torch.cuda.synchronize(dev)
    result = {"tool": "bench_f16", "points": n, "dim": dim, "top": top, "dtype": "f16", "device": torch.cuda.get_device_name(0), "hbm_gbs": args.hbm_gbs,
              "distances": {}}
    stream = torch.cuda.Stream(device=dev)
    qa.set_option("f16_wide_min_queries", 1)
    for dname in [d for d in args.distances.split(",") if d]:
        dist = {"dot": qa.Distance.Dot, "euclid": qa.Distance.Euclid, "cosine": qa.Distance.Cosine}[dname]
        data = rows
        if dname == "cosine":      # normalise in f32, then cast, in slabs
            data = torch.empty_like(rows)
            for i in range(0, n, 1 << 20):
                x = rows[i:i + (1 << 20)].float()
                data[i:i + (1 << 20)] = (x / x.norm(dim=1, keepdim=True)).half()
        t0 = time.perf_counter()
        storages = {"f16_wide": qa.VectorStorage(data, dist, qa.VectorStorageDatatype.Float16, flags=F.SEG_F16_WIDE),
                    "exact": qa.VectorStorage(data, dist, qa.VectorStorageDatatype.Float16)}
        info = storages["f16_wide"].info()
        res = {"derived_copy": info["derived_copy"], "derived_copy_bytes": info["derived_copy_bytes"], "create_s": round(time.perf_counter() - t0, 3), "batches": {}}
        for nq in [int(x) for x in args.queries.split(",") if x]:
            queries = torch.randn((nq, dim), device=dev).cpu().numpy()
            scorers = {k: qa.new_raw_scorer(queries, st) for k, st in storages.items()}
            for sc in scorers.values():
                F.check(lib.qmx_query_set_stream(sc._h, F.ptr(int(stream.cuda_stream))))
            out = {k: torch.zeros((nq, top, 2), dtype=torch.int32, device=dev) for k in scorers}
            counts = {k: torch.zeros(nq, dtype=torch.int32, device=dev) for k in scorers}
            times = {k: [] for k in scorers}
            legs = {}
            for step in range(args.warmup + args.steps):
                for name, sc in scorers.items():
                    t1 = time.perf_counter()
                    F.check(lib.qmx_search_topk_async(sc._h, top, None, 0, F.ptr(out[name]), F.ptr(counts[name])))
                    stream.synchronize()
                    if step >= args.warmup:
                        times[name].append(1e3 * (time.perf_counter() - t1))
                    if step == args.warmup + args.steps - 1:
                        legs[name] = leg(times[name], sc)
            wide = scorers["f16_wide"]
            F.check(lib.qmx_query_set_timing(wide._h, 1))
            for _ in range(3):
                F.check(lib.qmx_search_topk_async(wide._h, top, None, 0, F.ptr(out["f16_wide"]), F.ptr(counts["f16_wide"])))
                stream.synchronize()
            ms, launches = C.c_float(), C.c_uint32()
            F.check(lib.qmx_query_timing(wide._h, C.byref(ms), C.byref(launches)))
            F.check(lib.qmx_query_set_timing(wide._h, 0))
            scan_ms = ms.value / max(launches.value, 1)
            scan_bytes = n * (2 * dim + (4 if dname == "euclid" else 0))
            res["batches"][str(nq)] = {"f16_wide": legs["f16_wide"], "exact": legs["exact"], "lists": compare(out["f16_wide"], out["exact"]),
                                       "exact_over_f16_wide": round(legs["exact"]["median_ms"] / legs["f16_wide"]["median_ms"], 3),
                                       "scan_ms_per_launch": round(scan_ms, 4), "scan_launches_timed": int(launches.value),
                                       "scan_fraction_of_hbm": round(scan_bytes / (scan_ms * 1e-3) / (args.hbm_gbs * 1e9), 3) if scan_ms > 0 else None}
            del scorers, wide
        result["distances"][dname] = res
        del storages, data
    qa.set_option("f16_wide_min_queries", -1)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
