#!/usr/bin/env python3
"""Per-request payload filters (qmx_query_set_filters) against the only way to serve such a batch without them: one batch per distinct filter.

Data: `--points` x `--dim` f32 cosine rows with the int8 copy (the generator and the segment of bench.py), `--queries` queries, top `--top`.
Tenants: point i belongs to tenant hash(i) % F (a multiplicative hash: tenants are scattered over the block, as ids of a shared collection are - with
i % F the strided sample of the prefilter would see the rows of a few tenants only), request j to tenant j % F - each tenant owns 1 / F of the points
and `queries / F` requests of the batch.
Settings: F in `--tenants` (1, 8, 128), and `mixed`: F = 8 with every second request unfiltered (QMX_FILTER_NONE).

Per setting, on ONE stream and with device-resident outputs (qmx_search_topk_async, then one synchronise):
  per_request : one call over the whole batch under qmx_query_set_filters;
  split       : F batches of queries / F requests, each under qmx_query_set_filter of its tenant, enqueued back to back (the mixed setting: a ninth
                batch without a filter);
and once for all settings `unfiltered`: the whole batch without any filter.  Reported per leg: wall time per batch (median, min, max over `--steps`
timed repetitions after `--warmup`), fallback_queries and verified_rows of the last repetition (summed over the batches of the split leg), and the
ratios split / per_request and per_request / unfiltered.  The lists of the two legs are compared once per setting (ids and score bits).
One JSON line on stdout; `--out` also writes it to a file."""
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


def tenant_bitmaps(n, n_tenants, dev):
    """[n_tenants][ceil(n / 64)] u64 words (as int64) on the device: bit i of bitmap f is set iff i < n and hash(i) % n_tenants == f"""
    words = (n + 63) // 64
    ids = torch.arange(words * 64, device=dev, dtype=torch.int64)
    hashed = ((ids * 2654435761) & 0xFFFFFFFF) >> 7      # (Knuth's multiplicative hash of the 32-bit id, its low bits dropped)
    owner = torch.where(ids < n, hashed % n_tenants, torch.full_like(ids, -1)).view(words, 64)
    shifts = torch.arange(64, device=dev, dtype=torch.int64)
    out = torch.empty((n_tenants, words), dtype=torch.int64, device=dev)
    for f in range(n_tenants):
        out[f] = ((owner == f).to(torch.int64) << shifts).sum(dim=1)      # (bit 63 wraps into the sign: the same 64 bits)
    return out


class Batch:
    """a query batch with device outputs on a shared stream"""

    def __init__(self, queries, storage, top, stream, dev):
        self.scorer = qa.new_raw_scorer(queries, storage)
        self.nq, self.top = len(queries), top
        self.out = torch.zeros((self.nq, top, 2), dtype=torch.int32, device=dev)
        self.counts = torch.zeros(self.nq, dtype=torch.int32, device=dev)
        F.check(F.lib().qmx_query_set_stream(self.scorer._h, F.ptr(int(stream.cuda_stream))))

    def enqueue(self):
        F.check(F.lib().qmx_search_topk_async(self.scorer._h, self.top, None, 0, F.ptr(self.out), F.ptr(self.counts)))

    def counters(self):
        return self.scorer.last_counters()


def timed(batches, stream, warmup, steps):
    def call():
        for b in batches:
            b.enqueue()
        stream.synchronize()

    for _ in range(warmup):
        call()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        times.append(1e3 * (time.perf_counter() - t0))
    cs = [b.counters() for b in batches]
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "steps": steps,
            "batches": len(batches), "fallback_queries": int(sum(c.fallback_queries for c in cs)), "verified_rows": int(sum(c.verified_rows for c in cs)),
            "prefilter_queries": int(sum(c.prefilter_queries for c in cs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=128)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--tenants", default="1,8,128")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dim, nq, top = args.points, args.dim, args.queries, args.top
    lib, dev = F.lib(), torch.device("cuda:0")
    seed = 0x5EED0013
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    F.check(lib.qmx_synth_fill_f32(0, seed, 0, n, dim, F.ptr(rows)))
    queries_dev = torch.empty((nq, dim), dtype=torch.float32, device=dev)
    F.check(lib.qmx_synth_fill_f32(0, seed + 1, 0, nq, dim, F.ptr(queries_dev)))
    F.check(lib.qmx_preprocess_f32(0, int(qa.Distance.Cosine), F.ptr(rows), n, dim, F.ptr(rows)))
    torch.cuda.synchronize(dev)
    storage = qa.VectorStorage(rows, qa.Distance.Cosine, flags=F.SEG_I8_COPY)
    queries = queries_dev.cpu().numpy()
    stream = torch.cuda.Stream(device=dev)

    whole = Batch(queries, storage, top, stream, dev)
    result = {"tool": "bench_filters", "points": n, "dim": dim, "queries": nq, "top": top, "dtype": "f32", "distance": "cosine", "copy": "i8",
              "device": torch.cuda.get_device_name(0), "kernel": None, "settings": {}}
    result["unfiltered"] = timed([whole], stream, args.warmup, args.steps)
    result["kernel"] = F.last_kernel(whole.scorer._h).split("(")[0]
    base_ms = result["unfiltered"]["median_ms"]

    settings = [("tenants_%d" % int(t), int(t), False) for t in args.tenants.split(",") if t] + [("mixed_8_half_unfiltered", 8, True)]
    for name, n_tenants, mixed in settings:
        if nq % n_tenants:
            raise SystemExit("--queries must be a multiple of every tenant count")
        bitmaps = tenant_bitmaps(n, n_tenants, dev)
        owner = np.arange(nq) % n_tenants
        fof = owner.astype(np.uint32)
        if mixed:
            fof[1::2] = F.FILTER_NONE
        F.check(lib.qmx_query_set_filters(whole.scorer._h, F.ptr(bitmaps), n, n_tenants, F.ptr(fof)))
        per_request = timed([whole], stream, args.warmup, args.steps)
        got = whole.out.cpu().numpy().copy()
        got_counts = whole.counts.cpu().numpy().copy()
        # the same requests without per-request filters: one batch per distinct filter
        groups = [(f, np.flatnonzero(fof == f)) for f in range(n_tenants)] + [(None, np.flatnonzero(fof == F.FILTER_NONE))]
        groups = [(f, idx) for f, idx in groups if len(idx)]
        parts = []
        for f, idx in groups:
            b = Batch(queries[idx], storage, top, stream, dev)
            if f is not None:
                F.check(lib.qmx_query_set_filter(b.scorer._h, F.ptr(bitmaps[f]), n))
            parts.append(b)
        split = timed(parts, stream, args.warmup, args.steps)
        same = True
        for (f, idx), b in zip(groups, parts):
            o, c = b.out.cpu().numpy(), b.counts.cpu().numpy()
            same = same and np.array_equal(c, got_counts[idx]) and all(np.array_equal(o[j, :c[j]], got[i, :c[j]]) for j, i in enumerate(idx))
        result["settings"][name] = {
            "tenants": n_tenants, "unfiltered_requests": int((fof == F.FILTER_NONE).sum()), "keep_rate": round(1.0 / n_tenants, 5),
            "per_request": per_request, "split": split, "lists_equal": bool(same),
            "split_over_per_request": round(split["median_ms"] / per_request["median_ms"], 3),
            "per_request_over_unfiltered": round(per_request["median_ms"] / base_ms, 3)}
        del parts
        F.check(lib.qmx_query_set_filter(whole.scorer._h, None, 0))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
