#!/usr/bin/env python3
"""Brute-force MaxSim over dense f32 multi-vector points: the fused route (qdrant_amd/csrc/maxsim_fused.hip) against the two-step route (the
[tokens][rows] similarity matrix + maxsim_kernel) in ONE process over the SAME storage, option no_maxsim_fused alternating 0 / 1 call by call.

Data: `--rows` x `--dim` standard normal f32 rows (seeded), cut into points of 50 .. 150 rows.  Multi-queries of `--tokens` tokens, batches of
`--queries`.  Two shapes per batch: "rerank" - qmx_multi_search_topk over `--candidates` random points - and "block" - the same call without a
candidate list.  The call is synchronous (it ends with a stream synchronise), so the wall time of a call is device-synchronised; per leg the median,
min and max over `--steps` timed calls after `--warmup` of both legs.  "lists_equal": ids and score bits of the two legs' lists.  One JSON line on
stdout; `--out` also writes it to a file.

`--dtype f16`: the same rows as f16 in a segment created with SEG_F16_WIDE, three legs alternating call by call: "fused" = maxsim_f16.hip, "two_step" =
the f16 scans + maxsim_kernel (no_maxsim_fused = 1), "f32_fused" = maxsim_fused.hip over the f32 rows.  Per cell also "oracle_equal" - the f16 fused
leg's scores against the CPU oracle's MaxSim of the listed points, bit for bit, and that no unlisted candidate scores higher (rerank cells; block cells
at one query) - and "flagged_share": the share of (token, candidate) pairs whose best and second best similarity lie inside the token's band, counted on
the host from f32 similarities (numpy) with f16w_band's formula - an estimate of what the kernel flags, not a counter read from it.

`--dtype u8`: uniform random u8 rows and integer-valued tokens, one storage per distance (Dot, Cosine, Euclid) over the same rows; per cell and distance
the legs "fused" = maxsim_u8.hip and "two_step" = the exact u8 scans + maxsim_kernel (no_maxsim_fused = 1), alternating call by call, with "lists_equal"
and "fused_row_gbytes_per_s" (the candidates' row bytes, once per 64-token group, over the fused leg's median).  Beside the Dot legs, for scale:
"f32_fused" and "f16_fused", the sibling kernels over normal rows of the same shape."""
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


def flagged_share(rows, lens, tokens, seg_subnormal, rowmax):
    """share of (token, point) pairs with second best >= best - band(token); rows / tokens: the f16 values as f32, every point non-empty"""
    dim, u = rows.shape[1], 2.0 ** -24
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    sims = rows @ tokens.T
    m1 = np.maximum.reduceat(sims, starts, axis=0)
    at_max = sims == np.repeat(m1, lens, axis=0)
    ties = np.add.reduceat(at_max, starts, axis=0, dtype=np.int64)
    sims[at_max] = -np.inf
    m2 = np.where(ties > 1, m1, np.maximum.reduceat(sims, starts, axis=0))
    t64 = tokens.astype(np.float64)
    b = np.sqrt((t64 * t64).sum(axis=1)) * rowmax
    e_ar = (1.001 * dim / 4194304.0 + 1.0 / 262144.0 + 38.0 * 1.001 * u) * b
    e_sub = ((np.abs(t64).sum(axis=1) if seg_subnormal else 0.0) + np.sqrt(((t64 != 0) & (np.abs(t64) < 2.0 ** -14)).sum(axis=1)) * rowmax) / 16384.0
    band = (2.0 * (e_ar + e_sub) + 4.0 * u * b).astype(np.float32)
    return float((~(m2 < m1 - band[None, :])).mean())


def oracle_equal(O, rows16, offsets, points, queries, lists):
    """the lists of one leg against the oracle's MaxSim over `points` (all of them scored): score bits in order, and each listed id has its score"""
    lens = (offsets[points.astype(np.int64) + 1] - offsets[points]).astype(np.int64)
    take = np.concatenate([np.arange(int(offsets[p]), int(offsets[p + 1])) for p in points])
    sub = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    first = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.uint32)
    full = O.multi_scores(O.DenseStorage(O.F16, O.DOT, rows16[take]), np.concatenate(queries), first, sub, np.arange(len(points)))
    where = {int(p): i for i, p in enumerate(points)}
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)       # noqa: E731
    return all(np.array_equal(bits(res["score"]), bits(np.sort(sc)[::-1][:len(res)])) and
               np.array_equal(bits(sc[[where[int(i)] for i in res["idx"]]]), bits(res["score"])) for res, sc in zip(lists, full))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("f32", "f16", "u8"), default="f32")
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
    st32 = qa.MultiDenseVectorStorage(rows, offsets, qa.Distance.Dot)
    ids = np.ascontiguousarray(rng.permutation(n_points)[:args.candidates], dtype=np.uint32)
    result = {"tool": "bench_maxsim", "dtype": args.dtype, "rows": args.rows, "dim": args.dim, "points": n_points, "tokens": args.tokens, "candidates": len(ids),
              "candidate_rows": int((offsets[ids.astype(np.int64) + 1] - offsets[ids]).sum()), "top": args.top, "cells": {}}
    legs = [("fused", st32, 0), ("two_step", st32, 1)]
    if args.dtype == "f16":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_ffi as O      # (the checker: not timed)
        rows16 = O.to_f16(rows)
        vals16 = O.f16_to_f32(rows16)
        seg_subnormal = bool(((vals16 != 0) & (np.abs(vals16) < 2.0 ** -14)).any())
        rowmax = float(np.sqrt((vals16.astype(np.float64) ** 2).sum(axis=1).max()))
        inner = qa.VectorStorage(rows16.view(np.float16), qa.Distance.Dot, qa.VectorStorageDatatype.Float16, flags=F.SEG_F16_WIDE)
        st16 = qa.MultiDenseVectorStorage(None, offsets, qa.Distance.Dot, inner_storage=inner)
        legs = [("fused", st16, 0), ("two_step", st16, 1), ("f32_fused", st32, 0)]
    if args.dtype == "u8":
        return main_u8(args, rng, rows, offsets, n_points, ids, st32, result)
    all_points = np.arange(n_points, dtype=np.uint32)
    for nq in [int(x) for x in args.queries.split(",") if x]:
        queries = [rng.standard_normal((args.tokens, args.dim), dtype=np.float32) for _ in range(nq)]
        scorers = {id(s): s._queries(queries) for s in {id(leg[1]): leg[1] for leg in legs}.values()}
        for shape, cand in (("rerank", ids), ("block", None)):
            cell, out, counts = timed_cell(args, legs, scorers, nq, offsets, n_points, cand)
            cell["lists_equal"] = bool(np.array_equal(out["fused"]["idx"], out["two_step"]["idx"]) and
                                       np.array_equal(out["fused"]["score"].copy().view(np.uint32), out["two_step"]["score"].copy().view(np.uint32)))
            cell["two_step_over_fused"] = round(cell["two_step"]["median_ms"] / cell["fused"]["median_ms"], 3)
            if args.dtype == "f16":
                points = all_points if cand is None else cand
                lens = (offsets[points.astype(np.int64) + 1] - offsets[points]).astype(np.int64)
                row_bytes = int(lens.sum()) * args.dim * 2 * ((nq * args.tokens + 63) // 64)      # one pass of the candidates' rows per 64-token group
                cell["fused_row_gbytes_per_s"] = round(row_bytes / cell["fused"]["median_ms"] / 1e6, 1)
                cell["f32_fused_over_fused"] = round(cell["f32_fused"]["median_ms"] / cell["fused"]["median_ms"], 3)
                if cand is not None or nq == 1:
                    cell["oracle_equal"] = bool(oracle_equal(O, rows16, offsets, points, queries, [out["fused"][j, :counts[j]] for j in range(nq)]))
                take = np.concatenate([np.arange(int(offsets[p]), int(offsets[p + 1])) for p in points])
                cell["flagged_share"] = round(flagged_share(vals16[take], lens, O.f16_to_f32(O.to_f16(queries[0])), seg_subnormal, rowmax), 5)
            result["cells"]["%s_q%d" % (shape, nq)] = cell
    emit(args, result)


def emit(args, result):
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def timed_cell(args, legs, scorers, nq, offsets, n_points, cand):
    """the legs (name, storage, no_maxsim_fused) alternating call by call: per leg median / min / max of the timed calls and the kernel; the lists"""
    lib = F.lib()
    out = {leg[0]: np.zeros((nq, args.top), dtype=ScoredPointOffset) for leg in legs}
    counts = np.zeros(nq, dtype=np.uint32)
    times = {k: [] for k in out}
    kernels = {}
    for step in range(args.warmup + args.steps):
        for name, st, off in legs:
            scorer, first = scorers[id(st)]
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
    return cell, out, counts


def main_u8(args, rng, rows32, offsets, n_points, ids, st32, result):
    rows8 = rng.integers(0, 256, (args.rows, args.dim), dtype=np.uint8)
    dists = (("dot", qa.Distance.Dot), ("cosine", qa.Distance.Cosine), ("euclid", qa.Distance.Euclid))
    st8 = {name: qa.MultiDenseVectorStorage(None, offsets, d, inner_storage=qa.VectorStorage(rows8, d, qa.VectorStorageDatatype.Uint8)) for name, d in dists}
    inner16 = qa.VectorStorage(rows32.astype(np.float16), qa.Distance.Dot, qa.VectorStorageDatatype.Float16, flags=F.SEG_F16_WIDE)
    st16 = qa.MultiDenseVectorStorage(None, offsets, qa.Distance.Dot, inner_storage=inner16)
    for nq in [int(x) for x in args.queries.split(",") if x]:
        queries8 = [rng.integers(0, 256, (args.tokens, args.dim)).astype(np.float32) for _ in range(nq)]
        queries32 = [rng.standard_normal((args.tokens, args.dim), dtype=np.float32) for _ in range(nq)]
        scorers = {id(s): s._queries(queries8) for s in st8.values()}
        scorers[id(st32)], scorers[id(st16)] = st32._queries(queries32), st16._queries(queries32)
        for shape, cand in (("rerank", ids), ("block", None)):
            points = np.arange(n_points, dtype=np.uint32) if cand is None else cand
            n_rows = int((offsets[points.astype(np.int64) + 1] - offsets[points]).sum())
            row_bytes = n_rows * args.dim * ((nq * args.tokens + 63) // 64)      # one pass of the candidates' rows per 64-token group
            cells = {}
            for name, _ in dists:
                legs = [("fused", st8[name], 0), ("two_step", st8[name], 1)]
                if name == "dot":
                    legs += [("f32_fused", st32, 0), ("f16_fused", st16, 0)]
                cell, out, _ = timed_cell(args, legs, scorers, nq, offsets, n_points, cand)
                cell["lists_equal"] = bool(np.array_equal(out["fused"]["idx"], out["two_step"]["idx"]) and
                                           np.array_equal(out["fused"]["score"].copy().view(np.uint32), out["two_step"]["score"].copy().view(np.uint32)))
                cell["two_step_over_fused"] = round(cell["two_step"]["median_ms"] / cell["fused"]["median_ms"], 3)
                cell["fused_row_gbytes_per_s"] = round(row_bytes / cell["fused"]["median_ms"] / 1e6, 1)
                cells[name] = cell
            result["cells"]["%s_q%d" % (shape, nq)] = cells
    emit(args, result)


if __name__ == "__main__":
    main()
