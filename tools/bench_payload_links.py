#!/usr/bin/env python3
"""The payload-block build (qmx_hnsw_build_payload_links) at collection size: what it costs and what it buys under a tenant filter.

Data: `--points` x `--dim` clustered f32 rows (a mixture of gaussians, dot product) and their scalar-int8 form; tenants by a multiplicative hash of the
point id, `--tenants` settings (16, 256, 4096).  Per storage kind a main graph is built once (`--m`, `--ef-construct`); per setting
  merged : the main graph + the payload links of every tenant (`--payload-m`), one call;
  m0     : the payload links alone (main_graph = NULL: Qdrant's multi-tenant setting m = 0, payload_m = 16).
Reported per run: build seconds, info.launches / blocks_built / links_added / longest_row, and recall@10 at ef `--ef` of `--queries` requests - request j
under the filter of tenant j - over the main-only, merged and m0 graphs against the exact filtered search of the f32 rows (one batch under
qmx_query_set_filters; the SQ walks are not rescored: their recall is the quantized scorer's).  Controls per run: the main graph's unfiltered recall, and
tenant 0's rows alone as their own storage under an ordinary hierarchical graph and under the flat graph of the same rows (ef `--ef`, and 512).
One JSON line on stdout; `--out` also writes it to a file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: one HIP runtime for both)

import qdrant_amd as qa  # noqa: E402


def clustered(n, dim, seed, k=256):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((k, dim)).astype(np.float32) * 2.0
    out = np.empty((n, dim), dtype=np.float32)
    for lo in range(0, n, 1 << 16):      # in slices: the noise of a million rows at once is several GB of temporaries
        hi = min(n, lo + (1 << 16))
        out[lo:hi] = centers[rng.integers(0, k, hi - lo)] + rng.standard_normal((hi - lo, dim), dtype=np.float32) * 0.6
    return out


def tenant_of(n, tenants):
    return (((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(7)) % np.uint64(tenants)


def recall(got, want):
    return sum(len(set(g["idx"].tolist()) & set(w["idx"].tolist())) for g, w in zip(got, want)) / float(max(1, sum(len(w) for w in want)))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--tenants", default="16,256,4096")
    ap.add_argument("--kinds", default="f32,sq")
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--payload-m", type=int, default=16)
    ap.add_argument("--ef-construct", type=int, default=100)
    ap.add_argument("--ef", type=int, default=64)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, dim, nq = a.points, a.dim, a.queries
    rows = clustered(n, dim, 1)
    queries = clustered(nq, dim, 2)
    vs = qa.VectorStorage(rows, qa.Distance.Dot)
    result = {"points": n, "dim": dim, "m": a.m, "payload_m": a.payload_m, "ef_construct": a.ef_construct, "ef": a.ef, "queries": nq, "runs": []}
    for kind in a.kinds.split(","):
        storage = vs
        if kind == "sq":
            quant = qa.ScalarQuantizer.from_min_max(rows[:: max(1, n // 100000)], dim, qa.Distance.Dot)
            storage = qa.EncodedVectorsU8(quant.encode(rows), quant)
        main_graph, main_s = timed(lambda: qa.GraphLayers.build(storage, m=a.m, ef_construct=a.ef_construct, seed=1))
        # control: the main graph without any filter, on the same rows and queries
        exact_all = qa.BatchFilteredSearcher(queries, vs, a.top).peek_top_all()
        recall_unfiltered = round(recall(main_graph.search(a.top, a.ef, qa.new_raw_scorer(queries, storage)), exact_all), 4)
        print("%s: main graph of %d points in %.1f s, unfiltered recall@%d at ef %d %.3f" % (kind, n, main_s, a.top, a.ef, recall_unfiltered), file=sys.stderr, flush=True)
        for tenants in [int(t) for t in a.tenants.split(",")]:
            tenant = tenant_of(n, tenants)
            order = np.argsort(tenant, kind="stable").astype(np.uint32)
            offsets = np.zeros(tenants + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum(np.bincount(tenant.astype(np.int64), minlength=tenants))
            q_tenant = (np.arange(nq) % tenants).astype(np.int64)
            used = sorted(set(q_tenant.tolist()))
            masks = np.stack([tenant == t for t in used])
            filter_of = np.array([used.index(t) for t in q_tenant], dtype=np.uint32)
            exact_s = qa.BatchFilteredSearcher(queries, vs, a.top)
            exact_s.scorer.set_filters(masks, filter_of)
            exact = exact_s.peek_top_all()

            def walk(graph):
                scorer = qa.new_raw_scorer(queries, storage)
                scorer.set_filters(masks, filter_of)
                return recall(graph.search(a.top, a.ef, scorer), exact)
            merged, merged_s = timed(lambda: qa.GraphLayers.build_payload_links(storage, (offsets, order), payload_m=a.payload_m, ef_construct=a.ef_construct,
                                                                                 main=main_graph))
            flat, flat_s = timed(lambda: qa.GraphLayers.build_payload_links(storage, (offsets, order), payload_m=a.payload_m, ef_construct=a.ef_construct))
            run = {"kind": kind, "tenants": tenants, "main_build_s": round(main_s, 3), "merged_build_s": round(merged_s, 3), "m0_build_s": round(flat_s, 3)}
            for name, g in (("merged", merged), ("m0", flat)):
                i = g.payload_info
                run[name] = {"launches": i.launches, "blocks_built": i.blocks_built, "links_added": i.links_added, "longest_row": i.longest_row}
            run["recall_main_only"], run["recall_merged"], run["recall_m0"] = round(walk(main_graph), 4), round(walk(merged), 4), round(walk(flat), 4)
            # controls that tell the data from the build: tenant 0's rows alone as a storage of their own, every query against it unfiltered - under an
            # ordinary hierarchical graph (m = payload_m) and under the flat graph of the same rows built as one block
            ids0 = order[int(offsets[0]):int(offsets[1])]
            sub_vs = qa.VectorStorage(rows[ids0], qa.Distance.Dot)
            sub = sub_vs if kind != "sq" else qa.EncodedVectorsU8(quant.encode(rows[ids0]), quant)
            sub_exact = qa.BatchFilteredSearcher(queries, sub_vs, a.top).peek_top_all()
            sub_scorer = qa.new_raw_scorer(queries, sub)
            g_h = qa.GraphLayers.build(sub, m=a.payload_m, ef_construct=a.ef_construct, seed=1)
            g_f = qa.GraphLayers.build_payload_links(sub, [np.arange(len(ids0), dtype=np.uint32)], payload_m=a.payload_m, ef_construct=a.ef_construct)
            run["recall_main_unfiltered"] = recall_unfiltered
            run["tenant0_points"] = int(len(ids0))
            run["recall_tenant0_hierarchical_graph"] = round(recall(g_h.search(a.top, a.ef, sub_scorer), sub_exact), 4)
            run["recall_tenant0_flat_graph"] = round(recall(g_f.search(a.top, a.ef, sub_scorer), sub_exact), 4)
            run["recall_tenant0_flat_graph_ef512"] = round(recall(g_f.search(a.top, 512, sub_scorer), sub_exact), 4)
            g_h.close()
            g_f.close()
            print(json.dumps(run), file=sys.stderr, flush=True)
            result["runs"].append(run)
            merged.close()
            flat.close()
        main_graph.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
