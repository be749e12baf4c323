#!/usr/bin/env python3
"""The HNSW walk over a sparse mirror (pgv_hnsw_upload_sparse + pgv_hnsw_search_sparse) at 1 M elements over 2048
dimensions with about 64 stored integer-valued elements each, by inner product, beside (a) the same walk of the same graph
over the elements' dense fp16 expansion (exact for these small integers; 4 GB of rows against the mirror's 0.5 GB) and (b)
the exact pgv_sparse_topk on the same rows and queries -- for ef_search 40, 100 and 400 with 1024 queries, k = 10, with the
walk's recall@10 against the exact answer (an element counts when its distance is at most the exact 10th distance: ties
are answers too).  Every vector has one element in each of its strata of the dimensions (sorted and distinct by
construction); a vector belongs to one of 256 topics that fix most of its indices, so that near neighbours exist.  The
graph is built on the device by pgv_host_hnsw_build over the fp16 expansion (--native-build: by pgv_host_hnsw_build_sparse over a buildable sparse mirror; the
same graph on these integer rows) and set on both mirrors (--graph FILE keeps it
between runs: the A/B runs of PGV_HNSW_SPARSE_PREFETCH are two processes).  Times are HIP events on the library's stream;
the routes are timed in alternating rounds after a warm-up of every shape, median and minimum over --reps rounds.
Prints one JSON line; --md FILE also writes the table.

usage: python tools/bench_sparse_hnsw.py [--rows 1000000] [--dim 2048] [--queries 1024] [--reps 5] [--graph FILE] [--md FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pgvector_amd import _host, api  # noqa: E402

EFS = (40, 100, 400)
K = 10
NNZ, TOPICS = 64, 256


def draw(torch, g, n, dim, topic_offset):
    """n sparse vectors as a CSR triple on the device: 48 .. 80 stored elements, one per stratum; three quarters of a
    vector's indices are its topic's, values 1 .. 8"""
    dev = g.device
    hi = NNZ + NNZ // 4
    width = dim // hi
    topic = torch.randint(0, TOPICS, (n,), generator=g, device=dev)
    own = torch.randint(0, width, (n, hi), generator=g, device=dev)
    off = torch.where(torch.rand((n, hi), generator=g, device=dev) < 0.75, topic_offset[topic], own)
    cand = torch.arange(hi, device=dev, dtype=torch.int64)[None, :] * width + off
    count = torch.randint(NNZ - NNZ // 4, hi + 1, (n,), generator=g, device=dev)
    keep = torch.rand((n, hi), generator=g, device=dev).argsort(dim=1).argsort(dim=1) < count[:, None]
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(count, 0)
    val = torch.randint(1, 9, (n, hi), generator=g, device=dev).float()
    return ptr.contiguous(), cand[keep].to(torch.int32).contiguous(), val[keep].contiguous()


def expand16(torch, csr, dim):
    ptr, idx, val = csr
    n = len(ptr) - 1
    out = torch.zeros((n, dim), dtype=torch.float16, device=val.device)
    row_of = torch.repeat_interleave(torch.arange(n, device=val.device), ptr[1:] - ptr[:-1])
    out[row_of, idx.long()] = val.half()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--ef-construction", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--graph", default=None, help="npz file: the built graph is loaded from it when it exists, else saved to it")
    ap.add_argument("--native-build", action="store_true",
                    help="build the graph on the sparse mirror itself (pgv_hnsw_upload_sparse_buildable + "
                         "pgv_host_hnsw_build_sparse) instead of over the fp16 twin; on these integer rows it is the same graph")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(24)
    hi = NNZ + NNZ // 4
    topic_offset = torch.randint(0, a.dim // hi, (TOPICS, hi), generator=g, device=dev)
    rows = draw(torch, g, a.rows, a.dim, topic_offset)
    queries = draw(torch, g, a.queries, a.dim, topic_offset)
    ctx = api.Context(0, stream=0)
    rows16, q16 = expand16(torch, rows, a.dim), expand16(torch, queries, a.dim)
    twin = api.Hnsw(ctx, api.PGV_NEG_IP, api.PGV_F16, a.dim, rows16)
    build_s = None
    if a.graph and os.path.exists(a.graph):
        built = dict(np.load(a.graph))
    elif a.native_build:
        builder = api.SparseHnsw(ctx, api.PGV_NEG_IP, a.dim, rows, buildable=True)
        host_csr = tuple(x.cpu().numpy() for x in rows)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        built = _host.hnsw_build(builder, None, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=1024, rows_csr=host_csr)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        builder.close()
        del host_csr
    else:
        host_rows = rows16.cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        built = _host.hnsw_build(twin, host_rows, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=1024)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        del host_rows
        if a.graph:
            np.savez(a.graph, entry=built["entry"], levels=built["levels"], nbr_start=built["nbr_start"], nbr=built["nbr"])
    del rows16
    graph = (a.m, int(built["entry"]), built["levels"], built["nbr_start"], built["nbr"])
    twin.set_graph(*graph)
    mirror = api.SparseHnsw(ctx, api.PGV_NEG_IP, a.dim, rows)
    mirror.set_graph(*graph)

    res = {"rows": a.rows, "dim": a.dim, "row_nnz_total": int(rows[0][-1]), "query_nnz_total": int(queries[0][-1]), "m": a.m,
           "ef_construction": a.ef_construction, "queries": a.queries, "k": K, "reps": a.reps, "build_secs": build_s,
           "graph_built_on": "sparse mirror" if a.native_build else "fp16 twin",
           "sparse_prefetch": os.environ.get("PGV_HNSW_SPARSE_PREFETCH", "1 (default)"),
           "row_bytes_mean": {"sparse": 8.0 * int(rows[0][-1]) / a.rows, "fp16_twin": 2 * a.dim}, "ef": []}
    exact_d, exact_i = api.sparse_topk(ctx, api.PGV_NEG_IP, a.dim, queries, rows, K)  # warm-up, and the exact answer
    kth = exact_d[:, -1:]
    for ef in EFS:
        routes = {"sparse_walk": lambda: mirror.search(queries, ef, K), "fp16_twin_walk": lambda: twin.search(q16, ef, K),
                  "sparse_topk": lambda: api.sparse_topk(ctx, api.PGV_NEG_IP, a.dim, queries, rows, K)}
        outs = {name: fn() for name, fn in routes.items()}  # warm-up of every shape, and the answers
        ms = {name: [] for name in routes}
        for _ in range(a.reps):
            for name, fn in routes.items():
                ctx.timer_start()
                fn()
                ms[name].append(ctx.timer_stop())
        rec = {"ef": ef}
        for name in routes:
            med, best = statistics.median(ms[name]), min(ms[name])
            rec[name] = {"ms_median": med, "ms_min": best, "qps_median": a.queries / med * 1e3, "qps_best": a.queries / best * 1e3}
        for name in ("sparse_walk", "fp16_twin_walk"):
            elem, dist, scored = outs[name]
            rec[name]["recall_at_10"] = ((dist <= kth) & (elem >= 0)).sum().item() / (a.queries * K)
            rec[name]["scored_per_query"] = float(scored.float().mean().item())
        rec["walks_agree"] = all(bool(torch.equal(x, y)) for x, y in zip(outs["sparse_walk"], outs["fp16_twin_walk"]))
        res["ef"].append(rec)
    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("| ef | sparse walk q/s (median / best) | fp16-twin walk q/s (median / best) | sparse / twin | `pgv_sparse_topk` q/s "
                    "(ms a batch) | walk recall@10 | elements scored per query | walks agree |\n|---|---|---|---|---|---|---|---|\n")
            for r in res["ef"]:
                f.write("| %d | %.0f / %.0f | %.0f / %.0f | %.2f | %.0f (%.1f) | %.4f | %.0f | %s |\n" % (
                    r["ef"], r["sparse_walk"]["qps_median"], r["sparse_walk"]["qps_best"], r["fp16_twin_walk"]["qps_median"],
                    r["fp16_twin_walk"]["qps_best"], r["sparse_walk"]["qps_median"] / r["fp16_twin_walk"]["qps_median"],
                    r["sparse_topk"]["qps_median"], r["sparse_topk"]["ms_median"], r["sparse_walk"]["recall_at_10"],
                    r["sparse_walk"]["scored_per_query"], "yes" if r["walks_agree"] else "NO"))
    mirror.close()
    twin.close()
    ctx.close()


if __name__ == "__main__":
    main()
