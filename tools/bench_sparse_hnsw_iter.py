#!/usr/bin/env python3
"""HNSW iterative scans over a sparse mirror (pgv_hnsw_scan_begin_sparse + pgv_hnsw_scan_next / _drain) at
tools/bench_sparse_hnsw.py's learned-sparse shape (1 M elements over 2048 dimensions, 48 .. 80 stored integer-valued
elements each in 256 topics, inner product, m 16, ef_construction 64; the graph built on a buildable sparse mirror by
pgv_host_hnsw_build_sparse, or loaded from --graph), all in one process:

  first_batch   a scan's first batch against pgv_hnsw_search_sparse at the same ef (k = ef), ef 40 / 100 / 400: the price of
                the per-query visited set and of keeping the discards.  Alternating, median / min / max over --reps rounds;
                the begin (staging the queries, allocating and zeroing the state) is timed on the host beside it
  resumed       the time of each of the first --batches batches of one scan at ef 40 with the mean pool its entry step
                read, and the state's bytes per query
  filtered      k = 10 under a filter keeping 10 % and 1 % of the rows: hnsw_iterative_search at ef 40 against one
                pgv_hnsw_search_sparse at each ef of a ladder up to 1000 -- the share of queries that get their 10 rows
                with one batch and with the scan, and the share for which no ef <= 1000 does

Device times are HIP events on the library's stream; `filtered` and `begin` are wall-clock (their loops run on the host).
Prints one JSON line; --md FILE also writes the tables.

usage: python tools/bench_sparse_hnsw_iter.py [--rows 1000000] [--dim 2048] [--queries 1024] [--reps 7] [--graph FILE] [--md FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sparse_hnsw import NNZ, TOPICS, draw  # noqa: E402
from pgvector_amd import _host, api  # noqa: E402

EFS = (40, 100, 400)
LADDER = (40, 100, 200, 400, 1000)
K = 10


def spread(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "runs": len(ms)}


def timed(ctx, fn):
    ctx.timer_start()
    out = fn()
    return ctx.timer_stop(), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--ef-construction", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--graph", default=None, help="npz file: the built graph is loaded from it when it exists, else saved to it")
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
    build_s = None
    if a.graph and os.path.exists(a.graph):
        built = dict(np.load(a.graph))
    else:
        builder = api.SparseHnsw(ctx, api.PGV_NEG_IP, a.dim, rows, buildable=True)
        host_csr = tuple(x.cpu().numpy() for x in rows)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        built = _host.hnsw_build(builder, None, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=1024, rows_csr=host_csr)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        builder.close()
        del host_csr
        if a.graph:
            np.savez(a.graph, entry=built["entry"], levels=built["levels"], nbr_start=built["nbr_start"], nbr=built["nbr"])
    mirror = api.SparseHnsw(ctx, api.PGV_NEG_IP, a.dim, rows)
    mirror.set_graph(a.m, int(built["entry"]), built["levels"], built["nbr_start"], built["nbr"])
    nq = a.queries
    q_nnz = int(queries[0][-1])
    res = {"rows": a.rows, "dim": a.dim, "row_nnz_total": int(rows[0][-1]), "query_nnz_total": q_nnz, "m": a.m,
           "ef_construction": a.ef_construction, "queries": nq, "reps": a.reps, "build_secs": build_s}

    # ---- a scan's first batch against the plain search
    res["first_batch"] = []
    for ef in EFS:
        plain_out = mirror.search(queries, ef, ef)
        with mirror.scan_sparse(queries, ef) as s:
            first = s.next()
        agree = all(bool(torch.equal(x, y)) for x, y in zip(plain_out, (first[0], first[1], first[3])))
        ms = {"search": [], "scan_first": [], "begin_host": []}
        for _ in range(a.reps):
            ms["search"].append(timed(ctx, lambda: mirror.search(queries, ef, ef))[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = mirror.scan_sparse(queries, ef)  # (returns after a synchronise of its own)
            ms["begin_host"].append(1e3 * (time.perf_counter() - t0))
            with s:
                ms["scan_first"].append(timed(ctx, s.next)[0])
        rec = {"ef": ef, "agree": agree, "search": spread(ms["search"]), "scan_first": spread(ms["scan_first"]),
               "begin_host": spread(ms["begin_host"]), "discards_per_query": float(first[4].float().mean().item())}
        rec["ratio_of_medians"] = rec["scan_first"]["ms_median"] / rec["search"]["ms_median"]
        res["first_batch"].append(rec)

    # ---- resumed batches, and what the state takes
    words = (a.rows + 31) // 32 + 1
    cap = min(a.rows, 65536)
    copy = 8.0 * (nq + 1 + q_nnz) / nq
    res["state_bytes_per_query"] = {"pool": 8 * cap, "visited_bitmap": 4 * words, "counters": 16, "query_copy_mean": copy,
                                    "total_mean": 8 * cap + 4 * words + 16 + copy, "discard_cap": cap}
    res["resumed"] = []
    with mirror.scan_sparse(queries, 40) as s:
        pool = 0.0
        for b in range(a.batches):
            t, out = timed(ctx, s.next)
            res["resumed"].append({"batch": b, "ms": t, "us_per_query": 1e3 * t / nq, "pool_read_mean": pool,
                                   "scored_mean": float(out[3].float().mean().item())})
            pool = float(out[4].float().mean().item())

    # ---- the use case: k = 10 under a filter
    res["filtered"] = []
    first64 = tuple(x.contiguous() for x in (queries[0][:65], queries[1][:int(queries[0][64])], queries[2][:int(queries[0][64])]))
    for share in (0.10, 0.01):
        keep = np.random.default_rng(7).random(a.rows) < share
        keep_dev = torch.from_numpy(keep).to(dev)
        api.hnsw_iterative_search(mirror, first64, K, keep, 40)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, _, scored = api.hnsw_iterative_search(mirror, queries, K, keep, 40)
        torch.cuda.synchronize()
        it_s = time.perf_counter() - t0
        rec = {"keep_share": share, "iterative_ef40": {"secs": it_s, "qps": nq / it_s, "queries_with_k": sum(len(x) >= K for x in ids) / nq,
                                                        "scored_mean": float(np.mean(scored))}, "single_search": []}
        served = torch.zeros(nq, dtype=torch.bool, device=dev)
        for ef in LADDER:
            mirror.search(queries, ef, ef)
            t, (elem, _, _) = timed(ctx, lambda: mirror.search(queries, ef, ef))
            ok = (keep_dev[elem.clamp(min=0)] & (elem >= 0)).sum(1) >= K
            served |= ok
            rec["single_search"].append({"ef": ef, "ms": t, "qps": nq / t * 1e3, "queries_with_k": float(ok.float().mean().item())})
        rec["no_ef_up_to_1000"] = 1.0 - float(served.float().mean().item())
        res["filtered"].append(rec)

    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("%d x %d, %d stored elements, m %d, ef_construction %d, %d queries (%d stored elements), %d rounds\n\n" % (
                a.rows, a.dim, res["row_nnz_total"], a.m, a.ef_construction, nq, q_nnz, a.reps))
            f.write("| ef | `pgv_hnsw_search_sparse` ms (median, min - max) | scan's first batch ms (median, min - max) | ratio | "
                    "begin, host ms (median) | discards kept per query | same answers |\n|---|---|---|---|---|---|---|\n")
            for r in res["first_batch"]:
                f.write("| %d | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.3f | %.2f | %.0f | %s |\n" % (
                    r["ef"], r["search"]["ms_median"], r["search"]["ms_min"], r["search"]["ms_max"], r["scan_first"]["ms_median"],
                    r["scan_first"]["ms_min"], r["scan_first"]["ms_max"], r["ratio_of_medians"], r["begin_host"]["ms_median"],
                    r["discards_per_query"], "yes" if r["agree"] else "NO"))
            f.write("\n| batch (ef 40) | ms | us per query | mean pool its entry step read | mean so->tuples after |\n|---|---|---|---|---|\n")
            for r in res["resumed"]:
                f.write("| %d | %.2f | %.2f | %.0f | %.0f |\n" % (r["batch"], r["ms"], r["us_per_query"], r["pool_read_mean"], r["scored_mean"]))
            f.write("\nstate per query: %s\n" % json.dumps(res["state_bytes_per_query"]))
            for r in res["filtered"]:
                f.write("\nfilter keeps %.0f %%: iterative ef 40: %.0f q/s, %.4f of the queries get %d rows, %.0f scored per query; "
                        "no ef <= 1000 serves %.4f of the queries\n\n| one search at ef | q/s | queries with %d kept rows |\n|---|---|---|\n" % (
                            100 * r["keep_share"], r["iterative_ef40"]["qps"], r["iterative_ef40"]["queries_with_k"], K,
                            r["iterative_ef40"]["scored_mean"], r["no_ef_up_to_1000"], K))
                for x in r["single_search"]:
                    f.write("| %d | %.0f | %.4f |\n" % (x["ef"], x["qps"], x["queries_with_k"]))
    mirror.close()
    ctx.close()


if __name__ == "__main__":
    main()
