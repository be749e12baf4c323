#!/usr/bin/env python3
"""Exact cosine search over rows as stored, 1 M x 1536, k = 10, batches of 1024 and 128 queries, fp32 and fp16, in one
process on the same data (seeded normal rows, device memory in and out):

  cosine_topk     pgv_cosine_topk over the rows as they are
  normalised_ip   pgv_exact_topk(PGV_NEG_IP) over a normalised copy of rows and queries -- another value (a dot product
                  of two rounded unit vectors); the time to make the copy (torch, on the device) is stated separately
  batch_loop      for a few queries: pgv_cosine_distance_batch over all rows, the n float8 values copied back, a host
                  argpartition + sort -- the only faithful path before pgv_cosine_topk; ms per query

Times are HIP events around the call (the host loop: wall clock), medians over --reps calls after a warm-up.  Run under
`rocprofv3 --kernel-trace --stats` the same process gives cosine_tile_kernel beside mfma_dense_kernel<T, 1>.  Prints one
JSON line; --md FILE also writes the table.

usage: python tools/bench_cosine_topk.py [--rows 1000000] [--dim 1536] [--reps 5] [--md profiles/r35_cosine_topk_table.md]
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

BATCHES = (1024, 128)
K = 10
LOOP_QUERIES = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch

    from pgvector_amd import api
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(35)
    ctx = api.Context(0, stream=0)
    res = {"rows": a.rows, "dim": a.dim, "k": K, "reps": a.reps, "runs": []}
    for name, tdtype, dtype in (("fp32", torch.float32, api.PGV_F32), ("fp16", torch.float16, api.PGV_F16)):
        rows = torch.cat([torch.randn((min(65536, a.rows - lo), a.dim), generator=g, device=dev).to(tdtype)
                          for lo in range(0, a.rows, 65536)]).contiguous()
        all_queries = torch.randn((max(BATCHES), a.dim), generator=g, device=dev).to(tdtype).contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        unit = torch.nn.functional.normalize(rows.float(), dim=1).to(tdtype).contiguous()
        torch.cuda.synchronize()
        copy_ms = (time.perf_counter() - t0) * 1e3
        for nq in BATCHES:
            queries = all_queries[:nq].contiguous()
            unit_q = torch.nn.functional.normalize(queries.float(), dim=1).to(tdtype).contiguous()
            out_c = (torch.empty((nq, K), dtype=torch.float64, device=dev), torch.empty((nq, K), dtype=torch.int64, device=dev))
            out_e = (torch.empty((nq, K), dtype=torch.float32, device=dev), torch.empty((nq, K), dtype=torch.int64, device=dev))
            fns = {"cosine_topk": lambda: api.cosine_topk(ctx, queries, rows, K, out=out_c),
                   "normalised_ip": lambda: api.exact_topk(ctx, api.PGV_NEG_IP, dtype, a.dim, unit_q, unit, K, out=out_e)}
            times = {n_: [] for n_ in fns}
            for fn in fns.values():  # warm-up
                fn()
            for _ in range(a.reps):  # the two in alternation
                for n_, fn in fns.items():
                    ctx.timer_start()
                    fn()
                    times[n_].append(ctx.timer_stop())
            ctx.sync()
            run = {"dtype": name, "nq": nq, "normalised_copy_ms": copy_ms,
                   "same_top1": float((out_c[1][:, 0] == out_e[1][:, 0]).float().mean().item())}
            for n_, t in times.items():
                run[n_ + "_ms"] = statistics.median(t)
            res["runs"].append(run)
        loop = []
        for q in range(LOOP_QUERIES):
            t0 = time.perf_counter()
            d = api.cosine_distance_batch(ctx, dtype, a.dim, all_queries[q], rows)
            ctx.sync()
            d = d.cpu().numpy()
            part = np.argpartition(d, K)[:K]
            part[np.argsort(d[part], kind="stable")]
            loop.append((time.perf_counter() - t0) * 1e3)
        for run in res["runs"]:
            if run["dtype"] == name:
                run["batch_loop_ms_per_query"] = statistics.median(loop)
        del rows, unit, all_queries
    ctx.close()
    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("| dtype | queries | `pgv_cosine_topk` ms | `pgv_exact_topk(PGV_NEG_IP)` over the normalised copy ms | "
                    "making the copy ms | `pgv_cosine_distance_batch` + host sort, ms per query | same top-1 |\n"
                    "|---|---|---|---|---|---|---|\n")
            for r in res["runs"]:
                f.write("| %s | %d | %.2f | %.2f | %.0f | %.1f | %.4f |\n" % (
                    r["dtype"], r["nq"], r["cosine_topk_ms"], r["normalised_ip_ms"], r["normalised_copy_ms"],
                    r["batch_loop_ms_per_query"], r["same_top1"]))


if __name__ == "__main__":
    main()
