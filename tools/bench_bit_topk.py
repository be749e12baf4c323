#!/usr/bin/env python3
"""Binary-quantized search at 1 M x 1536 bits: pgv_bit_topk for batches of 1, 32, 256 and 1024 queries at k = 100 --
the scan kernel alone (the context's profiling events around hamming_tile_kernel), the whole call, and
api.binary_search at kc = 100, k = 10 with its recall@10 against a float64 brute force -- beside the only route the
library had before: one pgv_bit_distance_batch call per query (at most 64 calls are made and the time is extrapolated
linearly to the batch; the sort that route leaves to the host is NOT included).  The rows are quantised on the device
from a seeded fp32 mixture.  Times are HIP events, medians over --reps calls after a warm-up.  Prints one JSON line;
--md FILE also writes the table.

usage: python tools/bench_bit_topk.py [--rows 1000000] [--dim 1536] [--reps 5] [--md profiles/r14_bit_topk.md]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pgvector_amd import api  # noqa: E402

BATCHES = (1, 32, 256, 1024)
K, KC, K2 = 100, 100, 10


def popcount_bound_ms(rows, nbits, nq, cus):
    """the least time the vector ALUs need: one xor and one accumulating popcount per 32-bit word and (row, query) pair,
    64 lane-operations per clock and CU at 2.4 GHz (2.6 ms for 1 M x 1536 bits x 1024 queries on 256 CUs)"""
    return rows * nq * ((nbits + 31) // 32) * 2 / (cus * 64 * 2.4e9) * 1e3


def timed(ctx, fn, reps):
    fn()
    out = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        out.append(ctx.timer_stop())
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator(device=dev)
    g.manual_seed(14)
    # a mixture of 256 components around the origin; inside a component the rows vary along 64 latent directions (what
    # makes a row's neighbours its own and lets sign bits tell them apart) plus a little isotropic noise
    comps = torch.randn((256, a.dim), generator=g, device=dev)
    latent = torch.randn((64, a.dim), generator=g, device=dev) / 8.0

    def draw(n):
        x = comps[torch.randint(0, 256, (n,), generator=g, device=dev)]
        x = x + torch.randn((n, 64), generator=g, device=dev) @ latent
        return (x + 0.05 * torch.randn((n, a.dim), generator=g, device=dev)).contiguous()
    data = draw(a.rows)
    nqmax = max(BATCHES)
    queries = draw(nqmax)
    ctx = api.Context(0, stream=0)
    bits = api.binary_quantize(ctx, api.PGV_F32, a.dim, data)
    qbits = api.binary_quantize(ctx, api.PGV_F32, a.dim, queries)
    quant_ms = timed(ctx, lambda: api.binary_quantize(ctx, api.PGV_F32, a.dim, data), a.reps)

    # float64 brute force: the 10 nearest rows of every query by L2
    q64 = queries.double()
    qn = (q64 * q64).sum(1)
    best_d = torch.full((nqmax, K2), float("inf"), dtype=torch.float64, device=dev)
    best_i = torch.full((nqmax, K2), -1, dtype=torch.int64, device=dev)
    for lo in range(0, a.rows, 50000):
        x = data[lo:lo + 50000].double()
        d = qn[:, None] - 2.0 * (q64 @ x.T) + (x * x).sum(1)[None, :]
        cd, ci = torch.topk(d, K2, dim=1, largest=False)
        md, mi = torch.topk(torch.cat([best_d, cd], 1), K2, dim=1, largest=False)
        best_i = torch.gather(torch.cat([best_i, ci + lo], 1), 1, mi)
        best_d = md
    del x, d
    truth = best_i.cpu().numpy()

    res = {"rows": a.rows, "nbits": a.dim, "k": K, "kc": KC, "k2": K2, "reps": a.reps, "cus": cus,
           "binary_quantize_rows_ms": quant_ms, "batches": []}
    for nq in BATCHES:
        qb, qf = qbits[:nq].contiguous(), queries[:nq].contiguous()
        out = (torch.empty((nq, K), dtype=torch.float32, device=dev), torch.empty((nq, K), dtype=torch.int64, device=dev))
        call_ms = timed(ctx, lambda: api.bit_topk(ctx, a.dim, qb, bits, K, out=out), a.reps)
        ctx.set_profiling(True)
        ctx.reset_stats()
        for _ in range(a.reps):
            api.bit_topk(ctx, a.dim, qb, bits, K, out=out)
        scan_ms = ctx.stats()["aux_ms"] / a.reps
        ctx.set_profiling(False)
        search_ms = timed(ctx, lambda: api.binary_search(ctx, api.PGV_L2SQ, api.PGV_F32, a.dim, qf, data, bits, KC, K2), a.reps)
        _, idx = api.binary_search(ctx, api.PGV_L2SQ, api.PGV_F32, a.dim, qf, data, bits, KC, K2)
        idx = idx.cpu().numpy()
        recall = float(np.mean([len(set(idx[i]) & set(truth[i])) / K2 for i in range(nq)]))
        # the route before pgv_bit_topk: one call per query, float8 per row, the sort left to the host
        calls = min(nq, 64)

        def per_query():
            for i in range(calls):
                api.bit_distance_batch(ctx, api.PGV_BIT_HAMMING, a.dim, qb[i], bits)
        dev_ms = timed(ctx, per_query, a.reps) * nq / calls
        bound = popcount_bound_ms(a.rows, a.dim, nq, cus)
        res["batches"].append({"nq": nq, "scan_kernel_ms": scan_ms, "bit_topk_ms": call_ms, "binary_search_ms": search_ms,
                               "recall_at_10": recall, "per_query_route_ms": dev_ms, "per_query_calls_made": calls,
                               "per_query_extrapolated": calls < nq, "popcount_bound_ms": bound,
                               "scan_fraction_of_bound": bound / scan_ms if scan_ms > 0 else None})
    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("| queries | scan kernel ms | popcount bound ms | bound / scan | `pgv_bit_topk` ms | per-query route ms | "
                    "`binary_search` ms | recall@10 |\n|---|---|---|---|---|---|---|---|\n")
            for b in res["batches"]:
                f.write("| %d | %.3f | %.3f | %.2f | %.3f | %.3f%s | %.3f | %.3f |\n" % (
                    b["nq"], b["scan_kernel_ms"], b["popcount_bound_ms"], b["scan_fraction_of_bound"], b["bit_topk_ms"],
                    b["per_query_route_ms"], " (%d calls, extrapolated)" % b["per_query_calls_made"] if b["per_query_extrapolated"] else "",
                    b["binary_search_ms"], b["recall_at_10"]))
    ctx.close()


if __name__ == "__main__":
    main()
