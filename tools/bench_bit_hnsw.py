#!/usr/bin/env python3
"""Stage one of the indexed binary-quantization query at 1 M x 1536 bits: the HNSW walk over a bit mirror
(pgv_hnsw_upload_bits + pgv_hnsw_search) beside (a) the same walk of the same graph over the elements' 0/1 fp16
expansion under L2 -- the twin that existed before bit mirrors, reading 16 times the row bytes -- and (b) the brute-force
pgv_bit_topk at 1024 queries, for ef_search = k = 40, 100 and 400, with each walk's recall against the exact Hamming
top-k (an element counts when its distance is at most the exact k-th distance: ties are answers too).  The rows are the
binary_quantize image of tools/bench_bit_topk.py's seeded fp32 mixture; the graph is built on the device by
pgv_host_hnsw_build over the fp16 expansion and set on both mirrors.  Times are HIP events on the library's stream; the
three routes are timed in alternating rounds after a warm-up of every shape, median and minimum over --reps rounds.
Prints one JSON line; --md FILE also writes the table.

usage: python tools/bench_bit_hnsw.py [--rows 1000000] [--dim 1536] [--queries 4096] [--reps 5] [--md FILE]
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
TOPK_QUERIES = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--queries", type=int, default=4096, help="queries in flight per walk call")
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--ef-construction", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(14)
    comps = torch.randn((256, a.dim), generator=g, device=dev)
    latent = torch.randn((64, a.dim), generator=g, device=dev) / 8.0

    def draw(n):  # tools/bench_bit_topk.py's mixture
        x = comps[torch.randint(0, 256, (n,), generator=g, device=dev)]
        x = x + torch.randn((n, 64), generator=g, device=dev) @ latent
        return (x + 0.05 * torch.randn((n, a.dim), generator=g, device=dev)).contiguous()

    def expand16(bits):  # packed bits -> 0/1 fp16 rows, first bit = top bit of byte 0
        shifts = torch.arange(7, -1, -1, device=dev, dtype=torch.uint8)
        out = torch.empty((bits.shape[0], a.dim), dtype=torch.float16, device=dev)
        for lo in range(0, bits.shape[0], 100000):
            b = bits[lo:lo + 100000]
            out[lo:lo + 100000] = ((b[:, :, None] >> shifts[None, None, :]) & 1).reshape(b.shape[0], -1)[:, :a.dim].half()
        return out

    nq = max(a.queries, TOPK_QUERIES)
    ctx = api.Context(0, stream=0)
    data = draw(a.rows)
    bits = api.binary_quantize(ctx, api.PGV_F32, a.dim, data)
    del data
    qbits = api.binary_quantize(ctx, api.PGV_F32, a.dim, draw(nq))
    rows16, q16 = expand16(bits), expand16(qbits)
    twin = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F16, a.dim, rows16)
    host_rows = rows16.cpu().numpy()
    del rows16
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    built = _host.hnsw_build(twin, host_rows, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=1024)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    del host_rows
    mirror = api.BitHnsw(ctx, a.dim, bits)
    mirror.set_graph(a.m, built["entry"], built["levels"], built["nbr_start"], built["nbr"])

    qb, qh = qbits[:a.queries].contiguous(), q16[:a.queries].contiguous()
    qt = qbits[:TOPK_QUERIES].contiguous()
    res = {"rows": a.rows, "nbits": a.dim, "m": a.m, "ef_construction": a.ef_construction, "walk_queries": a.queries,
           "topk_queries": TOPK_QUERIES, "reps": a.reps, "build_secs": build_s, "elements_linked": built["nelements"],
           "row_bytes": {"bit": mirror_row_bytes(a.dim), "fp16_twin": 2 * a.dim}, "ef": []}
    for ef in EFS:
        routes = {"bit_walk": lambda: mirror.search(qb, ef, ef), "fp16_twin_walk": lambda: twin.search(qh, ef, ef),
                  "bit_topk": lambda: api.bit_topk(ctx, a.dim, qt, bits, ef)}
        outs = {name: fn() for name, fn in routes.items()}  # warm-up of every shape, and the answers
        ms = {name: [] for name in routes}
        for _ in range(a.reps):
            for name, fn in routes.items():
                ctx.timer_start()
                fn()
                ms[name].append(ctx.timer_stop())
        exact_d = outs["bit_topk"][0]  # [1024 x ef] ascending
        kth = exact_d[:, -1:]
        rec = {"ef": ef}
        for name, count in (("bit_walk", a.queries), ("fp16_twin_walk", a.queries), ("bit_topk", TOPK_QUERIES)):
            med, best = statistics.median(ms[name]), min(ms[name])
            rec[name] = {"ms_median": med, "ms_min": best, "qps_median": count / med * 1e3, "qps_best": count / best * 1e3}
        for name in ("bit_walk", "fp16_twin_walk"):
            elem, dist, scored = outs[name]
            nrec = min(a.queries, TOPK_QUERIES)
            hit = ((dist[:nrec] <= kth[:nrec]) & (elem[:nrec] >= 0)).sum().item()
            rec[name]["recall_vs_exact_hamming"] = hit / (nrec * ef)
            rec[name]["scored_per_query"] = float(scored.float().mean().item())
        rec["walks_agree"] = bool(torch.equal(outs["bit_walk"][0], outs["fp16_twin_walk"][0]) and
                                  torch.equal(outs["bit_walk"][1], outs["fp16_twin_walk"][1]) and
                                  torch.equal(outs["bit_walk"][2], outs["fp16_twin_walk"][2]))
        res["ef"].append(rec)
    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("| ef = k | bit walk q/s (median / best) | fp16-twin walk q/s (median / best) | bit / twin | `pgv_bit_topk` q/s "
                    "at %d queries | walk recall | elements scored per query | walks agree |\n|---|---|---|---|---|---|---|---|\n"
                    % TOPK_QUERIES)
            for r in res["ef"]:
                f.write("| %d | %.0f / %.0f | %.0f / %.0f | %.2f | %.0f | %.4f | %.0f | %s |\n" % (
                    r["ef"], r["bit_walk"]["qps_median"], r["bit_walk"]["qps_best"], r["fp16_twin_walk"]["qps_median"],
                    r["fp16_twin_walk"]["qps_best"], r["bit_walk"]["qps_median"] / r["fp16_twin_walk"]["qps_median"],
                    r["bit_topk"]["qps_median"], r["bit_walk"]["recall_vs_exact_hamming"], r["bit_walk"]["scored_per_query"],
                    "yes" if r["walks_agree"] else "NO"))
    mirror.close()
    twin.close()
    ctx.close()


def mirror_row_bytes(nbits):
    return ((nbits + 7) // 8 + 15) // 16 * 16


if __name__ == "__main__":
    main()
