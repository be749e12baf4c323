#!/usr/bin/env python3
"""The HNSW walk over a bit mirror under bit_jaccard_ops beside the same walk under bit_hamming_ops: one set of rows
(tools/bench_bit_hnsw.py's: 1 M x 1536 bits, the binary_quantize image of the seeded fp32 mixture), one graph (built on
the device by pgv_host_hnsw_build over the 0/1 fp16 expansion under L2, i.e. a Hamming graph), one set of queries; two
mirrors, pgv_hnsw_upload_bits and pgv_hnsw_upload_jaccard, each walked with pgv_hnsw_search at ef_search = k = 40, 100
and 400.  The two metrics rank differently, so the walks visit different elements: next to queries/s the table gives the
elements scored per query and the time per scored element.  Recall is against the exact top-k of each metric
(pgv_bit_distance_batch over all rows) for the first --exact queries; an element counts when its distance is at most the
exact k-th distance.  Times are HIP events on the library's stream, the two walks timed in alternating rounds after a
warm-up of every shape, median and minimum over --reps rounds.  Prints one JSON line; --md FILE also writes the table.

usage: python tools/bench_jaccard_hnsw.py [--rows 1000000] [--dim 1536] [--queries 4096] [--reps 5] [--md FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pgvector_amd import _host, api  # noqa: E402

EFS = (40, 100, 400)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--queries", type=int, default=4096, help="queries in flight per walk call")
    ap.add_argument("--exact", type=int, default=64, help="queries whose exact top-k is computed for the recall")
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

    ctx = api.Context(0, stream=0)
    data = draw(a.rows)
    bits = api.binary_quantize(ctx, api.PGV_F32, a.dim, data)
    del data
    qbits = api.binary_quantize(ctx, api.PGV_F32, a.dim, draw(max(a.queries, 1024)))[:a.queries].contiguous()
    rows16 = expand16(bits)
    twin = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F16, a.dim, rows16)
    host_rows = rows16.cpu().numpy()
    del rows16
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    built = _host.hnsw_build(twin, host_rows, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=1024)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    del host_rows
    twin.close()
    mirrors = {"hamming": api.BitHnsw(ctx, a.dim, bits), "jaccard": api.JaccardHnsw(ctx, a.dim, bits)}
    for h in mirrors.values():
        h.set_graph(a.m, built["entry"], built["levels"], built["nbr_start"], built["nbr"])
    metric = {"hamming": api.PGV_BIT_HAMMING, "jaccard": api.PGV_BIT_JACCARD}
    nexact = min(a.exact, a.queries)
    exact = {name: torch.stack([torch.as_tensor(api.bit_distance_batch(ctx, metric[name], a.dim, qbits[q], bits)).float()
                                for q in range(nexact)]) for name in mirrors}  # (the walks hand back float32)
    res = {"rows": a.rows, "nbits": a.dim, "m": a.m, "ef_construction": a.ef_construction, "walk_queries": a.queries,
           "exact_queries": nexact, "reps": a.reps, "build_secs": build_s, "elements_linked": built["nelements"], "ef": []}
    for ef in EFS:
        routes = {name: (lambda h=h: h.search(qbits, ef, ef)) for name, h in mirrors.items()}
        outs = {name: fn() for name, fn in routes.items()}  # warm-up of every shape, and the answers
        ms = {name: [] for name in routes}
        for _ in range(a.reps):
            for name, fn in routes.items():
                ctx.timer_start()
                fn()
                ms[name].append(ctx.timer_stop())
        rec = {"ef": ef}
        for name in routes:
            elem, dist, scored = outs[name]
            med, best = statistics.median(ms[name]), min(ms[name])
            per_query = float(scored.float().mean().item())
            kth = torch.topk(exact[name], ef, dim=1, largest=False).values[:, -1:]
            hit = ((dist[:nexact] <= kth) & (elem[:nexact] >= 0)).sum().item()
            rec[name] = {"ms_median": med, "ms_min": best, "qps_median": a.queries / med * 1e3, "qps_best": a.queries / best * 1e3,
                         "scored_per_query": per_query, "ns_per_scored_element": med * 1e6 / (a.queries * per_query),
                         "recall_vs_exact": hit / (nexact * ef)}
        res["ef"].append(rec)
    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("| ef = k | Hamming walk q/s (median / best) | Jaccard walk q/s (median / best) | Jaccard / Hamming | scored per "
                    "query, Hamming / Jaccard | ns per scored element, Hamming / Jaccard | recall, Hamming / Jaccard |\n"
                    "|---|---|---|---|---|---|---|\n")
            for r in res["ef"]:
                hm, jc = r["hamming"], r["jaccard"]
                f.write("| %d | %.0f / %.0f | %.0f / %.0f | %.3f | %.0f / %.0f | %.2f / %.2f | %.4f / %.4f |\n" % (
                    r["ef"], hm["qps_median"], hm["qps_best"], jc["qps_median"], jc["qps_best"], jc["qps_median"] / hm["qps_median"],
                    hm["scored_per_query"], jc["scored_per_query"], hm["ns_per_scored_element"], jc["ns_per_scored_element"],
                    hm["recall_vs_exact"], jc["recall_vs_exact"]))
    for h in mirrors.values():
        h.close()
    ctx.close()


if __name__ == "__main__":
    main()
