#!/usr/bin/env python3
"""IVFFlat over bit strings at 1 M x 1536 bits, lists 1000, 1024 queries, k = 100: `pgv_search_batch` on a bit index
(api.build_bit_ivf: pgv_bit_kmeans over 50 rows a list, pgv_bit_assign, the upload) at probes 10 and 32 -- the list scan
alone (the context's profiling events around hamming_list_kernel, with the pairs and rows the plan counted on the
device), the whole call, and its recall@k against the exact Hamming top-k -- beside `pgv_bit_topk` over the same rows in
the same run and, with --hnsw, `BitHnsw.search` over a graph built as tools/bench_bit_hnsw.py builds it, at ef = k = 40,
100 and 400 with the same recall measure (an answer counts when its distance is at most the exact k-th: ties are answers
too).  The rows are the binary_quantize image of tools/bench_bit_topk.py's seeded fp32 mixture.  Times are HIP events on
the library's stream; the routes are timed in alternating rounds after a warm-up of every shape, median and minimum over
--reps rounds.  Prints one JSON line; --md FILE also writes the tables.

usage: python tools/bench_bit_ivf.py [--rows 1000000] [--dim 1536] [--lists 1000] [--queries 1024] [--reps 5] [--hnsw] [--md FILE]
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

K = 100
PROBES = (10, 32)
EFS = (40, 100, 400)
CLOCK_HZ, HBM_BYTES_PER_S = 2.4e9, 8e12


def popcount_bound_ms(pairs, nbits, cus):
    """the least time the vector ALUs need: one xor and one accumulating popcount per 32-bit word of a
    (row, query) pair, 64 lane-operations per clock and CU"""
    return pairs * ((nbits + 31) // 32) * 2 / (cus * 64 * CLOCK_HZ) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--lists", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hnsw", action="store_true", help="also build an HNSW graph over the same rows and time BitHnsw.search")
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--ef-construction", type=int, default=64)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator(device=dev)
    g.manual_seed(14)
    comps = torch.randn((256, a.dim), generator=g, device=dev)
    latent = torch.randn((64, a.dim), generator=g, device=dev) / 8.0

    def draw(n):  # tools/bench_bit_topk.py's mixture
        x = comps[torch.randint(0, 256, (n,), generator=g, device=dev)]
        x = x + torch.randn((n, 64), generator=g, device=dev) @ latent
        return (x + 0.05 * torch.randn((n, a.dim), generator=g, device=dev)).contiguous()

    ctx = api.Context(0, stream=0)
    data = draw(a.rows)
    bits = api.binary_quantize(ctx, api.PGV_F32, a.dim, data)
    del data
    qbits = api.binary_quantize(ctx, api.PGV_F32, a.dim, draw(a.queries))
    row_bytes = ((a.dim + 7) // 8 + 15) // 16 * 16

    # the build: k-means over 50 rows a list (the reference's sample, src/ivfbuild.c), assignment, sort, upload
    host_bits = bits.cpu().numpy()
    srng = np.random.default_rng(16)
    samples = host_bits[np.sort(srng.choice(a.rows, min(a.rows, 50 * a.lists), replace=False))]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    centers, _, iters = api.bit_kmeans(ctx, a.dim, samples, a.lists, rng=api.make_rng(seed=16), want_closest=False)
    torch.cuda.synchronize()
    kmeans_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    assigned, _ = api.bit_assign(ctx, a.dim, centers, host_bits, want_dist=False)
    torch.cuda.synchronize()
    assign_s = time.perf_counter() - t0
    order = np.argsort(assigned, kind="stable")
    offsets = np.zeros(a.lists + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(assigned, minlength=a.lists))
    ix = api.BitIvfIndex(ctx, a.dim, centers, offsets, host_bits[order], tids=order.astype(np.uint64))
    lens = np.diff(offsets)

    out_t = (torch.empty((a.queries, K), dtype=torch.float32, device=dev), torch.empty((a.queries, K), dtype=torch.int64, device=dev))
    out_i = (torch.empty((a.queries, K), dtype=torch.float32, device=dev), torch.empty((a.queries, K), dtype=torch.int64, device=dev),
             torch.empty((a.queries, K), dtype=torch.int64, device=dev))
    routes = {"bit_topk": lambda: api.bit_topk(ctx, a.dim, qbits, bits, K, out=out_t)}
    for p in PROBES:
        routes["ivf_probes_%d" % p] = (lambda p=p: ix.search_batch(qbits, p, K, want_tid=True, out=out_i))
    exact_d = routes["bit_topk"]()[0].clone()
    kth = exact_d[:, -1:]
    recall = {}
    for p in PROBES:
        dist, slot, _ = routes["ivf_probes_%d" % p]()
        recall[p] = ((dist <= kth) & (slot >= 0)).sum().item() / (a.queries * K)
    ms = {name: [] for name in routes}
    for _ in range(a.reps):
        for name, fn in routes.items():
            ctx.timer_start()
            fn()
            ms[name].append(ctx.timer_stop())

    res = {"rows": a.rows, "nbits": a.dim, "lists": a.lists, "queries": a.queries, "k": K, "reps": a.reps, "cus": cus,
           "build": {"kmeans_samples": int(samples.shape[0]), "kmeans_iterations": iters, "kmeans_secs": kmeans_s,
                     "assign_secs": assign_s, "list_len_min": int(lens.min()), "list_len_max": int(lens.max())},
           "bit_topk": {"ms_median": statistics.median(ms["bit_topk"]), "ms_min": min(ms["bit_topk"])}, "probes": []}
    # the scan kernel alone: profiling events around it, pairs and streamed rows accumulated by the plan on the device
    ctx.set_profiling(True)
    for p in PROBES:
        ctx.reset_stats()
        for _ in range(a.reps):
            routes["ivf_probes_%d" % p]()
        st = ctx.stats()
        scan_ms, pairs, rows = st["scan_ms"] / a.reps, st["scan_pairs"] / a.reps, st["scan_rows"] / a.reps
        bound = popcount_bound_ms(pairs, a.dim, cus)
        name = "ivf_probes_%d" % p
        res["probes"].append({"probes": p, "share": a.queries * p / a.lists, "call_ms_median": statistics.median(ms[name]),
                              "call_ms_min": min(ms[name]), "scan_kernel_ms": scan_ms, "pairs": pairs, "rows_streamed": rows,
                              "popcount_bound_ms": bound, "fraction_of_popcount_bound": bound / scan_ms if scan_ms else None,
                              "fraction_of_hbm_peak": rows * row_bytes / (scan_ms * 1e-3) / HBM_BYTES_PER_S if scan_ms else None,
                              "recall_at_k": recall[p],
                              "speedup_over_bit_topk": statistics.median(ms["bit_topk"]) / statistics.median(ms[name])})
    ctx.set_profiling(False)

    if a.hnsw:
        shifts = torch.arange(7, -1, -1, device=dev, dtype=torch.uint8)
        rows16 = torch.empty((a.rows, a.dim), dtype=torch.float16, device=dev)
        for lo in range(0, a.rows, 100000):  # packed bits -> 0/1 fp16 rows: what the graph is built over
            b = bits[lo:lo + 100000]
            rows16[lo:lo + 100000] = ((b[:, :, None] >> shifts[None, None, :]) & 1).reshape(b.shape[0], -1)[:, :a.dim].half()
        twin = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F16, a.dim, rows16)
        host_rows = rows16.cpu().numpy()
        del rows16
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        built = _host.hnsw_build(twin, host_rows, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=1024)
        torch.cuda.synchronize()
        res["hnsw"] = {"m": a.m, "ef_construction": a.ef_construction, "build_secs": time.perf_counter() - t0, "ef": []}
        del host_rows
        twin.close()
        mirror = api.BitHnsw(ctx, a.dim, bits)
        mirror.set_graph(a.m, built["entry"], built["levels"], built["nbr_start"], built["nbr"])
        for ef in EFS:
            exact_ef = api.bit_topk(ctx, a.dim, qbits, bits, ef)[0][:, -1:]
            elem, dist, _ = mirror.search(qbits, ef, ef)
            t = []
            for _ in range(a.reps):
                ctx.timer_start()
                mirror.search(qbits, ef, ef)
                t.append(ctx.timer_stop())
            res["hnsw"]["ef"].append({"ef": ef, "ms_median": statistics.median(t), "ms_min": min(t),
                                      "recall_at_ef": ((dist <= exact_ef) & (elem >= 0)).sum().item() / (a.queries * ef)})
        mirror.close()

    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("| probes | queries per list | scan kernel ms | pairs | popcount bound ms | bound / scan | rows streamed | "
                    "of 8 TB/s | `pgv_search_batch` ms (median / best) | `pgv_bit_topk` ms (median / best) | bit_topk / search | "
                    "recall@%d |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n" % K)
            for r in res["probes"]:
                f.write("| %d | %.1f | %.3f | %.0f | %.3f | %.2f | %.0f | %.3f | %.3f / %.3f | %.3f / %.3f | %.1f | %.4f |\n" % (
                    r["probes"], r["share"], r["scan_kernel_ms"], r["pairs"], r["popcount_bound_ms"], r["fraction_of_popcount_bound"],
                    r["rows_streamed"], r["fraction_of_hbm_peak"], r["call_ms_median"], r["call_ms_min"],
                    res["bit_topk"]["ms_median"], res["bit_topk"]["ms_min"], r["speedup_over_bit_topk"], r["recall_at_k"]))
            if a.hnsw:
                f.write("\n| ef = k | `BitHnsw.search` ms for %d queries (median / best) | recall@ef |\n|---|---|---|\n" % a.queries)
                for r in res["hnsw"]["ef"]:
                    f.write("| %d | %.3f / %.3f | %.4f |\n" % (r["ef"], r["ms_median"], r["ms_min"], r["recall_at_ef"]))
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
