#!/usr/bin/env python3
"""`ORDER BY emb <-> $1 LIMIT k` under a filter on an IVFFlat index: 1 M x 1536 fp32 L2, lists 1000, probes 10, 1024
queries, k = 10, filters that keep 100 %, 10 %, 1 % and 0.1 % of the rows (at 0.1 % a batch of 10 lists keeps about 10 rows:
the share at which queries start to need a second batch) -- one bitmap for all queries and one per query -- with
max_probes 10 (one batch) and 100 (the iterative scan).  Three routes, in one process:

  filtered    pgv_search_filtered (IvfIndex.search_filtered), bitmap and outputs on the device
  unfiltered  pgv_search_batch at the same probes with no filter: the fastest unfiltered answer (matrix cores + exact
              tail; the filtered route is exact-ALU, so it is expected to be slower at 100 %: the ratio is reported)
  host loop   the way to the same rows without the entry: pgv_rank_lists, then per query pgv_scan_lists batch by batch
              with the sort, the filter and the stop rule on the host.  Timed over the first --host-queries queries.

Times are wall-clock (time.perf_counter around a call that ends in a device synchronise), medians over --reps rounds in
which the routes alternate, after a warm-up of every shape.  Reported besides: the share of queries that reach k, the
mean probes_used, and the bytes the score kernel read (the kept rows of the rounds it ran: the context's profiling
counts) against the bytes of the lists those rounds probed.  Prints one JSON line; --md FILE also writes the table.

usage: python tools/bench_ivf_filtered.py [--rows 1000000] [--dim 1536] [--lists 1000] [--queries 1024] [--reps 5] [--md FILE]
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

from pgvector_amd import api  # noqa: E402

K, PROBES = 10, 10
SHARES = (1.0, 0.1, 0.01, 0.001)
MAX_PROBES = (10, 100)


def host_loop(ix, queries, ranked, offsets, keep, probes, max_probes, k):
    """the reference's loop with the list scan on the device and everything else here; keep: booleans [nq x n] or [n]"""
    out = []
    P = min(max(max_probes, probes), len(offsets) - 1)
    for q in range(len(queries)):
        kq = keep if keep.ndim == 1 else keep[q]
        got, used = [], 0
        while len(got) < k and used < P:
            batch, used = ranked[q, used:min(used + probes, P)], min(used + probes, P)
            dist, slot = ix.scan_lists(queries[q], batch)
            order = np.argsort(dist, kind="stable")
            kept = slot[order][kq[slot[order]]]
            got += kept[:k - len(got)].tolist()
        out.append(got)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--lists", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--host-queries", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(32)
    comps = torch.randn((256, a.dim), generator=g, device=dev)

    def draw(n):  # a mixture of 256 components: lists of uneven length, queries near the data
        x = comps[torch.randint(0, 256, (n,), generator=g, device=dev)]
        return (x + 0.5 * torch.randn((n, a.dim), generator=g, device=dev)).contiguous()

    ctx = api.Context(0, stream=0)
    data = draw(a.rows)
    queries = draw(a.queries)
    sample = data[torch.randperm(a.rows, generator=g, device=dev)[:min(a.rows, 50 * a.lists)]].contiguous()
    centers, _, _ = api.kmeans(ctx, api.PGV_OPS_L2, api.PGV_F32, a.dim, sample, a.lists, rng=api.make_rng(seed=32), want_closest=False)
    assigned, _ = api.assign(ctx, api.PGV_L2SQ, api.PGV_F32, a.dim, centers, data, want_dist=False)
    order = torch.argsort(assigned.long(), stable=True)
    offsets = torch.zeros(a.lists + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(torch.bincount(assigned.long(), minlength=a.lists), 0)
    rows = data[order].contiguous()
    del data
    ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, a.dim, centers, offsets, rows, tids=order.contiguous())
    del rows
    lens = (offsets[1:] - offsets[:-1])
    row_bytes = (a.dim * 4 + 15) // 16 * 16
    host_offsets = offsets.cpu().numpy()
    host_queries = queries[:a.host_queries].cpu().numpy()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    configs = []
    for share in SHARES:
        for kind in ("shared", "per query"):
            booleans = torch.rand((a.queries, a.rows) if kind == "per query" else (a.rows,), generator=g, device=dev) < share
            words = api.pack_keep(booleans)
            host_keep = (booleans[:a.host_queries] if kind == "per query" else booleans).cpu().numpy()
            del booleans
            for mp in MAX_PROBES:
                configs.append({"share": share, "kind": kind, "max_probes": mp, "words": words, "host_keep": host_keep})
    ranked = {mp: ix.rank_lists(queries, mp, want_dist=False)[0] for mp in MAX_PROBES}
    host_ranked = {mp: r[:a.host_queries].cpu().numpy() for mp, r in ranked.items()}

    def run_filtered(c):
        return ix.search_filtered(queries, PROBES, K, keep=c["words"], max_probes=c["max_probes"])

    def run_host(c):
        return host_loop(ix, host_queries, host_ranked[c["max_probes"]], host_offsets, c["host_keep"], PROBES, c["max_probes"], K)

    # warm-up of every shape, and the answers of the two routes to the same question side by side
    wall(lambda: ix.search_batch(queries, PROBES, K))
    for c in configs:
        _, (dist, slot, count, used) = wall(lambda: run_filtered(c))
        want = run_host(c)
        got = [s[:n].tolist() for s, n in zip(slot[:a.host_queries].cpu().numpy(), count[:a.host_queries].cpu().numpy())]
        c["same_rows_as_host_loop"] = got == want
        c["reach_k"] = (count == K).float().mean().item()
        c["probes_used"] = used.float().mean().item()
        ends = torch.cumsum(lens[ranked[c["max_probes"]].long()], 1)  # rows of a query's first j + 1 ranked lists
        c["probed_bytes"] = ends.gather(1, (used.long() - 1).clamp(min=0)[:, None]).sum().item() * row_bytes
        ctx.set_profiling(True)
        ctx.reset_stats()
        run_filtered(c)
        c["scored_bytes"] = ctx.stats()["scan_rows"] * row_bytes
        ctx.set_profiling(False)
        c["ms"], c["host_ms"] = [], []
    unfiltered_ms = []
    for _ in range(a.reps):
        unfiltered_ms.append(wall(lambda: ix.search_batch(queries, PROBES, K))[0])
        for c in configs:
            c["ms"].append(wall(lambda: run_filtered(c))[0])
            c["host_ms"].append(wall(lambda: run_host(c))[0])
    un = statistics.median(unfiltered_ms)
    res = {"rows": a.rows, "dim": a.dim, "lists": a.lists, "queries": a.queries, "probes": PROBES, "k": K, "reps": a.reps,
           "host_queries": a.host_queries, "list_len_min": int(lens.min()), "list_len_max": int(lens.max()),
           "unfiltered": {"ms_median": un, "ms_min": min(unfiltered_ms), "qps": a.queries / un * 1e3}, "configs": []}
    for c in configs:
        ms, hms = statistics.median(c["ms"]), statistics.median(c["host_ms"])
        res["configs"].append({"keep_share": c["share"], "bitmap": c["kind"], "max_probes": c["max_probes"], "ms_median": ms,
                               "ms_min": min(c["ms"]), "qps": a.queries / ms * 1e3, "over_unfiltered": ms / un,
                               "host_loop_qps": a.host_queries / hms * 1e3, "host_loop_ms_median": hms,
                               "speedup_over_host_loop": (a.queries / ms) / (a.host_queries / hms),
                               "reach_k": c["reach_k"], "probes_used_mean": c["probes_used"], "scored_bytes": c["scored_bytes"],
                               "probed_bytes": c["probed_bytes"], "same_rows_as_host_loop": c["same_rows_as_host_loop"]})
    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("`pgv_search_batch`, no filter, probes %d: %.3f ms median / %.3f best for %d queries = %.0f queries/s\n\n" % (
                PROBES, un, min(unfiltered_ms), a.queries, res["unfiltered"]["qps"]))
            f.write("| keep | bitmap | max_probes | `pgv_search_filtered` ms (median / best) | queries/s | time / unfiltered | host loop "
                    "queries/s (%d queries) | filtered / host loop | reach k | mean probes_used | bytes scored | bytes of the probed "
                    "lists | scored / probed | same rows as host loop |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n" % a.host_queries)
            for r in res["configs"]:
                f.write("| %g %% | %s | %d | %.3f / %.3f | %.0f | %.2f | %.0f | %.1f | %.3f | %.2f | %.3e | %.3e | %.4f | %s |\n" % (
                    100 * r["keep_share"], r["bitmap"], r["max_probes"], r["ms_median"], r["ms_min"], r["qps"], r["over_unfiltered"],
                    r["host_loop_qps"], r["speedup_over_host_loop"], r["reach_k"], r["probes_used_mean"], r["scored_bytes"],
                    r["probed_bytes"], r["scored_bytes"] / r["probed_bytes"] if r["probed_bytes"] else 0.0,
                    "yes" if r["same_rows_as_host_loop"] else "NO"))
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
