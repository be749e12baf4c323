#!/usr/bin/env python3
"""Filtered HNSW search with the iterative scan's loop on the device (pgv_hnsw_scan_filtered, api.hnsw_filtered_search)
against the same loop on the host (api.hnsw_iterative_search: one synchronised launch and five copies back per batch), at
tools/bench_hnsw_iter.py's shape: unit rows around 64 components, inner product, m 16, ef_construction 64, graph built on
the device; ef 40, k 10, max_scan_tuples 20 000, filters keeping 10 % and 1 % of the rows.

  rounds   both paths in one process, alternating, wall-clock (scan begin, launches, copies back, scan end), median / min /
           max over --reps rounds after a warm-up.  The fused path is timed with the filter as packed words in device memory
           (what a caller that filters often keeps) and once more with the boolean mask on the host, packed and uploaded
           inside the call.  Both paths must give the same element slots for every query: asserted
  launch   the HIP-event time of the single fused launch (the copies back of device-resident outputs are none), the mean
           batches, so->tuples and rows per query
  small    the same two paths with 1 and with 16 queries: where the launch round trips are the whole cost

Prints one JSON line; --md FILE also writes the tables.

usage: python tools/bench_hnsw_filtered.py [--rows 1000000] [--dim 1536] [--queries 2048] [--reps 7] [--graph FILE] [--md FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_hnsw_iter import K, make_data, spread, timed  # noqa: E402  (puts the tree's package on the path)
from pgvector_amd import api  # noqa: E402

EF, LIMIT = 40, 20000


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--ef-construction", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--graph", default=None, help="npz file: the built graph is loaded from it when it exists, else saved to it")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    assert a.reps >= 5, "at least five rounds"
    import torch
    dev = torch.device("cuda:0")
    data, q = make_data(torch, dev, a.rows, a.dim, a.queries)
    ctx = api.Context(0, stream=0)
    mirror = api.Hnsw(ctx, api.PGV_NEG_IP, api.PGV_F32, a.dim, data)
    if a.graph and os.path.exists(a.graph):
        built = dict(np.load(a.graph))
    else:
        from pgvector_amd import _host
        host_rows = data.cpu().numpy()
        built = _host.hnsw_build(mirror, host_rows, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=1024)
        del host_rows
        if a.graph:
            np.savez(a.graph, entry=built["entry"], levels=built["levels"], nbr_start=built["nbr_start"], nbr=built["nbr"])
    mirror.set_graph(a.m, int(built["entry"]), built["levels"], built["nbr_start"], built["nbr"])
    nq = a.queries
    res = {"rows": a.rows, "dim": a.dim, "m": a.m, "ef_construction": a.ef_construction, "queries": nq, "reps": a.reps,
           "ef": EF, "k": K, "max_scan_tuples": LIMIT, "filters": []}

    for share in (0.10, 0.01):
        keep = np.random.default_rng(7).random(a.rows) < share
        words = api.pack_keep(torch.from_numpy(keep).to(dev))

        def host_loop(qs):
            return api.hnsw_iterative_search(mirror, qs, K, keep, EF, max_scan_tuples=LIMIT)

        def fused(qs, filt=words):
            return api.hnsw_filtered_search(mirror, qs, K, filt, EF, max_scan_tuples=LIMIT)

        host_loop(q[:64].contiguous()), fused(q[:64].contiguous()), fused(q[:64].contiguous(), keep)  # warm-up
        ms = {"host_loop": [], "fused": [], "fused_host_mask": []}
        for _ in range(a.reps):
            t, want = wall(torch, lambda: host_loop(q))
            ms["host_loop"].append(t)
            t, got = wall(torch, lambda: fused(q))
            ms["fused"].append(t)
            assert got[0] == want[0], "the two paths disagree about a query's rows"
            assert np.array_equal(got[2], want[2]), "the two paths disagree about so->tuples"
            t, got = wall(torch, lambda: fused(q, keep))
            ms["fused_host_mask"].append(t)
            assert got[0] == want[0]
        rec = {"keep_share": share, "same_ids_every_query": True, "queries_with_k": sum(len(x) >= K for x in want[0]) / nq}
        for name, runs in ms.items():
            rec[name] = dict(spread(runs), qps_at_median=nq / statistics.median(runs) * 1e3)
        rec["host_loop_over_fused"] = rec["host_loop"]["ms_median"] / rec["fused"]["ms_median"]
        launches = []
        for _ in range(a.reps):
            with mirror.scan(q, EF) as s:
                t, out = timed(ctx, lambda: s.filtered(K, words, LIMIT))
            launches.append(t)
        rec["launch"] = dict(spread(launches), batches_mean=float(out[4].float().mean().item()),
                             batches_max=int(out[4].max().item()), scored_mean=float(out[3].float().mean().item()),
                             rows_mean=float(out[2].float().mean().item()))
        rec["small"] = []
        for n_small in (1, 16):
            qs = q[:n_small].contiguous()
            host_loop(qs), fused(qs)
            small = {"host_loop": [], "fused": []}
            for _ in range(a.reps):
                t, want_s = wall(torch, lambda: host_loop(qs))
                small["host_loop"].append(t)
                t, got_s = wall(torch, lambda: fused(qs))
                small["fused"].append(t)
                assert got_s[0] == want_s[0]
            rec["small"].append({"queries": n_small, "host_loop": spread(small["host_loop"]), "fused": spread(small["fused"])})
        res["filters"].append(rec)

    print(json.dumps(res))
    if a.md:
        def cell(s):
            return "%.2f (%.2f - %.2f)" % (s["ms_median"], s["ms_min"], s["ms_max"])
        with open(a.md, "w") as f:
            f.write("%d x %d, m %d, ef_construction %d, %d queries, ef %d, k %d, max_scan_tuples %d, %d rounds, wall-clock ms "
                    "(median, min - max)\n\n" % (a.rows, a.dim, a.m, a.ef_construction, nq, EF, K, LIMIT, a.reps))
            f.write("| filter keeps | host loop ms | fused ms (filter words on the device) | fused ms (boolean mask on the host) | host loop / "
                    "fused | host loop q/s | fused q/s | same ids |\n|---|---|---|---|---|---|---|---|\n")
            for r in res["filters"]:
                f.write("| %.0f %% | %s | %s | %s | %.2f | %.0f | %.0f | %s |\n" % (
                    100 * r["keep_share"], cell(r["host_loop"]), cell(r["fused"]), cell(r["fused_host_mask"]), r["host_loop_over_fused"],
                    r["host_loop"]["qps_at_median"], r["fused"]["qps_at_median"], "yes" if r["same_ids_every_query"] else "NO"))
            f.write("\n| filter keeps | the fused launch, HIP events ms | batches per query (mean, max) | so->tuples per query | rows per "
                    "query |\n|---|---|---|---|---|\n")
            for r in res["filters"]:
                x = r["launch"]
                f.write("| %.0f %% | %s | %.1f, %d | %.0f | %.2f |\n" % (100 * r["keep_share"], cell(x), x["batches_mean"], x["batches_max"],
                                                                    x["scored_mean"], x["rows_mean"]))
            f.write("\n| filter keeps | queries | host loop ms | fused ms |\n|---|---|---|---|\n")
            for r in res["filters"]:
                for x in r["small"]:
                    f.write("| %.0f %% | %d | %s | %s |\n" % (100 * r["keep_share"], x["queries"], cell(x["host_loop"]), cell(x["fused"])))
    mirror.close()
    ctx.close()


if __name__ == "__main__":
    main()
