#!/usr/bin/env python3
"""hnswvacuum's RepairGraph on the device (pgv_host_hnsw_repair) at the HNSW config's shape -- the graph of
tools/bench_hnsw_iter.py: unit rows around 64 components, inner product, m 16, ef_construction 64, built on the device.

For 1 %, 10 % and 30 % of the elements marked dead, uniformly at random:
  repair    wall time of api.Hnsw.repair at --max-batch with its phase split and counters
  rebuild   wall time of a fresh pgv_host_hnsw_build over the survivors in the same process: what a caller can do without
            the repair
  recall    recall@10 at ef 100 against the exact 10 nearest SURVIVORS of each query, of (a) the unrepaired graph with the
            dead dropped from its answers, (b) the repaired graph, (c) the rebuilt graph

Wall-clock times (the repair's back-link replay and the build's host side run on the CPU).  Prints one JSON line per dead
share as it goes and one at the end; --md FILE also writes the table.

usage: python tools/bench_hnsw_repair.py [--rows 1000000] [--dim 1536] [--queries 2048] [--max-batch 1024] [--graph FILE]
                                         [--shares 0.01,0.1,0.3] [--md FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_hnsw_iter import make_data  # noqa: E402
from pgvector_amd import _host, api  # noqa: E402

K, EF = 10, 100


def exact_topk(torch, data, q, live_dev):
    """the K nearest live rows of every query under the negative inner product, by brute force on the device"""
    out = []
    for lo in range(0, q.shape[0], 128):
        s = q[lo:lo + 128] @ data.T
        s[:, ~live_dev] = -float("inf")
        out.append(s.topk(K, dim=1).indices)
    return torch.cat(out).cpu().numpy()


def recall(found_rows, truth):
    hit = sum(len(set(f[:K]) & set(t)) for f, t in zip(found_rows, truth))
    return hit / float(truth.size)


def live_answers(elem, live, rows_of=None):
    """per query the first K live elements of its answer, as row numbers"""
    out = []
    for row in np.asarray(elem.cpu() if hasattr(elem, "cpu") else elem):
        ids = [int(e) for e in row if e >= 0 and (rows_of is not None or live[e])][:K]
        out.append([int(rows_of[e]) for e in ids] if rows_of is not None else ids)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--ef-construction", type=int, default=64)
    ap.add_argument("--max-batch", type=int, default=1024)
    ap.add_argument("--shares", default="0.01,0.1,0.3")
    ap.add_argument("--graph", default=None, help="npz file: the built graph is loaded from it when it exists, else saved to it")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    data, q = make_data(torch, dev, a.rows, a.dim, a.queries)
    host_rows = data.cpu().numpy()
    ctx = api.Context(0, stream=0)
    mirror = api.Hnsw(ctx, api.PGV_NEG_IP, api.PGV_F32, a.dim, data)
    build_s = None
    if a.graph and os.path.exists(a.graph):
        built = dict(np.load(a.graph))
    else:
        t0 = time.perf_counter()
        built = _host.hnsw_build(mirror, host_rows, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=1024)
        build_s = time.perf_counter() - t0
        if a.graph:
            np.savez(a.graph, entry=built["entry"], levels=built["levels"], nbr_start=built["nbr_start"], nbr=built["nbr"])
    graph = (int(built["entry"]), built["levels"], built["nbr_start"], built["nbr"])
    res = {"rows": a.rows, "dim": a.dim, "m": a.m, "ef_construction": a.ef_construction, "queries": a.queries,
           "max_batch": a.max_batch, "build_secs": build_s, "shares": []}
    for share in [float(s) for s in a.shares.split(",")]:
        live = np.random.default_rng(11).random(a.rows) >= share
        live_dev = torch.from_numpy(live).to(dev)
        truth = exact_topk(torch, data, q, live_dev)
        rec = {"dead_share": share, "dead": int((~live).sum())}
        # (a) the graph as the deletes left it, the dead dropped from the answers
        mirror.set_graph(a.m, *graph)
        rec["recall_unrepaired_filtered"] = recall(live_answers(mirror.search(q, EF, EF)[0], live), truth)
        # (b) repaired
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = mirror.repair(live, a.m, a.ef_construction, max_batch=a.max_batch, graph=graph)
        torch.cuda.synchronize()
        rec["repair_secs"] = time.perf_counter() - t0
        rec["repair"] = {k: out[k] for k in ("examined", "repaired", "batches", "overflow_redos", "device_pairs", "reselections",
                                             "dead_cap", "phase_secs")}
        elem = mirror.search(q, EF, EF)[0]
        found = np.asarray(elem.cpu())
        rec["dead_in_repaired_answers"] = int((~live[found[found >= 0]]).sum())
        rec["recall_repaired"] = recall(live_answers(elem, live), truth)
        # (c) rebuilt over the survivors
        rows_of = np.nonzero(live)[0]
        sub = np.ascontiguousarray(host_rows[rows_of])
        fresh = api.Hnsw(ctx, api.PGV_NEG_IP, api.PGV_F32, a.dim, sub)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b2 = _host.hnsw_build(fresh, sub, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=1024)
        torch.cuda.synchronize()
        rec["rebuild_secs"] = time.perf_counter() - t0
        fresh.set_graph(a.m, int(b2["entry"]), b2["levels"], b2["nbr_start"], b2["nbr"])
        rec["recall_rebuilt"] = recall(live_answers(fresh.search(q, EF, EF)[0], live, rows_of), truth)
        fresh.close()
        del sub, b2
        res["shares"].append(rec)
        print("SHARE " + json.dumps(rec), flush=True)
    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("%d x %d, m %d, ef_construction %d, %d queries, max_batch %d; recall@%d at ef %d against the exact nearest survivors\n\n"
                    % (a.rows, a.dim, a.m, a.ef_construction, a.queries, a.max_batch, K, EF))
            f.write("| dead | repair s | searches + selection | back-link replay | pair scoring | graph patch | repaired | batches | "
                    "reselections | overflow redos | rebuild s | recall unrepaired, filtered | recall repaired | recall rebuilt |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in res["shares"]:
                p = r["repair"]["phase_secs"]
                f.write("| %.0f %% | %.2f | %.2f | %.2f | %.2f | %.2f | %d | %d | %d | %d | %.2f | %.4f | %.4f | %.4f |\n" % (
                    100 * r["dead_share"], r["repair_secs"], p["search"], p["links"], p["pairs"], p["patch"], r["repair"]["repaired"],
                    r["repair"]["batches"], r["repair"]["reselections"], r["repair"]["overflow_redos"], r["rebuild_secs"],
                    r["recall_unrepaired_filtered"], r["recall_repaired"], r["recall_rebuilt"]))
    mirror.close()
    ctx.close()


if __name__ == "__main__":
    main()
