#!/usr/bin/env python3
"""HNSW iterative scans on the device (pgv_hnsw_scan_*) at the HNSW config's shape (bench.py's hnsw_section: unit rows
around 64 components, inner product, m 16, ef_construction 64, graph built on the device by pgv_host_hnsw_build):

  first_batch   a scan's first batch against pgv_hnsw_search at the same ef (k = ef), ef 40 / 100 / 400: the price of
                keeping the discards.  Same process, alternating, median / min / max over --reps rounds
  resumed       the time of each of the first --batches batches of one scan at ef 40 with the mean pool its entry step
                read, and the state's bytes per query
  filtered      k = 10 under a filter keeping 10 % and 1 % of the rows: hnsw_iterative_search at ef 40 against one
                pgv_hnsw_search at each ef of a ladder up to 1000 -- the share of queries that get their 10 rows, and the
                share for which no ef <= 1000 does
  parent        with --parent-tree DIR (a built checkout of the parent commit): pgv_hnsw_search of this tree against that
                one's, one process per run, alternating, each importing its own tree's package and library; each side's
                run-to-run spread beside the difference of their medians

Device times are HIP events on the library's stream; `filtered` is wall-clock (its loop runs on the host).  Prints one
JSON line; --md FILE also writes the tables.

usage: python tools/bench_hnsw_iter.py [--rows 1000000] [--dim 1536] [--queries 2048] [--reps 7] [--graph FILE]
                                       [--parent-tree DIR] [--md FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the runs of `parent` import another checkout's package -- and with it that checkout's library)
sys.path.insert(0, os.environ.get("PGV_BENCH_TREE") or ROOT)

from pgvector_amd import _lib, api  # noqa: E402

EFS = (40, 100, 400)
LADDER = (40, 100, 200, 400, 1000)
K = 10


def spread(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "runs": len(ms)}


def make_data(torch, dev, rows, dim, nq, seed=21):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    comps = torch.rand((64, dim), generator=g, device=dev)
    data = torch.empty((rows, dim), device=dev)
    for lo in range(0, rows, 100000):
        hi = min(rows, lo + 100000)
        data[lo:hi] = comps[torch.randint(0, 64, (hi - lo,), generator=g, device=dev)] + \
            0.1 * torch.randn((hi - lo, dim), generator=g, device=dev)
        data[lo:hi] /= data[lo:hi].norm(dim=1, keepdim=True)
    q = comps[torch.randint(0, 64, (nq,), generator=g, device=dev)] + 0.1 * torch.randn((nq, dim), generator=g, device=dev)
    return data, (q / q.norm(dim=1, keepdim=True)).contiguous()


def timed(ctx, fn):
    ctx.timer_start()
    out = fn()
    return ctx.timer_stop(), out


def plain_only(a, ctx, mirror, q):
    """the child of `parent`: pgv_hnsw_search alone, median over --reps after a warm-up, one JSON line"""
    res = {"lib": _lib.LIB_PATH}
    for ef in EFS:
        mirror.search(q, ef, K)
        res[str(ef)] = statistics.median(timed(ctx, lambda: mirror.search(q, ef, K))[0] for _ in range(a.reps))
    print("PLAIN " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--ef-construction", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--graph", default=None, help="npz file: the built graph is loaded from it when it exists, else saved to it")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    data, q = make_data(torch, dev, a.rows, a.dim, a.queries)
    ctx = api.Context(0, stream=0)
    mirror = api.Hnsw(ctx, api.PGV_NEG_IP, api.PGV_F32, a.dim, data)
    build_s = None
    if a.graph and os.path.exists(a.graph):
        built = dict(np.load(a.graph))
    else:
        from pgvector_amd import _host
        host_rows = data.cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        built = _host.hnsw_build(mirror, host_rows, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=1024)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        del host_rows
        if a.graph:
            np.savez(a.graph, entry=built["entry"], levels=built["levels"], nbr_start=built["nbr_start"], nbr=built["nbr"])
    mirror.set_graph(a.m, int(built["entry"]), built["levels"], built["nbr_start"], built["nbr"])
    if a.plain_only:
        plain_only(a, ctx, mirror, q)
        return
    nq = a.queries
    res = {"rows": a.rows, "dim": a.dim, "m": a.m, "ef_construction": a.ef_construction, "queries": nq, "reps": a.reps,
           "build_secs": build_s}

    # ---- a scan's first batch against the plain search
    res["first_batch"] = []
    for ef in EFS:
        plain_out = mirror.search(q, ef, ef)
        with mirror.scan(q, ef) as s:
            first = s.next()
        agree = all(bool(torch.equal(x, y)) for x, y in zip(plain_out, (first[0], first[1], first[3])))
        ms = {"search": [], "scan_first": []}
        for _ in range(a.reps):
            ms["search"].append(timed(ctx, lambda: mirror.search(q, ef, ef))[0])
            with mirror.scan(q, ef) as s:
                ms["scan_first"].append(timed(ctx, s.next)[0])
        rec = {"ef": ef, "agree": agree, "search": spread(ms["search"]), "scan_first": spread(ms["scan_first"]),
               "discards_per_query": float(first[4].float().mean().item())}
        rec["ratio_of_medians"] = rec["scan_first"]["ms_median"] / rec["search"]["ms_median"]
        res["first_batch"].append(rec)

    # ---- resumed batches, and what the state takes
    words = (a.rows + 31) // 32 + 1
    cap = min(a.rows, 65536)
    res["state_bytes_per_query"] = {"pool": 8 * cap, "visited_bitmap": 4 * words, "counters": 16, "query_row": 4 * a.dim,
                                    "total": 8 * cap + 4 * words + 16 + 4 * a.dim, "discard_cap": cap}
    res["resumed"] = []
    with mirror.scan(q, 40) as s:
        pool = 0.0
        for b in range(a.batches):
            t, out = timed(ctx, s.next)
            res["resumed"].append({"batch": b, "ms": t, "us_per_query": 1e3 * t / nq, "pool_read_mean": pool,
                                   "scored_mean": float(out[3].float().mean().item())})
            pool = float(out[4].float().mean().item())

    # ---- the use case: k = 10 under a filter
    res["filtered"] = []
    for share in (0.10, 0.01):
        keep = np.random.default_rng(7).random(a.rows) < share
        keep_dev = torch.from_numpy(keep).to(dev)
        api.hnsw_iterative_search(mirror, q[:64].contiguous(), K, keep, 40)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, _, scored = api.hnsw_iterative_search(mirror, q, K, keep, 40)
        torch.cuda.synchronize()
        it_s = time.perf_counter() - t0
        rec = {"keep_share": share, "iterative_ef40": {"secs": it_s, "qps": nq / it_s, "queries_with_k": sum(len(x) >= K for x in ids) / nq,
                                                        "scored_mean": float(np.mean(scored))}, "single_search": []}
        served = torch.zeros(nq, dtype=torch.bool, device=dev)
        for ef in LADDER:
            mirror.search(q, ef, ef)
            t, (elem, _, _) = timed(ctx, lambda: mirror.search(q, ef, ef))
            ok = (keep_dev[elem.clamp(min=0)] & (elem >= 0)).sum(1) >= K
            served |= ok
            rec["single_search"].append({"ef": ef, "ms": t, "qps": nq / t * 1e3, "queries_with_k": float(ok.float().mean().item())})
        rec["no_ef_up_to_1000"] = 1.0 - float(served.float().mean().item())
        res["filtered"].append(rec)

    # ---- the plain search against another build of the library
    if a.parent_tree:
        graph = a.graph
        if not graph:
            graph = os.path.join(ROOT, "build", "bench_hnsw_iter_graph.npz")
            os.makedirs(os.path.dirname(graph), exist_ok=True)
            np.savez(graph, entry=built["entry"], levels=built["levels"], nbr_start=built["nbr_start"], nbr=built["nbr"])
        runs = {"this": [], "parent": []}
        for _ in range(max(5, a.reps)):
            for side, tree in (("this", ROOT), ("parent", os.path.abspath(a.parent_tree))):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--graph", graph, "--rows", str(a.rows),
                                    "--dim", str(a.dim), "--queries", str(nq), "--m", str(a.m), "--reps", str(a.reps)],
                                   env=dict(os.environ, PGV_BENCH_TREE=tree), stdout=subprocess.PIPE, text=True, timeout=300, check=True)
                runs[side].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("PLAIN ")][-1][6:]))
        res["parent"] = []
        res["parent_libs"] = sorted({r["lib"] for side in runs.values() for r in side})
        for ef in EFS:
            this, parent = [r[str(ef)] for r in runs["this"]], [r[str(ef)] for r in runs["parent"]]
            rec = {"ef": ef, "this": spread(this), "parent": spread(parent)}
            rec["median_difference_ms"] = rec["this"]["ms_median"] - rec["parent"]["ms_median"]
            rec["inside_parent_spread"] = rec["parent"]["ms_min"] <= rec["this"]["ms_median"] <= rec["parent"]["ms_max"]
            res["parent"].append(rec)
    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("%d x %d, m %d, ef_construction %d, %d queries, %d rounds\n\n" % (a.rows, a.dim, a.m, a.ef_construction, nq, a.reps))
            f.write("| ef | `pgv_hnsw_search` ms (median, min - max) | scan's first batch ms (median, min - max) | ratio | discards kept per "
                    "query | same answers |\n|---|---|---|---|---|---|\n")
            for r in res["first_batch"]:
                f.write("| %d | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.3f | %.0f | %s |\n" % (
                    r["ef"], r["search"]["ms_median"], r["search"]["ms_min"], r["search"]["ms_max"], r["scan_first"]["ms_median"],
                    r["scan_first"]["ms_min"], r["scan_first"]["ms_max"], r["ratio_of_medians"], r["discards_per_query"],
                    "yes" if r["agree"] else "NO"))
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
            if "parent" in res:
                f.write("\n| ef | this tree ms (median, min - max) | parent ms (median, min - max) | difference of medians | inside the parent's "
                        "spread |\n|---|---|---|---|---|\n")
                for r in res["parent"]:
                    f.write("| %d | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %+.3f | %s |\n" % (
                        r["ef"], r["this"]["ms_median"], r["this"]["ms_min"], r["this"]["ms_max"], r["parent"]["ms_median"],
                        r["parent"]["ms_min"], r["parent"]["ms_max"], r["median_difference_ms"], "yes" if r["inside_parent_spread"] else "no"))
    mirror.close()
    ctx.close()


if __name__ == "__main__":
    main()
