#!/usr/bin/env python3
"""CREATE INDEX over a sparsevec column on the device: the HNSW build over a sparse mirror
(pgv_hnsw_upload_sparse_buildable + pgv_host_hnsw_build_sparse), beside the route that existed before it --
pgv_host_hnsw_build over the elements' dense fp16 expansion -- in the same process, alternating which of the two goes first.

  the twin shape   tools/bench_sparse_hnsw.py's rows: --rows elements over --dim dimensions, about 64 stored integer-valued
                   elements each, inner product.  Seconds and phase_secs of every build, the device bytes each mirror's
                   rows hold (pgv_device_memory before and after the upload), whether the two graphs are equal array for
                   array (integer data: they should be).
  --big-dim D      a shape no twin can hold (D = 30522: a learned-sparse vocabulary; the dense types stop at 2 000 / 4 000
                   dimensions): the same draw over D dimensions with float values, --big-rows elements.  Build seconds and
                   recall@10 of the walk at ef 40 / 100 against pgv_sparse_topk (an element at the k-th distance counts).
  the scorer       PGV_HNSW_PAIRS_GATHER is read once per process: run the tool twice, with --only native, unset and = 1,
                   and compare the builds' `pairs` and `update` phases (sparse_groups_kernel against the gathered route
                   through sparse_pair_kernel on the build's own pair load).

Prints one JSON line; --md FILE also writes the table.

usage: python tools/bench_sparse_hnsw_build.py [--rows 1000000] [--dim 2048] [--rounds 2] [--only native] [--big-dim 30522] [--md FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_sparse_hnsw as walk_bench  # noqa: E402  (the draw and the fp16 expansion)
from pgvector_amd import _host, api  # noqa: E402

EFS = (40, 100)
K = 10
GRAPH = ("levels", "nbr_start", "nbr", "dup_of")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--ef-construction", type=int, default=64)
    ap.add_argument("--max-batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=2, help="native / twin pairs of builds; the order alternates")
    ap.add_argument("--only", choices=("native", "twin"), default=None, help="one kind of build per round (scorer A/B runs)")
    ap.add_argument("--big-dim", type=int, default=0, help="also build a float-valued shape over this many dimensions")
    ap.add_argument("--big-rows", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(24)
    hi = walk_bench.NNZ + walk_bench.NNZ // 4
    ctx = api.Context(0, stream=0)

    def free_bytes():
        free, total = C.c_uint64(), C.c_uint64()
        api.check(api.lib.pgv_device_memory(0, C.byref(free), C.byref(total)))
        return free.value

    def host(csr):
        return tuple(x.cpu().numpy() for x in csr)

    def build(kind, metric, dim, rows, host_rows, host_twin):
        """one upload and one build -> (record, graph, mirror)"""
        torch.cuda.synchronize()
        before = free_bytes()
        if kind == "fp16_twin":
            mirror = api.Hnsw(ctx, metric, api.PGV_F16, dim, host_twin)
        else:
            mirror = api.SparseHnsw(ctx, metric, dim, rows, buildable=True)
        held = before - free_bytes()
        t0 = time.perf_counter()
        if kind == "fp16_twin":
            built = _host.hnsw_build(mirror, host_twin, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=a.max_batch)
        else:
            built = _host.hnsw_build(mirror, None, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=a.max_batch,
                                     rows_csr=host_rows)
        ctx.sync()
        secs = time.perf_counter() - t0
        return ({"kind": kind, "dim": dim, "secs": secs, "phase_secs": built["phase_secs"], "row_bytes_on_device": held,
                 "elements_linked": built["nelements"], "batches": built["batches"], "device_pairs": built["device_pairs"]},
                built, mirror)

    res = {"rows": a.rows, "dim": a.dim, "m": a.m, "ef_construction": a.ef_construction, "max_batch": a.max_batch,
           "pairs_gather": os.environ.get("PGV_HNSW_PAIRS_GATHER", "0 (default)"), "builds": []}
    topic_offset = torch.randint(0, a.dim // hi, (walk_bench.TOPICS, hi), generator=g, device=dev)
    rows = walk_bench.draw(torch, g, a.rows, a.dim, topic_offset)
    host_rows = host(rows)
    res["row_nnz_total"] = int(host_rows[0][-1])
    host_twin = walk_bench.expand16(torch, rows, a.dim).cpu().numpy() if a.only != "native" else None
    torch.cuda.empty_cache()
    equal = []
    for r in range(a.rounds):
        order = ("native", "fp16_twin") if r % 2 == 0 else ("fp16_twin", "native")
        order = tuple(k for k in order if a.only is None or k.endswith(a.only))
        graphs = {}
        for kind in order:
            rec, built, mirror = build(kind, api.PGV_NEG_IP, a.dim, rows, host_rows, host_twin)
            rec["round"], rec["first_of_round"] = r, kind == order[0]
            mirror.close()
            graphs[kind] = built
            res["builds"].append(rec)
        if len(graphs) == 2:
            x, y = graphs["native"], graphs["fp16_twin"]
            equal.append(bool(x["entry"] == y["entry"] and x["batches"] == y["batches"] and x["nelements"] == y["nelements"] and
                              all(np.array_equal(x[k], y[k]) for k in GRAPH)))
    res["native_graph_equals_twin_graph"] = equal
    del host_twin, rows, host_rows
    if a.big_dim:
        topic_offset = torch.randint(0, a.big_dim // hi, (walk_bench.TOPICS, hi), generator=g, device=dev)
        ptr, idx, val = walk_bench.draw(torch, g, a.big_rows, a.big_dim, topic_offset)
        rows = (ptr, idx, (val * (0.25 + torch.rand(val.shape, generator=g, device=dev))).contiguous())   # float weights
        qp, qi, qv = walk_bench.draw(torch, g, a.queries, a.big_dim, topic_offset)
        queries = (qp, qi, (qv * (0.25 + torch.rand(qv.shape, generator=g, device=dev))).contiguous())
        rec, built, mirror = build("native", api.PGV_NEG_IP, a.big_dim, rows, host(rows), None)
        kth = api.sparse_topk(ctx, api.PGV_NEG_IP, a.big_dim, queries, rows, K)[0][:, -1:]
        rec["rows"], rec["recall_at_10"] = a.big_rows, {}
        for ef in EFS:
            elem, dist, _ = mirror.search(queries, ef, K)
            rec["recall_at_10"]["ef_%d" % ef] = ((dist <= kth) & (elem >= 0)).sum().item() / (a.queries * K)
        mirror.close()
        res["builds"].append(rec)
    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("| build | dim | round | first of its round | seconds | search / pairs / select / records / update / patch (s) | "
                    "row bytes on the device | elements linked | batches | recall@10 at ef 40 / 100 |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for b in res["builds"]:
                p = b["phase_secs"]
                rc = b.get("recall_at_10")
                f.write("| %s | %d | %s | %s | %.3f | %s | %d | %d | %d | %s |\n" % (
                    b["kind"], b["dim"], b.get("round", "-"), "yes" if b.get("first_of_round") else "-", b["secs"],
                    " / ".join("%.3f" % p[k] for k in ("search", "pairs", "select", "records", "update", "patch")),
                    b["row_bytes_on_device"], b["elements_linked"], b["batches"],
                    "%.4f / %.4f" % (rc["ef_40"], rc["ef_100"]) if rc else "-"))
            f.write("\nPGV_HNSW_PAIRS_GATHER: %s.  Native graph equal to the twin's, array for array, per round: %s\n" %
                    (res["pairs_gather"], ", ".join("yes" if e else "NO" for e in equal) or "-"))
    ctx.close()


if __name__ == "__main__":
    main()
