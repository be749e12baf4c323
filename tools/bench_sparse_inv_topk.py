#!/usr/bin/env python3
"""Exact sparse retrieval by posting lists beside the pair scan, at tools/bench_sparse_topk.py's shape: 1 M rows of about
128 stored elements out of 30 522 dimensions, batches of 64 and 1024 queries of about 32 and about 128 stored elements,
inner product, k = 10.  pgv_sparse_rows_topk over an uploaded mirror (api.SparseRows, kernels_sparse_inv.hip) and
pgv_sparse_topk(PGV_NEG_IP) run in the same process on the same data, alternating; per shape and path: the whole call and
the scan kernel alone (the context's profiling events around it).  The mirror's upload is timed too.  Values are the
integers 1 .. 8, so every sum is exact in fp32 whatever its order, and the tool ASSERTS that both paths return the same row
ids and the same distance bits.  Times are HIP events, medians over --reps after a warm-up; every array lives on the
device.  Prints one JSON line; --md FILE also writes the table (--label: a note for its heading, the build's block and
tile sizes for instance).

usage: python tools/bench_sparse_inv_topk.py [--rows 1000000] [--dim 30522] [--reps 5] [--md FILE] [--label TEXT]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_sparse_topk import BATCHES, K, QUERY_NNZ, ROW_NNZ, draw, timed  # noqa: E402
from pgvector_amd import _lib, api  # noqa: E402


def scan_ms(ctx, fn, reps):
    ctx.set_profiling(True)
    ctx.reset_stats()
    for _ in range(reps):
        fn()
    ms = ctx.stats()["aux_ms"] / reps
    ctx.set_profiling(False)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=30522)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(21)

    def integers(triple):
        return triple[0], triple[1], torch.floor(triple[2] * 4).clamp_(1, 8).contiguous()
    rows = integers(draw(torch, g, a.rows, a.dim, ROW_NNZ))
    ctx = api.Context(0, stream=0)
    uploads = []
    for _ in range(a.reps + 1):
        ctx.timer_start()
        mirror = api.SparseRows(ctx, a.dim, rows)
        uploads.append(ctx.timer_stop())
        if len(uploads) <= a.reps:
            mirror.free()
    res = {"label": a.label, "rows": a.rows, "dim": a.dim, "row_nnz_total": int(rows[0][-1]), "k": K, "reps": a.reps,
           "block_rows": _lib.SPARSE_INV_ROWS, "tile_queries": _lib.SPARSE_INV_QUERIES,
           "upload_ms": statistics.median(uploads[1:]), "shapes": []}
    for qnnz in QUERY_NNZ:
        allq = integers(draw(torch, g, max(BATCHES), a.dim, qnnz))
        for nq in BATCHES:
            end = int(allq[0][nq])
            queries = (allq[0][:nq + 1].contiguous(), allq[1][:end].contiguous(), allq[2][:end].contiguous())
            outs = [(torch.empty((nq, K), dtype=torch.float32, device=dev), torch.empty((nq, K), dtype=torch.int64, device=dev))
                    for _ in range(2)]

            def inv():
                return mirror.topk(queries, K, out=outs[0])

            def pair():
                return api.sparse_topk(ctx, api.PGV_NEG_IP, a.dim, queries, rows, K, out=outs[1])
            s = {"query_nnz": qnnz, "nq": nq}
            for name, fn in (("inv", inv), ("pair", pair), ("inv_again", inv)):
                s[name + "_call_ms"] = timed(ctx, fn, a.reps)
                s[name + "_scan_ms"] = scan_ms(ctx, fn, a.reps)
            ctx.sync()
            assert torch.equal(outs[0][1], outs[1][1]), "row ids differ at %d x %d" % (qnnz, nq)
            assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), "distances differ at %d x %d" % (qnnz, nq)
            s["same_answer"] = True
            res["shapes"].append(s)
    print(json.dumps(res))
    if a.md:
        with open(a.md, "a") as f:
            f.write("\n%s: upload %.1f ms\n\n| query nnz | queries | inverted scan ms | inverted call ms | (second pass) | pair scan ms | "
                    "`pgv_sparse_topk` ms | call ratio | same answer |\n|---|---|---|---|---|---|---|---|---|\n"
                    % (a.label or "rows %d" % a.rows, res["upload_ms"]))
            for s in res["shapes"]:
                f.write("| %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.1f | yes |\n" % (
                    s["query_nnz"], s["nq"], s["inv_scan_ms"], s["inv_call_ms"], s["inv_again_call_ms"], s["pair_scan_ms"],
                    s["pair_call_ms"], s["pair_call_ms"] / s["inv_call_ms"]))
    mirror.free()
    ctx.close()


if __name__ == "__main__":
    main()
