#!/usr/bin/env python3
"""Exact sparse retrieval at a learned-sparse shape: pgv_sparse_topk by inner product over 1 M rows of about 128 stored
elements out of 30 522 dimensions (a BERT word-piece vocabulary), for batches of 64 and 1024 queries of about 32 and
about 128 stored elements, k = 10.  Per (query nnz, batch): the whole call, the scan kernel alone (the context's
profiling events around sparse_tile_kernel) and the kernel's row-stream rate -- 8 bytes per stored row element, read once
per query TILE (the host plan's rule is restated in tiles_of below) -- beside the 8 TB/s HBM peak.  The rate counts what
the algorithm must read; re-reads of a row block by consecutive tiles that hit the caches are in it, so it is no HBM
measurement.  Every vector has one element in each of its strata of the dimensions (sorted and distinct by construction)
with positive weights; the nnz of a vector varies by a quarter around the nominal.  Times are HIP events, medians over
--reps calls after a warm-up call; every array lives on the device.  Two queries per shape are checked against a dense
torch scan.  Prints one JSON line; --md FILE also writes the table.

usage: python tools/bench_sparse_topk.py [--rows 1000000] [--dim 30522] [--reps 5] [--md profiles/r21_sparse_topk.md]
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

BATCHES = (64, 1024)
QUERY_NNZ = (32, 128)
ROW_NNZ = 128
K = 10
TILE_NNZ, TILE_QUERIES = 2048, 128  # kSparseTileNnz, kSparseTileQueries (pgvector_amd/csrc/kernels_sparse.hip)
HBM_PEAK = 8e12


def tiles_of(ptr):
    """sparse_plan_tiles: consecutive queries while they fit TILE_NNZ stored elements and TILE_QUERIES queries"""
    nnz = np.diff(ptr)
    tiles, q = 0, 0
    while q < len(nnz):
        cnt, held = 0, 0
        while q < len(nnz) and cnt < TILE_QUERIES and (cnt == 0 or held + nnz[q] <= TILE_NNZ):
            held += nnz[q]
            cnt += 1
            q += 1
        tiles += 1
    return tiles


def draw(torch, g, n, dim, nominal):
    """n sparse vectors as a CSR triple on the device: nnz in [3/4, 5/4] of nominal, one element per stratum"""
    dev = g.device
    hi = nominal + nominal // 4
    width = dim // hi
    cand = torch.arange(hi, device=dev, dtype=torch.int64)[None, :] * width + torch.randint(0, width, (n, hi), generator=g, device=dev)
    count = torch.randint(nominal - nominal // 4, hi + 1, (n,), generator=g, device=dev)
    keep = torch.rand((n, hi), generator=g, device=dev).argsort(dim=1).argsort(dim=1) < count[:, None]
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(count, 0)
    val = torch.rand((n, hi), generator=g, device=dev) * 2 + 0.01
    return ptr.contiguous(), cand[keep].to(torch.int32).contiguous(), val[keep].contiguous()


def timed(ctx, fn, reps):
    fn()
    out = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        out.append(ctx.timer_stop())
    return statistics.median(out)


def dense_check(torch, dim, queries, rows, q, dist, idx):
    """query q's head against a dense scan: the same rows up to ties, values within 1e-5 of the terms' size"""
    qp, qi, qv = queries
    rp, ri, rv = rows
    dense = torch.zeros(dim, dtype=torch.float64, device=rv.device)
    dense[qi[qp[q]:qp[q + 1]].long()] = qv[qp[q]:qp[q + 1]].double()
    row_of = torch.repeat_interleave(torch.arange(len(rp) - 1, device=rv.device), rp[1:] - rp[:-1])
    score = torch.zeros(len(rp) - 1, dtype=torch.float64, device=rv.device).index_add_(0, row_of, dense[ri.long()] * rv.double())
    want = torch.topk(score, K).values
    got = -dist[q].double()
    return bool(torch.allclose(got, want, rtol=1e-5, atol=0)) and bool(torch.allclose(score[idx[q]], want, rtol=1e-5, atol=0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=30522)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(21)
    rows = draw(torch, g, a.rows, a.dim, ROW_NNZ)
    row_elems = int(rows[0][-1])
    ctx = api.Context(0, stream=0)
    res = {"rows": a.rows, "dim": a.dim, "row_nnz_total": row_elems, "k": K, "reps": a.reps,
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "shapes": []}
    for qnnz in QUERY_NNZ:
        allq = draw(torch, g, max(BATCHES), a.dim, qnnz)
        for nq in BATCHES:
            end = int(allq[0][nq])
            queries = (allq[0][:nq + 1].contiguous(), allq[1][:end].contiguous(), allq[2][:end].contiguous())
            out = (torch.empty((nq, K), dtype=torch.float32, device=dev), torch.empty((nq, K), dtype=torch.int64, device=dev))

            def call():
                return api.sparse_topk(ctx, api.PGV_NEG_IP, a.dim, queries, rows, K, out=out)
            call_ms = timed(ctx, call, a.reps)
            ctx.set_profiling(True)
            ctx.reset_stats()
            for _ in range(a.reps):
                call()
            scan_ms = ctx.stats()["aux_ms"] / a.reps
            ctx.set_profiling(False)
            dist, idx = call()
            ok = all(dense_check(torch, a.dim, queries, rows, q, dist, idx) for q in (0, nq - 1))
            passes = tiles_of(queries[0].cpu().numpy())
            stream = 8.0 * row_elems * passes
            res["shapes"].append({"query_nnz": qnnz, "nq": nq, "query_nnz_total": end, "tiles": passes, "sparse_topk_ms": call_ms,
                                  "scan_kernel_ms": scan_ms, "row_stream_bytes": stream,
                                  "row_stream_tb_s": stream / (scan_ms * 1e-3) / 1e12 if scan_ms > 0 else None,
                                  "share_of_hbm_peak": stream / (scan_ms * 1e-3) / HBM_PEAK if scan_ms > 0 else None,
                                  "pairs_per_s": a.rows * nq / (scan_ms * 1e-3) if scan_ms > 0 else None,
                                  "matches_dense_scan": ok})
    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("| query nnz | queries | tiles (row passes) | scan kernel ms | `pgv_sparse_topk` ms | row stream TB/s | of 8 TB/s | "
                    "G pairs/s | dense check |\n|---|---|---|---|---|---|---|---|---|\n")
            for s in res["shapes"]:
                f.write("| %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.2f | %s |\n" % (
                    s["query_nnz"], s["nq"], s["tiles"], s["scan_kernel_ms"], s["sparse_topk_ms"], s["row_stream_tb_s"],
                    s["share_of_hbm_peak"], s["pairs_per_s"] / 1e9, "ok" if s["matches_dense_scan"] else "MISMATCH"))
    ctx.close()


if __name__ == "__main__":
    main()
