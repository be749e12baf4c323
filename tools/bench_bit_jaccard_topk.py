#!/usr/bin/env python3
"""Exact Tanimoto search at a fingerprint shape, 1 M x 2048 bits: pgv_bit_jaccard_topk for batches of 32 and 1024 queries
at k = 100 -- the scan kernel alone (the context's profiling events around jaccard_tile_kernel) and the whole call --
beside pgv_bit_topk's over the same rows and queries in the same process, the two in alternation, and what share of the
Jaccard scan its epilogue (the order image: two 32-bit divisions a pair) is: from the same pair of scans over a quarter
of the rows at four times the bits, where a pair's epilogue is the same and its counting four times as long.  The fingerprints are seeded random bits of density 0.1.
Times are HIP events, medians over --reps calls after a warm-up.

Each batch size runs in a child process of its own under a time limit; the first one that fails ends the run.  Prints
one JSON line; --md FILE also writes the table.

usage: python tools/bench_bit_jaccard_topk.py [--rows 1000000] [--nbits 2048] [--reps 5] [--md profiles/r33_bit_jaccard_topk.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (32, 1024)
K = 100
STEP_SECONDS = 240


def one(a, nq):
    import torch

    from pgvector_amd import api
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(33)

    def draw(n, nbits):
        weights = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.int32, device=dev)
        parts = [((torch.rand((min(65536, n - lo), nbits // 8, 8), generator=g, device=dev) < 0.1).int() * weights).sum(2)
                 for lo in range(0, n, 65536)]
        return torch.cat(parts).to(torch.uint8).contiguous()
    ctx = api.Context(0, stream=0)
    res = {"nq": nq}
    for nbits, rows in ((a.nbits, a.rows), (4 * a.nbits, a.rows // 4)):
        data, queries = draw(rows, nbits), draw(nq, nbits)
        out = (torch.empty((nq, K), dtype=torch.float32, device=dev), torch.empty((nq, K), dtype=torch.int64, device=dev))
        fns = {"hamming": api.bit_topk, "jaccard": api.bit_jaccard_topk}
        times = {name: ([], []) for name in fns}
        for fn in fns.values():  # warm-up
            fn(ctx, nbits, queries, data, K, out=out)
        for _ in range(a.reps):  # the two entries in alternation: the whole call, then the scan kernel's events alone
            for name, fn in fns.items():
                ctx.timer_start()
                fn(ctx, nbits, queries, data, K, out=out)
                times[name][0].append(ctx.timer_stop())
                ctx.set_profiling(True)
                ctx.reset_stats()
                fn(ctx, nbits, queries, data, K, out=out)
                times[name][1].append(ctx.stats()["aux_ms"])
                ctx.set_profiling(False)
        for name, (calls, scans) in times.items():
            res["%s_call_ms_%d" % (name, nbits)] = statistics.median(calls)
            res["%s_scan_ms_%d" % (name, nbits)] = statistics.median(scans)
            res["%s_scan_ms_%d_all" % (name, nbits)] = scans
        del data, queries
    ctx.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--nbits", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a, a.one)
    res = {"rows": a.rows, "nbits": a.nbits, "k": K, "reps": a.reps, "batches": []}
    for nq in BATCHES:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--nbits", str(a.nbits),
                                "--reps", str(a.reps), "--one", str(nq)], capture_output=True, text=True, timeout=STEP_SECONDS)
        if child.returncode != 0:
            sys.stderr.write(child.stderr)
            sys.exit("batch of %d queries ended with status %d: stopping" % (nq, child.returncode))
        b = json.loads(child.stdout.strip().splitlines()[-1])
        # the epilogue e of the Jaccard scan at nbits: what Jaccard costs over Hamming is e plus the row popcounts (p, in
        # proportion to the bits scanned) -- j - h = e + p at nbits and, with a quarter of the rows and four times the
        # bits, e / 4 + p
        j1, j4 = b["jaccard_scan_ms_%d" % a.nbits], b["jaccard_scan_ms_%d" % (4 * a.nbits)]
        h1, h4 = b["hamming_scan_ms_%d" % a.nbits], b["hamming_scan_ms_%d" % (4 * a.nbits)]
        b["scan_ratio"] = j1 / h1
        b["call_ratio"] = b["jaccard_call_ms_%d" % a.nbits] / b["hamming_call_ms_%d" % a.nbits]
        b["epilogue_share"] = ((j1 - h1) - (j4 - h4)) / 0.75 / j1
        res["batches"].append(b)
    print(json.dumps(res))
    if a.md:
        n1, n4 = a.nbits, 4 * a.nbits
        with open(a.md, "w") as f:
            f.write("| queries | `jaccard_tile_kernel` ms | `hamming_tile_kernel` ms | scan ratio | `pgv_bit_jaccard_topk` ms | "
                    "`pgv_bit_topk` ms | call ratio | Jaccard / Hamming scan ms at %d bits, rows / 4 | epilogue share of the "
                    "Jaccard scan |\n|---|---|---|---|---|---|---|---|---|\n" % n4)
            for b in res["batches"]:
                f.write("| %d | %.3f | %.3f | %.2f | %.3f | %.3f | %.2f | %.3f / %.3f | %.2f |\n" % (
                    b["nq"], b["jaccard_scan_ms_%d" % n1], b["hamming_scan_ms_%d" % n1], b["scan_ratio"],
                    b["jaccard_call_ms_%d" % n1], b["hamming_call_ms_%d" % n1], b["call_ratio"],
                    b["jaccard_scan_ms_%d" % n4], b["hamming_scan_ms_%d" % n4], b["epilogue_share"]))


if __name__ == "__main__":
    main()
