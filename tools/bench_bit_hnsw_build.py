#!/usr/bin/env python3
"""CREATE INDEX of the indexed binary-quantization query at 1 M x 1536 bits, on the device: the HNSW build over a bit
mirror (pgv_hnsw_upload_bits_buildable + pgv_host_hnsw_build_bits) under bit_hamming_ops, beside the route that existed
before it -- pgv_host_hnsw_build over the elements' 0/1 fp16 expansion under L2, 16 times the row bytes -- in the same
process, alternating which of the two goes first, and the build under bit_jaccard_ops, which has no dense twin.  The rows
are the binary_quantize image of tools/bench_bit_topk.py's seeded fp32 mixture (tools/bench_bit_hnsw.py's rows).

Reports seconds and phase_secs of every build, the device bytes each mirror's rows hold (pgv_device_memory before and
after the upload), whether the Hamming and the twin graphs are equal array for array, and recall@10 of the walk at ef 40 and
100 against the exact top-10 (pgv_bit_topk for Hamming; pgv_bit_distance_batch and a sort for Jaccard; an element at the
k-th distance counts: ties are answers too).  Prints one JSON line; --md FILE also writes the tables.

usage: python tools/bench_bit_hnsw_build.py [--rows 1000000] [--dim 1536] [--rounds 2] [--md FILE]
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

from pgvector_amd import _host, api  # noqa: E402

EFS = (40, 100)
K = 10
GRAPH = ("levels", "nbr_start", "nbr", "dup_of")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--ef-construction", type=int, default=64)
    ap.add_argument("--max-batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=2, help="Hamming / twin pairs of builds; the order alternates")
    ap.add_argument("--queries", type=int, default=1024, help="Hamming recall queries")
    ap.add_argument("--jaccard-queries", type=int, default=128)
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

    def expand16(bits):  # packed bits -> 0/1 fp16 rows on the host, first bit = top bit of byte 0
        shifts = torch.arange(7, -1, -1, device=dev, dtype=torch.uint8)
        out = np.empty((bits.shape[0], a.dim), dtype=np.float16)
        for lo in range(0, bits.shape[0], 100000):
            b = bits[lo:lo + 100000]
            out[lo:lo + 100000] = ((b[:, :, None] >> shifts[None, None, :]) & 1).reshape(b.shape[0], -1)[:, :a.dim].half().cpu().numpy()
        return out

    def free_bytes():
        free, total = C.c_uint64(), C.c_uint64()
        api.check(api.lib.pgv_device_memory(0, C.byref(free), C.byref(total)))
        return free.value

    ctx = api.Context(0, stream=0)
    data = draw(a.rows)
    bits = api.binary_quantize(ctx, api.PGV_F32, a.dim, data)
    del data
    qbits = api.binary_quantize(ctx, api.PGV_F32, a.dim, draw(max(a.queries, a.jaccard_queries)))
    host_bits = bits.cpu().numpy()
    host_twin = expand16(bits)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    def build(kind):
        """one upload and one build -> (record, graph, mirror)"""
        torch.cuda.synchronize()
        before = free_bytes()
        if kind == "fp16_twin":
            mirror, rows = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F16, a.dim, host_twin), host_twin
        else:
            metric = api.PGV_BIT_JACCARD if kind == "jaccard" else api.PGV_BIT_HAMMING
            mirror, rows = api.BitHnsw(ctx, a.dim, bits, metric=metric, buildable=True), host_bits
        held = before - free_bytes()
        t0 = time.perf_counter()
        built = _host.hnsw_build(mirror, rows, a.m, a.ef_construction, api.make_rng(seed=1), max_batch=a.max_batch)
        ctx.sync()
        secs = time.perf_counter() - t0
        return ({"kind": kind, "secs": secs, "phase_secs": built["phase_secs"], "row_bytes_on_device": held,
                 "elements_linked": built["nelements"], "batches": built["batches"], "device_pairs": built["device_pairs"]},
                built, mirror)

    def recall(mirror, kth, nq):
        out = {}
        for ef in EFS:
            elem, dist, _ = mirror.search(qbits[:nq].contiguous(), ef, K)
            out["ef_%d" % ef] = ((dist <= kth[:nq, None]) & (elem >= 0)).sum().item() / (nq * K)
        return out

    res = {"rows": a.rows, "nbits": a.dim, "m": a.m, "ef_construction": a.ef_construction, "max_batch": a.max_batch, "builds": []}
    ham_kth = api.bit_topk(ctx, a.dim, qbits[:a.queries].contiguous(), bits, K)[0][:, -1]
    equal = []
    for r in range(a.rounds):
        order = ("hamming", "fp16_twin") if r % 2 == 0 else ("fp16_twin", "hamming")
        graphs = {}
        for kind in order:
            rec, built, mirror = build(kind)
            rec["round"], rec["first_of_round"] = r, kind == order[0]
            if r == 0 and kind == "hamming":
                rec["recall_at_10"] = recall(mirror, ham_kth, a.queries)
            mirror.close()
            graphs[kind] = built
            res["builds"].append(rec)
        x, y = graphs["hamming"], graphs["fp16_twin"]
        equal.append(bool(x["entry"] == y["entry"] and x["batches"] == y["batches"] and x["nelements"] == y["nelements"] and
                          all(np.array_equal(x[k], y[k]) for k in GRAPH)))
    res["hamming_graph_equals_twin_graph"] = equal
    del host_twin
    rec, built, mirror = build("jaccard")
    kth = torch.empty(a.jaccard_queries, dtype=torch.float32, device=dev)
    for q in range(a.jaccard_queries):   # the exact distances of one query at a time, float8; the k-th as the walk's float
        d = api.bit_distance_batch(ctx, api.PGV_BIT_JACCARD, a.dim, qbits[q], bits)
        kth[q] = torch.kthvalue(d, K).values.float()
    rec["recall_at_10"] = recall(mirror, kth, a.jaccard_queries)
    mirror.close()
    res["builds"].append(rec)
    print(json.dumps(res))
    if a.md:
        with open(a.md, "w") as f:
            f.write("| build | round | first of its round | seconds | search / pairs / select / records / update / patch (s) | "
                    "row bytes on the device | elements linked | batches | recall@10 at ef 40 / 100 |\n|---|---|---|---|---|---|---|---|---|\n")
            for b in res["builds"]:
                p = b["phase_secs"]
                rc = b.get("recall_at_10")
                f.write("| %s | %s | %s | %.3f | %s | %d | %d | %d | %s |\n" % (
                    b["kind"], b.get("round", "-"), "yes" if b.get("first_of_round") else "-", b["secs"],
                    " / ".join("%.3f" % p[k] for k in ("search", "pairs", "select", "records", "update", "patch")),
                    b["row_bytes_on_device"], b["elements_linked"], b["batches"],
                    "%.4f / %.4f" % (rc["ef_40"], rc["ef_100"]) if rc else "-"))
            f.write("\nHamming graph equal to the twin's, array for array, per round: %s\n" % ", ".join("yes" if e else "NO" for e in equal))
    ctx.close()


if __name__ == "__main__":
    main()
