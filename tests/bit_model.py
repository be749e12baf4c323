"""numpy model of the binary-quantization entries (pgv_bit_topk, pgv_binary_quantize, pgv_rerank): what
tests/test_gpu_bit_topk.py compares the device against, itself pinned by tests/test_bit_model_cpu.py to the oracle's
ora_bit_hamming (the compiled restatement of src/bitutils.c) and to the reference's recorded binary_quantize results."""
import numpy as np

POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)

# pgv_metric -> (the oracle's fp32 kernel, its fp16 kernel, sign): L2 squared, NEGATIVE inner product, L1
KERNELS = {0: ("ora_vector_l2_squared", "ora_halfvec_l2_squared", 1.0),
           1: ("ora_vector_inner_product", "ora_halfvec_inner_product", -1.0),
           2: ("ora_vector_l1", "ora_halfvec_l1", 1.0)}


def hamming(query, rows):
    """popcount(a ^ b) over whole bytes (BitHammingDistanceDefault, src/bitutils.c:49-73) -> int64 [n]"""
    rows = np.asarray(rows, dtype=np.uint8)
    if rows.shape[1] == 0:
        return np.zeros(rows.shape[0], dtype=np.int64)
    return POPCOUNT[rows ^ np.asarray(query, dtype=np.uint8)[None, :]].sum(axis=1)


def hamming_topk(queries, rows, k):
    """(dist [nq x k] float32, idx [nq x k] int64): ascending by (distance, index), +inf / -1 beyond n"""
    queries, rows = np.asarray(queries, dtype=np.uint8), np.asarray(rows, dtype=np.uint8)
    nq, n = queries.shape[0], rows.shape[0]
    dist = np.full((nq, k), np.inf, dtype=np.float32)
    idx = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        d = hamming(queries[q], rows)
        order = np.argsort(d, kind="stable")[:k]  # stable: equal distances keep index order
        dist[q, :len(order)] = d[order]
        idx[q, :len(order)] = order
    return dist, idx


def binary_quantize(x):
    """bit i = x[i] > 0 (src/vector.c:952-979), first element in the top bit of byte 0; NaN > 0 is false"""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        return np.packbits(x > 0, axis=1)


def rerank(ora, metric, half, queries, rows, cand, k):
    """the oracle's kernel per (query, candidate) pair, stable sort by value: ties to the lower candidate position;
    a candidate of -1 scores +inf and keeps -1"""
    name, hname, sign = KERNELS[metric]
    cand = np.asarray(cand, dtype=np.int64)
    nq, kc = cand.shape
    dist = np.full((nq, k), np.inf, dtype=np.float32)
    idx = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        vals = np.full(kc, np.inf, dtype=np.float32)
        for j, c in enumerate(cand[q]):
            if c >= 0:
                vals[j] = np.float32(sign) * np.float32(ora.kernel(hname if half else name, rows[c], queries[q], half=half))
        order = np.argsort(vals, kind="stable")[:k]
        dist[q] = vals[order]
        idx[q] = cand[q][order]
    return dist, idx
