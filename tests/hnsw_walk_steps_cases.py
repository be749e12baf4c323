"""The cases of tests/test_gpu_hnsw_walk_steps.py, and what tools/record_hnsw_walk_answers.py records of them: every form of
hnsw_search_kernel at the smallest shapes where its merge positions, its wavefront compactions, its result epilogue and its
LDS layout can go wrong, answered by whatever library is loaded.

300 rows of dimension 8 with integers in {0 .. 3} (most distances tie, so the order among equal keys is on show), a
knn_graph with m = 4 and three layers, 4 queries.  Some layer-1 tuples list an element that lives on layer 0 only, so that
the drop of entries below the layer has something to drop, in the middle of a batch.  ef:
   1  W of one entry, T can hold nothing         3  a batch larger than W
   8  |W| + batch meets ef exactly (8 = 2 m), then exceeds it
  65  the lane loops cross one wavefront
pgv_hnsw_build_search refuses ef_construction < 4 (src/hnsw.h:58-59), so the build forms run at 4, 8 and 65; the layers above
an insert level are walked with ef = 1 there whatever ef_construction is.

answers(ctx) -> {case name: JSON-able answer}.  Distances are recorded as bit patterns, run-length coded (W is ascending and
full of ties); element ids in full."""
import numpy as np

import hnsw_scan_cases as sc
from pgvector_amd import api

N, DIM, NQ, M, TOP, SEED = 300, 8, 4, 4, 2, 41
EFS = (1, 3, 8, 65)
BUILD_EFS = (4, 8, 65)
LAYER_CAP = 3
BUILD_ELEMENTS, BUILD_LEVELS = (0, 17, 100, 250), (2, 0, 1, 2)
SCAN_BATCHES, DRAIN = 3, 5

_inputs = []


def inputs():
    """(rows, queries, graph), once: the integer data and the graph with its planted below-the-layer neighbours"""
    if not _inputs:
        rows, queries = sc.rows_and_queries(SEED, N, DIM, NQ, True)
        m, entry, levels, start, nbr = sc.knn_graph(rows, M, SEED + 1, top=TOP)
        low = np.flatnonzero(levels == 0)
        planted = 0
        for e in np.flatnonzero(levels >= 1):
            o = int(start[e]) + (int(levels[e]) - 1) * m  # its layer-1 slice: the second slot gets a layer-0 element
            if nbr[o + 1] >= 0:
                nbr[o + 1] = low[(7 * int(e) + 3) % len(low)]
                planted += 1
        assert planted >= 8 and (levels == TOP).sum() >= 2
        _inputs.append((rows, queries, (m, entry, levels, start, nbr)))
    return _inputs[0]


def as_bits(x):
    """integers {0 .. 3} -> packed bit strings of 2 * DIM bits: the low bits, then the high bits"""
    x = x.astype(np.uint8)
    return np.packbits(np.concatenate([x & 1, x >> 1], axis=1), axis=1)


def as_csr(x):
    """the nonzero entries of each row -> (ptr, idx, val)"""
    nz = x != 0
    ptr = np.concatenate([[0], np.cumsum(nz.sum(1))]).astype(np.int64)
    return ptr, np.nonzero(nz)[1].astype(np.int32), x[nz].astype(np.float32)


def mirror(ctx, form, buildable=False):
    """form -> (mirror with the graph set, the queries as it takes them)"""
    rows, queries, graph = inputs()
    if form == "f32_l2":
        h, q = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, DIM, rows), queries
    elif form == "f16_ip":
        h, q = api.Hnsw(ctx, api.PGV_NEG_IP, api.PGV_F16, DIM, rows), queries
    elif form == "hamming":
        h, q = api.BitHnsw(ctx, 2 * DIM, as_bits(rows), buildable=buildable), as_bits(queries)
    elif form == "jaccard":
        h, q = api.JaccardHnsw(ctx, 2 * DIM, as_bits(rows), buildable=buildable), as_bits(queries)
    else:
        assert form == "sparse_l1"
        h, q = api.SparseHnsw(ctx, api.PGV_L1, DIM, as_csr(rows)), as_csr(queries)
    h.set_graph(*graph)
    return h, q


def rle(dist):
    """float32 values -> [[bit pattern, run length], ..]"""
    out = []
    for b in np.ascontiguousarray(dist, dtype=np.float32).view(np.uint32).ravel().tolist():
        if out and out[-1][0] == b:
            out[-1][1] += 1
        else:
            out.append([b, 1])
    return out


def ints(x):
    return np.asarray(x).ravel().tolist()


def answers(ctx):
    out = {}
    # a plain search: k = ef, the whole W
    for form in ("f32_l2", "f16_ip", "hamming", "jaccard", "sparse_l1"):
        h, q = mirror(ctx, form)
        for ef in EFS:
            elem, dist, scored = h.search(q, ef, ef)
            out["search %s ef %d" % (form, ef)] = {"elem": ints(elem), "dist": rle(dist), "scored": ints(scored)}
        h.close()
    # a scan: three batches, then a drain of 5 -- ids, distances, per-batch counts, so->tuples, pool sizes
    for form in ("f32_l2", "jaccard"):
        h, q = mirror(ctx, form)
        for ef in EFS:
            with h.scan(q, ef) as s:
                batches = []
                for _ in range(SCAN_BATCHES):
                    e, d, c, t, left = s.next()
                    batches.append({"elem": ints(e), "dist": rle(d), "count": ints(c), "scored": ints(t), "left": ints(left)})
                e, d, c = s.drain(DRAIN)
                out["scan %s ef %d" % (form, ef)] = {"batches": batches,
                                                     "drain": {"elem": ints(e), "dist": rle(d), "count": ints(c)}}
        h.close()
    # the build's search: W of every layer at or below the insert level (layers above it: ef = 1, nothing returned)
    elems, levels = np.asarray(BUILD_ELEMENTS, np.int32), np.asarray(BUILD_LEVELS, np.int32)
    for form in ("f32_l2", "hamming", "jaccard"):
        h, _ = mirror(ctx, form, buildable=True)
        for efc in BUILD_EFS:
            per = len(elems) * LAYER_CAP
            ids, dist, cnt = np.full((per, efc), -7, np.int32), np.zeros((per, efc), np.float32), np.full(per, -7, np.int32)
            api.check(api.lib.pgv_hnsw_build_search(h.h, api.ptr(elems), api.ptr(levels), len(elems), efc, LAYER_CAP,
                                                    api.ptr(ids), api.ptr(dist), api.ptr(cnt)))
            live = np.arange(efc)[None, :] < cnt[:, None]  # (what lies past a layer's count is not written)
            out["build %s ef %d" % (form, efc)] = {"ids": ints(ids[live]), "dist": rle(dist[live]), "count": ints(cnt)}
        h.close()
    return out
