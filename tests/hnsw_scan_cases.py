"""Inputs of the iterative-scan tests (tests/test_hnsw_scan_model_cpu.py, tests/test_gpu_hnsw_scan.py): random graphs in
the neighbour-tuple layout, tie-free float data and small-integer data full of ties.  Data only; the models are
tests/hnsw_scan_model.py."""
import json
import os

import numpy as np

from hnsw_walk_model import tuples

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnsw_iterative_known_answers.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def rows_and_queries(seed, n, dim, nq, integer):
    """float32 rows [n x dim] and queries [nq x dim]: standard normal, or integers in {0 .. 3} (every distance a small
    integer, exact in fp32 and fp16, most of them shared)"""
    rng = np.random.default_rng(seed)
    if integer:
        return rng.integers(0, 4, (n, dim)).astype(np.float32), rng.integers(0, 4, (nq, dim)).astype(np.float32)
    return rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((nq, dim)).astype(np.float32)


def knn_graph(rows, m, seed, top=0):
    """a searchable graph over the rows without a build: on every layer an element lists its nearest elements of that
    layer (m of them on layer 0, m // 2 above) and as many random ones, self excluded, duplicates dropped.  top > 0: levels
    drawn so that about 1 in 8 elements reaches each next layer, element 0 raised to `top` and made the entry point.
    -> (m, entry, levels, nbr_start, nbr)"""
    rng = np.random.default_rng(seed)
    n = len(rows)
    levels = np.zeros(n, dtype=np.int32)
    for lc in range(1, top + 1):
        levels[(levels == lc - 1) & (rng.random(n) < 0.125)] = lc
    levels[0] = top
    x = rows.astype(np.float64)
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    lists = {}
    for lc in range(top + 1):
        members = np.flatnonzero(levels >= lc)
        near = m if lc == 0 else max(1, m // 2)
        for i in members:
            order = members[np.argsort(d[i, members], kind="stable")]
            want = [int(e) for e in order if e != i][:near] + [int(e) for e in rng.choice(members, near)]
            lists[int(i), lc] = [e for e in dict.fromkeys(want) if e != i]
    lv, start, nbr = tuples(m, levels, lists)
    return m, 0, lv, start, nbr


def reachable(graph, entry):
    """elements a layer-0 walk from `entry` can reach"""
    m, _, levels, start, nbr = graph
    seen, todo = {int(entry)}, [int(entry)]
    while todo:
        c = todo.pop()
        o = int(start[c]) + int(levels[c]) * m
        for e in nbr[o:o + 2 * m]:
            if e >= 0 and int(e) not in seen:
                seen.add(int(e))
                todo.append(int(e))
    return seen


def l2_table(queries, rows):
    """[nq x n] squared L2 distances in float64 (exact on integer data)"""
    q, r = queries.astype(np.float64)[:, None, :], rows.astype(np.float64)[None, :, :]
    return ((q - r) ** 2).sum(-1)
