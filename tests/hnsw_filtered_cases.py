"""What the filtered-scan tests share (tests/test_hnsw_filtered_cpu.py, tests/test_gpu_hnsw_filtered.py): the shape and the
seeds, the filters, the cases at the edges of k and of the pool, and a way to run model_scan.iterative_search -- the
specification of pgv_hnsw_scan_filtered -- many times over one scan without walking it many times.

hnswgettuple's loop takes batches from a scan in an order that depends on max_scan_tuples alone (walk until so->tuples
reaches it, then drain); the filter, strict_order and k only decide where the loop STOPS.  `recorded` holds one model_scan
and the batches taken from it so far under one limit, extended on demand; `replay` hands them to
model_scan.iterative_search itself, which runs unchanged, and notes what the loop took: the batches, so->tuples, the pool
left and the kind and pool size of every step."""
import numpy as np

import hnsw_scan_cases as sc
from hnsw_scan_model import model_scan

N, DIM, M, TOP, NQ, SEED = 600, 48, 16, 2, 64, 11  # the smallest shape that reaches every branch
K = 10
EFS = (5, 16)
SELECTIVITIES = (1.0, 0.3, 0.05, 0.0)
LIMITS = (20000, 150, 1)  # max_scan_tuples: never reached, reached in the middle of a scan, reached by the first batch


def float_case():
    """rows [N x DIM], queries [NQ x DIM] (standard normal) and a graph with two upper layers"""
    rows, queries = sc.rows_and_queries(SEED, N, DIM, NQ, False)
    return rows, queries, sc.knn_graph(rows, M, SEED + 1, top=TOP)


def keep_mask(selectivity, n, seed=3):
    """a filter keeping about `selectivity` of n elements: all of them at 1.0, none at 0.0"""
    return np.random.default_rng(seed).random(n) < selectivity


class recorded:
    """one scan (make() -> model_scan) and the steps hnswgettuple's loop takes from it under `limit`"""

    def __init__(self, make, limit):
        self.ms, self.limit, self.steps = make(), limit, []

    def step(self, i):
        """-> (kind, ids, dist, so->tuples after it, pool before it, pool after it)"""
        ms = self.ms
        while len(self.steps) <= i:
            before = len(ms.pool)
            if ms.started and ms.tuples >= self.limit:
                kind, (e, d) = "drain", ms.drain(ms.ef)
            else:
                kind, (e, d, _) = "walk", ms.next()
            self.steps.append((kind, e, d, ms.tuples, before, len(ms.pool)))
        return self.steps[i]


class replay:
    """what model_scan.iterative_search asks of a scan, served from a `recorded` one"""

    def __init__(self, rec):
        self.rec, self.ef, self.at, self.started, self.tuples, self.left, self.batches = rec, rec.ms.ef, 0, False, 0, 0, 0

    def _step(self, kind):
        k, e, d, self.tuples, _, self.left = self.rec.step(self.at)
        assert k == kind, "the loop and the record disagree about max_scan_tuples"
        self.at += 1
        self.started = True
        self.batches += bool(e)  # (an empty batch is the end of the scan, not a walk or a drain)
        return e, d

    def next(self):
        e, d = self._step("walk")
        return e, d, self.tuples

    def drain(self, count):
        assert count == self.ef
        return self._step("drain")

    iterative_search = model_scan.iterative_search

    def taken(self):
        """the steps the loop took"""
        return self.rec.steps[:self.at]


def run_loop(rec, k, keep, strict):
    """model_scan.iterative_search over a recorded scan from its start -> (ids, dist, tuples, batches, left, replay)"""
    rp = replay(rec)
    ids, dist, tuples = rp.iterative_search(k, keep, max_scan_tuples=rec.limit, strict=strict)
    return ids, dist, tuples, rp.batches, rp.left, rp


def tags(rp, ids, k, keep):
    """which branches of the loop one query took (non-strict)"""
    steps = rp.taken()
    out = {"k" if len(ids) == k else "short"}
    if steps and not steps[-1][1]:
        out.add("exhausted")
    drains = [s for s in steps if s[0] == "drain" and s[1]]
    walks = [s for s in steps if s[0] == "walk" and s[1]]
    if drains:
        out.add("drained")
        out.add("walked then drained" if len(walks) > 1 else "drained after the first batch")
        for s in drains:
            out.add("pool below ef" if s[4] < rp.ef else "pool at ef" if s[4] == rp.ef else "pool above ef")
            if s[4] > 256:
                out.add("pool above 256")
    if len(ids) == k and steps[-1][1]:
        last = steps[-1][1]
        tail = last[last.index(ids[-1]) + 1:]
        out.add("k at the end of a batch" if not tail else "k in the middle of a batch")
        if any(keep[e] for e in tail):
            out.add("kept elements dropped")
    return out


# the edges of k and of the pool, on the float case under L2 / fp32: name -> (ef, k, selectivity, limit, the branches
# that some query of the case must take)
EDGES = {
    "middle of a batch": (16, 10, 0.3, 20000, {"k in the middle of a batch", "kept elements dropped"}),
    "end of a batch": (5, 10, 1.0, 20000, {"k at the end of a batch"}),
    "k = 1": (5, 1, 0.3, 20000, {"k"}),
    "exhausted": (16, 100, 0.05, 20000, {"short", "exhausted"}),
    "drain": (5, 10, 0.05, 150, {"walked then drained"}),
    "drain after the first batch": (16, 10, 0.05, 1, {"drained after the first batch"}),
    "mixed": (5, 10, 0.05, 150, {"k", "short", "drained", "exhausted"}),
    "pool": (5, 10, 0.0, 400, {"pool below ef", "pool at ef", "pool above ef", "pool above 256"}),
}


def edge_tags(name, models):
    """the union of the branches the NQ queries of an edge case take; models(ef) -> one model_scan per query"""
    ef, k, selectivity, limit, _ = EDGES[name]
    keep = keep_mask(selectivity, N)
    seen = set()
    for make in models(ef):
        ids, _, _, _, _, rp = run_loop(recorded(make, limit), k, keep, False)
        seen |= tags(rp, ids, k, keep)
    return seen
