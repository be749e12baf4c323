"""What tests/test_gpu_sparse_hnsw_scan.py rests on, checked without a GPU on the same seeds: over the sparse distance
model's table (tests/sparse_model.py) the device's array form of an iterative scan (hnsw_scan_model.model_scan) is the
reference transliterated (ref_scan) on the tie-free draw, its pools reach every edge of a resumed batch's entry step there,
and on the tied draw it runs to exhaustion inside its own assertions and takes hnswgettuple's drain branch.  And the entry
the GPU file drives, pgv_hnsw_scan_begin_sparse, is declared and listed."""
import os
import re

import numpy as np
import pytest

import sparse_hnsw_model as shm
from hnsw_scan_model import model_scan, ref_scan
from pgvector_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EFS = (1, 5, 16, 65)
CHUNK = 256  # entries the entry step's compaction reads at a time
TIE_FREE_GRAPH = (400, 8, 5)      # shm.random_graph's arguments: with m = 4 the pools stay below the chunk under L2 and L1
TIED = dict(nq=8, n=600, dim=1536, seed=13)
TIED_GRAPH = (600, 8, 7)


@pytest.fixture(scope="module")
def tie_free_case():
    queries, rows = shm.tie_free(**shm.TIE_FREE)
    return {metric: shm.all_distances(metric, queries, rows) for metric in shm.METRICS}, shm.random_graph(*TIE_FREE_GRAPH)


@pytest.fixture(scope="module")
def tied_case():
    queries, rows = shm.tied(**TIED)
    return {metric: shm.all_distances(metric, queries, rows) for metric in shm.METRICS}, shm.random_graph(*TIED_GRAPH)


def stepped(ms):
    """every batch of a model scan -> ([(ids, dist, tuples)], [the pool each RESUMED batch's entry step read])"""
    batches, before = [], []
    while True:
        pool = len(ms.pool)
        started = ms.started
        b = ms.next()
        if not b[0]:
            return batches, before
        batches.append(b)
        if started:
            before.append(pool)


@pytest.mark.parametrize("metric", shm.METRICS)
@pytest.mark.parametrize("ef", EFS)
def test_tie_free_model_is_the_reference_and_reaches_the_pool_edges(tie_free_case, metric, ef):
    tables, (m, entry, levels, start, nbr) = tie_free_case
    d = tables[metric]
    n = d.shape[1]
    befores, peak = [], 0
    for q in range(d.shape[0]):
        assert len(np.unique(d[q])) == n  # no two elements equally far: the walk is determined
        dist = d[q].tolist().__getitem__
        ms = model_scan(dist, levels, start, nbr, m, entry, ef)
        got, before = stepped(ms)
        assert got == ref_scan(dist, levels, start, nbr, m, entry, ef), (metric, ef, q)
        assert got[-1][2] == n and sorted(e for b in got for e in b[0]) == list(range(n))
        befores += before
        peak = max(peak, ms.max_pool)
    assert peak > CHUNK, peak
    assert any(b > ef for b in befores)
    assert any(b == ef for b in befores) == (ef != 65), (ef, sorted(set(befores))[:4])
    assert any(0 < b < ef for b in befores) == (ef == 65)
    print(metric, ef, "max_pool", peak, "resumed from a pool <, =, > ef:", sum(0 < b < ef for b in befores),
          sum(b == ef for b in befores), sum(b > ef for b in befores))


@pytest.mark.parametrize("metric", shm.METRICS)
def test_tied_model_runs_to_exhaustion(tied_case, metric):
    """(model_scan asserts |T| < ef and merge == one-by-one admission on every batch it merges)"""
    tables, (m, entry, levels, start, nbr) = tied_case
    d = tables[metric]
    n = d.shape[1]
    distinct = [len(np.unique(d[q])) for q in range(d.shape[0])]
    assert max(distinct) < n // 8, distinct
    for ef in EFS:
        for q in range(d.shape[0]):
            ms = model_scan(d[q].tolist().__getitem__, levels, start, nbr, m, entry, ef)
            got = ms.run()
            ids = [e for b in got for e in b[0]]
            assert got[-1][2] == n and sorted(ids) == list(range(n)), (metric, ef, q)
            assert ms.max_pool <= n


@pytest.mark.parametrize("strict", (False, True))
def test_tied_iterative_search_takes_the_drain_branch(tied_case, strict):
    """ef 16, k 10, hnsw.max_scan_tuples 60: the first batch alone scores more, so what follows it is the pool, drained"""
    tables, (m, entry, levels, start, nbr) = tied_case
    d = tables[shm.METRICS[0]]
    keep = np.random.default_rng(3).random(d.shape[1]) < 0.1
    for q in range(d.shape[0]):
        ms = model_scan(d[q].tolist().__getitem__, levels, start, nbr, m, entry, 16)
        drains = []
        drain = ms.drain
        ms.drain = lambda count: drains.append(count) or drain(count)
        ids, dist, t = ms.iterative_search(10, keep, max_scan_tuples=60, strict=strict)
        assert t >= 60 and drains and all(keep[e] for e in ids), (q, t, drains)
        first = model_scan(d[q].tolist().__getitem__, levels, start, nbr, m, entry, 16).next()
        assert t == first[2]  # one walk, then the pool


def test_the_entry_is_declared_and_listed():
    text = open(os.path.join(ROOT, "include", "pgv_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pgv_hnsw_scan_begin_sparse\s*\(", text)
    assert "pgv_hnsw_scan_begin_sparse" in _lib.SYMBOLS
    assert hasattr(_lib.lib, "pgv_hnsw_scan_begin_sparse")
