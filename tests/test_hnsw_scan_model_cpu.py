"""The iterative scan's formulation, settled without a GPU: the array form the device runs (hnsw_scan_model.model_scan:
W, the tie list, the stable merge and a pool of discarded candidates taken by (distance, position)) against the reference
transliterated with real heaps (hnsw_scan_model.ref_scan), batch by batch to exhaustion; the invariants that hold in every
tie order; the reference's own recorded answer; and the library's symbols."""
import numpy as np
import pytest

import hnsw_scan_cases as sc
from hnsw_scan_model import model_scan, ref_scan
from hnsw_walk_model import tuples, walk

EFS = (1, 2, 5, 16)


def both(seed, ef, integer, top=0, n=200, m=4):
    rows, queries = sc.rows_and_queries(seed, n, 6 if integer else 8, 1, integer)
    graph = sc.knn_graph(rows, m, seed + 1000, top=top)
    m_, entry, levels, start, nbr = graph
    d = sc.l2_table(queries, rows)[0].tolist()
    if not integer:
        assert len(set(d)) == len(d)
    ref = ref_scan(d.__getitem__, levels, start, nbr, m_, entry, ef)
    ms = model_scan(d.__getitem__, levels, start, nbr, m_, entry, ef)
    return graph, d, ref, ms.run(), ms


@pytest.mark.parametrize("top", (0, 2))
@pytest.mark.parametrize("ef", EFS)
def test_model_equals_reference_without_ties(ef, top):
    """elements, distances and cumulative tuples of every batch, every scan run until nothing is left"""
    batches = 0
    for seed in range(12):
        graph, d, ref, mod, _ = both(seed, ef, False, top=top)
        assert mod == ref, (seed, ef, top)
        batches += len(ref)
        if top:
            assert int(graph[2][graph[1]]) == top
    assert batches > 12 * (150 // ef) // 2  # (the scans are long: most of the 200 elements come out, ef at a time)


@pytest.mark.parametrize("ef", EFS)
def test_first_batch_is_the_walk(ef):
    """the model's first batch is hnsw_walk_model.walk's answer, ties included, upper layers included"""
    for integer in (False, True):
        for seed in range(6):
            graph, d, _, mod, _ = both(seed, ef, integer, top=2)
            m, entry, levels, start, nbr = graph
            w = walk(d.__getitem__, levels, start, nbr, m, entry, ef)
            assert (mod[0][0], mod[0][1], mod[0][2]) == (w.ids, w.dist, w.scored)


@pytest.mark.parametrize("ef", (1, 5, 16))
def test_invariants_hold_with_ties(ef):
    """on integer data the two may order equal distances differently; for both: every reachable element is returned
    exactly once, the tuples at exhaustion are the elements returned, and the pool never holds more than n entries, each
    a distinct visited element outside W"""
    differ = 0
    for seed in range(12):
        graph, d, ref, mod, ms = both(seed, ef, True)
        want = sc.reachable(graph, graph[1])
        for run in (ref, mod):
            ids = [e for b in run for e in b[0]]
            assert len(ids) == len(set(ids)) and set(ids) == want, (seed, ef)
            assert run[-1][2] == len(ids)
            assert all(b[1] == sorted(b[1]) and len(b[0]) <= ef for b in run)
        assert ms.max_pool <= len(d) and not ms.pool
        differ += ref != mod
        # batch by batch the pool is distinct visited elements outside W
        step = model_scan(d.__getitem__, graph[2], graph[3], graph[4], graph[0], graph[1], ef)
        while True:
            ids, _, _ = step.next()
            if not ids:
                break
            pooled = [e for _, e in step.pool]
            assert len(pooled) == len(set(pooled)) and set(pooled) <= step.visited and not set(pooled) & set(ids)
    print("ef", ef, "streams that differ between the two tie orders:", differ, "of 12")


def test_drain_takes_the_nearest_by_distance_then_position():
    graph, d, _, _, _ = both(3, 5, True)
    ms = model_scan(d.__getitem__, graph[2], graph[3], graph[4], graph[0], graph[1], 5)
    ms.next()
    pool = list(ms.pool)
    assert len(pool) > 7
    ids, dist = ms.drain(7)
    order = sorted(range(len(pool)), key=lambda p: (pool[p][0], p))
    assert ids == [pool[p][1] for p in order[:7]] and dist == [pool[p][0] for p in order[:7]]
    assert ms.pool == [pool[p] for p in sorted(order[7:])]
    rest, _ = ms.drain(len(pool))
    assert len(rest) == len(pool) - 7 and not ms.pool and ms.next()[0] == []


def test_gettuple_loop_filter_strict_and_limit():
    graph, d, ref, _, _ = both(5, 4, False)
    args = (d.__getitem__, graph[2], graph[3], graph[4], graph[0], graph[1], 4)
    stream = [(e, x) for b in ref for e, x in zip(b[0], b[1])]
    keep = np.random.default_rng(1).random(len(d)) < 0.3
    # relaxed: the stream through the filter, cut at k
    ids, dist, _ = model_scan(*args).iterative_search(10, keep)
    assert ids == [e for e, _ in stream if keep[e]][:10]
    # strict: never a step back
    ids, dist, _ = model_scan(*args).iterative_search(len(d), np.ones(len(d), bool), strict=True)
    assert dist == sorted(dist) and 0 < len(ids) <= len(stream)
    prev, want = float("-inf"), []
    for e, x in stream:
        if x >= prev:
            prev = x
            want.append(e)
    assert ids == want
    # nothing kept: ends by exhaustion with every element scored, or at the limit with the pool drained and no walk after
    ids, _, tuples_all = model_scan(*args).iterative_search(10, np.zeros(len(d), bool))
    assert ids == [] and tuples_all == len(stream)
    ms = model_scan(*args)
    ids, _, t = ms.iterative_search(10, np.zeros(len(d), bool), max_scan_tuples=40)
    assert ids == [] and 40 <= t < tuples_all and not ms.pool


def test_reference_recorded_answer():
    """test/expected/hnsw_vector.out:111-132: three rows, ef_search 1, strict and relaxed order"""
    g = sc.golden()
    rows, q = np.array(g["rows"], dtype=np.float32), np.array([g["query"]], dtype=np.float32)
    assert g["ef_search"] == 1 and len(g["cases"]) == 2
    levels, start, nbr = tuples(2, [0, 0, 0], {(0, 0): [1, 2], (1, 0): [0, 2], (2, 0): [0, 1]})
    d = sc.l2_table(q, rows)[0].tolist()
    for entry in range(3):
        for case in g["cases"]:
            ms = model_scan(d.__getitem__, levels, start, nbr, 2, entry, 1)
            ids, _, _ = ms.iterative_search(10, np.ones(3, bool), strict=case["iterative_scan"] == "strict_order")
            assert rows[ids].tolist() == case["expected"], (entry, case["iterative_scan"])
        ref = ref_scan(d.__getitem__, levels, start, nbr, 2, entry, 1)
        assert [rows[b[0][0]].tolist() for b in ref] == g["cases"][1]["expected"]


def test_library_declares_the_scan_entries():
    from pgvector_amd import _lib
    for name in ("pgv_hnsw_scan_begin", "pgv_hnsw_scan_next", "pgv_hnsw_scan_drain", "pgv_hnsw_scan_end"):
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib, name) is not None
    with open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "pgv_hip.h")) as f:
        header = f.read()
    assert all(("pgv_hnsw_scan_%s(" % n) in header for n in ("begin", "next", "drain", "end"))
