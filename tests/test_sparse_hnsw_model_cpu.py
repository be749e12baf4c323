"""What tests/test_gpu_sparse_hnsw.py rests on, checked without a GPU on the same seeds: the generators of
tests/sparse_hnsw_model.py, the exactness of fp32 on their integer data, and the walk model driven by the sparse
distance model against the compiled oracle's walk over the dense expansion."""
import numpy as np
import pytest

import hnsw_walk_model as wm
import sparse_hnsw_model as shm
import sparse_model as sm
from oracle import pyoracle as po

OPS = {sm.L2SQ: po.OPS_L2, sm.NEG_IP: po.OPS_IP, sm.L1: po.OPS_L1}


@pytest.fixture(scope="module")
def tie_free_case():
    return shm.tie_free(**shm.TIE_FREE)


@pytest.fixture(scope="module")
def tied_case():
    return shm.tied(**shm.TIED)


def test_generators_make_valid_csr(tie_free_case, tied_case):
    for (queries, rows), dim in ((tie_free_case, shm.TIE_FREE["dim"]), (tied_case, shm.TIED["dim"])):
        for ptr, idx, val in (queries, rows):
            assert ptr[0] == 0 and (np.diff(ptr) >= 0).all() and ptr.dtype == np.int64 and idx.dtype == np.int32
            assert np.isfinite(val).all() and np.array_equal(val, np.round(val)) and np.abs(val).max() <= 8
            assert (idx >= 0).all() and (idx < dim).all()
            for v in range(len(ptr) - 1):
                assert (np.diff(idx[ptr[v]:ptr[v + 1]]) > 0).all()
        assert np.diff(rows[0]).max() <= shm.HNSW_MAX_NNZ and np.diff(queries[0]).max() <= shm.SPARSE_MAX_NNZ
    assert np.diff(tie_free_case[1][0]).max() > 256 and np.diff(tie_free_case[1][0]).min() <= 64  # both row paths


def test_expand_dense_is_the_vector():
    rows = shm.rand_csr([0, 1, 5, 64], 3, dim=100)
    dense = shm.expand_dense(rows, 100)
    assert dense.shape == (4, 100) and (dense[0] == 0).all()
    for r in range(4):
        idx, val = sm.vector(rows, r)
        assert np.array_equal(np.flatnonzero(dense[r]), idx) and np.array_equal(dense[r][idx], val)
    # the dense distances are the sparse model's
    q = shm.rand_csr([7], 4, dim=100)
    d = shm.expand_dense(q, 100)[0].astype(np.float64)
    assert np.array_equal(shm.all_distances(sm.L2SQ, q, rows)[0], ((dense - d) ** 2).sum(1).astype(np.float32))
    assert np.array_equal(shm.all_distances(sm.NEG_IP, q, rows)[0], (-(dense * d).sum(1)).astype(np.float32))
    assert np.array_equal(shm.all_distances(sm.L1, q, rows)[0], np.abs(dense - d).sum(1).astype(np.float32))


def test_partial_sums_stay_exact_in_fp32(tie_free_case, tied_case):
    """every pair's sum of |term| is below 2^24: integer terms, so every partial sum in any order is an exact fp32"""
    assert shm.max_abs_sum(*tie_free_case) < 2 ** 24
    assert shm.max_abs_sum(*tied_case) < 2 ** 24


def test_the_tie_free_set_is_tie_free(tie_free_case):
    queries, rows = tie_free_case
    n = len(rows[0]) - 1
    for metric in shm.METRICS:
        d = shm.all_distances(metric, queries, rows)
        for q in range(d.shape[0]):
            assert len(np.unique(d[q])) == n, (metric, q)


def test_the_tied_set_holds_ties(tied_case):
    queries, rows = tied_case
    for metric in shm.METRICS:
        d = shm.all_distances(metric, queries, rows)
        assert all(len(np.unique(d[q])) < d.shape[1] // 10 for q in range(d.shape[0])), metric


@pytest.mark.parametrize("metric", shm.METRICS)
def test_walk_model_equals_the_oracle_on_tie_free_data(oracle, tie_free_case, metric):
    """hnsw_walk_model.walk driven by sparse_model.distances over the CSR == the oracle's HnswGraph.search over the dense
    expansion: elements, distances and so->tuples"""
    queries, rows = tie_free_case
    dim = shm.TIE_FREE["dim"]
    g = po.HnswGraph(oracle, OPS[metric], po.ORA_F32, shm.expand_dense(rows, dim), m=8, ef_construction=32, seed=7)
    ex = g.export_tuples()
    elements = shm.take(rows, ex["rows"])
    d_all = shm.all_distances(metric, queries, elements)
    dense_q = shm.expand_dense(queries, dim)
    assert int(ex["levels"].max()) >= 1
    for ef, k in ((40, 10), (1, 1)):
        for q in range(d_all.shape[0]):
            w = wm.walk(lambda e: float(d_all[q][e]), ex["levels"], ex["nbr_start"], ex["nbr"], 8, ex["entry"], ef)
            want_rows, want_dist, want_scored = g.search(dense_q[q], ef, k)
            assert ex["rows"][w.ids[:k]].tolist() == want_rows.tolist(), (ef, q)
            assert w.dist[:k] == want_dist.tolist(), (ef, q)
            assert w.scored == want_scored, (ef, q)
    g.close()
