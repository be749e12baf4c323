"""tests/sparse_model.py against the reference's recorded sparsevec results (test/sql/sparsevec.sql:89-127 with
test/expected/sparsevec.out, kept as data in tests/golden/sparsevec_known_answers.json): the float64 model that
tests/test_gpu_sparse.py holds the device to reproduces every printed answer, and its pieces agree with a plain
two-pointer merge written straight from the reference's loops."""
import numpy as np
import pytest

import sparse_model as sm
from helpers import golden

CASES = golden("sparsevec_known_answers.json")["cases"]


@pytest.mark.parametrize("case", CASES, ids=["%s-%d" % (c["fn"], c["sql_line"]) for c in CASES])
def test_model_reproduces_the_recorded_answer(case):
    assert sm.known_answer(case) == case["result"]


def test_golden_file_covers_the_transcript():
    fns = [c["fn"] for c in CASES]
    assert len(CASES) == 33 and {f: fns.count(f) for f in set(fns)} == {
        "l2_distance": 6, "inner_product": 8, "negative_inner_product": 1, "cosine_distance": 12, "l1_distance": 6}
    assert {c["result"] for c in CASES} >= {"NaN", "Infinity", "0", "2", "36", "45"}


def merge(metric, a, b):
    """the reference's loop shape: two sorted lists walked together, terms added in index order, in float64"""
    (ai, av), (bi, bv) = a, b
    i = j = 0
    total, S, m = 0.0, 0.0, 0
    while i < len(ai) or j < len(bi):
        if j >= len(bi) or (i < len(ai) and ai[i] < bi[j]):
            x, y, i = float(av[i]), None, i + 1
        elif i >= len(ai) or bi[j] < ai[i]:
            x, y, j = None, float(bv[j]), j + 1
        else:
            x, y, i, j = float(av[i]), float(bv[j]), i + 1, j + 1
        if metric == sm.NEG_IP:
            if x is None or y is None:
                continue
            t = x * y
        else:
            d = (x or 0.0) - (y or 0.0)
            t = d * d if metric == sm.L2SQ else abs(d)
        total, S, m = total + t, S + abs(t), m + 1
    return total, S, m


def rand_vec(rng, dim, nnz):
    idx = np.sort(rng.choice(dim, nnz, replace=False)).astype(np.int32)
    return idx, rng.standard_normal(nnz).astype(np.float32)


@pytest.mark.parametrize("metric", [sm.L2SQ, sm.NEG_IP, sm.L1])
def test_model_matches_a_two_pointer_merge(metric):
    rng = np.random.default_rng(5)
    query = rand_vec(rng, 300, 70)
    vectors = [rand_vec(rng, 300, nnz) for nnz in (0, 1, 64, 150, 300)] + [query]
    rows = sm.csr(vectors)
    value, exact, S, m = sm.distances(metric, query, rows)
    for r, vec in enumerate(vectors):
        t, s, cnt = merge(metric, query, vec)
        want = -t if metric == sm.NEG_IP else t
        assert abs(exact[r] - want) <= 1e-12 * max(s, 1.0) and abs(S[r] - s) <= 1e-12 * max(s, 1.0) and m[r] == cnt
    assert value.dtype == np.float32
    if metric != sm.NEG_IP:
        assert exact[-1] == 0.0 and value[-1] == 0.0  # a vector against itself: every term is exactly zero
    empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    assert np.array_equal(sm.distances(metric, empty, sm.csr([empty]))[0], np.zeros(1, dtype=np.float32))


def test_model_topk_is_stable_and_padded():
    """integer values: many equal distances, which must come in row order; k past n pads with +inf / -1"""
    rng = np.random.default_rng(6)
    rows = sm.csr([(np.arange(4, dtype=np.int32), rng.integers(0, 2, 4).astype(np.float32)) for _ in range(40)])
    queries = sm.csr([(np.arange(4, dtype=np.int32), np.ones(4, dtype=np.float32))] * 2)
    dist, idx, exact, _, _ = sm.topk(sm.L2SQ, queries, rows, 50)
    assert (idx[:, 40:] == -1).all() and np.isinf(dist[:, 40:]).all()
    for q in range(2):
        keys = list(zip(dist[q, :40].tolist(), idx[q, :40].tolist()))
        assert keys == sorted(keys) and sorted(idx[q, :40].tolist()) == list(range(40))
        assert np.array_equal(dist[q, :40], exact[q][idx[q, :40]].astype(np.float32))


def test_bound_switches_at_the_projects_rtol():
    from helpers import RTOL
    assert (165 + 2) * 2.0 ** -24 <= RTOL < (166 + 2) * 2.0 ** -24
    assert sm.bound(2.0, 165, RTOL) == RTOL * 2.0 and sm.bound(2.0, 32000, RTOL) == 32002 * 2.0 ** -24 * 2.0
