"""HNSW over sparsevec elements on the device -- pgv_hnsw_upload_sparse, pgv_hnsw_score_sparse, pgv_hnsw_search_sparse, the
sparse element kind of hnsw_search_kernel, sparse_pair_kernel and api.SparseHnsw.  The yardsticks: pgv_sparse_distance_batch
(existing code, pinned by tests/test_gpu_sparse.py) bit for bit, the numpy models (tests/sparse_model.py,
tests/hnsw_walk_model.py, tests/sparse_hnsw_model.py), the compiled oracle's walk over the dense expansion, and the existing
fp32 walk of the same graph over that expansion.  On the integer data every comparison is exact equality
(tests/test_sparse_hnsw_model_cpu.py checks the preconditions on the same seeds)."""
import ctypes as C

import numpy as np
import pytest

import hnsw_tie_cases as tc
import hnsw_walk_model as wm
import sparse_hnsw_model as shm
import sparse_model as sm
from oracle import pyoracle as po
from pgvector_amd import _lib, api

pytestmark = pytest.mark.gpu

METRIC = {sm.L2SQ: api.PGV_L2SQ, sm.NEG_IP: api.PGV_NEG_IP, sm.L1: api.PGV_L1}
OPS = {sm.L2SQ: po.OPS_L2, sm.NEG_IP: po.OPS_IP, sm.L1: po.OPS_L1}
ELEM_LENGTHS = [0, 1, 63, 64, 65, 128, 256, 257, 999, 1000]      # register-chunk switches, the row_side_mem boundary
QUERY_LENGTHS = [0, 1, 31, 32, 33, 64, 1000, 1001, 16000]        # bitmap-word and descent-depth boundaries


def last_error():
    return _lib.lib.pgv_last_error().decode()


def mirror(ctx, metric, dim, rows, graph=None, payload=None):
    h = api.SparseHnsw(ctx, METRIC[metric], dim, rows, payload=payload)
    if graph is not None:
        h.set_graph(*graph)
    return h


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def refused(code, *needles):
    """a context manager: the call raises PgvError `code` and pgv_last_error holds every needle"""
    class _R:
        def __enter__(self):
            self.cm = pytest.raises(api.PgvError)
            self.e = self.cm.__enter__()
            return self

        def __exit__(self, *a):
            out = self.cm.__exit__(*a)
            assert self.e.value.code == code, (self.e.value.code, last_error())
            for s in needles:
                assert s in last_error(), (s, last_error())
            return out
    return _R()


# ------------------------------------------------------------------------------------------------------- 1. scores
def score_case(floats, dim=20000, seed=100):
    """three elements of every length and one query of every length; the shorter queries take half of their indices from
    an element's, so that every pair kind (hit, miss, empty) occurs"""
    rows = shm.rand_csr(ELEM_LENGTHS * 3, seed, dim=dim, floats=floats)
    rng = np.random.default_rng(seed + 1)
    queries = []
    for j, qn in enumerate(QUERY_LENGTHS):
        donor = sm.vector(rows, 10 + (j % 10))[0]
        own = donor[rng.permutation(len(donor))[:min(qn // 2, len(donor))]]
        idx = own
        while len(idx) < qn:
            idx = np.unique(np.concatenate([idx, rng.integers(0, dim, qn - len(idx))]))
        idx = np.sort(idx).astype(np.int32)
        val = rng.standard_normal(qn).astype(np.float32) if floats else \
            rng.choice(np.array([-8, -3, -1, 1, 2, 8], dtype=np.float32), qn)
        queries.append((idx, val))
    return rows, sm.csr(queries)


@pytest.mark.parametrize("metric", shm.METRICS)
@pytest.mark.parametrize("floats", [False, True])
def test_scores_are_sparse_distance_batch_bit_for_bit(ctx, metric, floats):
    dim = 20000
    rows, queries = score_case(floats)
    n, nq = len(rows[0]) - 1, len(queries[0]) - 1
    h = mirror(ctx, metric, dim, rows)
    slot = np.tile(np.arange(n, dtype=np.int32), nq)
    query_of = np.repeat(np.arange(nq, dtype=np.int32), n)
    got = h.score(queries, slot, query_of).reshape(nq, n)
    want = np.stack([api.sparse_distance_batch(ctx, METRIC[metric], dim, sm.vector(queries, q), rows) for q in range(nq)])
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5].tolist()
    # query_of None: every pair against query 0
    assert np.array_equal(bits(h.score(shm.take(queries, [5]), slot[:n])), bits(want[5]))
    # element against element, b as the query
    a, b = np.repeat(np.arange(n, dtype=np.int32), n), np.tile(np.arange(n, dtype=np.int32), n)
    pairs = h.score_pairs(a, b).reshape(n, n)
    want_pairs = np.stack([api.sparse_distance_batch(ctx, METRIC[metric], dim, sm.vector(rows, e), rows) for e in range(n)]).T
    assert np.array_equal(bits(pairs), bits(want_pairs))
    if metric != sm.NEG_IP:  # a vector against itself is exactly 0
        assert (np.diag(pairs) == 0).all()
        assert (h.score(rows, np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)) == 0).all()
    if not floats:
        assert np.array_equal(got, shm.all_distances(metric, queries, rows))
        assert np.array_equal(pairs.T, shm.all_distances(metric, rows, rows))
    h.close()


def test_scores_at_the_largest_dimension(ctx):
    """dim = 10^9, indices next to 0 and next to dim - 1"""
    dim = 10 ** 9
    edge = np.array([0, 1, 2, dim - 3, dim - 2, dim - 1], dtype=np.int32)
    pool = np.unique(np.concatenate([edge, np.random.default_rng(5).integers(0, dim, 3000)])).astype(np.int32)
    rows = shm.rand_csr([6, 64, 300, 1000, 0, 2], 6, pool=pool)
    rows = sm.csr([(edge, np.arange(1, 7, dtype=np.float32))] + [sm.vector(rows, r) for r in range(1, 6)])
    queries = sm.csr([(edge[[0, 5]], np.array([2, -3], dtype=np.float32)), sm.vector(shm.rand_csr([2000], 7, pool=pool), 0)])
    slot, query_of = np.tile(np.arange(6, dtype=np.int32), 2), np.repeat(np.arange(2, dtype=np.int32), 6)
    for metric in shm.METRICS:
        h = mirror(ctx, metric, dim, rows)
        got = h.score(queries, slot, query_of).reshape(2, 6)
        assert np.array_equal(got, shm.all_distances(metric, queries, rows)), metric
        for q in range(2):
            want = api.sparse_distance_batch(ctx, METRIC[metric], dim, sm.vector(queries, q), rows)
            assert np.array_equal(bits(got[q]), bits(want))
        h.close()


def test_an_empty_intersection_is_plus_zero(ctx):
    rows = sm.csr([([1, 3], [1.0, 2.0]), ([], []), ([5], [-4.0])])
    queries = sm.csr([([0, 2, 4], [7.0, -7.0, 1.0]), ([], [])])
    h = mirror(ctx, sm.NEG_IP, 8, rows)
    got = h.score(queries, np.tile(np.arange(3, dtype=np.int32), 2), np.repeat(np.arange(2, dtype=np.int32), 3))
    assert (bits(got) == 0).all(), bits(got).tolist()
    assert (bits(h.score_pairs([0, 1, 2], [2, 0, 1])) == 0).all()
    h.close()


# ------------------------------------------------------------------- 2. the walk's scorer, independent of tie order
@pytest.mark.parametrize("m", [8, 32])
@pytest.mark.parametrize("metric", shm.METRICS)
def test_walk_scores_a_complete_graph(ctx, metric, m):
    """whatever the tie order, the walk over a one-layer complete graph scores everything: the entry, then one batch of
    2 m (m = 32: 16 rows a wavefront); elements of every length class, 0 and 1000 among them"""
    n, entry, levels, nbr_start, nbr = shm.complete_graph(m)
    dim = 4096
    lengths = (ELEM_LENGTHS * 7)[:n]
    rows = shm.rand_csr(lengths, 300 + m, dim=dim)
    queries = shm.rand_csr([0, 1, 33, 64, 1000, 3000], 400 + m, dim=dim)
    h = mirror(ctx, metric, dim, rows, (m, entry, levels, nbr_start, nbr))
    d_all = shm.all_distances(metric, queries, rows)
    for ef, k in ((n, n), (n, 5), (5, 5)):
        elem, dist, scored = h.search(queries, ef, k)
        assert (scored == n).all(), (ef, k, scored.tolist())
        shm.assert_topk_up_to_ties(elem, dist, d_all, k, what="metric %d m %d ef %d k %d" % (metric, m, ef, k))
    h.close()


# -------------------------------------------------------------------------------------- 3. the dense twin, ties and all
@pytest.fixture(scope="module")
def tied_case():
    return shm.tied(**shm.TIED)


@pytest.mark.parametrize("metric", shm.METRICS)
def test_walk_equals_the_dense_twin(ctx, oracle, tied_case, metric):
    """small integers on 40 shared indices: ties everywhere.  The same graph over the same elements as a sparse mirror and
    as their dense fp32 expansion: the keys are the same integers and the walk code is shared"""
    queries, rows = tied_case
    dim = shm.TIED["dim"]
    g = po.HnswGraph(oracle, OPS[metric], po.ORA_F32, shm.expand_dense(rows, dim), m=16, ef_construction=32, seed=9)
    ex = g.export_tuples()
    g.close()
    elements = shm.take(rows, ex["rows"])
    graph = (16, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"])
    h = mirror(ctx, metric, dim, elements, graph)
    twin = api.Hnsw(ctx, METRIC[metric], api.PGV_F32, dim, shm.expand_dense(elements, dim))
    twin.set_graph(*graph)
    elem, dist, scored = h.search(queries, 64, 10)
    t_elem, t_dist, t_scored = twin.search(shm.expand_dense(queries, dim), 64, 10)
    assert int(ex["levels"].max()) >= 1 and (scored < len(ex["rows"])).all()
    assert np.array_equal(elem, t_elem) and np.array_equal(dist, t_dist) and np.array_equal(scored, t_scored)
    assert max(np.unique(dist[q], return_counts=True)[1].max() for q in range(len(dist))) >= 2  # the case holds ties
    twin.close()
    h.close()


# --------------------------------------------------------------------------------------- 4. the oracle's walk, tie-free
@pytest.fixture(scope="module")
def tie_free_case():
    return shm.tie_free(**shm.TIE_FREE)


@pytest.mark.parametrize("metric", shm.METRICS)
def test_walk_equals_the_oracle_on_tie_free_data(ctx, oracle, tie_free_case, metric):
    """no two candidates equally far: the walk is determined, so elements, distances and so->tuples equal the oracle's"""
    queries, rows = tie_free_case
    dim = shm.TIE_FREE["dim"]
    g = po.HnswGraph(oracle, OPS[metric], po.ORA_F32, shm.expand_dense(rows, dim), m=8, ef_construction=32, seed=7)
    ex = g.export_tuples()
    h = mirror(ctx, metric, dim, shm.take(rows, ex["rows"]), (8, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"]))
    dense_q = shm.expand_dense(queries, dim)
    for ef, k in ((40, 10), (1, 1)):
        elem, dist, scored = h.search(queries, ef, k)
        for i in range(len(dense_q)):
            want_rows, want_dist, want_scored = g.search(dense_q[i], ef, k)
            assert len(want_rows) == k
            assert ex["rows"][elem[i]].tolist() == want_rows.tolist(), (ef, i)
            assert dist[i].astype(np.float64).tolist() == want_dist.tolist(), (ef, i)
            assert int(scored[i]) == want_scored, (ef, i)
    g.close()
    h.close()


# --------------------------------------------------------------------------------------------- 5. the model, float data
BIG = 10 ** 9


def model_walk(ctx, metric, dim, query, rows, graph, ef):
    """hnsw_walk_model.walk with dist(e) = pgv_sparse_distance_batch's value"""
    m, entry, levels, nbr_start, nbr = graph
    d = api.sparse_distance_batch(ctx, METRIC[metric], dim, query, rows)
    return wm.walk(lambda e: float(d[e]), levels, nbr_start, nbr, m, entry, ef)


def assert_walk_is_the_model(ctx, h, metric, dim, queries, rows, graph, ef, k):
    elem, dist, scored = h.search(queries, ef, k)
    for q in range(len(queries[0]) - 1):
        w = model_walk(ctx, metric, dim, sm.vector(queries, q), rows, graph, ef)
        assert elem[q][:len(w.ids[:k])].tolist() == w.ids[:k], (ef, q)
        assert (elem[q][len(w.ids):] == -1).all()
        assert dist[q][:len(w.ids[:k])].astype(np.float64).tolist() == w.dist[:k], (ef, q)
        assert int(scored[q]) == w.scored, (ef, q)


@pytest.fixture(scope="module")
def float_case():
    """float values over dim 10^9: no dense twin can hold these vectors.  A random graph (any graph can be walked)"""
    pool = np.unique(np.concatenate([[0, BIG - 1], np.random.default_rng(21).integers(0, BIG, 5000)])).astype(np.int32)
    rng = np.random.default_rng(22)
    rows = shm.rand_csr(rng.choice(ELEM_LENGTHS + [20, 40, 90, 200], 700), 23, pool=pool, floats=True)
    queries = shm.rand_csr([0, 1, 40, 64, 500, 1001, 3000, 4000], 24, pool=pool, floats=True)
    return pool, rows, queries, shm.random_graph(700, 8, 25)


@pytest.mark.parametrize("metric", shm.METRICS)
def test_walk_equals_the_model_on_float_data(ctx, float_case, metric):
    _, rows, queries, graph = float_case
    h = mirror(ctx, metric, BIG, rows, graph)
    assert int(graph[2].max()) >= 1
    for ef, k in ((40, 10), (1, 1), (200, 200)):
        assert_walk_is_the_model(ctx, h, metric, BIG, queries, rows, graph, ef, k)
    h.close()


@pytest.mark.parametrize("name", sorted(tc.planted()))
@pytest.mark.parametrize("metric_name", tc.METRICS)
def test_planted_ties(ctx, name, metric_name):
    """the hand-written graphs of tests/hnsw_tie_cases.py whose answer holds in every tie order: an element at distance d
    stores d ones, the query nothing (L2, L1) or DIM minus ones (negative inner product)"""
    case = tc.planted()[name]
    metric = {"l2": sm.L2SQ, "negip": sm.NEG_IP, "l1": sm.L1}[metric_name]
    rows = sm.csr([(np.arange(d, dtype=np.int32), np.ones(d, dtype=np.float32)) for d in case["dists"]])
    qn = tc.DIM if metric_name == "negip" else 0
    query = sm.csr([(np.arange(qn, dtype=np.int32), -np.ones(qn, dtype=np.float32))])
    h = mirror(ctx, metric, tc.DIM, rows, (case["m"], case["entry"], case["levels"], case["nbr_start"], case["nbr"]))
    ef = case["ef"]
    elem, dist, scored = h.search(query, ef, ef)
    tc.check_head(case, elem[0], dist[0][elem[0] >= 0], what="%s %s" % (name, metric_name))
    assert int(scored[0]) == case["scored"]
    assert not set(elem[0].tolist()) & set(case["unscored"])
    h.close()


# ---------------------------------------------------------------------------------------------------- 6. long queries
def test_a_16000_element_query(ctx, float_case):
    """the longest query the type allows at ef 40 / m 16 fits the LDS budget and returns the model's answer; ef 1000 with
    the same query does not fit under L2 and L1 (their matched bitmaps): PGV_ERR_ARG before any launch, the text naming the
    three sizes"""
    pool, rows, _, _ = float_case
    n = len(rows[0]) - 1
    graph = shm.random_graph(n, 16, 31)
    wide = np.unique(np.concatenate([pool, np.random.default_rng(32).integers(0, BIG, 40000)])).astype(np.int32)
    queries = shm.rand_csr([16000, 7], 33, pool=wide, floats=True)
    for metric in shm.METRICS:
        h = mirror(ctx, metric, BIG, rows, graph)
        assert_walk_is_the_model(ctx, h, metric, BIG, queries, rows, graph, 40, 10)
        if metric == sm.NEG_IP:
            # no matched bitmaps: 128 000 + 1000 * 20 + 16 * 16 + 64 bytes fit, the largest ef included
            assert_walk_is_the_model(ctx, h, metric, BIG, queries, rows, graph, 1000, 10)
        else:
            with refused(api.PGV_ERR_ARG, "ef 1000", "m 16", "16000"):
                h.search(queries, 1000, 10)
        h.close()


# ------------------------------------------------------------------------------------------ 7. views, payload, patches
@pytest.fixture(scope="module")
def small_case():
    m, dim = 8, 500
    n, entry, levels, nbr_start, nbr = shm.complete_graph(m)
    rows = shm.rand_csr(([0, 1, 5, 64, 65, 300] * 3)[:n], 71, dim=dim)
    queries = shm.rand_csr([3, 0, 100, 400, 17], 72, dim=dim)
    payload = (np.arange(n, dtype=np.uint32)[:, None] * 31 + np.arange(3, dtype=np.uint32)[None, :]).astype(np.uint32)
    return dim, rows, queries, (m, entry, levels, nbr_start, nbr), payload


def test_share_view_returns_the_owners_answers(ctx, small_case):
    dim, rows, queries, graph, payload = small_case
    h = mirror(ctx, sm.L2SQ, dim, rows, graph, payload)
    own = h.search(queries, 10, 10)
    ctx2 = api.Context(0)
    view = h.share(ctx2)
    got = view.search(queries, 10, 10)
    for a, b in zip(own, got):
        assert np.array_equal(a, b)
    n = len(rows[0]) - 1
    slot = np.arange(n, dtype=np.int32)
    assert np.array_equal(view.score(queries, slot), shm.all_distances(sm.L2SQ, queries, rows)[0])
    assert np.array_equal(view.score_pairs(slot, slot[::-1]), h.score_pairs(slot, slot[::-1]))
    assert np.array_equal(view.get_payload(np.array([3, -1])), np.stack([payload[3], np.zeros(3, np.uint32)]))
    assert _lib.lib.pgv_hnsw_device(view.h) == _lib.lib.pgv_hnsw_device(h.h) == 0
    view.close()
    ctx2.close()
    h.close()


def test_payload_round_trip(ctx, small_case):
    dim, rows, _, _, payload = small_case
    h = mirror(ctx, sm.L1, dim, rows, payload=payload)
    ids = np.array([0, 16, -1, 5, 5], dtype=np.int64)
    want = np.where(ids[:, None] >= 0, payload[np.clip(ids, 0, None)], 0)
    assert np.array_equal(h.get_payload(ids), want)
    h.close()


def test_update_graph_is_seen_by_the_next_search(ctx, small_case):
    dim, rows, queries, (m, entry, levels, nbr_start, nbr), _ = small_case
    n = len(rows[0]) - 1
    h = mirror(ctx, sm.L1, dim, rows, (m, entry, levels, nbr_start, np.full_like(nbr, -1)))
    elem, dist, scored = h.search(queries, n, n)
    assert (elem[:, 0] == 0).all() and (elem[:, 1:] == -1).all() and (scored == 1).all()  # nothing but the entry point
    # element 3 becomes the entry point and gets its full tuple: everything is one hop away
    h.update_graph(3, np.array([3], dtype=np.int32), np.array([0, 2 * m], dtype=np.int64), nbr[nbr_start[3]:nbr_start[4]])
    elem, dist, scored = h.search(queries, n, n)
    assert (scored == n).all()
    shm.assert_topk_up_to_ties(elem, dist, shm.all_distances(sm.L1, queries, rows), n)
    h.close()


# ------------------------------------------------------------------------------------------------------- 8. refusals
def upload_raw(ctx, dim, ptr, idx, val):
    h = C.c_void_p()
    rc = _lib.lib.pgv_hnsw_upload_sparse(ctx.h, api.PGV_L2SQ, dim, api.ptr(ptr), api.ptr(idx), api.ptr(val), len(ptr) - 1, None, 0,
                                         C.byref(h))
    return rc, h


def test_upload_refusals(ctx):
    import torch
    dim = 5000
    good = shm.rand_csr([3, 1000, 5], 81, dim=dim)
    over = shm.rand_csr([3, 1001, 5], 82, dim=dim)
    text = "sparsevec cannot have more than 1000 non-zero elements for hnsw index"
    with refused(_lib.PGV_ERR_DIMS, text, "element 1"):
        api.SparseHnsw(ctx, api.PGV_L2SQ, dim, over)
    # a device row_ptr is copied to the host and checked like a host one
    dev = [torch.from_numpy(x).cuda() for x in over]
    with refused(_lib.PGV_ERR_DIMS, text, "element 1"):
        api.SparseHnsw(ctx, api.PGV_L2SQ, dim, dev)
    with refused(api.PGV_ERR_ARG, "not monotone"):
        api.SparseHnsw(ctx, api.PGV_L2SQ, dim, [torch.tensor([0, 5, 3], dtype=torch.int64).cuda(), dev[1], dev[2]])
    ptr, idx, val = (x.copy() for x in good)
    idx[1], idx[2] = idx[2], idx[1]
    with refused(api.PGV_ERR_ARG, "does not ascend", "vector 0"):
        api.SparseHnsw(ctx, api.PGV_L2SQ, dim, (ptr, idx, val))
    ptr, idx, val = (x.copy() for x in good)
    val[4] = np.inf
    with refused(api.PGV_ERR_ARG, "not finite", "vector 1"):
        api.SparseHnsw(ctx, api.PGV_L2SQ, dim, (ptr, idx, val))
    with refused(_lib.PGV_ERR_DIMS, "dimensions"):
        api.SparseHnsw(ctx, api.PGV_L2SQ, 10 ** 9 + 1, good)
    with refused(api.PGV_ERR_ARG, "metric"):
        api.SparseHnsw(ctx, 7, dim, good)
    api.SparseHnsw(ctx, api.PGV_L2SQ, dim, good).close()  # 1000 stored elements are fine


def test_entries_that_do_not_serve_a_sparse_mirror(ctx, small_case):
    dim, rows, queries, graph, _ = small_case
    m = graph[0]
    n = len(rows[0]) - 1
    h = mirror(ctx, sm.L2SQ, dim, rows, graph)
    L, P = _lib.lib, api.ptr
    dense = np.zeros((2, dim), dtype=np.float32)
    i32, f32, i64, u8 = (np.zeros(4096, dtype=t) for t in (np.int32, np.float32, np.int64, np.uint8))
    calls = {
        "pgv_hnsw_search": lambda: L.pgv_hnsw_search(h.h, P(dense), 2, 10, 5, P(i64), P(f32), None),
        "pgv_hnsw_score": lambda: L.pgv_hnsw_score(h.h, P(dense), 2, P(i32), None, 4, P(f32)),
        "pgv_hnsw_export": lambda: L.pgv_hnsw_export(h.h, C.create_string_buffer(256)),
        "pgv_hnsw_build_search": lambda: L.pgv_hnsw_build_search(h.h, P(i32), P(i32), 2, 8, 2, P(i32), P(f32), P(i32)),
        "pgv_hnsw_build_neighbors": lambda: L.pgv_hnsw_build_neighbors(h.h, P(i32), P(i32), 2, 8, 2, P(i32), P(f32), P(u8),
                                                                     P(i32), None),
        "pgv_hnsw_build_search_keep": lambda: L.pgv_hnsw_build_search_keep(h.h, P(i32), P(i32), 2, 8, 2, 0),
        "pgv_hnsw_build_select_kept": lambda: L.pgv_hnsw_build_select_kept(h.h, 0, P(i32), P(f32), P(u8), P(i32), None),
        "pgv_hnsw_score_groups": lambda: L.pgv_hnsw_score_groups(h.h, P(i32), P(i64), P(i32), P(i64), 1, C.c_int64(2), C.c_int64(1),
                                                                 P(f32)),
        "pgv_hnsw_link_begin": lambda: L.pgv_hnsw_link_begin(h.h),
        "pgv_hnsw_link_prepare": lambda: L.pgv_hnsw_link_prepare(h.h, P(i32), P(u8), 2, 2, P(i32), P(f32), P(u8), P(i32), None),
        "pgv_hnsw_link_apply": lambda: L.pgv_hnsw_link_apply(h.h, 0),
        "pgv_hnsw_link_end": lambda: L.pgv_hnsw_link_end(h.h, P(i32), None, None),
    }
    built = [s for s in _lib.SYMBOLS if s.startswith(("pgv_hnsw_build_", "pgv_hnsw_link_"))]
    assert set(built) <= set(calls), set(built) - set(calls)
    for name, call in calls.items():
        rc = call()
        assert rc == api.PGV_ERR_ARG, (name, rc, last_error())
        assert name in last_error() and "sparse mirror" in last_error(), (name, last_error())
        if name in ("pgv_hnsw_search", "pgv_hnsw_score"):
            assert name + "_sparse" in last_error(), last_error()
    # the mirror still answers
    elem, _, scored = h.search(queries, n, n)
    assert (scored == n).all()
    h.close()


def test_sparse_entries_refuse_other_mirrors(ctx):
    dense = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, 8, np.zeros((4, 8), dtype=np.float32))
    bit = api.BitHnsw(ctx, 16, np.zeros((4, 2), dtype=np.uint8))
    q = sm.csr([([1], [1.0])])
    for other in (dense, bit):
        with refused(api.PGV_ERR_ARG, "pgv_hnsw_search_sparse", "not a sparse mirror"):
            api.SparseHnsw.search(other, q, 4, 2)
        with refused(api.PGV_ERR_ARG, "pgv_hnsw_score_sparse", "not a sparse mirror"):
            api.SparseHnsw.score(other, q, np.zeros(2, dtype=np.int32))
    dense.close()
    bit.close()


def test_query_refusals(ctx, small_case):
    dim, rows, queries, graph, _ = small_case
    h = mirror(ctx, sm.L2SQ, dim, rows, graph)
    with refused(api.PGV_ERR_ARG, "does not ascend"):
        h.search(sm.csr([([5, 5], [1.0, 2.0])]), 4, 2)
    with refused(api.PGV_ERR_ARG, "not finite"):
        h.score(sm.csr([([5], [np.nan])]), np.zeros(1, dtype=np.int32))
    with refused(_lib.PGV_ERR_DIMS, "16000"):
        h.search(sm.csr([(np.arange(16001, dtype=np.int32), np.ones(16001, dtype=np.float32))]), 4, 2)
    with refused(api.PGV_ERR_ARG, "outside"):
        h.search(sm.csr([([dim], [1.0])]), 4, 2)
    with refused(api.PGV_ERR_ARG, "ef_search"):
        h.search(queries, 1001, 2)
    h.close()


# ---------------------------------------------------------------------------------------------------- 9. empty cases
def test_empty_index_and_no_elements(ctx, small_case):
    dim, rows, queries, (m, entry, levels, nbr_start, nbr), _ = small_case
    nq = len(queries[0]) - 1
    h = mirror(ctx, sm.L2SQ, dim, rows, (m, -1, levels, nbr_start, nbr))  # an empty index: no entry point
    elem, dist, scored = h.search(queries, 10, 4)
    assert (elem == -1).all() and np.isposinf(dist).all() and (scored == 0).all()
    h.close()
    none = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    h = api.SparseHnsw(ctx, api.PGV_NEG_IP, dim, none)
    h.set_graph(m, -1, np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    elem, dist, scored = h.search(queries, 10, 4)
    assert elem.shape == (nq, 4) and (elem == -1).all() and np.isposinf(dist).all() and (scored == 0).all()
    h.close()
