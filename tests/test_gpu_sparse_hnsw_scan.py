"""pgv_hnsw_scan_begin_sparse -- hnsw.iterative_scan over sparsevec elements on the device -- and what serves such a scan
(pgv_hnsw_scan_next / _drain / _end, api.SparseHnsw.scan_sparse, api.hnsw_iterative_search) against
tests/hnsw_scan_model.py: the first batch against pgv_hnsw_search_sparse, whole streams to exhaustion against the reference
transliterated (tie-free and float data) and against the array form's own tie order (tied data), the pool's edges, `want`,
several open scans, views, graph patches, buildable mirrors, drain, hnswgettuple's loop, the LDS limit, the argument
errors and the overflow of a pool.

As in tests/test_gpu_hnsw_scan.py the models get the DEVICE's distances -- a table from pgv_hnsw_score_sparse over all n
elements -- and every comparison is equality: elements, distance bits, so->tuples, pool sizes.
tests/test_sparse_hnsw_scan_model_cpu.py checks the preconditions on the same seeds."""
import ctypes as C

import numpy as np
import pytest

import sparse_hnsw_model as shm
import sparse_model as sm
from hnsw_scan_model import model_scan, ref_scan
from pgvector_amd import _lib, api

pytestmark = pytest.mark.gpu

METRIC = {sm.L2SQ: api.PGV_L2SQ, sm.NEG_IP: api.PGV_NEG_IP, sm.L1: api.PGV_L1}
EFS = (1, 5, 16, 65)
CHUNK = 256  # entries the entry step's compaction reads at a time
FLOAT_DIM = 20000
TIED = dict(nq=8, n=600, dim=1536, seed=13)


def count(csr):
    return len(csr[0]) - 1


def mirror(ctx, metric, dim, rows, graph, buildable=False):
    h = api.SparseHnsw(ctx, METRIC[metric], dim, rows, buildable=buildable)
    h.set_graph(*graph)
    return h


def table(h, queries, n):
    """the device's distance of every query to every element [nq x n] float32"""
    nq = count(queries)
    d = h.score(queries, np.tile(np.arange(n, dtype=np.int32), nq), np.repeat(np.arange(nq, dtype=np.int32), n))
    return np.asarray(d).reshape(nq, n)


def bits(x):
    return (np.asarray(x, dtype=np.float32) + np.float32(0)).view(np.uint32).tolist()  # (-0 has key +0)


def device_stream(scan, schedule=None, limit=100000):
    """every batch of every query until all are exhausted -> per query [(ids, distance bits, scored, left)].
    schedule(step, live) -> the queries to advance in that step (None: all live ones)"""
    nq, ef = scan.nq, scan.ef
    out = [[] for _ in range(nq)]
    live = np.ones(nq, dtype=bool)
    for step in range(limit):
        if not live.any():
            return out
        want = live.copy() if schedule is None else (schedule(step, live) & live)
        if not want.any():
            continue
        e, d, c, s, left = scan.next(None if schedule is None and want.all() else want)
        assert (c[~want] == 0).all() and (e[~want] == -1).all() and np.isinf(d[~want]).all()
        for q in np.flatnonzero(want):
            k = int(c[q])
            assert (e[q, k:] == -1).all() and np.isinf(d[q, k:]).all() and 0 <= k <= ef
            if k == 0:
                live[q] = False
                assert left[q] == 0
            else:
                out[q].append((e[q, :k].tolist(), bits(d[q, :k]), int(s[q]), int(left[q])))
    raise AssertionError("the scan did not end")


def model_stream(ms):
    """a model scan to exhaustion in device_stream's form: left is the pool after the batch"""
    out = []
    while True:
        ids, dist, t = ms.next()
        if not ids:
            return out
        out.append((ids, bits(dist), t, len(ms.pool)))


def as_batches(run):
    return [(ids, bits(d), t) for ids, d, t in run]


def strip(stream):
    return [b[:3] for b in stream]


def model_of(d, q, graph, ef):
    m, entry, levels, start, nbr = graph
    return model_scan(d[q].tolist().__getitem__, levels, start, nbr, m, entry, ef)


def ref_of(d, q, graph, ef):
    m, entry, levels, start, nbr = graph
    return as_batches(ref_scan(d[q].tolist().__getitem__, levels, start, nbr, m, entry, ef))


# ----------------------------------------------------------------------------------------------------------- the cases
_cases = {}


def case(ctx, name, metric):
    """(mirror, queries CSR, graph, the device's table) of a named draw under a metric, once per session"""
    key = (name, metric)
    if key not in _cases:
        if name == "tie_free":
            dim = shm.TIE_FREE["dim"]
            if "tie_free_data" not in _cases:
                _cases["tie_free_data"] = shm.tie_free(**shm.TIE_FREE)
            queries, rows = _cases["tie_free_data"]
            graph = shm.random_graph(400, 8, 5)
        elif name == "tied":
            dim = TIED["dim"]
            if "tied_data" not in _cases:
                _cases["tied_data"] = shm.tied(**TIED)
            queries, rows = _cases["tied_data"]
            graph = shm.random_graph(600, 8, 7)
        else:  # every row path of the walk (register copy, long rows, an empty element) and query lengths around the bitmap words
            dim = FLOAT_DIM
            rows = shm.rand_csr([0, 1, 64, 65, 256, 257, 1000] + [40] * 393, 41, dim=dim, floats=True)
            queries = shm.rand_csr([0, 30, 64, 700, 1500], 42, dim=dim, floats=True)
            graph = shm.random_graph(400, 8, 43)
        h = mirror(ctx, metric, dim, rows, graph)
        _cases[key] = h, queries, graph, table(h, queries, count(rows))
    return _cases[key]


# ------------------------------------------------------------------------------------------------------ 1. the first batch
@pytest.mark.parametrize("metric", shm.METRICS)
@pytest.mark.parametrize("name", ("float", "tied"))
def test_first_batch_is_the_plain_search(ctx, name, metric):
    """elements, distance bits and scored of pgv_hnsw_search_sparse(ef, k = ef)"""
    h, queries, graph, d = case(ctx, name, metric)
    for ef in (1, 10, 65):
        elem, dist, scored = h.search(queries, ef, ef)
        with h.scan_sparse(queries, ef) as s:
            assert (s.nq, s.ef) == (count(queries), ef)
            e, dd, c, sco, left = s.next()
        assert np.array_equal(e, elem) and np.array_equal(dd.view(np.uint32), dist.view(np.uint32)), (name, metric, ef)
        assert np.array_equal(sco, scored) and np.array_equal(c, (elem >= 0).sum(1))
        assert (left >= 0).all() and (left + c <= scored).all()


# -------------------------------------------------------------------------------------------------- 2. tie-free streams
@pytest.mark.parametrize("metric", shm.METRICS)
@pytest.mark.parametrize("ef", EFS)
def test_tie_free_stream_is_the_reference(ctx, metric, ef):
    """every batch of every query to exhaustion: the elements, the distance bits and so->tuples of the reference's
    GetScanItems / ResumeScanItems and of the array form, `left` the model's pool after each batch; and from `left` the
    edges of the entry step: a resumed batch from a pool below, at and above ef, pools past the compaction's chunk"""
    h, queries, graph, d = case(ctx, "tie_free", metric)
    n = d.shape[1]
    with h.scan_sparse(queries, ef) as s:
        got = device_stream(s)
    befores, peak = [], 0
    for q in range(count(queries)):
        assert len(np.unique(d[q])) == n, "query %d has two elements at one distance" % q
        assert got[q] == model_stream(model_of(d, q, graph, ef)), (metric, ef, q)
        assert strip(got[q]) == ref_of(d, q, graph, ef), (metric, ef, q)
        assert got[q][-1][2] == n
        lefts = [b[3] for b in got[q]]
        for before, batch in zip(lefts, got[q][1:]):  # `before`: the pool the batch's entry step read
            assert len(batch[0]) >= min(ef, before)  # (its entry points; W never shrinks)
        befores += lefts[:-1]
        peak = max(peak, max(lefts))
    print(metric, ef, "peak", peak, "resumed from a pool <, =, > ef:", sum(0 < b < ef for b in befores),
          sum(b == ef for b in befores), sum(b > ef for b in befores))
    assert peak > CHUNK and any(0 < b <= CHUNK for b in befores)
    assert any(b > ef for b in befores)
    assert any(b == ef for b in befores) == (ef != 65)
    assert any(0 < b < ef for b in befores) == (ef == 65)


# ----------------------------------------------------------------------------------------------------- 3. tied streams
@pytest.mark.parametrize("metric", shm.METRICS)
@pytest.mark.parametrize("ef", EFS)
def test_tied_stream_is_the_model(ctx, metric, ef):
    """most distances shared: the device's stream is model_scan's batch by batch, tie order and pool sizes included"""
    h, queries, graph, d = case(ctx, "tied", metric)
    n = d.shape[1]
    with h.scan_sparse(queries, ef) as s:
        got = device_stream(s)
    for q in range(count(queries)):
        assert len(np.unique(d[q])) < n // 8
        assert got[q] == model_stream(model_of(d, q, graph, ef)), (metric, ef, q)
        ids = [e for b in got[q] for e in b[0]]
        assert sorted(ids) == list(range(n)) and got[q][-1][2] == n


# ---------------------------------------------------------------------------------------------------- 4. float streams
@pytest.mark.parametrize("metric", shm.METRICS)
def test_float_stream_is_the_model_and_the_reference(ctx, metric):
    """float values, elements of 0 .. 1000 and queries of 0 .. 1500 stored elements at ef 16: model_scan for every query,
    ref_scan too wherever the query's table row has no repeated value (the empty query under inner product is all +0.0)"""
    h, queries, graph, d = case(ctx, "float", metric)
    n = d.shape[1]
    with h.scan_sparse(queries, 16) as s:
        got = device_stream(s)
    compared = 0
    for q in range(count(queries)):
        assert got[q] == model_stream(model_of(d, q, graph, 16)), (metric, q)
        assert got[q][-1][2] == n
        if len(np.unique(bits(d[q]))) == n:
            compared += 1
            assert strip(got[q]) == ref_of(d, q, graph, 16), (metric, q)
    if metric == sm.NEG_IP:
        assert len(np.unique(bits(d[0]))) == 1 and bits(d[0])[0] == 0  # the empty query: +0.0 everywhere
    print(metric, "queries compared with ref_scan:", compared)
    assert compared > 0 or metric == sm.NEG_IP  # (under inner product a query that misses two elements has a repeated +0.0)


# ------------------------------------------------------------------------------------------------------------- 5. want
def test_want_advances_a_subset_and_leaves_the_rest(ctx):
    h, queries, graph, d = case(ctx, "tie_free", sm.L2SQ)
    queries = shm.take(queries, [0, 1, 2, 3, 4, 5, 5, 4])  # 8 queries
    with h.scan_sparse(queries, 5) as s:
        lock_step = device_stream(s)
    rng = np.random.default_rng(5)
    with h.scan_sparse(queries, 5) as s:
        e, dd, c, sco, left = s.next(np.array([1, 0, 0, 1, 0, 0, 0, 0]))
        assert c.tolist() == [5, 0, 0, 5, 0, 0, 0, 0] and sco[1] == 0 and left[1] == 0
        assert (e[0].tolist(), bits(dd[0]), int(sco[0]), int(left[0])) == lock_step[0][0]
        # an unwanted query reports its state and keeps it
        e, dd, c, sco, left = s.next(np.array([0, 1, 0, 0, 0, 0, 0, 0]))
        assert c.tolist() == [0, 5, 0, 0, 0, 0, 0, 0] and (int(sco[0]), int(left[0])) == lock_step[0][0][2:]
        rest = device_stream(s, schedule=lambda step, live: rng.random(8) < 0.4)
    for q in range(8):
        head = lock_step[q][:1] if q in (0, 1, 3) else []
        assert head + rest[q] == lock_step[q], q
    assert lock_step[6] == lock_step[5] and lock_step[7] == lock_step[4]


def patched(graph, elements, rng):
    """the graph with the layer-0 neighbours of `elements` shuffled and thinned -> (graph, update_graph's arguments)"""
    m, entry, levels, start, nbr = graph
    nbr = nbr.copy()
    offs, packed = [0], []
    for e in elements:
        a, b = int(start[e]), int(start[e + 1])
        o = a + int(levels[e]) * m
        live = [x for x in nbr[o:o + 2 * m] if x >= 0]
        rng.shuffle(live)
        live = live[:max(1, len(live) // 2)]
        nbr[o:o + 2 * m] = live + [-1] * (2 * m - len(live))
        packed += nbr[a:b].tolist()
        offs.append(len(packed))
    return (m, entry, levels, start, nbr), (np.asarray(elements, np.int32), np.asarray(offs, np.int64), np.asarray(packed, np.int32))


def test_open_scans_searches_views_patches_and_buildable_mirrors(ctx):
    """two scans open on one mirror and one on a view of it in another context, a plain search between their batches:
    every stream is the one it is alone, and a buildable mirror's is the plain mirror's; then a pgv_hnsw_update_graph
    between two batches is followed from that batch on"""
    _, queries, graph, _ = case(ctx, "tie_free", sm.L2SQ)
    rows = _cases["tie_free_data"][1]
    n, dim = count(rows), shm.TIE_FREE["dim"]
    m, entry, levels, start, nbr = graph
    h = mirror(ctx, sm.L2SQ, dim, rows, graph)  # (its own mirror: the patch below stays out of the shared one)
    nq = count(queries)
    alone = {}
    for ef in (2, 16):
        with h.scan_sparse(queries, ef) as s:
            alone[ef] = device_stream(s)
    built_on = mirror(ctx, sm.L2SQ, dim, rows, graph, buildable=True)
    with built_on.scan_sparse(queries, 16) as s:
        assert device_stream(s) == alone[16]
    built_on.close()
    plain = h.search(queries, 40, 10)
    ctx2 = api.Context(0)
    view = h.share(ctx2)
    a, b, c = h.scan_sparse(queries, 2), h.scan_sparse(queries, 16), view.scan_sparse(queries, 16)
    got = {id(a): [[] for _ in range(nq)], id(b): [[] for _ in range(nq)], id(c): [[] for _ in range(nq)]}
    for step in range(12):
        for s in (a, b, c):
            e, d, cnt, sco, left = s.next()
            for q in range(nq):
                if cnt[q]:
                    got[id(s)][q].append((e[q, :cnt[q]].tolist(), bits(d[q, :cnt[q]]), int(sco[q]), int(left[q])))
            again = (h if step % 2 else view).search(queries, 40, 10)
            assert all(np.array_equal(x, y) for x, y in zip(again, plain))
    for s, ef in ((a, 2), (b, 16), (c, 16)):
        for q in range(nq):
            assert got[id(s)][q] == alone[ef][q][:len(got[id(s)][q])] and len(got[id(s)][q]) == min(12, len(alone[ef][q]))
        s.close()
    # the patch, through the view; the owner's scan sees it in its next batch
    d = table(h, queries, n)
    rng = np.random.default_rng(9)
    with h.scan_sparse(queries, 5) as s:
        models = [model_of(d, q, graph, 5) for q in range(nq)]
        for _ in range(3):
            e, dd, cnt, sco, left = s.next()
            for q, ms in enumerate(models):
                ids, dist, t = ms.next()
                assert (e[q, :cnt[q]].tolist(), bits(dd[q, :cnt[q]]), int(sco[q])) == (ids, bits(dist), t)
        unvisited = sorted(set(range(n)) - set().union(*[ms.visited for ms in models]))
        assert len(unvisited) >= 40
        graph2, (els, offs, packed) = patched(graph, unvisited[::2] + sorted(models[0].visited)[:10], rng)
        view.update_graph(entry, els, offs, packed)
        for ms in models:
            ms.set_graph(*graph2[2:], graph2[0], graph2[1])
        got2 = device_stream(s)
        for q, ms in enumerate(models):
            assert strip(got2[q]) == as_batches(ms.run()), q
        unpatched = [model_of(d, q, graph, 5).run() for q in range(nq)]
        assert any(as_batches(unpatched[q])[3:] != strip(got2[q]) for q in range(nq))  # (the patch mattered)
    view.close()
    ctx2.close()
    h.close()


# ------------------------------------------------------------------------------------------------------------ 6. drain
def test_drain_returns_the_pool_nearest_first(ctx):
    h, queries, graph, d = case(ctx, "tied", sm.L2SQ)
    nq = count(queries)
    nobody = np.zeros(nq, dtype=np.uint8)
    with h.scan_sparse(queries, 16) as s:
        models = [model_of(d, q, graph, 16) for q in range(nq)]
        left = s.next()[4]
        for q, ms in enumerate(models):
            ms.next()
            assert left[q] == len(ms.pool) > 17
        for cnt_want in (1, 16, 300):
            e, dd, cnt = s.drain(cnt_want)
            now = s.next(nobody)[4]  # (an unwanted query reports its state)
            for q, ms in enumerate(models):
                ids, dist = ms.drain(cnt_want)
                take = min(cnt_want, int(left[q]))
                assert cnt[q] == take == len(ids) and (e[q, :take].tolist(), bits(dd[q, :take])) == (ids, bits(dist)), (cnt_want, q)
                assert (e[q, take:] == -1).all() and np.isinf(dd[q, take:]).all()
                assert now[q] == left[q] - take == len(ms.pool)
            left = now
        s.drain(1000)
        e, dd, cnt = s.drain(3)  # a drained-out scan has nothing
        assert (cnt == 0).all() and (e == -1).all() and np.isinf(dd).all()
        e, dd, cnt, sco, left = s.next()
        assert (cnt == 0).all() and (left == 0).all() and (e == -1).all()
    # a walk after a drain goes on from the pool that is left; an unwanted query's pool is not drained
    with h.scan_sparse(queries, 16) as s:
        models = [model_of(d, q, graph, 16) for q in range(nq)]
        s.next()
        e, dd, cnt = s.drain(7, np.array([1, 0] * (nq // 2)))
        for q, ms in enumerate(models):
            ms.next()
            if q % 2:
                assert cnt[q] == 0 and (e[q] == -1).all()
            else:
                ids, dist = ms.drain(7)
                assert cnt[q] == 7 and (e[q].tolist(), bits(dd[q])) == (ids, bits(dist))
        e, dd, cnt, sco, left = s.next()
        for q, ms in enumerate(models):
            ids, dist, t = ms.next()
            assert cnt[q] > 0
            assert (e[q, :cnt[q]].tolist(), bits(dd[q, :cnt[q]]), int(sco[q]), int(left[q])) == (ids, bits(dist), t, len(ms.pool))


# ----------------------------------------------------------------------------------------------- 7. hnswgettuple's loop
@pytest.mark.parametrize("strict", (False, True))
@pytest.mark.parametrize("selectivity,limit", [(0.5, 20000), (0.1, 20000), (0.1, 60), (0.0, 60)])
def test_iterative_search_is_the_models_loop(ctx, selectivity, limit, strict):
    h, queries, graph, d = case(ctx, "tied", sm.L2SQ)
    keep = np.random.default_rng(3).random(d.shape[1]) < selectivity
    ids, dist, scored = api.hnsw_iterative_search(h, queries, 10, keep, 16, max_scan_tuples=limit, strict=strict)
    for q in range(count(queries)):
        w_ids, w_dist, w_t = model_of(d, q, graph, 16).iterative_search(10, keep, max_scan_tuples=limit, strict=strict)
        assert (ids[q], bits(dist[q]), int(scored[q])) == (w_ids, bits(w_dist), w_t), (q, selectivity, limit, strict)
        assert all(keep[e] for e in ids[q]) and (not strict or dist[q] == sorted(dist[q]))
        if selectivity == 0.0:
            assert ids[q] == [] and w_t >= limit
        if limit == 60:
            assert w_t == model_of(d, q, graph, 16).next()[2] >= 60  # one walk, then the drain branch


# --------------------------------------------------------------------------------------------------------- 8. the LDS edge
def test_a_16000_element_query_scans_up_to_the_lds_limit(ctx):
    """m 16, one query of 16 000 stored elements: ef 40 fits (136 000 bytes of query region + 800 + 256 + 64 + 1 088) and
    its first batch is the plain search's; ef 1000 (+ 20 000) does not, and begin says so"""
    rows = shm.rand_csr([0, 1, 64, 65, 256, 257, 1000] + [40] * 393, 41, dim=FLOAT_DIM, floats=True)
    query = shm.rand_csr([shm.SPARSE_MAX_NNZ], 44, dim=FLOAT_DIM, floats=True)
    h = mirror(ctx, sm.L2SQ, FLOAT_DIM, rows, shm.random_graph(400, 16, 45))
    elem, dist, scored = h.search(query, 40, 40)
    with h.scan_sparse(query, 40) as s:
        e, dd, c, sco, left = s.next()
        assert np.array_equal(e, elem) and np.array_equal(dd.view(np.uint32), dist.view(np.uint32)) and np.array_equal(sco, scored)
        assert c[0] == 40 and left[0] > 0
        e2, dd2, c2, sco2, _ = s.next()
        assert c2[0] == 40 and sco2[0] > sco[0] and not set(e2[0].tolist()) & set(e[0].tolist())
    out = C.c_void_p()
    rc = _lib.lib.pgv_hnsw_scan_begin_sparse(h.h, api.ptr(query[0]), api.ptr(query[1]), api.ptr(query[2]), 1, 1000, 0, C.byref(out))
    text = _lib.lib.pgv_last_error().decode()
    assert rc == _lib.PGV_ERR_ARG and out.value is None, (rc, text)
    assert all(w in text for w in ("ef 1000", "m 16", "16000", "LDS")), text
    assert all(np.array_equal(x, y) for x, y in zip(h.search(query, 40, 40), (elem, dist, scored)))
    h.close()


# ----------------------------------------------------------------------------------------------------------- 9. errors
def test_errors_before_any_launch(ctx):
    _, queries, graph, _ = case(ctx, "tie_free", sm.L2SQ)
    rows = _cases["tie_free_data"][1]
    dim = shm.TIE_FREE["dim"]
    lib = _lib.lib
    out = C.c_void_p()
    qp, qi, qv = (np.ascontiguousarray(x) for x in queries)
    nq = count(queries)

    def begin(h, ptr_=qp, idx=qi, val=qv, ef=10, cap=0, no_out=False):
        return lib.pgv_hnsw_scan_begin_sparse(h, api.ptr(ptr_), api.ptr(idx), api.ptr(val), nq, ef, cap, None if no_out else C.byref(out))

    def fails(rc, *words):
        assert rc == _lib.PGV_ERR_ARG, (rc, lib.pgv_last_error().decode())
        text = lib.pgv_last_error().decode()
        assert all(w in text for w in words), text
        assert out.value is None

    # the new entry on a dense and on a bit mirror; the dense entry on a sparse mirror names its twin
    dense = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, 8, np.zeros((4, 8), np.float32))
    bitm = api.BitHnsw(ctx, 64, np.zeros((4, 8), np.uint8))
    for other in (dense, bitm):
        other.set_graph(2, 0, np.zeros(4, np.int32), np.arange(5, dtype=np.int64) * 4, np.full(16, -1, np.int32))
        fails(begin(other.h), "not a sparse mirror")
        other.close()
    bare = api.SparseHnsw(ctx, api.PGV_L2SQ, dim, rows)
    fails(begin(bare.h), "pgv_hnsw_set_graph")
    bare.set_graph(*graph)
    before = bare.search(queries, 10, 10)
    fails(lib.pgv_hnsw_scan_begin(bare.h, api.ptr(np.zeros((1, dim), np.float32)), 1, 10, 0, C.byref(out)), "sparse",
          "pgv_hnsw_scan_begin_sparse")
    with pytest.raises(api.PgvError) as err:
        bare.scan(queries, 10)
    assert "scan_sparse" in err.value.message
    for ef in (0, 1001):
        fails(begin(bare.h, ef=ef), "ef_search", str(ef))
    fails(begin(bare.h, cap=-1), "discard_cap")
    fails(begin(None), "NULL")
    fails(begin(bare.h, no_out=True), "NULL")
    fails(begin(bare.h, ptr_=None), "NULL")
    unsorted = qi.copy()
    unsorted[[3, 4]] = unsorted[[4, 3]]
    fails(begin(bare.h, idx=unsorted), "does not ascend", "queries")
    assert all(np.array_equal(x, y) for x, y in zip(bare.search(queries, 10, 10), before))
    # nothing above left anything behind: a scan begins and its first batch is the search's
    with bare.scan_sparse(queries, 10) as s:
        e, d, c, sco, left = s.next()
        assert np.array_equal(e, before[0]) and np.array_equal(sco, before[2])
    # an empty index and an empty batch of queries
    bare.set_graph(graph[0], -1, *graph[2:])
    with bare.scan_sparse(queries, 10) as s:
        for _ in range(2):
            e, d, c, sco, left = s.next()
            assert (c == 0).all() and (e == -1).all() and np.isinf(d).all() and (sco == 0).all() and (left == 0).all()
        assert (s.drain(5)[2] == 0).all()
    with bare.scan_sparse(shm.take(queries, []), 10) as s:
        assert s.next()[0].shape == (0, 10)
    bare.close()


# -------------------------------------------------------------------------------------------------------- 10. overflow
def test_overflow_ends_the_scan_and_nothing_else(ctx):
    h, queries, graph, d = case(ctx, "tie_free", sm.L2SQ)
    before = h.search(queries, 5, 5)
    with h.scan_sparse(queries, 5, discard_cap=8) as s:
        for _ in range(2):
            with pytest.raises(api.PgvError) as err:
                s.next()
            assert err.value.code == _lib.PGV_ERR_NOMEM and "query " in err.value.message and "8 entries" in err.value.message
        with pytest.raises(api.PgvError) as err:
            s.drain(3)
        assert err.value.code == _lib.PGV_ERR_NOMEM
    assert all(np.array_equal(x, y) for x, y in zip(h.search(queries, 5, 5), before))
    with h.scan_sparse(queries, 5) as s:
        full = device_stream(s)
    for q in range(count(queries)):
        assert full[q] == model_stream(model_of(d, q, graph, 5)), q
