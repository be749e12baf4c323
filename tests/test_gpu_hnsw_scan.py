"""pgv_hnsw_scan_* -- hnsw.iterative_scan on the device -- against tests/hnsw_scan_model.py: the first batch against
pgv_hnsw_search, whole streams to exhaustion against the reference transliterated (tie-free data) and against the array
form's own tie order (integer data), the pool's edges, `want`, several open scans, graph patches between batches, drain,
hnswgettuple's loop, the argument errors and the overflow of a pool.

The models get the DEVICE's distances: a table from pgv_hnsw_score over all n elements (n is small), so that a stream is
compared element for element and bit for bit.  The selection of a resumed batch has no fast path: one radix descent and
one pass in chunks of 256 entries whatever the pool holds, so the edges are a pool below / at / above ef and below / above
256 entries."""
import ctypes as C

import numpy as np
import pytest

import hnsw_scan_cases as sc
import hnsw_tie_cases as tc
from hnsw_scan_model import model_scan, ref_scan
from pgvector_amd import _lib, api

pytestmark = pytest.mark.gpu

METRIC = {"l2": api.PGV_L2SQ, "negip": api.PGV_NEG_IP, "l1": api.PGV_L1}
DTYPE = {"f32": api.PGV_F32, "f16": api.PGV_F16}
FORMS = [(m, t) for m in ("l2", "negip", "l1") for t in ("f32", "f16")] + [("l2", "bits")]
CHUNK = 256  # entries the entry step's compaction reads at a time


def mirror_of(ctx, metric, kind, rows, graph):
    if kind == "bits":
        h = api.BitHnsw(ctx, rows.shape[1], np.packbits(rows.astype(np.uint8), axis=1))
    else:
        h = api.Hnsw(ctx, METRIC[metric], DTYPE[kind], rows.shape[1], rows)
    h.set_graph(*graph)
    return h


def as_queries(kind, queries):
    return np.packbits(queries.astype(np.uint8), axis=1) if kind == "bits" else queries


def table(h, queries, n):
    """the device's distance of every query to every element [nq x n] float32"""
    nq = len(queries)
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


def as_batches(run):
    return [(ids, bits(d), t) for ids, d, t in run]


def strip(stream):
    return [b[:3] for b in stream]


# ------------------------------------------------------------------------------------------------------ the first batch
_float_case = {}


def float_case(n, dim, m, top, nq, seed):
    key = (n, dim, m, top, nq, seed)
    if key not in _float_case:
        rows, queries = sc.rows_and_queries(seed, n, dim, nq, False)
        _float_case[key] = rows, queries, sc.knn_graph(rows, m, seed + 1, top=top)
    return _float_case[key]


@pytest.mark.parametrize("metric,kind", FORMS)
def test_first_batch_is_the_plain_search(ctx, oracle, metric, kind):
    """elements, distance bits and scored of pgv_hnsw_search(ef, k = ef): on float data (a leveled graph, 64 queries) and
    on the tie data of the walk's own tests"""
    cases = []
    if kind != "bits":
        rows, queries, graph = float_case(600, 48, 16, 2, 64, 11)
        cases.append((rows, queries, graph, (1, 40, 65)))
    elements, tq, ex, _ = tc.random_graph(oracle, "bits" if kind == "bits" else metric)
    cases.append((elements, tq, (8, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"]), (2, 10, 64, 200)))
    for rows, queries, graph, efs in cases:
        h = mirror_of(ctx, metric, kind, rows, graph)
        q = as_queries(kind, queries)
        for ef in efs:
            elem, dist, scored = h.search(q, ef, ef)
            with h.scan(q, ef) as s:
                e, d, c, sco, left = s.next()
            assert np.array_equal(e, elem) and np.array_equal(d.view(np.uint32), dist.view(np.uint32)), (metric, kind, ef)
            assert np.array_equal(sco, scored) and np.array_equal(c, (elem >= 0).sum(1))
            assert (left >= 0).all() and (left + c <= scored).all()
        h.close()


# -------------------------------------------------------------------------------------------------- tie-free streams
# (n, dim, m, top, nq, seed, efs): seeds for which no query's fp32 distance table has a duplicate
STREAMS = [(300, 8, 4, 0, 4, 21, (1, 2, 5, 16)), (400, 48, 16, 2, 3, 28, (16, 40, 64, 65)), (300, 8, 4, 2, 3, 29, (1, 5, 64, 65)),
           (1500, 8, 16, 0, 2, 30, (1000,))]
_streams = {}


def tie_free_streams(ctx, i):
    """case i of STREAMS on the device and through ref_scan, once per session"""
    if i not in _streams:
        n, dim, m, top, nq, seed, efs = STREAMS[i]
        rows, queries, graph = float_case(n, dim, m, top, nq, seed)
        h = mirror_of(ctx, "l2", "f32", rows, graph)
        d = table(h, queries, n)
        for q in range(nq):
            assert len(np.unique(d[q])) == n, "query %d of case %d has two elements at one distance: pick another seed" % (q, i)
        got, want = {}, {}
        for ef in efs:
            with h.scan(queries, ef) as s:
                got[ef] = device_stream(s)
            want[ef] = [as_batches(ref_scan(d[q].tolist().__getitem__, graph[2], graph[3], graph[4], graph[0], graph[1], ef))
                        for q in range(nq)]
        h.close()
        _streams[i] = got, want
    return _streams[i]


@pytest.mark.parametrize("i", range(len(STREAMS)))
def test_tie_free_stream_is_the_reference(ctx, i):
    """every batch of every query to exhaustion: the elements, the distance bits and so->tuples of the reference's
    GetScanItems / ResumeScanItems"""
    got, want = tie_free_streams(ctx, i)
    for ef in STREAMS[i][6]:
        for q in range(STREAMS[i][4]):
            assert strip(got[ef][q]) == want[ef][q], (STREAMS[i], ef, q)
            assert len(want[ef][q]) > 1


def test_pool_edges_occurred(ctx):
    """from out_left: a resumed batch that found fewer than ef entries, one that found exactly ef, pools above and below
    the compaction's chunk of 256 entries at their entry step and one that crossed it"""
    short = exact = big = small = crossing = 0
    for i in range(len(STREAMS)):
        got, _ = tie_free_streams(ctx, i)
        for ef, streams in got.items():
            for stream in streams:
                lefts = [b[3] for b in stream]
                for before, batch in zip(lefts, stream[1:]):  # `before`: the pool the batch's entry step read
                    assert len(batch[0]) >= min(ef, before)  # (its entry points; W never shrinks)
                    short += 0 < before < ef
                    exact += before == ef
                    big += before > CHUNK
                    small += before <= CHUNK
                crossing += max(lefts) > CHUNK and any(0 < x <= CHUNK for x in lefts[lefts.index(max(lefts)):])
    print("short", short, "exact", exact, "above the chunk", big, "within it", small, "crossing", crossing)
    assert short > 0 and exact > 0 and big > 0 and small > 0 and crossing > 0


# ----------------------------------------------------------------------------------------------------- tied streams
_tied = {}


def tied_case(ctx, kind):
    if kind not in _tied:
        n, nq = 300, 4
        rows, queries = sc.rows_and_queries(31, n, 8, nq, True)
        graph = sc.knn_graph(rows, 4, 32)  # flat: the layer-0 entry point, and so what is reachable, is the same in every tie order
        h = mirror_of(ctx, "l2", kind, rows, graph)
        d = table(h, queries, n)
        assert np.array_equal(d, sc.l2_table(queries, rows))  # integers: exact in fp32 and fp16
        _tied[kind] = h, queries, graph, d
    return _tied[kind]


@pytest.mark.parametrize("kind", ("f32", "f16"))
@pytest.mark.parametrize("ef", (1, 5, 16, 65))
def test_tied_stream_is_the_model(ctx, kind, ef):
    """integer data, most distances shared: the device's stream is model_scan's batch by batch -- (distance, pool
    position) decides --, and what holds in every tie order holds against ref_scan: the same elements once each, the
    same tuples at exhaustion"""
    h, queries, graph, d = tied_case(ctx, kind)
    m, entry, levels, start, nbr = graph
    with h.scan(queries, ef) as s:
        got = device_stream(s)
    for q in range(len(queries)):
        dq = d[q].tolist()
        assert len(set(dq)) < len(dq) // 4
        ms = model_scan(dq.__getitem__, levels, start, nbr, m, entry, ef)
        assert strip(got[q]) == as_batches(ms.run()), (kind, ef, q)
        ref = ref_scan(dq.__getitem__, levels, start, nbr, m, entry, ef)
        ids, ref_ids = [e for b in got[q] for e in b[0]], [e for b in ref for e in b[0]]
        assert len(ids) == len(set(ids)) and set(ids) == sc.reachable(graph, entry) == set(ref_ids)
        assert got[q][-1][2] == len(ids) == ref[-1][2]
        assert max(b[3] for b in got[q]) <= len(dq)


# -------------------------------------------------------------------------------------------------------------- want
def test_want_advances_a_subset_and_leaves_the_rest(ctx):
    rows, queries, graph = float_case(300, 8, 4, 0, 4, 21)
    queries = np.concatenate([queries, queries[::-1]])  # 8 queries
    h = mirror_of(ctx, "l2", "f32", rows, graph)
    with h.scan(queries, 5) as s:
        lock_step = device_stream(s)
    rng = np.random.default_rng(5)
    with h.scan(queries, 5) as s:
        e, d, c, sco, left = s.next(np.array([1, 0, 0, 1, 0, 0, 0, 0]))
        assert c.tolist() == [5, 0, 0, 5, 0, 0, 0, 0] and sco[1] == 0 and left[1] == 0
        assert (e[0].tolist(), bits(d[0]), int(sco[0]), int(left[0])) == lock_step[0][0]
        # an unwanted query reports its state and keeps it
        e, d, c, sco, left = s.next(np.array([0, 1, 0, 0, 0, 0, 0, 0]))
        assert c.tolist() == [0, 5, 0, 0, 0, 0, 0, 0] and (int(sco[0]), int(left[0])) == lock_step[0][0][2:]
        rest = device_stream(s, schedule=lambda step, live: rng.random(8) < 0.4)
    for q in range(8):
        head = lock_step[q][:1] if q in (0, 1, 3) else []
        assert head + rest[q] == lock_step[q], q
    h.close()


# -------------------------------------------------------------------------------------------------------- open scans
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


def test_open_scans_searches_views_and_patches(ctx):
    """two scans open on one mirror and one on a view of it, a plain search between their batches: every stream is the
    one it is alone; then a pgv_hnsw_update_graph between two batches is followed from that batch on"""
    rows, queries, graph = float_case(300, 8, 4, 0, 4, 21)
    m, entry, levels, start, nbr = graph
    h = mirror_of(ctx, "l2", "f32", rows, graph)
    alone = {}
    for ef in (2, 16):
        with h.scan(queries, ef) as s:
            alone[ef] = device_stream(s)
    plain = h.search(queries, 40, 10)
    ctx2 = api.Context(0)
    view = h.share(ctx2)
    a, b, c = h.scan(queries, 2), h.scan(queries, 16), view.scan(queries, 16)
    got = {id(a): [[] for _ in queries], id(b): [[] for _ in queries], id(c): [[] for _ in queries]}
    for step in range(12):
        for s in (a, b, c):
            e, d, cnt, sco, left = s.next()
            for q in range(len(queries)):
                if cnt[q]:
                    got[id(s)][q].append((e[q, :cnt[q]].tolist(), bits(d[q, :cnt[q]]), int(sco[q]), int(left[q])))
            again = (h if step % 2 else view).search(queries, 40, 10)
            assert all(np.array_equal(x, y) for x, y in zip(again, plain))
    for s, ef in ((a, 2), (b, 16), (c, 16)):
        for q in range(len(queries)):
            assert got[id(s)][q] == alone[ef][q][:len(got[id(s)][q])] and len(got[id(s)][q]) == min(12, len(alone[ef][q]))
        s.close()
    # the patch, through the view; the owner's scan sees it in its next batch
    d = table(h, queries, len(rows))
    rng = np.random.default_rng(9)
    with h.scan(queries, 5) as s:
        models = [model_scan(d[q].tolist().__getitem__, levels, start, nbr, m, entry, 5) for q in range(len(queries))]
        for _ in range(3):
            e, dd, cnt, sco, left = s.next()
            for q, ms in enumerate(models):
                ids, dist, t = ms.next()
                assert (e[q, :cnt[q]].tolist(), bits(dd[q, :cnt[q]]), int(sco[q])) == (ids, bits(dist), t)
        unvisited = sorted(set(range(len(rows))) - set().union(*[ms.visited for ms in models]))
        assert len(unvisited) >= 40
        graph2, (els, offs, packed) = patched(graph, unvisited[::2] + sorted(models[0].visited)[:10], rng)
        view.update_graph(entry, els, offs, packed)
        for ms in models:
            ms.set_graph(*graph2[2:], graph2[0], graph2[1])
        got2 = device_stream(s)
        for q, ms in enumerate(models):
            assert strip(got2[q]) == as_batches(ms.run()), q
        unpatched = [model_scan(d[q].tolist().__getitem__, levels, start, nbr, m, entry, 5).run() for q in range(len(queries))]
        assert any(as_batches(unpatched[q])[3:] != strip(got2[q]) for q in range(len(queries)))  # (the patch mattered)
    view.close()
    ctx2.close()
    h.close()


# ------------------------------------------------------------------------------------------------------------- drain
def test_drain_returns_the_pool_nearest_first(ctx):
    h, queries, graph, d = tied_case(ctx, "f32")
    m, entry, levels, start, nbr = graph
    nq = len(queries)
    with h.scan(queries, 5) as s:
        models = [model_scan(d[q].tolist().__getitem__, levels, start, nbr, m, entry, 5) for q in range(nq)]
        for _ in range(2):
            s.next()
            for ms in models:
                ms.next()
        e, dd, cnt = s.drain(7, np.array([1, 0, 1, 1]))
        assert cnt[1] == 0 and (e[1] == -1).all()
        for q in (0, 2, 3):
            ids, dist = models[q].drain(7)
            assert cnt[q] == 7 and (e[q].tolist(), bits(dd[q])) == (ids, bits(dist))
        # a walk after a drain goes on from the pool that is left
        e, dd, cnt, sco, left = s.next()
        for q, ms in enumerate(models):
            ids, dist, t = ms.next()
            assert (e[q, :cnt[q]].tolist(), bits(dd[q, :cnt[q]]), int(sco[q]), int(left[q])) == (ids, bits(dist), t, len(ms.pool))
        sizes = [len(ms.pool) for ms in models]
        assert max(sizes) > 0
        e, dd, cnt = s.drain(1000)
        for q, ms in enumerate(models):
            ids, dist = ms.drain(1000)
            assert cnt[q] == sizes[q] and (e[q, :cnt[q]].tolist(), bits(dd[q, :cnt[q]])) == (ids, bits(dist))
        assert (s.drain(3)[2] == 0).all()
        e, dd, cnt, sco, left = s.next()
        assert (cnt == 0).all() and (left == 0).all() and (e == -1).all()


# ----------------------------------------------------------------------------------------------- hnswgettuple's loop
@pytest.mark.parametrize("strict", (False, True))
@pytest.mark.parametrize("selectivity,limit", [(0.5, 20000), (0.1, 20000), (0.1, 60), (0.0, 20000), (0.0, 60)])
def test_iterative_search_is_the_models_loop(ctx, selectivity, limit, strict):
    h, queries, graph, d = tied_case(ctx, "f32")
    m, entry, levels, start, nbr = graph
    keep = np.random.default_rng(3).random(d.shape[1]) < selectivity
    ids, dist, scored = api.hnsw_iterative_search(h, queries, 10, keep, 5, max_scan_tuples=limit, strict=strict)
    for q in range(len(queries)):
        ms = model_scan(d[q].tolist().__getitem__, levels, start, nbr, m, entry, 5)
        w_ids, w_dist, w_t = ms.iterative_search(10, keep, max_scan_tuples=limit, strict=strict)
        assert (ids[q], bits(dist[q]), int(scored[q])) == (w_ids, bits(w_dist), w_t), (q, selectivity, limit, strict)
        assert all(keep[e] for e in ids[q]) and (not strict or dist[q] == sorted(dist[q]))
        if selectivity == 0.0:
            assert ids[q] == [] and (w_t >= limit or w_t == len(sc.reachable(graph, entry)))


def test_iterative_search_known_answer(ctx):
    """the reference's recorded case (test/expected/hnsw_vector.out:111-132)"""
    from hnsw_walk_model import tuples
    g = sc.golden()
    rows = np.array(g["rows"], dtype=np.float32)
    levels, start, nbr = tuples(2, [0, 0, 0], {(0, 0): [1, 2], (1, 0): [0, 2], (2, 0): [0, 1]})
    for kind in ("f32", "f16"):
        for entry in range(3):
            h = mirror_of(ctx, "l2", kind, rows, (2, entry, levels, start, nbr))
            for case in g["cases"]:
                ids, _, scored = api.hnsw_iterative_search(h, np.array([g["query"]], dtype=np.float32), 10, np.ones(3, bool),
                                                           g["ef_search"], strict=case["iterative_scan"] == "strict_order")
                assert rows[ids[0]].tolist() == case["expected"] and scored[0] == 3
            h.close()


# ------------------------------------------------------------------------------------------------------------ errors
def test_errors_before_any_launch(ctx):
    rows, queries, graph = float_case(300, 8, 4, 0, 4, 21)
    lib, P = _lib.lib, C.c_void_p
    out = P()
    q = np.ascontiguousarray(queries)

    def fails(rc, *words):
        assert rc == _lib.PGV_ERR_ARG, rc
        text = lib.pgv_last_error().decode()
        assert all(w in text for w in words), text

    sparse = api.SparseHnsw(ctx, api.PGV_L2SQ, 8, (np.array([0, 1, 2], np.int64), np.array([0, 1], np.int32), np.ones(2, np.float32)))
    sparse.set_graph(2, 0, np.zeros(2, np.int32), np.array([0, 4, 8], np.int64), np.full(8, -1, np.int32))
    fails(lib.pgv_hnsw_scan_begin(sparse.h, api.ptr(q), 1, 10, 0, C.byref(out)), "sparse")
    with pytest.raises(api.PgvError):
        sparse.scan((np.array([0, 1], np.int64), np.array([0], np.int32), np.ones(1, np.float32)), 10)
    sparse.close()
    bare = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, 8, rows)
    fails(lib.pgv_hnsw_scan_begin(bare.h, api.ptr(q), 4, 10, 0, C.byref(out)), "pgv_hnsw_set_graph")
    bare.set_graph(*graph)
    for ef in (0, 1001):
        fails(lib.pgv_hnsw_scan_begin(bare.h, api.ptr(q), 4, ef, 0, C.byref(out)), "ef_search", str(ef))
    fails(lib.pgv_hnsw_scan_begin(None, api.ptr(q), 4, 10, 0, C.byref(out)), "NULL")
    fails(lib.pgv_hnsw_scan_begin(bare.h, api.ptr(q), 4, 10, 0, None), "NULL")
    fails(lib.pgv_hnsw_scan_begin(bare.h, None, 4, 10, 0, C.byref(out)), "NULL")
    fails(lib.pgv_hnsw_scan_begin(bare.h, api.ptr(q), 4, 10, -1, C.byref(out)), "discard_cap")
    assert out.value is None
    e, d, c = np.zeros((4, 10), np.int64), np.zeros((4, 10), np.float32), np.zeros(4, np.int32)
    fails(lib.pgv_hnsw_scan_next(None, None, api.ptr(e), api.ptr(d), api.ptr(c), None, None), "NULL")
    with bare.scan(q, 10) as s:
        fails(lib.pgv_hnsw_scan_next(s.s, None, None, api.ptr(d), api.ptr(c), None, None), "NULL")
        fails(lib.pgv_hnsw_scan_next(s.s, None, api.ptr(e), api.ptr(d), None, None, None), "NULL")
        for count in (0, 1001):
            fails(lib.pgv_hnsw_scan_drain(s.s, None, count, api.ptr(e), api.ptr(d), api.ptr(c)), "count", str(count))
        fails(lib.pgv_hnsw_scan_drain(s.s, None, 5, api.ptr(e), None, api.ptr(c)), "NULL")
        # scored / left are optional, and nothing above touched the scan
        api.check(lib.pgv_hnsw_scan_next(s.s, None, api.ptr(e), api.ptr(d), api.ptr(c), None, None))
        first = bare.search(q, 10, 10)
        assert np.array_equal(e, first[0]) and c.tolist() == [10] * 4
    lib.pgv_hnsw_scan_end(None)
    # an empty index: count 0 everywhere, for ever
    bare.set_graph(4, -1, graph[2], graph[3], graph[4])
    with bare.scan(q, 10) as s:
        for _ in range(2):
            e, d, c, sco, left = s.next()
            assert (c == 0).all() and (e == -1).all() and np.isinf(d).all() and (sco == 0).all() and (left == 0).all()
        assert (s.drain(5)[2] == 0).all()
    with bare.scan(q[:0], 10) as s:
        assert s.next()[0].shape == (0, 10)
    bare.close()


def test_overflow_ends_the_scan_and_nothing_else(ctx):
    rows, queries, graph = float_case(400, 48, 16, 2, 3, 28)
    h = mirror_of(ctx, "l2", "f32", rows, graph)
    d = table(h, queries, len(rows))
    before = h.search(queries, 5, 5)
    with h.scan(queries, 5, discard_cap=4) as s:
        for _ in range(2):
            with pytest.raises(api.PgvError) as err:
                s.next()
            assert err.value.code == _lib.PGV_ERR_NOMEM and "query " in err.value.message and "4 entries" in err.value.message
        with pytest.raises(api.PgvError) as err:
            s.drain(3)
        assert err.value.code == _lib.PGV_ERR_NOMEM
    assert all(np.array_equal(x, y) for x, y in zip(h.search(queries, 5, 5), before))
    # a cap that the first batches respect and a later one does not: the batches before it are the model's
    with h.scan(queries, 5) as s:
        full = device_stream(s)
    peak = max(b[3] for st in full for b in st)
    with h.scan(queries, 5, discard_cap=peak - 1) as s:
        with pytest.raises(api.PgvError) as err:
            device_stream(s)
        assert err.value.code == _lib.PGV_ERR_NOMEM
    with h.scan(queries, 5, discard_cap=peak) as s:
        assert device_stream(s) == full
    m, entry, levels, start, nbr = graph
    for q in range(len(queries)):
        ms = model_scan(d[q].tolist().__getitem__, levels, start, nbr, m, entry, 5)
        assert strip(full[q]) == as_batches(ms.run())
    h.close()
