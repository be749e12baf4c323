"""Building HNSW graphs over sparsevec elements on the device: pgv_hnsw_upload_sparse_buildable, sparse_groups_kernel behind
pgv_hnsw_score_groups, the build form of hnsw_search_kernel<SparseRow, M> (element slots as queries),
pgv_host_hnsw_build_sparse.

The rule under test: score_element's last bit depends on which vector is the row and which the query, so on
a buildable sparse mirror the build-side value of the pair {a, b} of element slots is pgv_hnsw_score_pairs(min, max) -- the
smaller slot is the row -- wherever it is computed.  The yardsticks: pgv_hnsw_score_pairs (existing code, pinned to
pgv_sparse_distance_batch by tests/test_gpu_sparse_hnsw.py) bit for bit; on integer-valued data, whose sums are exact in
fp32 in any order, tests/sparse_model.py and the dense build over the rows' expansion (pinned to the oracle by
test_hnsw_build_serial_is_the_reference_loop); tests/bit_build_model.py over tests/sparse_build_model.py's functions (pinned
on the CPU by tests/test_sparse_build_model_cpu.py) for a serial float build.  Everything is compared by equality, distances
by their bits.

Smallest shapes at which each kernel can go wrong:
  score_groups   element lengths 0 (both sides too), 1, 63 / 64 / 65 (a register chunk's end), 256 (the last register row),
                 257 (the first row_side_mem row), 1000; groups of 1, 2, 4, 5, 9, 33 and 80 members (more than one 64-lane
                 pass over a group's ids), from = 1, 3, n - 1 and past the size; slots shuffled inside every group
  build search   a few hundred elements in >= 3 layers, ef_construction 12; insert levels above, at and below the entry's,
                 layer_cap at and below the layers present
  select         ef_construction 12 (hnsw_select_wave_kernel) and 80 (hnsw_select_kernel), lists longer than lm
  whole build    the issue's shapes"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bit_build_model as bm
import hnsw_walk_model as wm
import mp_sparse_build_worker as wk
import sparse_build_model as sbm
import sparse_hnsw_model as shm
import sparse_model as sm
from hnsw_link_model import host_select
from oracle import pyoracle as po
from pgvector_amd import _host, _lib, api

pytestmark = pytest.mark.gpu

L2, IP, L1 = api.PGV_L2SQ, api.PGV_NEG_IP, api.PGV_L1
METRICS = (L2, IP, L1)
MODEL = wk.MODEL_METRIC
OPS = {L2: po.OPS_L2, IP: po.OPS_IP, L1: po.OPS_L1}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pgv_hnsw_upload_sparse_buildable"


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).tolist()


def count(csr):
    return len(csr[0]) - 1


def buildable(ctx, metric, dim, rows, graph=None, payload=None):
    h = api.SparseHnsw(ctx, metric, dim, rows, payload=payload, buildable=True)
    if graph is not None:
        h.set_graph(*graph)
    return h


def plain(ctx, metric, dim, rows, graph=None, payload=None):
    h = api.SparseHnsw(ctx, metric, dim, rows, payload=payload)
    if graph is not None:
        h.set_graph(*graph)
    return h


def oriented(h, a, b):
    """the build-side values of the pairs {a[i], b[i]}: pgv_hnsw_score_pairs(min, max)"""
    return h.score_pairs(*sbm.oriented_pairs(a, b))


def build_search(h, elems, qlevels, efc, lcap):
    elems, qlevels = np.ascontiguousarray(elems, np.int32), np.ascontiguousarray(qlevels, np.int32)
    per = len(elems) * lcap
    ids, dist, cnt = np.full((per, efc), -7, np.int32), np.full((per, efc), np.nan, np.float32), np.full(per, -7, np.int32)
    api.check(api.lib.pgv_hnsw_build_search(h.h, api.ptr(elems), api.ptr(qlevels), len(elems), efc, lcap, api.ptr(ids),
                                            api.ptr(dist), api.ptr(cnt)))
    return ids, dist, cnt


def build(h, rows, m, efc, seed, max_batch):
    return _host.hnsw_build(h, None, m, efc, api.make_rng(seed=seed), max_batch=max_batch, rows_csr=rows)


# ---------------------------------------------------------------------------------------------------------- 1. gates
@pytest.fixture(scope="module")
def small_case():
    dim, m = 5000, 8
    n, entry, levels, nbr_start, nbr = shm.complete_graph(m)
    rows = shm.rand_csr([0, 1, 64, 65, 256, 257, 1000] + [40] * (n - 7), 71, dim=dim, floats=True)
    queries = shm.rand_csr([0, 30, 700, 1500, 64], 72, dim=dim, floats=True)
    payload = (np.arange(n, dtype=np.uint32)[:, None] * 31 + np.arange(3, dtype=np.uint32)[None, :]).astype(np.uint32)
    return dim, rows, queries, (m, entry, levels, nbr_start, nbr), payload


@pytest.mark.parametrize("metric", METRICS)
def test_a_buildable_mirror_answers_as_the_plain_mirror_does(ctx, small_case, metric):
    """search, score, score_pairs, payload and a shared view: the plain sparse mirror's answers over the same rows and
    graph.  The view builds.  Export and iterative scans stay refused."""
    dim, rows, queries, graph, payload = small_case
    n = count(rows)
    a, b = plain(ctx, metric, dim, rows, graph, payload), buildable(ctx, metric, dim, rows, graph, payload)
    assert api.lib.pgv_hnsw_buildable_sparse(a.h) == 0 and api.lib.pgv_hnsw_buildable_sparse(b.h) == dim
    assert api.lib.pgv_hnsw_buildable_sparse(None) == 0 and api.lib.pgv_hnsw_buildable_bits(b.h) == 0
    assert api.lib.pgv_hnsw_elements(b.h) == n and api.lib.pgv_hnsw_elements(None) == -1
    want = a.search(queries, 10, 10)
    for x, y in zip(want, b.search(queries, 10, 10)):
        assert np.array_equal(x, y)
    assert bits(want[1]) == bits(b.search(queries, 10, 10)[1])
    slot = np.arange(n, dtype=np.int32)
    assert bits(a.score(queries, slot, slot % 5)) == bits(b.score(queries, slot, slot % 5))
    assert bits(a.score_pairs(slot, slot[::-1])) == bits(b.score_pairs(slot, slot[::-1]))
    assert np.array_equal(b.get_payload(np.array([3, -1])), a.get_payload(np.array([3, -1])))
    with pytest.raises(api.PgvError) as e:
        b.export()
    assert e.value.code == api.PGV_ERR_ARG
    out = C.c_void_p()
    qd = np.zeros((1, 4), np.float32)
    assert api.lib.pgv_hnsw_scan_begin(b.h, api.ptr(qd), 1, 4, 0, C.byref(out)) == api.PGV_ERR_ARG
    # a view inherits the property (the host build runs on views)
    ctx2 = api.Context(0)
    view = b.share(ctx2)
    assert api.lib.pgv_hnsw_buildable_sparse(view.h) == dim and view.buildable and not a.buildable
    for x, y in zip(want, view.search(queries, 10, 10)):
        assert np.array_equal(x, y)
    ids, dist, cnt = build_search(view, [0, 5], [0, 0], 8, 1)
    assert cnt.tolist() == [8, 8] and ids[1, 0] == 5
    for i, e in enumerate((0, 5)):
        assert bits(dist[i]) == bits(b.score_pairs(ids[i], np.full(8, e, np.int32)))
    view.close()
    ctx2.close()
    a.close()
    b.close()


def test_what_does_not_build_says_so(ctx, small_case):
    """_host.hnsw_build with CSR rows on a plain sparse mirror, a dense mirror, a bit mirror and a buildable mirror of
    another dim or n: PGV_ERR_ARG naming the new upload entry, and no graph is set.  The new upload entry rejects what
    pgv_hnsw_upload_sparse rejects."""
    dim, rows, queries, graph, _ = small_case
    n = count(rows)
    dense = api.Hnsw(ctx, L2, api.PGV_F32, 16, np.zeros((n, 16), np.float32))
    bitm = api.BitHnsw(ctx, 64, np.zeros((n, 8), np.uint8), buildable=True)
    shorter = buildable(ctx, L2, dim, shm.take(rows, range(n - 1)))
    for h, d in ((plain(ctx, L2, dim, rows), dim), (dense, dim), (bitm, dim), (buildable(ctx, L2, dim + 1, rows), dim),
                 (shorter, dim)):
        with pytest.raises(api.PgvError) as e:
            _host.hnsw_build(h, None, 4, 8, api.make_rng(seed=1), max_batch=1, rows_csr=rows, dim=d)
        assert e.value.code == api.PGV_ERR_ARG and ENTRY in e.value.message, e.value.message
        with pytest.raises(api.PgvError):      # no graph was set on the way
            if h is dense:
                h.search(np.zeros((1, 16), np.float32), 5, 5)
            elif h is bitm:
                h.search(np.zeros((1, 8), np.uint8), 5, 5)
            else:
                h.search(queries, 5, 5)
        h.close()
    # the plain mirror keeps refusing the build-side entries, with the text it always had
    sp = plain(ctx, L2, dim, rows, graph)
    i32, f32, i64 = np.zeros(64, np.int32), np.zeros(64, np.float32), np.zeros(8, np.int64)
    assert api.lib.pgv_hnsw_build_search(sp.h, api.ptr(i32), api.ptr(i32), 2, 8, 1, api.ptr(i32), api.ptr(f32),
                                         api.ptr(i32)) == api.PGV_ERR_ARG
    assert "a sparse mirror (pgv_hnsw_upload_sparse) is searched and scored, not built on" in api.lib.pgv_last_error().decode()
    sp.close()
    # what pgv_hnsw_upload_sparse rejects
    too_long = shm.rand_csr([3, 1001], 5, dim=dim)
    with pytest.raises(api.PgvError) as e:
        buildable(ctx, L2, dim, too_long)
    assert e.value.code == _lib.PGV_ERR_DIMS and "element 1 has 1001 stored elements" in e.value.message
    assert "sparsevec cannot have more than 1000 non-zero elements for hnsw index" in e.value.message
    for bad_dim in (0, 10 ** 9 + 1):
        with pytest.raises(api.PgvError):
            buildable(ctx, L2, bad_dim, rows)
    with pytest.raises(api.PgvError):
        buildable(ctx, 7, dim, rows)
    unsorted = (np.array([0, 2], np.int64), np.array([5, 3], np.int32), np.ones(2, np.float32))
    with pytest.raises(api.PgvError):
        buildable(ctx, L2, dim, unsorted)
    out = C.c_void_p()
    assert api.lib.pgv_hnsw_upload_sparse_buildable(None, L2, 8, None, None, None, 0, None, 0, C.byref(out)) == api.PGV_ERR_ARG
    assert api.lib.pgv_hnsw_upload_sparse_buildable(ctx.h, L2, 8, None, None, None, 2, None, 0, C.byref(out)) == api.PGV_ERR_ARG


# ------------------------------------------------------------------------------------------- 2. pgv_hnsw_score_groups
@pytest.fixture(scope="module")
def groups_here(ctx):
    return wk.groups_on_device(ctx)


@pytest.fixture(scope="module")
def groups_by_gather(tmp_path_factory):
    """the same cases with PGV_HNSW_PAIRS_GATHER=1, in a child: the variable is read once per process"""
    out = str(tmp_path_factory.mktemp("groups") / "gather.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mp_sparse_build_worker.py"), "groups", out],
                       env=dict(os.environ, PYTHONPATH=ROOT, PGV_HNSW_PAIRS_GATHER="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and "GROUPS-OK %d" % (len(wk.DATA) * len(wk.METRICS)) in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    return np.load(out)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("data", wk.DATA)
def test_score_groups_on_sparse_rows_is_score_pairs_smaller_slot_first(groups_here, groups_by_gather, data, metric):
    """sparse_groups_kernel's values: pgv_hnsw_score_pairs(min slot, max slot) over the expanded pairs bit for bit, the
    gathered route's in a process of its own, sparse_model's on integer data; both orientations occur in the groups, and on
    float data there are pairs whose two orientations differ in bits -- else the rule would not be under test"""
    ids, ids_start, frm, pair_start, a, b = wk.groups_input()
    key = "%s/%d" % (data, metric)
    got, want, swapped = groups_here["groups/" + key], groups_here["pairs/" + key], groups_here["swapped/" + key]
    assert len(got) == len(a) == int(pair_start[-1]) and len(a) > 5000
    assert (a < b).sum() > 1000 and (a > b).sum() > 1000
    wrong = np.flatnonzero(np.asarray(bits(got)) != np.asarray(bits(want)))
    assert len(wrong) == 0, (len(wrong), wrong[:5].tolist(), a[wrong[:5]].tolist(), b[wrong[:5]].tolist())
    assert bits(groups_by_gather["groups/" + key]) == bits(got)
    differ = int((np.asarray(bits(want)) != np.asarray(bits(swapped))).sum())
    print("%s metric %d: %d of %d pairs differ in bits between the two orientations" % (data, metric, differ, len(a)))
    rows = wk.groups_rows(data)
    if data == "float":
        assert differ > 0
    else:
        model = shm.all_distances(MODEL[metric], rows, rows)      # [query, row]
        assert np.array_equal(got, model[np.maximum(a, b), np.minimum(a, b)])
    # slots 0 and 1 are empty rows: their pair is exactly zero, +0.0 under the inner product
    both_empty = np.flatnonzero((np.minimum(a, b) == 0) & (np.maximum(a, b) == 1))
    assert len(both_empty) >= len(wk.GROUP_SIZES) - 1 and all(x == 0 for x in bits(got[both_empty]))


# ---------------------------------------------------------------------------------- 3. pgv_hnsw_build_search on sparse
def leveled_graph(oracle, rows, dim, metric, m, extra=0):
    """the oracle's build over the dense expansion (any graph serves: the walk is under test), `extra` more elements appended
    at level 0 with empty tuples that nothing points to -> (elements in slot order, graph)"""
    g = po.HnswGraph(oracle, OPS[metric], po.ORA_F32, shm.expand_dense(rows, dim), m=m, ef_construction=24, seed=7)
    ex = g.export_tuples()
    g.close()
    levels = np.concatenate([ex["levels"], np.zeros(extra, np.int32)])
    nbr_start = np.zeros(len(levels) + 1, np.int64)
    nbr_start[1:] = np.cumsum((levels.astype(np.int64) + 2) * m)
    nbr = np.full(int(nbr_start[-1]), -1, np.int32)
    nbr[:len(ex["nbr"])] = ex["nbr"]
    assert int(levels.max()) >= 2, "three layers wanted"
    return ex["rows"], (m, int(ex["entry"]), levels, nbr_start, nbr)


def tie_free_elements(nq, n, dim, seed):
    """sparse_hnsw_model.tie_free's rejection loop with queries that can be ELEMENTS (its own store ~1500 elements, over
    HNSW_MAX_NNZ): nq query rows of 700 .. 1000 stored integers and n rows whose distances from every query are all
    distinct under each of the three metrics"""
    rng = np.random.default_rng(seed)
    queries = shm.rand_csr(rng.integers(700, 1001, nq), seed + 1, dim=dim)
    Q = shm.expand_dense(queries, dim).astype(np.int64)
    seen = {mt: [set() for _ in range(nq)] for mt in shm.METRICS}
    kept, trip = [], 0
    while len(kept) < n:
        trip += 1
        batch = shm.rand_csr(rng.integers(1, shm.HNSW_MAX_NNZ + 1, 32), seed + 1000 + trip, dim=dim)
        d = shm._dense_int_distances(Q, shm.expand_dense(batch, dim).astype(np.int64))
        for j in range(32):
            if len(kept) < n and not any(int(d[mt][q, j]) in seen[mt][q] for mt in shm.METRICS for q in range(nq)):
                for mt in shm.METRICS:
                    for q in range(nq):
                        seen[mt][q].add(int(d[mt][q, j]))
                kept.append(sm.vector(batch, j))
    return queries, sm.csr(kept)


def check_build_search(h, keys_of, graph, elems, qlevels, efc, lcap, what):
    """keys_of(e): the float32 distances of every element as a row to element e as the query"""
    m, entry, levels, nbr_start, nbr = graph
    ids, dist, cnt = build_search(h, elems, qlevels, efc, lcap)
    searched = 0
    for i, (e, ql) in enumerate(zip(elems, qlevels)):
        floats = keys_of(int(e))
        keys = floats.tolist()
        w = wm.walk(keys.__getitem__, levels, nbr_start, nbr, m, entry, efc, qlevel=int(ql))
        for lc in range(lcap):
            g = i * lcap + lc
            if lc not in w.layers:
                assert cnt[g] == 0, (what, e, lc)
                continue
            wi, wkeys = w.layers[lc]
            searched += 1
            assert cnt[g] == len(wi) and ids[g, :cnt[g]].tolist() == wi, (what, e, ql, lc)
            assert np.array_equal(dist[g, :cnt[g]], floats[wi]), (what, e, ql, lc)
            assert wkeys == sorted(wkeys)
    return searched, ids, dist, cnt


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("data", ["tied", "tie_free", "float"])
def test_build_search_on_sparse_rows_returns_every_layers_w(ctx, oracle, metric, data):
    """element slots as queries, insert levels below, at and above the entry's, layer_cap at and below the layers present:
    ids, counts and distances of every searched layer against hnsw_walk_model.walk(..., qlevel).layers over sparse_model's
    values (integer data) and over pgv_hnsw_score_pairs(candidate, element) (float data: bit for bit)"""
    m, efc = 4, 12
    if data == "tied":
        dim, n = 1536, 300
        _, base = shm.tied(4, n, dim, 13)
        order, graph = leveled_graph(oracle, base, dim, metric, m)
        elements, elems = shm.take(base, order), np.arange(0, len(order), 7)
    elif data == "tie_free":
        dim, n = 2000, 200
        queries, base = tie_free_elements(4, n, dim, 5)
        order, graph = leveled_graph(oracle, base, dim, metric, m, extra=4)
        elements = sm.csr([sm.vector(base, int(r)) for r in order] + [sm.vector(queries, q) for q in range(4)])
        elems = np.arange(len(order), len(order) + 4)
    else:
        dim, n = 2000, 300
        base = shm.rand_csr(np.random.default_rng(3).integers(0, 400, n), 303, dim=dim, floats=True)
        order, graph = leveled_graph(oracle, base, dim, metric, m)
        elements, elems = shm.take(base, order), np.arange(0, len(order), 7)
    nel = count(elements)
    top = int(graph[2][graph[1]])
    h = buildable(ctx, metric, dim, elements, graph)
    every = np.arange(nel, dtype=np.int32)
    if data == "float":
        def keys_of(e):
            return h.score_pairs(every, np.full(nel, e, np.int32))
    else:
        def keys_of(e):
            return sm.distances(MODEL[metric], sm.vector(elements, e), elements)[0]
    seen = 0
    for lcap in (top + 1, 2, 1):
        qlevels = np.array([(0, 1, top, top + 1, top - 1)[i % 5] for i in range(len(elems))], np.int32)
        got, ids, dist, cnt = check_build_search(h, keys_of, graph, elems, qlevels, efc, lcap, "%s lcap %d" % (data, lcap))
        seen += got
        # the distances are pgv_hnsw_score_pairs(candidate, element), bit for bit, on every kind of data
        for i, e in enumerate(elems[:6]):
            for lc in range(lcap):
                g = i * lcap + lc
                if cnt[g] > 0:
                    assert bits(dist[g, :cnt[g]]) == bits(h.score_pairs(ids[g, :cnt[g]], np.full(cnt[g], e, np.int32)))
    assert seen >= 3 * len(elems)
    h.close()


# ------------------------------------------------------------------------------- 4. pgv_hnsw_build_neighbors on sparse
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("efc", [12, 80])
def test_build_neighbors_on_sparse_rows_is_the_sweep_over_the_same_lists(ctx, oracle, metric, efc):
    """pgv_hnsw_build_neighbors against hnsw_link_model.host_select over pgv_hnsw_build_search's lists and the ORIENTED
    triangles (pgv_hnsw_score_pairs(min slot, max slot)), on float data: ids, distance bits, closer flags, counts,
    out_pairs.  ef_construction 12 runs hnsw_select_wave_kernel, 80 hnsw_select_kernel"""
    m, dim, n = 4, 2000, 300
    base = shm.rand_csr(np.random.default_rng(4).integers(0, 300, n), 401, dim=dim, floats=True)
    order, graph = leveled_graph(oracle, base, dim, metric, m)
    elements = shm.take(base, order)
    levels = graph[2]
    h = buildable(ctx, metric, dim, elements, graph)
    elems = np.arange(0, len(order), 3).astype(np.int32)
    qlevels = np.ascontiguousarray(levels[elems])
    lcap = int(levels[graph[1]]) + 1
    ids, dist, cnt = build_search(h, elems, qlevels, efc, lcap)
    per = len(elems) * lcap
    oi, od = np.empty((per, 2 * m), np.int32), np.empty((per, 2 * m), np.float32)
    oc, on = np.empty((per, 2 * m), np.uint8), np.empty(per, np.int32)
    pairs = C.c_int64()
    api.check(api.lib.pgv_hnsw_build_neighbors(h.h, api.ptr(elems), api.ptr(qlevels), len(elems), efc, lcap, api.ptr(oi),
                                               api.ptr(od), api.ptr(oc), api.ptr(on), C.byref(pairs)))
    thinned = want_pairs = 0
    for g in range(per):
        q, lc = divmod(g, lcap)
        lmax = 2 * m if lc == 0 else m
        nw = 0 if lc > qlevels[q] else int(cnt[g])
        tri = None
        if nw > lmax:
            thinned += 1
            want_pairs += nw * (nw - 1) // 2
            gi = ids[g, :nw]
            a = np.concatenate([np.full(u, gi[u], np.int32) for u in range(1, nw)])
            b = np.concatenate([gi[:u] for u in range(1, nw)])
            tri = oriented(h, a, b)
        wi, wd, wc = host_select(ids[g, :nw], dist[g, :nw], tri, lmax)
        assert on[g] == len(wi) and oi[g, :on[g]].tolist() == wi, (g, lc, nw)
        assert bits(od[g, :on[g]]) == bits(wd) and oc[g, :on[g]].tolist() == wc, (g, lc, nw)
    assert thinned >= len(elems) and pairs.value == want_pairs
    h.close()


# ------------------------------------------------------------------------------------------------- 5 - 8. whole builds
GRAPH_ARRAYS = ("levels", "nbr_start", "nbr", "dup_of")
GRAPH_SCALARS = ("entry", "batches", "nelements")


def assert_same_graph(a, b, what=""):
    for k in GRAPH_SCALARS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in GRAPH_ARRAYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (what, k))


def integer_rows(n, dim, seed, metric):
    """rows of 1 .. 48 stored integers in -8 .. 8; 40 copies of one row in a run (eleven heap TIDs meet an element that takes
    ten); under L2 / L1 a few empty rows"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 49, n)
    if metric != IP:
        lengths[[n // 5, n // 3, n - 3]] = 0
    base = shm.rand_csr(lengths, seed + 1, dim=dim)
    pick = np.arange(n)
    pick[n // 2:n // 2 + 40] = 7
    return shm.take(base, pick)


def search_own_graph(h, rows):
    elem, _, _ = h.search(shm.take(rows, range(16)), 40, 5)
    assert (np.asarray(elem)[:, 0] >= 0).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("max_batch,m,n", [(1, 6, 1500), (64, 8, 6000), (512, 8, 4000), (128, 36, 3000)])
def test_a_sparse_build_is_the_dense_build_over_the_expansion(ctx, max_batch, m, n, metric):
    """the native build and pgv_host_hnsw_build over the fp32 expansion of integer-valued rows, same seed: levels, nbr_start,
    nbr, dup_of, entry, batches, nelements (the graph arrays only: a zero inner product may be -0.0 on one side and +0.0 on
    the other, and the walk's keys merge them).  m 36 reaches the one-lane-per-list forms of the selection and the link
    replay.  The mirror then searches its own graph."""
    dim, efc = 256, max(24, 2 * m)
    rows = integer_rows(n, dim, 500 + n, metric)
    h = buildable(ctx, metric, dim, rows)
    native = build(h, rows, m, efc, 9, max_batch)
    search_own_graph(h, rows)
    h.close()
    twin_rows = shm.expand_dense(rows, dim)
    twin = api.Hnsw(ctx, metric, api.PGV_F32, dim, twin_rows)
    dense = _host.hnsw_build(twin, twin_rows, m, efc, api.make_rng(seed=9), max_batch=max_batch)
    twin.close()
    assert_same_graph(native, dense, "max_batch %d m %d metric %d" % (max_batch, m, metric))
    dup = native["dup_of"]
    print("rows that took a heap TID of an earlier element: %d" % int((dup >= 0).sum()))
    assert native["nelements"] + int((dup >= 0).sum()) == n
    # an element takes its own heap TID and nine more (HNSW_HEAPTIDS 10).  How many copies find one is the dense build's
    # figure too (dup_of is compared above): it depends on the lists the selection leaves and on what a batch sees
    assert np.bincount(dup[dup >= 0], minlength=n).max() <= 9
    for r in np.flatnonzero(dup >= 0):
        assert np.array_equal(twin_rows[r], twin_rows[dup[r]]) and dup[dup[r]] < 0


def float_rows(n, dim, seed, nnz=(8, 80)):
    """float rows sharing indices in plenty (so that hits and misses of both sides mix in a pair), four copies of one row"""
    rng = np.random.default_rng(seed)
    base = shm.rand_csr(rng.integers(nnz[0], nnz[1] + 1, n), seed + 1, dim=dim, floats=True)
    pick = np.arange(n)
    pick[[n // 3, n // 3 + 1, n - 9, n - 8]] = 4
    return shm.take(base, pick)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("max_batch", [1, 256])
def test_the_three_forms_of_a_sparse_build_agree(ctx, metric, max_batch):
    """float data; the default (graph updates on the device), PGV_HNSW_HOST_LINK=1 and PGV_HNSW_HOST_SELECT=1: one graph.
    The three take the distances of one pair from different places (the search's lists, the device's triangles, the
    host's requests): this is the test the orientation rule exists for"""
    n, dim, m, efc = (800, 300, 6, 24) if max_batch == 1 else (4000, 300, 8, 32)
    rows = float_rows(n, dim, 600 + max_batch)
    graphs = []
    for env in ({}, {"PGV_HNSW_HOST_LINK": "1"}, {"PGV_HNSW_HOST_SELECT": "1"}):
        os.environ.update(env)
        try:
            h = buildable(ctx, metric, dim, rows)
            graphs.append(build(h, rows, m, efc, 9, max_batch))
            search_own_graph(h, rows)
            h.close()
        finally:
            for k in env:
                os.environ.pop(k, None)
    for b, name in zip(graphs[1:], ("host link", "host select")):
        assert_same_graph(graphs[0], b, name)
    dup = graphs[0]["dup_of"]
    same = sbm.same_bytes(rows)
    for r in np.flatnonzero(dup >= 0):
        assert same(int(r), int(dup[r])) and dup[dup[r]] < 0


@pytest.mark.parametrize("metric", METRICS)
def test_a_serial_float_build_is_the_model(ctx, metric):
    """max_batch 1, n 400, about 40 stored floats a row over 10^6 dimensions (drawn from 600 of them, so that rows meet), m 4,
    ef_construction 12, levels from the build's output: nbr, dup_of, entry and nelements of tests/bit_build_model.py fed key,
    value and pair from pgv_hnsw_score_pairs under the rule and `same` from the CSR bytes"""
    n, dim, m, efc = 400, 10 ** 6, 4, 12
    rng = np.random.default_rng(70)
    pool = np.unique(np.concatenate([[0, dim - 1], rng.integers(0, dim, 600)])).astype(np.int32)
    base = shm.rand_csr(rng.integers(30, 51, n), 701, pool=pool, floats=True)
    pick = np.arange(n)
    pick[[n // 3, n // 3 + 1, n - 9]] = 4
    rows = shm.take(base, pick)
    h = buildable(ctx, metric, dim, rows)
    built = build(h, rows, m, efc, 3, 1)
    D = sbm.oriented_matrix(h.score_pairs, n)
    a, b = np.triu_indices(n, 1)
    swapped = h.score_pairs(b.astype(np.int32), a.astype(np.int32))
    h.close()
    print("pairs whose two orientations differ in bits: %d of %d" % (int((np.asarray(bits(D[a, b])) != np.asarray(bits(swapped))).sum()), len(a)))
    assert int(built["levels"].max()) >= 2
    want = bm.build(built["levels"], m, efc, *sbm.functions(D, rows))
    assert want["mismatches"] == 0
    assert built["entry"] == want["entry"] and built["nelements"] == want["nelements"]
    np.testing.assert_array_equal(built["dup_of"], want["dup_of"])
    np.testing.assert_array_equal(built["nbr"], want["nbr"])
    print("rows that took a heap TID of an earlier element: %d" % int((built["dup_of"] >= 0).sum()))


def sparse_recall(ctx, metric, dim, rows, built, m, queries, ef, k):
    """recall@k of the walk over the built graph against pgv_sparse_topk, by distance: an answer counts when it is no farther
    than the exact k-th"""
    h = plain(ctx, metric, dim, rows, (m, built["entry"], built["levels"], built["nbr_start"], built["nbr"]))
    _, dist, _ = h.search(queries, ef, k)
    h.close()
    exact, _ = api.sparse_topk(ctx, metric, dim, queries, rows, k)
    return float((np.asarray(dist) <= np.asarray(exact)[:, -1:]).sum()) / (count(queries) * k)


def test_a_batched_sparse_build_searches_as_well_as_the_serial_one(ctx):
    """n 6000 float rows, max_batch 256 against max_batch 1 over the same rows: recall@10 at ef 40 against pgv_sparse_topk
    within 0.03 (the margin the project gives batched against serial builds), and the structural invariants of
    test_a_batched_jaccard_build_searches_as_well_as_the_serial_one"""
    n, dim, m, efc, metric = 6000, 2000, 8, 40, L2
    rows, queries = float_rows(n, dim, 800, nnz=(20, 60)), float_rows(64, dim, 801, nnz=(20, 60))
    graphs = {}
    for max_batch in (256, 1):
        h = buildable(ctx, metric, dim, rows)
        graphs[max_batch] = build(h, rows, m, efc, 5, max_batch)
        h.close()
    b = graphs[256]
    assert b["nelements"] + int((b["dup_of"] >= 0).sum()) == n and b["batches"] < n / 4
    lv, st, nb = b["levels"], b["nbr_start"], b["nbr"]
    for e in range(0, n, 37):
        for lc in range(lv[e] + 1):
            o = st[e] + (lv[e] - lc) * m
            ids = nb[o:o + (2 * m if lc == 0 else m)]
            ids = ids[ids >= 0]
            assert len(set(ids.tolist())) == len(ids) and e not in ids
            assert (lv[ids] >= lc).all() and (b["dup_of"][ids] < 0).all()
    got, want = (sparse_recall(ctx, metric, dim, rows, graphs[mb], m, queries, 40, 10) for mb in (256, 1))
    print("recall@10 at ef 40: batched %.4f serial %.4f" % (got, want))
    assert got >= want - 0.03, (got, want)
