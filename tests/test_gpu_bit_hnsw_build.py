"""Building HNSW graphs over bit strings on the device: pgv_hnsw_upload_bits_buildable, the <BitRow, 0> / <BitRow, 1> forms
of score_groups_kernel, the build form of hnsw_search_kernel on bit rows, pgv_host_hnsw_build_bits.

The yardsticks.  Hamming: the Hamming distance of two bit strings is the squared L2 distance of their 0/1 expansions, exact
in fp32 in any order, so the dense build over the expansion -- pinned to the oracle by
test_hnsw_build_serial_is_the_reference_loop -- must give the native build's graph array for array.  Jaccard: there is no
dense twin and the oracle has no Jaccard build; tests/bit_build_model.py (pinned on the CPU by
tests/test_bit_build_model_cpu.py) is the reference's serial loop over exact ratios for the search and
jaccard_model.ref_float for every list.  Everything is compared by equality, distances by their bits.

Smallest shapes at which each kernel can go wrong:
  score_groups   nbits 1 (one vector, one lane), 8, 100, 128 (exactly one vector), 129 (a nearly empty second vector), 1536
                 (12 vectors on 16 lanes: the clamped last chunk), 64 000 (500 vectors, 8 trips of 64 lanes); groups of 1, 2
                 (one pair), 4, 5 (a second, ragged u-block), 9, 33 (more tiles than one round of workers at 64 lanes a row)
  build search   a few hundred elements in >= 3 layers, ef_construction 12; insert levels above, at and below the entry's,
                 layer_cap below the layers present
  select         ef_construction 12 (hnsw_select_wave_kernel) and 80 (hnsw_select_kernel), lists longer than lm
  whole build    the issue's shapes"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bit_build_model as bm
import bit_hnsw_model as bhm
import hnsw_walk_model as wm
import jaccard_model as jm
import mp_bit_build_worker as wk
from bit_model import hamming
from hnsw_link_model import host_select
from oracle import pyoracle as po
from pgvector_amd import _host, _lib, api

pytestmark = pytest.mark.gpu

HAMMING, JACCARD = api.PGV_BIT_HAMMING, api.PGV_BIT_JACCARD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).tolist()


def buildable(ctx, metric, nbits, rows, graph=None, payload=None):
    h = api.BitHnsw(ctx, nbits, rows, payload=payload, metric=metric, buildable=True)
    if graph is not None:
        h.set_graph(*graph)
    return h


def plain(ctx, metric, nbits, rows, graph=None, payload=None):
    h = api.JaccardHnsw(ctx, nbits, rows, payload=payload) if metric == JACCARD else api.BitHnsw(ctx, nbits, rows, payload=payload)
    if graph is not None:
        h.set_graph(*graph)
    return h


def floats_to(metric, query, rows):
    """the floats the device hands back for `query` against `rows`"""
    return jm.ref_floats(query, rows) if metric == JACCARD else hamming(query, rows).astype(np.float32)


def keys_to(metric, query, rows):
    """what the walk ranks by: exact"""
    return jm.fractions_of(query, rows) if metric == JACCARD else hamming(query, rows).tolist()


def build_search(h, elems, qlevels, efc, lcap):
    elems, qlevels = np.ascontiguousarray(elems, np.int32), np.ascontiguousarray(qlevels, np.int32)
    per = len(elems) * lcap
    ids, dist, cnt = np.full((per, efc), -7, np.int32), np.full((per, efc), np.nan, np.float32), np.full(per, -7, np.int32)
    api.check(api.lib.pgv_hnsw_build_search(h.h, api.ptr(elems), api.ptr(qlevels), len(elems), efc, lcap, api.ptr(ids),
                                            api.ptr(dist), api.ptr(cnt)))
    return ids, dist, cnt


# ---------------------------------------------------------------------------------------------------------- 1. gates
@pytest.fixture(scope="module")
def small_case():
    nbits, m = 200, 8
    n, entry, levels, nbr_start, nbr = bhm.complete_graph(m)
    rows, queries = bhm.rand_bits(n, nbits, 71), bhm.rand_bits(5, nbits, 72)
    payload = (np.arange(n, dtype=np.uint32)[:, None] * 31 + np.arange(3, dtype=np.uint32)[None, :]).astype(np.uint32)
    return nbits, rows, queries, (m, entry, levels, nbr_start, nbr), payload


@pytest.mark.parametrize("metric", [HAMMING, JACCARD])
def test_a_buildable_mirror_answers_as_the_plain_mirror_does(ctx, small_case, metric, tmp_path):
    """search, scan, score, score_pairs, payload, share and export -> import: the plain mirror's answers over the same rows
    and graph.  The view builds; the importer does not, and says `bit mirror` like any other."""
    nbits, rows, queries, graph, payload = small_case
    a, b = plain(ctx, metric, nbits, rows, graph, payload), buildable(ctx, metric, nbits, rows, graph, payload)
    assert api.lib.pgv_hnsw_buildable_bits(a.h) == 0 and api.lib.pgv_hnsw_buildable_bits(b.h) == nbits
    assert api.lib.pgv_hnsw_buildable_bits(None) == 0
    want = a.search(queries, 10, 10)
    for x, y in zip(want, b.search(queries, 10, 10)):
        assert np.array_equal(x, y)
    with a.scan(queries, 4) as s, b.scan(queries, 4) as t:
        for _ in range(3):
            for x, y in zip(s.next(), t.next()):
                assert np.array_equal(x, y)
    slot = np.arange(len(rows), dtype=np.int32)
    assert bits(a.score(queries[:1], slot)) == bits(b.score(queries[:1], slot)) == bits(floats_to(metric, queries[0], rows))
    assert bits(a.score_pairs(slot, slot[::-1])) == bits(b.score_pairs(slot, slot[::-1]))
    assert np.array_equal(b.get_payload(np.array([3, -1])), a.get_payload(np.array([3, -1])))
    # a view inherits the property (the host build runs on views)
    ctx2 = api.Context(0)
    view = b.share(ctx2)
    assert api.lib.pgv_hnsw_buildable_bits(view.h) == nbits and view.buildable
    for x, y in zip(want, view.search(queries, 10, 10)):
        assert np.array_equal(x, y)
    ids, dist, cnt = build_search(view, [0, 5], [0, 0], 8, 1)
    assert cnt.tolist() == [8, 8] and ids[0, 0] == 0 and ids[1, 0] == 5
    view.close()
    ctx2.close()
    # an importer of its export answers the same searches and builds nothing
    job, res = str(tmp_path / "job.npz"), str(tmp_path / "res.npz")
    np.savez(job, handle=np.frombuffer(b.export(), dtype=np.uint8), queries=queries, ef=10, k=10)
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mp_bit_build_worker.py"), "import", job, res], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(res)
    assert np.array_equal(out["elem"], want[0]) and bits(out["dist"]) == bits(want[1]) and np.array_equal(out["scored"], want[2])
    assert out["codes"].tolist() == [api.PGV_ERR_ARG] * 4 and int(out["buildable"]) == 0
    assert "bit mirror" in out["text"].tobytes().decode()
    a.close()
    b.close()


def test_what_does_not_build_says_so(ctx, small_case):
    """pgv_host_hnsw_build_bits on a plain bit mirror of either metric, on a buildable mirror of another nbits and on a
    dense mirror: PGV_ERR_ARG before any launch (no graph is set).  A sparse mirror keeps rejecting the build-side entries.
    The new upload entry checks what pgv_hnsw_upload_bits checks."""
    nbits, rows, queries, graph, _ = small_case
    dense = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, nbits, bhm.expand01(rows, nbits))
    dense.nbits = nbits
    for h in (plain(ctx, HAMMING, nbits, rows), plain(ctx, JACCARD, nbits, rows), buildable(ctx, HAMMING, 193, rows), dense):
        h.nbits = nbits
        with pytest.raises(api.PgvError) as e:
            _host.hnsw_build(h, rows, 4, 8, api.make_rng(seed=1), max_batch=1)
        assert e.value.code == api.PGV_ERR_ARG and "pgv_hnsw_upload_bits_buildable" in e.value.message
        with pytest.raises(api.PgvError):      # no graph was set on the way
            h.search(queries, 5, 5) if h is not dense else h.search(bhm.expand01(queries, nbits), 5, 5)
        h.close()
    sp = api.SparseHnsw(ctx, api.PGV_L2SQ, 16, (np.array([0, 1, 2], np.int64), np.array([1, 2], np.int32), np.ones(2, np.float32)))
    sp.set_graph(2, 0, np.zeros(2, np.int32), np.array([0, 4, 8], np.int64), np.full(8, -1, np.int32))
    i32, f32, i64 = np.zeros(64, np.int32), np.zeros(64, np.float32), np.zeros(8, np.int64)
    assert api.lib.pgv_hnsw_buildable_bits(sp.h) == 0
    assert api.lib.pgv_hnsw_build_search(sp.h, api.ptr(i32), api.ptr(i32), 2, 8, 1, api.ptr(i32), api.ptr(f32),
                                         api.ptr(i32)) == api.PGV_ERR_ARG
    assert "sparse mirror" in api.lib.pgv_last_error().decode()
    assert api.lib.pgv_hnsw_score_groups(sp.h, api.ptr(i32), api.ptr(i64), api.ptr(i32), api.ptr(i64), 1, 2, 1,
                                         api.ptr(f32)) == api.PGV_ERR_ARG
    sp.close()
    for bad in (0, 64001, -1):
        with pytest.raises(api.PgvError) as e:
            buildable(ctx, HAMMING, bad, np.zeros((2, max((bad + 7) // 8, 1)), dtype=np.uint8))
        assert e.value.code == _lib.PGV_ERR_DIMS, bad
    with pytest.raises(api.PgvError) as e:
        buildable(ctx, 2, nbits, rows)
    assert e.value.code == api.PGV_ERR_ARG
    out = C.c_void_p()
    assert api.lib.pgv_hnsw_upload_bits_buildable(None, HAMMING, 8, None, 0, None, 0, C.byref(out)) == api.PGV_ERR_ARG
    assert api.lib.pgv_hnsw_upload_bits_buildable(ctx.h, JACCARD, 8, None, 2, None, 0, C.byref(out)) == api.PGV_ERR_ARG


# ------------------------------------------------------------------------------------------- 2. pgv_hnsw_score_groups
@pytest.fixture(scope="module")
def groups_here(ctx):
    return wk.groups_on_device(ctx)


@pytest.fixture(scope="module")
def groups_by_gather(tmp_path_factory):
    """the same cases with PGV_HNSW_PAIRS_GATHER=1, in a child: the variable is read once per process"""
    out = str(tmp_path_factory.mktemp("groups") / "gather.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mp_bit_build_worker.py"), "groups", out],
                       env=dict(os.environ, PYTHONPATH=ROOT, PGV_HNSW_PAIRS_GATHER="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and "GROUPS-OK %d" % (2 * len(wk.GROUP_NBITS)) in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    return np.load(out)


@pytest.mark.parametrize("nbits", wk.GROUP_NBITS)
@pytest.mark.parametrize("metric", [HAMMING, JACCARD])
def test_score_groups_on_bits_is_score_pairs_and_the_model(groups_here, groups_by_gather, metric, nbits):
    """the 4 x 4 tiles' values: pgv_hnsw_score_pairs' over the expanded pairs bit for bit, bit_model.hamming /
    jaccard_model.ref_floats, and the gathered route's in a process of its own; slots of groups that want no pairs untouched"""
    ids, ids_start, frm, pair_start, a, b = wk.groups_input()
    rows = wk.groups_rows(nbits)
    got = groups_here["groups/%d/%d" % (metric, nbits)]
    want = np.array([floats_to(metric, rows[y], rows[x:x + 1])[0] for x, y in zip(a, b)], dtype=np.float32)
    assert len(got) == len(a) == int(pair_start[-1]) and len(a) > 1500
    assert bits(got) == bits(groups_here["pairs/%d/%d" % (metric, nbits)]), np.argwhere(got != want)[:5].tolist()
    assert bits(got) == bits(want), np.argwhere(got != want)[:5].tolist()
    assert bits(groups_by_gather["groups/%d/%d" % (metric, nbits)]) == bits(got)
    # group 0 of size 2 is the pair of all-zero rows; of size 4 rows 0 .. 3: (2, 3) are identical; size 9: (4, 5) disjoint
    at = {n: int(pair_start[6 * k]) for k, n in enumerate(wk.GROUP_SIZES)}
    zero, same, disjoint = got[at[2]], got[at[4] + 3 * 2 // 2 + 2], got[at[9] + 5 * 4 // 2 + 4]
    if metric == JACCARD:
        assert zero == 1.0 and disjoint == 1.0 and (same == 0.0 or not rows[2].any())
    else:
        assert zero == 0.0 and same == 0.0 and disjoint == nbits


# ------------------------------------------------------------------------------------ 3. pgv_hnsw_build_search on bits
def leveled_graph(oracle, rows, nbits, m, extra=0):
    """the oracle's build over the 0/1 expansion (any graph serves: the walk is under test), `extra` more elements appended
    at level 0 with empty tuples that nothing points to -> (elements, graph)"""
    g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, bhm.expand01(rows, nbits), m=m, ef_construction=24, seed=7)
    ex = g.export_tuples()
    g.close()
    levels = np.concatenate([ex["levels"], np.zeros(extra, np.int32)])
    nbr_start = np.zeros(len(levels) + 1, np.int64)
    nbr_start[1:] = np.cumsum((levels.astype(np.int64) + 2) * m)
    nbr = np.full(int(nbr_start[-1]), -1, np.int32)
    nbr[:len(ex["nbr"])] = ex["nbr"]
    assert int(levels.max()) >= 2, "three layers wanted"
    return ex["rows"], (m, int(ex["entry"]), levels, nbr_start, nbr)


def check_build_search(h, metric, elements, graph, elems, qlevels, efc, lcap, what):
    m, entry, levels, nbr_start, nbr = graph
    ids, dist, cnt = build_search(h, elems, qlevels, efc, lcap)
    searched = 0
    for i, (e, ql) in enumerate(zip(elems, qlevels)):
        keys, floats = keys_to(metric, elements[e], elements), floats_to(metric, elements[e], elements)
        w = wm.walk(keys.__getitem__, levels, nbr_start, nbr, m, entry, efc, qlevel=int(ql))
        for lc in range(lcap):
            g = i * lcap + lc
            if lc not in w.layers:
                assert cnt[g] == 0, (what, e, lc)
                continue
            wi, wkeys = w.layers[lc]
            searched += 1
            assert cnt[g] == len(wi) and ids[g, :cnt[g]].tolist() == wi, (what, e, ql, lc)
            assert bits(dist[g, :cnt[g]]) == bits(floats[wi]), (what, e, ql, lc)
            assert wkeys == sorted(wkeys)
    return searched


@pytest.mark.parametrize("metric", [HAMMING, JACCARD])
@pytest.mark.parametrize("data", ["tied", "tie_free"])
def test_build_search_on_bits_returns_every_layers_w(ctx, oracle, metric, data):
    """element slots as queries, insert levels below, at and above the entry's, layer_cap at and below the layers present:
    ids, counts and distance bits of every searched layer against hnsw_walk_model.walk(..., qlevel).layers"""
    m, efc = 4, 12
    if data == "tied":
        nbits, n = 16, 300
        base = bhm.rand_bits(n, nbits, 301)
        order, graph = leveled_graph(oracle, base, nbits, m)
        elements, elems = np.ascontiguousarray(base[order]), np.arange(0, len(order), 7)
    else:
        nbits, n = 4000, 200     # (room for 200 different distances from each of four queries)
        queries, base = (jm.tie_free if metric == JACCARD else bhm.tie_free)(4, n, nbits, 5)
        order, graph = leveled_graph(oracle, base, nbits, m, extra=4)
        elements, elems = np.ascontiguousarray(np.concatenate([base[order], queries])), np.arange(len(order), len(order) + 4)
    top = int(graph[2][graph[1]])
    h = buildable(ctx, metric, nbits, elements, graph)
    seen = 0
    for lcap in (top + 1, 2, 1):
        qlevels = np.array([(0, 1, top, top + 1, top - 1)[i % 5] for i in range(len(elems))], np.int32)
        seen += check_build_search(h, metric, elements, graph, elems, qlevels, efc, lcap, "%s lcap %d" % (data, lcap))
    assert seen >= 3 * len(elems)
    h.close()


def merged_pairs(count):
    """Farey neighbours p < q, ratios in [1 / 2, 9 / 10), that one float stands for, each pair wholly beyond the one before"""
    from fractions import Fraction
    found = sorted((pr for pr in jm.farey_pairs(lo=63900, least=Fraction(1, 2))
                    if jm.fp32_key(*pr[0]) == jm.fp32_key(*pr[1]) and jm.fraction(*pr[1]) < Fraction(9, 10)),
                   key=lambda pr: jm.fraction(*pr[0]))
    out = []
    for p, q in found:
        if not out or jm.ref_float(*p) > jm.ref_float(*out[-1][1]):
            out.append((p, q))
    assert len(out) >= count
    return out[:count]


def test_build_search_keeps_planted_neighbours_in_the_float8s_order(ctx):
    """64 000 bits: elements 1 .. 12 are six pairs at neighbouring ratios from element 13 that one fp32 value stands for, the
    farther of each pair first in the entry's tuple.  W is the Fractions' order -- an fp32 key would leave each pair in
    batch order -- and lw_dist are the floats, equal inside each pair"""
    pairs = merged_pairs(6)
    xu = [(63000, 64000)] + [x for p, q in pairs for x in (q, p)]
    rows = np.stack([jm.planted_row(x, u) for x, u in xu] + [jm.planted_query()[0]])
    m, n = 8, len(xu) + 1
    levels, nbr_start, nbr = wm.tuples(m, [0] * n, {(0, 0): list(range(1, 13))})
    graph = (m, 0, levels, nbr_start, nbr)
    h = buildable(ctx, JACCARD, jm.PLANT_BITS, rows, graph)
    ids, dist, cnt = build_search(h, [n - 1], [0], 16, 1)
    want = [e for k in range(6) for e in (2 + 2 * k, 1 + 2 * k)] + [0]
    assert cnt[0] == 13 and ids[0, :13].tolist() == want
    assert check_build_search(h, JACCARD, rows, graph, [n - 1], [0], 16, 1, "planted") == 1
    d = dist[0, :12].reshape(6, 2)
    assert (d[:, 0] == d[:, 1]).all() and (np.diff(d[:, 0]) > 0).all()
    by_float = sorted(range(13), key=lambda e: float(jm.ref_float(*xu[e])))      # stable: ties stay in id order
    assert by_float != want
    h.close()


# --------------------------------------------------------------------------------- 4. pgv_hnsw_build_neighbors on bits
@pytest.mark.parametrize("metric", [HAMMING, JACCARD])
@pytest.mark.parametrize("efc", [12, 80])
def test_build_neighbors_on_bits_is_the_sweep_over_the_same_lists(ctx, oracle, metric, efc):
    """pgv_hnsw_build_neighbors against hnsw_link_model.host_select over pgv_hnsw_build_search's lists and
    pgv_hnsw_score_pairs' triangles: ids, distance bits, closer flags, counts, out_pairs.  ef_construction 12 runs
    hnsw_select_wave_kernel, 80 hnsw_select_kernel; nbits 24 gives equal distances in plenty, Jaccard floats included"""
    m, nbits, n = 4, 24, 300
    base = bhm.rand_bits(n, nbits, 401)
    order, graph = leveled_graph(oracle, base, nbits, m)
    elements = np.ascontiguousarray(base[order])
    levels = graph[2]
    h = buildable(ctx, metric, nbits, elements, graph)
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
            tri = h.score_pairs(a, b)
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


@pytest.mark.parametrize("max_batch,m,nbits,n", [(1, 6, 100, 1500), (64, 8, 129, 6000), (512, 8, 1536, 4000), (128, 36, 256, 3000)])
def test_a_hamming_build_is_the_dense_build_over_the_expansion(ctx, max_batch, m, nbits, n):
    """the native build and pgv_host_hnsw_build over the fp32 0/1 expansion, same seed: levels, nbr_start, nbr, dup_of,
    entry, batches, nelements.  40 copies of one row: eleven heap TIDs fit an element.  m 36 reaches the one-lane-per-list
    forms of the selection and the link replay.  The mirror then searches its own graph."""
    efc = max(24, 2 * m)
    rows = bhm.rand_bits(n, nbits, 500 + nbits)
    rows[n // 2:n // 2 + 40] = rows[7]
    h = buildable(ctx, HAMMING, nbits, rows)
    native = _host.hnsw_build(h, rows, m, efc, api.make_rng(seed=9), max_batch=max_batch)
    elem, _, _ = h.search(rows[:16], 40, 5)
    assert (elem[:, 0] >= 0).all()
    h.close()
    twin_rows = bhm.expand01(rows, nbits)
    twin = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, nbits, twin_rows)
    dense = _host.hnsw_build(twin, twin_rows, m, efc, api.make_rng(seed=9), max_batch=max_batch)
    twin.close()
    assert_same_graph(native, dense, "max_batch %d m %d" % (max_batch, m))
    dup = native["dup_of"]
    print("rows that took a heap TID of an earlier element: %d" % int((dup >= 0).sum()))
    assert native["nelements"] + int((dup >= 0).sum()) == n
    for r in np.flatnonzero(dup >= 0):
        assert np.array_equal(rows[r], rows[dup[r]]) and dup[dup[r]] < 0


def jaccard_rows(n, nbits, seed):
    """rows of every density with three all-zero rows (at distance 1 from everything, each other included) and four copies
    of one row"""
    rng = np.random.default_rng(seed)
    b = rng.random((n, 8 * ((nbits + 7) // 8))) < rng.uniform(.1, .9, (n, 1))
    b[:, nbits:] = False
    rows = np.packbits(b, axis=1)
    rows[[n // 5, n // 2, n - 3]] = 0
    rows[[n // 3, n // 3 + 1, n - 9, n - 8]] = rows[4]
    return rows


@pytest.mark.parametrize("metric", [HAMMING, JACCARD])
@pytest.mark.parametrize("max_batch", [1, 256])
def test_the_three_forms_of_a_bit_build_agree(ctx, metric, max_batch):
    """the default (graph updates on the device), PGV_HNSW_HOST_LINK=1 and PGV_HNSW_HOST_SELECT=1: one graph"""
    n, nbits, m, efc = (1200, 128, 6, 24) if max_batch == 1 else (6000, 128, 8, 32)
    rows = jaccard_rows(n, nbits, 600 + max_batch)
    graphs = []
    for env in ({}, {"PGV_HNSW_HOST_LINK": "1"}, {"PGV_HNSW_HOST_SELECT": "1"}):
        os.environ.update(env)
        try:
            h = buildable(ctx, metric, nbits, rows)
            graphs.append(_host.hnsw_build(h, rows, m, efc, api.make_rng(seed=9), max_batch=max_batch))
            elem, _, _ = h.search(rows[:16], 40, 5)
            assert (elem[:, 0] >= 0).all()
            h.close()
        finally:
            for k in env:
                os.environ.pop(k, None)
    for b, name in zip(graphs[1:], ("host link", "host select")):
        assert_same_graph(graphs[0], b, name)
    dup = graphs[0]["dup_of"]
    for r in np.flatnonzero(dup >= 0):
        assert np.array_equal(rows[r], rows[dup[r]]) and dup[dup[r]] < 0


def test_a_serial_jaccard_build_is_the_model(ctx):
    """max_batch 1, n 400, nbits 96, m 4, ef_construction 12, levels from the build's output: nbr, dup_of and the entry point
    of tests/bit_build_model.py"""
    n, nbits, m, efc = 400, 96, 4, 12
    rows = jaccard_rows(n, nbits, 700)
    h = buildable(ctx, JACCARD, nbits, rows)
    built = _host.hnsw_build(h, rows, m, efc, api.make_rng(seed=3), max_batch=1)
    h.close()
    assert int(built["levels"].max()) >= 2
    want = bm.build(built["levels"], m, efc, *bm.jaccard_functions(rows))
    assert want["mismatches"] == 0
    assert built["entry"] == want["entry"] and built["nelements"] == want["nelements"]
    np.testing.assert_array_equal(built["dup_of"], want["dup_of"])
    np.testing.assert_array_equal(built["nbr"], want["nbr"])


def test_a_serial_jaccard_build_over_planted_rows_is_the_model(ctx):
    """n 40 at 64 000 bits: 38 planted rows, among them twelve pairs at neighbouring ratios from the planted query that one
    float stands for, then the query itself and a copy of it.  The query's lists are thinned (m 8: 38 candidates for 16
    slots) over floats that merge what its search told apart"""
    pairs = merged_pairs(12)
    rng = np.random.default_rng(8)
    xu = [x for p, q in pairs for x in (q, p)]
    while len(xu) < 38:
        u = int(rng.integers(32000, 64001))
        xu.append((int(rng.integers(u - 32000, u + 1)), u))
    order = rng.permutation(38)
    rows = np.stack([jm.planted_row(*xu[i]) for i in order] + [jm.planted_query()[0], jm.planted_query()[0]])
    n, m, efc = len(rows), 8, 40
    h = buildable(ctx, JACCARD, jm.PLANT_BITS, rows)
    built = _host.hnsw_build(h, rows, m, efc, api.make_rng(seed=5), max_batch=1)
    h.close()
    want = bm.build(built["levels"], m, efc, *bm.jaccard_functions(rows))
    assert built["entry"] == want["entry"] and built["nelements"] == want["nelements"] == n - 1
    np.testing.assert_array_equal(built["dup_of"], want["dup_of"])
    np.testing.assert_array_equal(built["nbr"], want["nbr"])
    assert built["dup_of"][n - 1] == n - 2


def jaccard_recall(ctx, rows, nbits, built, m, queries, ef, k):
    """recall@k of the walk against the exact Jaccard top-k, ties of the k-th ratio counting as answers"""
    h = plain(ctx, JACCARD, nbits, rows, (m, built["entry"], built["levels"], built["nbr_start"], built["nbr"]))
    elem, _, _ = h.search(queries, ef, k)
    h.close()
    hits = 0
    for q, e in zip(queries, elem):
        x, u = jm.counts(q, rows)
        x, u = np.where(u > x, x, 1), np.where(u > x, u, 1)       # no common bit (u = 0 included): 1 / 1
        # (ratios of denominators <= 256 differ by more than 1e-5: their doubles order exactly as they do)
        kth = int(np.argsort(x / u, kind="stable")[k - 1])
        e = e[e >= 0]
        hits += int((x[e] * u[kth] <= x[kth] * u[e]).sum())
    return hits / (len(queries) * k)


def test_a_batched_jaccard_build_searches_as_well_as_the_serial_one(ctx):
    """n 6000, nbits 256, max_batch 256 against max_batch 1 over the same rows: recall@10 at ef 40 within 0.03 (the margin
    test_hnsw_build_batched_quality gives batched against serial builds), and that test's structural invariants"""
    n, nbits, m, efc = 6000, 256, 8, 40
    rows, queries = jaccard_rows(n, nbits, 800), jaccard_rows(64, nbits, 801)
    graphs = {}
    for max_batch in (256, 1):
        h = buildable(ctx, JACCARD, nbits, rows)
        graphs[max_batch] = _host.hnsw_build(h, rows, m, efc, api.make_rng(seed=5), max_batch=max_batch)
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
    got, want = (jaccard_recall(ctx, rows, nbits, graphs[mb], m, queries, 40, 10) for mb in (256, 1))
    print("recall@10 at ef 40: batched %.4f serial %.4f" % (got, want))
    assert got >= want - 0.03, (got, want)
