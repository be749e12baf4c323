"""HNSW over bit strings under bit_jaccard_ops on the device -- pgv_hnsw_upload_jaccard, the <BitRow, 1> forms of
hnsw_search_kernel (plain and resumable) and of score_gather_kernel, api.JaccardHnsw.  The walk ranks by an integer key of
the ratio x / u (tests/jaccard_model.py) that orders and ties exactly as the reference's float8 does, and hands back the
float32 of that float8: every comparison here is equality -- of elements, of distance bits, of so->tuples.  The
yardsticks are exact: distances as fractions.Fraction fed to the walk's and the scan's host models
(tests/hnsw_walk_model.py, tests/hnsw_scan_model.py), whose fidelity to the reference the existing suite pins.
tests/test_jaccard_model_cpu.py checks the model against the oracle and that an fp32 key would fail the planted cases."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bit_hnsw_model as bhm
import hnsw_tie_cases as tc
import hnsw_walk_model as wm
import jaccard_model as jm
from hnsw_scan_model import model_scan, ref_scan
from oracle import pyoracle as po
from pgvector_amd import _lib, api
from test_gpu_bit_hnsw import NBITS

pytestmark = pytest.mark.gpu


def mirror(ctx, nbits, rows, graph=None, payload=None):
    h = api.JaccardHnsw(ctx, nbits, rows, payload=payload)
    if graph is not None:
        h.set_graph(*graph)
    return h


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).tolist()


def exact(queries, rows):
    """per query: the exact distances to every row (Fractions) and the float32 values the device must hand back"""
    return [jm.fractions_of(q, rows) for q in queries], [jm.ref_floats(q, rows) for q in queries]


# ------------------------------------------------------------------------------------------------------- 1. scores
@pytest.mark.parametrize("nbits", NBITS)
def test_score_is_the_float_of_the_references_double(ctx, nbits):
    n = 64 if nbits == 64000 else 300
    rows, queries = bhm.rand_bits(n, nbits, 1000 + nbits), bhm.rand_bits(7, nbits, 2000 + nbits)
    rows[0] = 0                 # an all-zero row
    queries[1] = 0              # an all-zero query: 1 against everything, the all-zero row included
    rows[2] = queries[0]        # identical strings
    rows[3] = queries[2] ^ np.packbits(np.arange(8 * rows.shape[1]) < nbits)  # disjoint: the complement inside nbits
    rng = np.random.default_rng(nbits)
    slot, query_of = rng.integers(0, n, 999).astype(np.int32), rng.integers(0, 7, 999).astype(np.int32)
    slot[:8], query_of[:8] = [0, 0, 2, 3, 2, 3, 0, 1], [0, 1, 0, 2, 1, 1, 2, 2]
    _, want = exact(queries, rows)
    h = mirror(ctx, nbits, rows)
    got = h.score(queries, slot, query_of)
    w = np.array([want[q][s] for s, q in zip(slot, query_of)], dtype=np.float32)
    assert got.dtype == np.float32 and bits(got) == bits(w), np.argwhere(got != w)[:5].tolist()
    assert got[1] == 1.0 and got[3] == 1.0 and got[4] == 1.0 and (got[2] == 0.0 or not queries[0].any())
    assert bits(h.score(queries[3:4], slot[:10])) == bits(want[3][slot[:10]])
    b = rng.integers(0, n, 999).astype(np.int32)
    b[:3] = [0, 2, 1]
    pair = np.array([jm.ref_floats(rows[y], rows[x:x + 1])[0] for x, y in zip(slot, b)], dtype=np.float32)
    got = h.score_pairs(slot, b)
    assert bits(got) == bits(pair) and got[0] == 1.0  # (two empty strings: 1)
    h.close()


# ------------------------------------------------------------------- 2. the walk's scorer, independent of tie order
def assert_topk_up_to_ties(elem, dist, fr, want, k, what=""):
    """one query: elem / dist [k] against the brute-force order by Fraction; inside a run of equal Fractions any order,
    the run cut by k drawn from its tie class without repeats"""
    order = sorted(range(len(fr)), key=lambda e: fr[e])[:k]
    got = [int(e) for e in elem if e >= 0]
    assert len(got) == min(k, len(fr)) == len(set(got)), (what, "ids repeat or are missing")
    assert [fr[e] for e in got] == [fr[e] for e in order], (what, "not the k nearest in order")
    assert bits(dist[:len(got)]) == bits(want[got]), (what, "distance bits")


@pytest.mark.parametrize("m", [8, 32])
@pytest.mark.parametrize("nbits", [b for b in NBITS if b <= 16000])
def test_walk_scores_a_complete_graph(ctx, nbits, m):
    n, entry, levels, nbr_start, nbr = bhm.complete_graph(m)
    rows, queries = bhm.rand_bits(n, nbits, 3000 + nbits + m), bhm.rand_bits(6, nbits, 4000 + nbits + m)
    rows[1], queries[5] = 0, 0
    fr, want = exact(queries, rows)
    h = mirror(ctx, nbits, rows, (m, entry, levels, nbr_start, nbr))
    for ef, k in ((n, n), (n, 5), (5, 5)):
        elem, dist, scored = h.search(queries, ef, k)
        assert (scored == n).all(), (ef, k, scored.tolist())
        for q in range(6):
            assert_topk_up_to_ties(elem[q], dist[q], fr[q], want[q], k, what="nbits %d m %d ef %d k %d q %d" % (nbits, m, ef, k, q))
    h.close()


# --------------------------------------------------------------------------------------------- 3. tie-free data
@pytest.fixture(scope="module")
def tie_free_case(oracle):
    """n 500, nbits 16 000, no two rows at one ratio from any query; the oracle's build over the 0/1 expansion gives a
    leveled graph (any graph serves: the walk, not the build, is under test)"""
    nq, n, nbits = 4, 500, 16000
    queries, rows = jm.tie_free(nq, n, nbits, 5)
    g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, bhm.expand01(rows, nbits), m=8, ef_construction=32, seed=7)
    ex = g.export_tuples()
    g.close()
    elements = np.ascontiguousarray(rows[ex["rows"]])
    fr, want = exact(queries, elements)
    for f in fr:
        assert len(set(f)) == n
    assert int(ex["levels"].max()) >= 1
    return queries, elements, nbits, (8, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"]), fr, want


def check_walk(h, queries, graph, fr, want, ef, k, what=""):
    m, entry, levels, nbr_start, nbr = graph
    elem, dist, scored = h.search(queries, ef, k)
    for q in range(len(queries)):
        w = wm.walk(fr[q].__getitem__, levels, nbr_start, nbr, m, entry, ef)
        ids = w.ids[:k]
        assert elem[q][:len(ids)].tolist() == ids and (elem[q][len(ids):] == -1).all(), (what, q, ef)
        assert bits(dist[q][:len(ids)]) == bits(want[q][ids]) and np.isinf(dist[q][len(ids):]).all(), (what, q, ef)
        assert int(scored[q]) == w.scored, (what, q, ef)


@pytest.mark.parametrize("ef,k", [(40, 10), (1, 1)])
def test_walk_equals_the_model_on_tie_free_data(ctx, tie_free_case, ef, k):
    queries, elements, nbits, graph, fr, want = tie_free_case
    h = mirror(ctx, nbits, elements, graph)
    check_walk(h, queries, graph, fr, want, ef, k, "tie-free")
    h.close()


# --------------------------------------------------------------------------------------------- 4. planted pairs
@pytest.mark.parametrize("name", ["stop_pq", "stop_qp", "cut_1", "cut_2"])
def test_planted_farey_neighbours_are_told_apart(ctx, name):
    """64 000 bits; two elements at neighbouring ratios that one fp32 value stands for, placed where the answer depends on
    telling them apart: the strict stop test and the cut by ef (tests/jaccard_model.py planted_cases;
    tests/test_jaccard_model_cpu.py shows that merged keys give another answer on each)"""
    c = jm.planted_cases()[name]
    rows, query = np.stack([jm.planted_row(x, u) for x, u in c["xu"]]), jm.planted_query()
    fr, want = exact(query, rows)
    assert fr[0] == [jm.fraction(x, u) for x, u in c["xu"]]
    graph = (c["m"], c["entry"], c["levels"], c["nbr_start"], c["nbr"])
    h = mirror(ctx, jm.PLANT_BITS, rows, graph)
    check_walk(h, query, graph, fr, want, c["ef"], c["ef"], name)
    slot = np.arange(len(rows), dtype=np.int32)
    assert bits(h.score(query, slot)) == bits(want[0])
    h.close()


# ------------------------------------------------------------------------------------------- 5. tie-heavy data
@pytest.fixture(scope="module")
def tied_case(oracle):
    """64 bits at density 0.5: a few hundred distinct ratios among 1500 rows.  The oracle's build over the 0/1 expansion
    (m 8: the shape of the walk's own tie cases, tests/hnsw_tie_cases.py) gives the graph."""
    rows, queries = bhm.rand_bits(tc.N, 64, 37), bhm.rand_bits(12, 64, 38)
    g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, bhm.expand01(rows, 64), m=8, ef_construction=32, seed=7)
    ex = g.export_tuples()
    g.close()
    elements = np.ascontiguousarray(rows[ex["rows"]])
    fr, want = exact(queries, elements)
    assert all(len(set(f)) < len(f) // 2 for f in fr)
    return queries, elements, (8, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"]), fr, want


@pytest.mark.parametrize("ef,k", tc.ef_k())
def test_walk_equals_the_model_on_tied_data(ctx, tied_case, ef, k):
    """results equal hnsw_walk_model in full, the order inside runs of equal ratios included"""
    queries, elements, graph, fr, want = tied_case
    h = mirror(ctx, 64, elements, graph)
    check_walk(h, queries, graph, fr, want, ef, k, "tied")
    h.close()


# ------------------------------------------------------------------------------------------- 6. resumable scans
def device_stream(scan):
    """every batch of every query until all are exhausted -> per query [(ids, distance bits, scored, left)]"""
    out = [[] for _ in range(scan.nq)]
    live = np.ones(scan.nq, dtype=bool)
    for _ in range(100000):
        if not live.any():
            return out
        e, d, c, s, left = scan.next(live)
        for q in np.flatnonzero(live):
            k = int(c[q])
            assert (e[q, k:] == -1).all() and np.isinf(d[q, k:]).all() and 0 <= k <= scan.ef
            if k == 0:
                live[q] = False
            else:
                out[q].append((e[q, :k].tolist(), bits(d[q, :k]), int(s[q]), int(left[q])))
    raise AssertionError("the scan did not end")


def as_batches(run, want):
    return [(ids, bits(want[ids]), t) for ids, _, t in run]


@pytest.mark.parametrize("ef", (2, 16, 65))
def test_tie_free_stream_is_the_reference(ctx, tie_free_case, ef):
    """whole streams to exhaustion: the elements, the distance bits and so->tuples of the reference's GetScanItems /
    ResumeScanItems (ref_scan) and of the device's array form (model_scan), both fed the exact ratios"""
    queries, elements, nbits, graph, fr, want = tie_free_case
    m, entry, levels, nbr_start, nbr = graph
    h = mirror(ctx, nbits, elements, graph)
    with h.scan(queries, ef) as s:
        got = device_stream(s)
    for q in range(len(queries)):
        ref = ref_scan(fr[q].__getitem__, levels, nbr_start, nbr, m, entry, ef)
        ms = model_scan(fr[q].__getitem__, levels, nbr_start, nbr, m, entry, ef)
        assert [b[:3] for b in got[q]] == as_batches(ref, want[q]) == as_batches(ms.run(), want[q]), (ef, q)
        assert len(ref) > 1
    h.close()


_pool_streams = {}
POOL_EFS = (5, 40, 300)


def pool_streams(ctx, oracle):
    """1000 rows of 512 bits, m 16: pools of more than a thousand entries, ties among them.  Streams of every ef of
    POOL_EFS on the device and through model_scan, once per session"""
    if not _pool_streams:
        n, nbits, m = 1000, 512, 16
        rows, queries = bhm.rand_bits(n, nbits, 11), bhm.rand_bits(2, nbits, 12)
        g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, bhm.expand01(rows, nbits), m=m, ef_construction=32, seed=7)
        ex = g.export_tuples()
        g.close()
        elements = np.ascontiguousarray(rows[ex["rows"]])
        fr, want = exact(queries, elements)
        h = mirror(ctx, nbits, elements, (m, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"]))
        for ef in POOL_EFS:
            with h.scan(queries, ef) as s:
                got = device_stream(s)
            models = [as_batches(model_scan(fr[q].__getitem__, ex["levels"], ex["nbr_start"], ex["nbr"], m, ex["entry"], ef).run(),
                                 want[q]) for q in range(len(queries))]
            _pool_streams[ef] = got, models
        h.close()
    return _pool_streams


@pytest.mark.parametrize("ef", POOL_EFS)
def test_tied_stream_with_large_pools_is_the_model(ctx, oracle, ef):
    got, models = pool_streams(ctx, oracle)[ef]
    for q in range(len(got)):
        assert [b[:3] for b in got[q]] == models[q], (ef, q)
        ids = [e for b in got[q] for e in b[0]]
        assert len(ids) == len(set(ids)) and got[q][-1][2] == len(ids)


def test_pool_edges_occurred(ctx, oracle):
    """from out_left: a resumed batch whose entry step found fewer than ef entries, exactly ef, more; pools above and
    within the entry step's chunk of 256 entries"""
    short = exact_ = above = big = small = 0
    for ef, (got, _) in pool_streams(ctx, oracle).items():
        for stream in got:
            lefts = [b[3] for b in stream]
            for before in lefts[:-1]:
                short += 0 < before < ef
                exact_ += before == ef
                above += before > ef
                big += before > 256
                small += 0 < before <= 256
    assert short > 0 and exact_ > 0 and above > 0 and big > 0 and small > 0, (short, exact_, above, big, small)


def test_drain_returns_the_pool_nearest_first(ctx, tie_free_case):
    queries, elements, nbits, graph, fr, want = tie_free_case
    m, entry, levels, nbr_start, nbr = graph
    h = mirror(ctx, nbits, elements, graph)
    models = [model_scan(fr[q].__getitem__, levels, nbr_start, nbr, m, entry, 5) for q in range(len(queries))]
    with h.scan(queries, 5) as s:
        for _ in range(3):
            s.next()
            for ms in models:
                ms.next()
        for count in (3, 7, 1000):
            e, d, c = s.drain(count)
            for q, ms in enumerate(models):
                ids, _ = ms.drain(count)
                k = len(ids)
                assert int(c[q]) == k and e[q, :k].tolist() == ids and (e[q, k:] == -1).all(), (count, q)
                assert bits(d[q, :k]) == bits(want[q][ids]) and np.isinf(d[q, k:]).all(), (count, q)
        e, d, c, sc, left = s.next()  # the pools are empty: the scans are over
        assert (c == 0).all() and (left == 0).all()
    h.close()


@pytest.mark.parametrize("strict", (False, True))
@pytest.mark.parametrize("limit", (20000, 60))
def test_iterative_search_under_a_filter(ctx, tie_free_case, limit, strict):
    """api.hnsw_iterative_search through JaccardHnsw.scan with a filter keeping 1 element in 20: the model's loop"""
    queries, elements, nbits, graph, fr, want = tie_free_case
    m, entry, levels, nbr_start, nbr = graph
    keep = np.arange(len(elements)) % 20 == 7
    h = mirror(ctx, nbits, elements, graph)
    ids, dist, scored = api.hnsw_iterative_search(h, queries, 10, keep, 5, max_scan_tuples=limit, strict=strict)
    for q in range(len(queries)):
        ms = model_scan(fr[q].__getitem__, levels, nbr_start, nbr, m, entry, 5)
        w_ids, _, w_tuples = ms.iterative_search(10, keep, max_scan_tuples=limit, strict=strict)
        assert ids[q] == w_ids and int(scored[q]) == w_tuples, (q, limit, strict)
        assert bits(dist[q]) == bits(want[q][w_ids]) and all(keep[e] for e in ids[q])
        assert len(w_ids) > 0
    h.close()


# ---------------------------------------------------------------------------------------------- 7. views and importers
@pytest.fixture(scope="module")
def small_case():
    nbits, m = 200, 8
    n, entry, levels, nbr_start, nbr = bhm.complete_graph(m)
    rows, queries = bhm.rand_bits(n, nbits, 71), bhm.rand_bits(5, nbits, 72)
    payload = (np.arange(n, dtype=np.uint32)[:, None] * 31 + np.arange(3, dtype=np.uint32)[None, :]).astype(np.uint32)
    fr, want = exact(queries, rows)
    return nbits, rows, queries, (m, entry, levels, nbr_start, nbr), payload, fr, want


def test_share_view_returns_the_owners_answers(ctx, small_case):
    nbits, rows, queries, graph, payload, fr, want = small_case
    h = mirror(ctx, nbits, rows, graph, payload)
    own = h.search(queries, 10, 10)
    ctx2 = api.Context(0)
    view = h.share(ctx2)
    assert isinstance(view, api.JaccardHnsw)
    for a, b in zip(own, view.search(queries, 10, 10)):
        assert np.array_equal(a, b)
    for q in range(len(queries)):
        assert_topk_up_to_ties(own[0][q], own[1][q], fr[q], want[q], 10, what="view q%d" % q)
    slot = np.arange(len(rows), dtype=np.int32)
    assert bits(view.score(queries[:1], slot)) == bits(want[0])
    assert np.array_equal(view.get_payload(np.array([3, -1])), np.stack([payload[3], np.zeros(3, np.uint32)]))
    with view.scan(queries, 4) as s:
        e, d, c, _, _ = s.next()
    assert np.array_equal(e, own[0][:, :4]) and bits(d) == bits(own[1][:, :4])
    view.close()
    ctx2.close()
    h.close()


def test_jaccard_mirror_across_processes(ctx, small_case, tmp_path):
    """the exported handle carries the bit metric: a fresh child process that opens it as a plain bit mirror walks it with
    Jaccard keys and gets Jaccard distances (a Hamming walk of the same rows would return bit counts)"""
    nbits, rows, queries, graph, payload, fr, want = small_case
    h = mirror(ctx, nbits, rows, graph, payload)
    own_elem, own_dist, own_scored = h.search(queries, 10, 10)
    job, res = str(tmp_path / "job.npz"), str(tmp_path / "res.npz")
    np.savez(job, handle=np.frombuffer(h.export(), dtype=np.uint8), queries=queries, ef=10, k=10, words=3)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "mp_bit_hnsw_import_worker.py"), job, res], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(res)
    assert np.array_equal(out["elem"], own_elem) and bits(out["dist"]) == bits(own_dist)
    assert np.array_equal(out["scored"], own_scored)
    assert bits(out["score"]) == bits([want[i][i] for i in range(len(queries))])
    assert np.array_equal(out["payload"], payload[own_elem.ravel()])
    for q in range(len(queries)):
        assert_topk_up_to_ties(out["elem"][q], out["dist"][q], fr[q], want[q], 10, what="import q%d" % q)
    h.close()


def test_payload_round_trip(ctx, small_case):
    nbits, rows, _, _, payload, _, _ = small_case
    h = mirror(ctx, nbits, rows, payload=payload)
    ids = np.array([0, 16, -1, 5, 5], dtype=np.int64)
    assert np.array_equal(h.get_payload(ids), np.where(ids[:, None] >= 0, payload[np.clip(ids, 0, None)], 0))
    h.close()


def test_update_graph_is_seen_by_the_next_search(ctx, small_case):
    nbits, rows, queries, (m, entry, levels, nbr_start, nbr), _, fr, want = small_case
    n = len(rows)
    h = mirror(ctx, nbits, rows, (m, entry, levels, nbr_start, np.full_like(nbr, -1)))
    elem, dist, scored = h.search(queries, n, n)
    assert (elem[:, 0] == 0).all() and (elem[:, 1:] == -1).all() and (scored == 1).all()
    h.update_graph(3, np.array([3], dtype=np.int32), np.array([0, 2 * m], dtype=np.int64), nbr[nbr_start[3]:nbr_start[4]])
    elem, dist, scored = h.search(queries, n, n)
    assert (scored == n).all()
    for q in range(len(queries)):
        assert_topk_up_to_ties(elem[q], dist[q], fr[q], want[q], n, what="patched q%d" % q)
    h.close()


# ------------------------------------------------------------------------------------------------------------ 8. edges
def test_empty_index_and_one_element(ctx):
    queries = bhm.rand_bits(3, 100, 81)
    for rows in (bhm.rand_bits(4, 100, 82), np.zeros((0, 13), dtype=np.uint8)):
        n = len(rows)
        h = mirror(ctx, 100, rows, (8, -1, np.zeros(n, np.int32), np.arange(n + 1, dtype=np.int64) * 16,
                                    np.full(max(16 * n, 1), -1, np.int32)))
        elem, dist, scored = h.search(queries, 5, 5)
        assert (elem == -1).all() and np.isinf(dist).all() and (dist > 0).all() and (scored == 0).all()
        with h.scan(queries, 5) as s:
            e, d, c, sc, left = s.next()
        assert (e == -1).all() and np.isinf(d).all() and (c == 0).all()
        h.close()
    rows = bhm.rand_bits(1, 100, 83)
    h = mirror(ctx, 100, rows, (8, 0, np.zeros(1, np.int32), np.array([0, 16], np.int64), np.full(16, -1, np.int32)))
    elem, dist, scored = h.search(queries, 3, 3)
    assert elem.tolist() == [[0, -1, -1]] * 3 and scored.tolist() == [1] * 3
    assert bits(dist[:, 0]) == bits([jm.ref_floats(q, rows)[0] for q in queries]) and np.isinf(dist[:, 1:]).all()
    h.close()


def test_argument_errors(ctx, small_case):
    nbits, rows, queries, graph = small_case[:4]
    h = mirror(ctx, nbits, rows, graph)
    for ef, k in ((5, 6), (1001, 10), (0, 1), (5, 0)):
        with pytest.raises(api.PgvError) as e:
            h.search(queries, ef, k)
        assert e.value.code == api.PGV_ERR_ARG, (ef, k)
    h.close()
    for bad in (0, 64001, -1):
        with pytest.raises(api.PgvError) as e:
            api.JaccardHnsw(ctx, bad, np.zeros((2, max((bad + 7) // 8, 1)), dtype=np.uint8))
        assert e.value.code == _lib.PGV_ERR_DIMS, bad
    with pytest.raises(api.PgvError) as e:
        api.JaccardHnsw(ctx, nbits, rows, payload=np.zeros((len(rows), 1025), dtype=np.uint32))
    assert e.value.code == api.PGV_ERR_ARG
    out = C.c_void_p()
    assert _lib.lib.pgv_hnsw_upload_jaccard(None, 8, None, 0, None, 0, C.byref(out)) == api.PGV_ERR_ARG
    assert _lib.lib.pgv_hnsw_upload_jaccard(ctx.h, 8, None, 2, None, 0, C.byref(out)) == api.PGV_ERR_ARG  # n > 0, no rows
    h = api.JaccardHnsw(ctx, nbits, rows)
    with pytest.raises(api.PgvError) as e:  # no graph yet
        h.search(queries, 5, 5)
    assert e.value.code == api.PGV_ERR_ARG
    h.close()


def test_upload_bits_still_turns_jaccard_away(ctx, small_case):
    nbits, rows = small_case[:2]
    with pytest.raises(api.PgvError) as e:
        api.BitHnsw(ctx, nbits, rows, metric=api.PGV_BIT_JACCARD)
    assert e.value.code == api.PGV_ERR_ARG and "jaccard" in e.value.message
    assert "pgv_hnsw_upload_jaccard" in e.value.message


def test_build_side_entries_reject_a_jaccard_mirror(ctx, small_case):
    nbits, rows, queries, graph = small_case[:4]
    h = mirror(ctx, nbits, rows, graph)
    before = h.search(queries, 10, 10)
    L = C.CDLL(_lib.LIB_PATH)  # a handle of its own: the prototypes other modules declare on _lib.lib do not apply
    L.pgv_last_error.restype = C.c_char_p
    i32 = lambda c: np.zeros(c, dtype=np.int32)  # noqa: E731
    f32, u8, i64 = np.zeros(4096, np.float32), np.zeros(4096, np.uint8), np.zeros(8, np.int64)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    el, lv, big, cnt = i32(2), i32(2), i32(4096), i32(2)
    calls = {
        "pgv_hnsw_build_search": lambda: L.pgv_hnsw_build_search(h.h, P(el), P(lv), C.c_int(2), C.c_int(8), C.c_int(1), P(big),
                                                                 P(f32), P(cnt)),
        "pgv_hnsw_build_neighbors": lambda: L.pgv_hnsw_build_neighbors(h.h, P(el), P(lv), C.c_int(2), C.c_int(8), C.c_int(1),
                                                                       P(big), P(f32), P(u8), P(cnt), P(i64)),
        "pgv_hnsw_build_search_keep": lambda: L.pgv_hnsw_build_search_keep(h.h, P(el), P(lv), C.c_int(2), C.c_int(8),
                                                                           C.c_int(1), C.c_int(0)),
        "pgv_hnsw_build_select_kept": lambda: L.pgv_hnsw_build_select_kept(h.h, C.c_int(0), P(big), P(f32), P(u8), P(cnt),
                                                                           P(i64)),
        "pgv_hnsw_link_begin": lambda: L.pgv_hnsw_link_begin(h.h),
        "pgv_hnsw_link_prepare": lambda: L.pgv_hnsw_link_prepare(h.h, P(el), P(u8), C.c_int(2), C.c_int(1), P(big), P(f32),
                                                                 P(u8), P(cnt), P(i64)),
        "pgv_hnsw_link_apply": lambda: L.pgv_hnsw_link_apply(h.h, C.c_int32(0)),
        "pgv_hnsw_link_end": lambda: L.pgv_hnsw_link_end(h.h, P(big), P(i64), P(i64)),
        "pgv_hnsw_score_groups": lambda: L.pgv_hnsw_score_groups(h.h, P(el), P(i64), P(cnt), P(i64), C.c_int(1),
                                                                 C.c_int64(2), C.c_int64(1), P(f32)),
    }
    declared = [s for s in _lib.SYMBOLS if s.startswith(("pgv_hnsw_build_", "pgv_hnsw_link_"))] + ["pgv_hnsw_score_groups"]
    assert sorted(calls) == sorted(declared)
    for name, call in calls.items():
        assert call() == api.PGV_ERR_ARG, name
        assert "bit mirror" in L.pgv_last_error().decode(), name
    for a, b in zip(before, h.search(queries, 10, 10)):
        assert np.array_equal(a, b)
    h.close()


def test_device_resident_inputs(ctx, small_case):
    import torch
    nbits, rows, queries, graph = small_case[:4]
    h = mirror(ctx, nbits, rows, graph)
    want = h.search(queries, 10, 10)
    slot = np.arange(len(rows), dtype=np.int32)
    want_score = h.score(queries[:1], slot)
    d = mirror(ctx, nbits, torch.from_numpy(rows).cuda(), graph)
    got = d.search(torch.from_numpy(queries).cuda(), 10, 10)
    assert all(g.is_cuda for g in got)
    for a, b in zip(want, got):
        assert np.array_equal(a, b.cpu().numpy())
    assert np.array_equal(d.score(torch.from_numpy(queries[:1].copy()).cuda(), slot), want_score)
    with d.scan(torch.from_numpy(queries).cuda(), 10) as s:
        e, dd, c, _, _ = s.next()
    assert e.is_cuda and np.array_equal(e.cpu().numpy(), want[0]) and np.array_equal(dd.cpu().numpy(), want[1])
    # 128 bits = 16 bytes: device rows and queries are read in place
    rows16, q16 = bhm.rand_bits(len(rows), 128, 91), bhm.rand_bits(4, 128, 92)
    a, b = mirror(ctx, 128, rows16, graph), mirror(ctx, 128, torch.from_numpy(rows16).cuda(), graph)
    for x, y in zip(a.search(q16, 10, 10), b.search(torch.from_numpy(q16).cuda(), 10, 10)):
        assert np.array_equal(x, y.cpu().numpy())
    for x in (h, d, a, b):
        x.close()
