"""hnsw_search_kernel's handling of equal distances -- the tie list T, the stable merge, the level filter -- against
tests/hnsw_walk_model.py, the plain-Python model of the same walk, on inputs made of ties (tests/hnsw_tie_cases.py; what
they reach is settled in tests/test_hnsw_walk_model_cpu.py): planted graphs whose answer holds in every tie order, through
every row type and metric the kernel is instantiated for, and small-integer random data on which the device must equal
the model exactly -- elements in order, distances bit for bit, scored counts, and the build side's W of every layer."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hnsw_tie_cases as tc
from hnsw_walk_model import walk
from pgvector_amd import _host, api

pytestmark = pytest.mark.gpu

METRIC = {"l2": api.PGV_L2SQ, "negip": api.PGV_NEG_IP, "l1": api.PGV_L1}
FORMS = [(m, t) for m in tc.METRICS for t in ("f32", "f16")] + [("l2", "bits")]
DTYPE = {"f32": api.PGV_F32, "f16": api.PGV_F16}


def mirror_of(ctx, metric, kind, rows, graph):
    """rows [n x dim] float32 of small integers (0 / 1 for bits) as a mirror of the given row type, with its graph"""
    if kind == "bits":
        h = api.BitHnsw(ctx, rows.shape[1], np.packbits(rows.astype(np.uint8), axis=1))
    else:
        h = api.Hnsw(ctx, METRIC[metric], DTYPE[kind], rows.shape[1], rows)
    h.set_graph(*graph)
    return h


def as_queries(kind, queries):
    return np.packbits(queries.astype(np.uint8), axis=1) if kind == "bits" else queries


def graph_of(case):
    return case["m"], case["entry"], case["levels"], case["nbr_start"], case["nbr"]


# ------------------------------------------------------------------------------------------------ the planted graphs
@pytest.mark.parametrize("name", sorted(tc.planted()))
@pytest.mark.parametrize("metric,kind", FORMS)
def test_planted_answer(ctx, name, metric, kind):
    """the answer that holds in every tie order (derived beside each case in tests/hnsw_tie_cases.py), and the model's
    own tie order exactly"""
    case = tc.planted()[name]
    ef = case["ef"]
    h = mirror_of(ctx, metric, kind, tc.planted_rows(case["dists"]), graph_of(case))
    elem, dist, scored = h.search(as_queries(kind, tc.planted_query(metric)), ef, ef)
    h.close()
    print(name, metric, kind, elem[0].tolist(), dist[0].tolist(), int(scored[0]))
    tc.check_head(case, elem[0], dist[0], what="%s %s %s" % (name, metric, kind))
    assert int(scored[0]) == case["scored"]
    assert not set(elem[0].tolist()) & set(case["unscored"])
    w = walk(lambda e: case["dists"][e], case["levels"], case["nbr_start"], case["nbr"], case["m"], 0, ef, tie_cap=ef)
    assert elem[0][elem[0] >= 0].tolist() == w.ids and w.counters["lost"] == 0


@pytest.mark.parametrize("name", sorted(tc.planted()))
def test_planted_answer_from_the_host_walk(ctx, name):
    """pgv_host_hnsw_search keeps the reference's two heaps on the host and scores on the device: a third tie order"""
    case = tc.planted()[name]
    ef = case["ef"]
    for metric in tc.METRICS:
        h = api.Hnsw(ctx, METRIC[metric], api.PGV_F32, tc.DIM, tc.planted_rows(case["dists"]))
        graph = _host.hnsw_graph(case["levels"], case["nbr_start"], case["nbr"], case["m"], case["entry"])
        elem, dist, scored = _host.hnsw_search(h, graph, tc.planted_query(metric), ef, ef)
        h.close()
        tc.check_head(case, elem[0], dist[0], what="host %s %s" % (name, metric))
        assert int(scored[0]) == case["scored"]


def test_more_queries_than_workgroups(ctx):
    """case A 1500 times in one launch: at most four workgroups per CU take the queries off the shared counter and reuse
    their LDS and visited bitmap; every row is the single query's answer"""
    case = tc.planted()["A"]
    h = mirror_of(ctx, "l2", "f32", tc.planted_rows(case["dists"]), graph_of(case))
    one = h.search(tc.planted_query("l2"), 2, 2)
    elem, dist, scored = h.search(np.repeat(tc.planted_query("l2"), 1500, axis=0), 2, 2)
    h.close()
    tc.check_head(case, one[0][0], one[1][0])
    assert (elem == one[0][0]).all() and (dist.view(np.uint32) == one[1][0].view(np.uint32)).all()
    assert (scored == 5).all()


# --------------------------------------------------------------------------------------------------- the random set
_model_cache = {}


def model_runs(oracle, form):
    """form -> (elements, queries, graph export, {(query, ef): Walk}) with T of ef entries, the device's; no append
    is ever lost to that capacity, so these are the unbounded model's walks as well"""
    if form not in _model_cache:
        elements, queries, ex, d = tc.random_graph(oracle, form)
        runs = {}
        for q in range(tc.NQ):
            dq = d[q].tolist()
            for ef in tc.EFS:
                runs[q, ef] = walk(dq.__getitem__, ex["levels"], ex["nbr_start"], ex["nbr"], 8, ex["entry"], ef, tie_cap=ef)
                assert runs[q, ef].counters["lost"] == 0
        _model_cache[form] = elements, queries, ex, runs
    return _model_cache[form]


def assert_equals_model(runs, ef, k, elem, dist, scored, what):
    for q in range(tc.NQ):
        w = runs[q, ef]
        n = min(k, len(w.ids))
        want_ids = w.ids[:n] + [-1] * (k - n)
        want_dist = np.array(w.dist[:n] + [np.inf] * (k - n), dtype=np.float32) + np.float32(0)  # (-0 has key +0)
        assert elem[q].tolist() == want_ids, (what, q, "elements")
        assert np.array_equal(dist[q].view(np.uint32), want_dist.view(np.uint32)), (what, q, "distances")
        assert int(scored[q]) == w.scored, (what, q, "scored", int(scored[q]), w.scored)


@pytest.mark.parametrize("metric,kind", FORMS)
def test_random_ties_equal_the_model(ctx, oracle, metric, kind):
    elements, queries, ex, runs = model_runs(oracle, "bits" if kind == "bits" else metric)
    h = mirror_of(ctx, metric, kind, elements, (8, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"]))
    for ef, k in tc.ef_k():
        elem, dist, scored = h.search(as_queries(kind, queries), ef, k)
        assert_equals_model(runs, ef, k, elem, dist, scored, "%s %s ef %d k %d" % (metric, kind, ef, k))
    h.close()


@pytest.mark.parametrize("metric", tc.METRICS)
def test_build_side_lists_equal_the_model(ctx, oracle, metric):
    """pgv_hnsw_build_search: elements of the mirror as queries, random insert levels, ef_construction on the layers at or
    below them -- W of every such layer, nearest first, against the model's"""
    elements, _, ex, _ = model_runs(oracle, metric)
    top = int(ex["levels"][ex["entry"]])
    lcap = top + 1
    assert top >= 1
    elems = np.random.default_rng(43).choice(len(elements), tc.NQ, replace=False).astype(np.int32)
    qlevels = tc.insert_levels(tc.NQ, top)
    d = tc.distances(metric, elements[elems], elements)
    for efc in (10, 40, 64, 65, 200):
        want = [walk(d[i].tolist().__getitem__, ex["levels"], ex["nbr_start"], ex["nbr"], 8, ex["entry"], efc,
                     qlevel=int(qlevels[i]), tie_cap=efc) for i in range(tc.NQ)]
        for kind in ("f32", "f16"):
            h = mirror_of(ctx, metric, kind, elements, (8, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"]))
            ids = np.full((tc.NQ, lcap, efc), -7, np.int32)
            dist = np.full((tc.NQ, lcap, efc), -7, np.float32)
            cnt = np.full((tc.NQ, lcap), -7, np.int32)
            api.check(api.lib.pgv_hnsw_build_search(h.h, api.ptr(elems), api.ptr(qlevels), tc.NQ, efc, lcap, api.ptr(ids),
                                                    api.ptr(dist), api.ptr(cnt)))
            h.close()
            for i in range(tc.NQ):
                assert want[i].counters["lost"] == 0
                for lc in range(lcap):
                    w_ids, w_dist = want[i].layers.get(lc, ([], []))
                    what = (metric, kind, efc, i, lc)
                    assert cnt[i, lc] == len(w_ids), what
                    assert ids[i, lc, :len(w_ids)].tolist() == w_ids, what
                    assert np.array_equal(dist[i, lc, :len(w_ids)].view(np.uint32),
                                          (np.array(w_dist, dtype=np.float32) + np.float32(0)).view(np.uint32)), what


# ------------------------------------------------------------------------------------------- the row-scoring forms
def test_rows_per_trip_forms_agree(oracle, tmp_path):
    """PGV_HNSW_ROWS_PER_TRIP = 1, 2 and 4 (the default) score a batch's rows one, two or four to a lane group at a time;
    the distances, and so the walks, must not depend on it: byte-identical outputs over the random set (fp32, fp16) and
    over non-integer fp16 data, and on the integer cases the model's walks"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for trip in ("1", "2", "4"):
        res = str(tmp_path / ("trip%s.npz" % trip))
        env = dict(os.environ, PYTHONPATH=root, PGV_HNSW_ROWS_PER_TRIP=trip)
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "mp_hnsw_trip_worker.py"), res], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0 and "TRIP-OK %s" % trip in r.stdout, (trip, r.stdout[-500:], r.stderr[-2000:])
        outs.append(dict(np.load(res)))
    for other in outs[1:]:
        assert sorted(other) == sorted(outs[0])
        for key, v in outs[0].items():
            assert v.dtype == other[key].dtype and v.tobytes() == other[key].tobytes(), key
    for form in tc.METRICS:
        runs = model_runs(oracle, form)[3]
        for name in ("f32", "f16"):
            for ef, k in tc.ef_k():
                key = "%s_%s_%d_%d" % (form, name, ef, k)
                assert_equals_model(runs, ef, k, outs[0][key + "_elem"], outs[0][key + "_dist"], outs[0][key + "_scored"], key)
