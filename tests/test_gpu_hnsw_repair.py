"""hnswvacuum's RepairGraph on the device -- pgv_hnsw_set_live, pgv_hnsw_repair_neighbors and pgv_host_hnsw_repair --
against tests/hnsw_repair_model.py, the plain-Python restatement of the reference's code.  Integer-valued vectors, so every
fp32 distance is exact and every comparison is equality: element slots, distance bits, closer flags, counts, status, whole
neighbour arrays and entry points.  tests/test_hnsw_repair_model_cpu.py pins the model and asserts on the same seeds what
these tests rely on: tie-free walks, what the planted cases claim, the dead_cap every case needs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hnsw_repair_model as rm
from pgvector_amd import _lib, api

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (api.PGV_F32, np.float32), "f16": (api.PGV_F16, np.float16)}
LAYER_CAP = 3  # knn_graph's levels are 0 .. 2


def mirror_of(ctx, pts, graph, m, dtype):
    entry, levels, start, nbr = graph
    h = api.Hnsw(ctx, api.PGV_L2SQ, DTYPES[dtype][0], pts.shape[1], pts.astype(DTYPES[dtype][1]))
    h.set_graph(m, entry, levels, start, nbr)
    return h


_models = {}


def model_lists(key, c, live, q):
    """the model's answer for query element q, computed once per (case, liveness)"""
    k = (key, q)
    if k not in _models:
        _models[k] = rm.find_neighbors(rm.sqdist(c["pts"]), c["levels"], c["nbr_start"], c["nbr"], c["m"], q, c["entry"],
                                       c["efc"], live)
    return _models[k]


def assert_lists(got, i, want, layer_cap, what):
    ids, dist, closer, count, _, _ = got
    for lc in range(layer_cap):
        w = want.get(lc, [])
        n = int(count[i, lc])
        assert n == len(w), (what, lc, n, len(w))
        assert ids[i, lc, :n].tolist() == [x for x, _, _ in w], (what, lc)
        assert dist[i, lc, :n].tolist() == [float(d) for _, d, _ in w], (what, lc)
        assert closer[i, lc, :n].tolist() == [f for _, _, f in w], (what, lc)


_cases = {}


def case_of(spec):
    if spec[0] not in _cases:
        _cases[spec[0]] = rm.make_case(spec)
    return _cases[spec[0]]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("spec", rm.CASES, ids=lambda s: s[0])
def test_repair_neighbors_equal_the_model(ctx, spec, dtype):
    """dead shares 25 % and 60 %; among the queries an element all of whose neighbours are dead, the centre of a dead
    cluster that makes W exceed ef by more than 16, and an element on the top layer"""
    c = case_of(spec)
    h = mirror_of(ctx, c["pts"], (c["entry"], c["levels"], c["nbr_start"], c["nbr"]), c["m"], dtype)
    h.set_live(c["live"])
    assert h.live_count() == int(c["live"].sum())
    got = h.repair_neighbors(c["queries"], c["m"], c["efc"], LAYER_CAP, rm.N)
    assert got[4].tolist() == [0] * len(c["queries"])
    for i, q in enumerate(c["queries"]):
        assert_lists(got, i, model_lists(spec[0], c, c["live"], q), LAYER_CAP, (spec[0], dtype, q))
    h.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("trap", rm.TRAPS, ids=lambda t: t.__name__)
def test_traps_where_truncating_to_ef_is_wrong(ctx, trap, dtype):
    (pts, live, levels, start, nbr), want = trap()
    h = mirror_of(ctx, pts, (1, levels, start, nbr), 4, dtype)
    h.set_live(live)
    ids, dist, closer, count, status, _ = h.repair_neighbors([0], 4, 4, 1, 8)
    d = rm.sqdist(pts)
    model = rm.find_neighbors(d, levels, start, nbr, 4, 0, 1, 4, live)
    assert sorted(x for x, _, _ in model[0]) == want
    assert status.tolist() == [0]
    assert_lists((ids, dist, closer, count, status, 0), 0, model, 1, trap.__name__)
    h.close()


def test_overflow_is_reported_per_element_and_touches_nobody_else(ctx):
    c = rm.make_overflow_case()
    h = mirror_of(ctx, c["pts"], (c["entry"], c["levels"], c["nbr_start"], c["nbr"]), c["m"], "f32")
    h.set_live(c["live"])
    got = h.repair_neighbors(c["queries"], c["m"], c["efc"], LAYER_CAP, c["dead_cap"])
    assert got[4].tolist() == [1] + [0] * (len(c["queries"]) - 1)
    assert got[3][0].tolist() == [0] * LAYER_CAP, "an overflowed element's counts are 0, never a shorter list"
    for i, q in enumerate(c["queries"][1:], start=1):
        assert_lists(got, i, model_lists("overflow", c, c["live"], q), LAYER_CAP, ("overflow", q))
    # ... and with room the planted element is served like any other
    got = h.repair_neighbors(c["queries"][:1], c["m"], c["efc"], LAYER_CAP, rm.N)
    assert got[4].tolist() == [0]
    assert_lists(got, 0, model_lists("overflow", c, c["live"], c["queries"][0]), LAYER_CAP, "overflow centre")
    h.close()


@pytest.mark.parametrize("bitmap", ["unset", "all_set"])
def test_without_a_dead_bit_it_is_the_search_at_ef_plus_one_less_the_element(ctx, bitmap):
    c = case_of(rm.CASES[0])
    h = mirror_of(ctx, c["pts"], (c["entry"], c["levels"], c["nbr_start"], c["nbr"]), c["m"], "f32")
    live = np.ones(rm.N, dtype=bool)
    if bitmap == "all_set":
        h.set_live(live)
    assert h.live_count() == rm.N
    got = h.repair_neighbors(c["queries"], c["m"], c["efc"], LAYER_CAP, 0)
    assert got[4].tolist() == [0] * len(c["queries"]), "no dead element: dead_cap 0 is enough"
    for i, q in enumerate(c["queries"]):
        assert_lists(got, i, model_lists("all_live", c, live, q), LAYER_CAP, ("all live", q))
    h.close()


_driver = {}
DRIVER = {spec[0]: spec for spec in rm.DRIVER_CASES}


def driver_model(name, max_batch):
    if (name, max_batch) not in _driver:
        c = case_of(DRIVER[name])
        rm.TIES[0] = 0
        _driver[name, max_batch] = rm.repair_graph(rm.sqdist(c["pts"]), c["levels"], c["nbr_start"], c["nbr"], c["entry"],
                                                   c["live"], c["m"], c["efc"], max_batch)
        assert rm.TIES[0] == 0
    return _driver[name, max_batch]


@pytest.mark.parametrize("name,dtype,max_batch", [
    ("driver_d8_m4_ef8_25", "f32", 1), ("driver_d8_m4_ef8_25", "f32", 7), ("driver_d8_m4_ef8_25", "f32", 64),
    ("driver_d8_m4_ef8_25", "f16", 1), ("driver_d8_m4_ef8_25", "f16", 64),
    ("driver_d20_m8_ef16_25", "f32", 1), ("driver_d20_m8_ef16_25", "f32", 64), ("driver_d20_m8_ef16_25", "f16", 7)])
def test_host_driver_equals_the_model(ctx, name, dtype, max_batch):
    """max_batch = 1 is the reference's serial loop; 7 and 64 against the model run at the same batch size.  The second
    shape has 16 links on layer 0 and a row tail in fp16."""
    c = case_of(DRIVER[name])
    h = mirror_of(ctx, c["pts"], (c["entry"], c["levels"], c["nbr_start"], c["nbr"]), c["m"], dtype)
    out = h.repair(c["live"], c["m"], c["efc"], max_batch=max_batch)
    want_nbr, want_entry, cnt = driver_model(name, max_batch)
    assert out["entry"] == want_entry
    # (the levels are an input the driver cannot change: it returns the neighbour array alone, in the input's layout)
    assert out["nbr"].shape == c["nbr"].shape
    assert np.array_equal(out["nbr"], want_nbr)
    assert (out["repaired"], out["batches"], out["examined"]) == (cnt["repaired"], cnt["batches"], cnt["examined"])
    # the driver drops a back link into a tuple that its owner's own repair overwrites later in the same batch; the model
    # applies it and counts its reselection.  In the serial loop there is no such link.
    assert out["reselections"] == cnt["reselections"] if max_batch == 1 else 0 < out["reselections"] <= cnt["reselections"]
    rm.check_invariants(c["levels"], c["nbr_start"], out["nbr"], out["entry"], c["live"], c["m"])
    # the mirror holds the repaired graph: 64 queries right on dead elements find no dead element, without any filter
    dead = np.nonzero(~c["live"])[0][:64]
    assert len(dead) == 64
    elem, _, _ = h.search(c["pts"][dead].astype(DTYPES[dtype][1]), 40, 10)
    found = np.asarray(elem)
    assert (found >= 0).any() and c["live"][found[found >= 0]].all()
    h.close()


def test_overflow_redo_gives_the_same_arrays(ctx):
    """the first dead_cap forced small: the overflowed elements are redone with it doubled until they fit"""
    c = case_of(rm.DRIVER_CASE)
    h = mirror_of(ctx, c["pts"], (c["entry"], c["levels"], c["nbr_start"], c["nbr"]), c["m"], "f32")
    out = h.repair(c["live"], c["m"], c["efc"], max_batch=64, dead_cap=4)
    want_nbr, want_entry, _ = driver_model(rm.DRIVER_CASE[0], 64)
    assert out["overflow_redos"] > 0 and out["dead_cap"] > 4
    assert out["entry"] == want_entry and np.array_equal(out["nbr"], want_nbr)
    h.close()


@pytest.mark.parametrize("seed", [11, 12])
def test_searches_and_scans_ignore_the_bitmap(ctx, seed):
    """the same bytes from pgv_hnsw_search and pgv_hnsw_scan_* before set_live, with the bitmap set and with it unset again"""
    c = case_of(rm.CASES[0] if seed == 11 else rm.CASES[1])
    h = mirror_of(ctx, c["pts"], (c["entry"], c["levels"], c["nbr_start"], c["nbr"]), c["m"], "f32")
    queries = rm.int_points(16, c["dim"], seed + 500, 300).astype(np.float32)

    def answers():
        out = [np.asarray(x).tobytes() for x in h.search(queries, 20, 10)]
        scan = h.scan(queries, 12)
        for _ in range(3):
            out += [np.asarray(x).tobytes() for x in scan.next()]
        out += [np.asarray(x).tobytes() for x in scan.drain(4)]
        scan.close()
        scan = h.scan(queries, 12)
        out += [np.asarray(x).tobytes() for x in scan.filtered(5, keep=c["live"])]
        scan.close()
        return out
    before = answers()
    h.set_live(c["live"])
    assert answers() == before
    h.set_live(None)
    assert h.live_count() == rm.N and answers() == before
    h.close()


def test_wrong_word_counts_are_refused(ctx):
    c = case_of(rm.CASES[0])
    h = mirror_of(ctx, c["pts"], (c["entry"], c["levels"], c["nbr_start"], c["nbr"]), c["m"], "f32")
    words = api.live_words(c["live"])
    for bad in (words[:-1], np.concatenate([words, words[:1]])):
        with pytest.raises(api.PgvError) as e:
            _lib.check(_lib.lib.pgv_hnsw_set_live(h.h, api.ptr(np.ascontiguousarray(bad)), int(bad.size)))
        assert e.value.code == _lib.PGV_ERR_ARG and "words" in e.value.message
    with pytest.raises(api.PgvError) as e:
        h.repair_neighbors([0], c["m"], c["efc"], LAYER_CAP, 1 << 20)
    assert e.value.code == _lib.PGV_ERR_ARG and "LDS" in e.value.message
    h.close()


def refused(call, name):
    with pytest.raises(api.PgvError) as e:
        call()
    assert e.value.code == _lib.PGV_ERR_ARG and name in e.value.message, e.value.message


def test_other_mirror_kinds_refuse_by_name(ctx):
    rng = np.random.RandomState(3)
    rows = rng.randint(0, 256, size=(40, 8)).astype(np.uint8)
    levels, start, nbr, entry = rm.knn_graph(rows.astype(np.int64), 4, 3)
    kinds = [(api.BitHnsw(ctx, 64, rows), "a bit mirror"), (api.JaccardHnsw(ctx, 64, rows), "a Jaccard bit mirror")]
    ptr = np.arange(0, 41 * 2, 2, dtype=np.int64)
    idx = np.tile(np.array([1, 5], dtype=np.int32), 40)
    val = rng.randint(1, 9, size=80).astype(np.float32)
    kinds.append((api.SparseHnsw(ctx, api.PGV_L2SQ, 16, (ptr, idx, val)), "a sparse mirror"))
    for h, name in kinds:
        h.set_graph(4, entry, levels, start, nbr)
        refused(lambda: h.set_live(np.ones(40, dtype=bool)), name)
        refused(lambda: h.repair_neighbors([0, 1], 4, 8, LAYER_CAP, 4), name)
        assert h.live_count() == -1 and name in _lib.lib.pgv_last_error().decode()
        h.close()


def test_imported_mirror_refuses_by_name(ctx, tmp_path):
    c = case_of(rm.CASES[0])
    h = mirror_of(ctx, c["pts"], (c["entry"], c["levels"], c["nbr_start"], c["nbr"]), c["m"], "f32")
    job, res = str(tmp_path / "job.npz"), str(tmp_path / "res.npz")
    np.savez(job, handle=np.frombuffer(h.export(), dtype=np.uint8), n=rm.N, m=c["m"])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "mp_hnsw_repair_import_worker.py"), job, res], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(res)
    assert out["codes"].tolist() == [_lib.PGV_ERR_ARG] * 2
    assert all("an imported mirror" in t for t in out["texts"].tolist())
    h.close()
