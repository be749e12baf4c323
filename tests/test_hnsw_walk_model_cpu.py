"""tests/hnsw_walk_model.py, the plain-Python model of the device's HNSW walk, against the compiled oracle, and the inputs of
tests/test_gpu_hnsw_ties.py against what they are for (tests/hnsw_tie_cases.py): each planted graph reaches the branch of
the tie list it was written for, and the random set reaches all of them."""
import numpy as np
import pytest

import bit_hnsw_model as bhm
import hnsw_tie_cases as tc
from bit_model import hamming
from hnsw_walk_model import walk
from oracle import pyoracle as po

OPS = {"l2": po.OPS_L2, "negip": po.OPS_IP, "l1": po.OPS_L1}


def model_of(case, ef=None, tie_cap=None):
    return walk(lambda e: case["dists"][e], case["levels"], case["nbr_start"], case["nbr"], case["m"], case["entry"],
                ef or case["ef"], tie_cap=tie_cap)


# ------------------------------------------------------------------------------------- the model's structure, tie-free
def test_model_equals_the_oracle_on_tie_free_data(oracle):
    """no two candidates equally far: the walk is determined, and the batch-at-a-time model must be the oracle's
    element-at-a-time walk -- ids, distances and scored, over several layers"""
    nq, n, nbits = 8, 500, 16000  # the draw of tests/test_bit_hnsw_model_cpu.py
    queries, rows = bhm.tie_free(nq, n, nbits, seed=5)
    g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, bhm.expand01(rows, nbits), m=5, ef_construction=32, seed=7)
    ex = g.export_tuples()
    assert len(ex["rows"]) == n and int(ex["levels"].max()) >= 2
    elements = rows[ex["rows"]]
    q01 = bhm.expand01(queries, nbits)
    for i in range(nq):
        d = hamming(queries[i], elements)
        assert len(set(d.tolist())) == n
        for ef, k in ((1, 1), (2, 2), (10, 10), (40, 10), (200, 200)):
            w = walk(lambda e: int(d[e]), ex["levels"], ex["nbr_start"], ex["nbr"], 5, ex["entry"], ef)
            want_rows, want_dist, want_scored = g.search(q01[i], ef, k)
            assert ex["rows"][w.ids[:k]].tolist() == want_rows.tolist(), (i, ef)
            assert [float(x) for x in w.dist[:k]] == want_dist.tolist(), (i, ef)
            assert w.scored == want_scored, (i, ef)
            assert w.counters["old_appends"] == w.counters["batch_appends"] == 0
    g.close()


# ------------------------------------------------------------------------------------------------ the planted graphs
@pytest.mark.parametrize("name", sorted(tc.planted()))
@pytest.mark.parametrize("metric", tc.METRICS)
def test_planted_answer_holds_for_model_and_oracle(oracle, name, metric):
    """the stated answer, up to the order inside a run of equal distances, from the model (unbounded T and T of ef
    entries: the same) and from the oracle's two heaps, whose tie order is another one"""
    case = tc.planted()[name]
    for cap in (None, case["ef"]):
        w = model_of(case, tie_cap=cap)
        tc.check_head(case, w.ids, w.dist, what="model %s" % name)
        assert w.scored == case["scored"] and w.counters["lost"] == 0
    g = po.HnswGraph.from_tuples(oracle, OPS[metric], po.ORA_F32, tc.planted_rows(case["dists"]), case["m"], case["levels"],
                                 case["nbr_start"], case["nbr"], case["entry"])
    ids, dist, scored = g.search(tc.planted_query(metric)[0], case["ef"], case["ef"])
    tc.check_head(case, ids, dist, what="oracle %s %s" % (name, metric))
    assert scored == case["scored"]
    assert not set(ids.tolist()) & set(case["unscored"])
    g.close()


def test_planted_cases_reach_what_they_are_for():
    p = {name: model_of(case).counters for name, case in tc.planted().items()}
    assert p["A"]["old_appends"] >= 1 and p["A"]["batch_appends"] == 0 and p["A"]["reads"] >= 1
    assert p["D"]["batch_appends"] >= 1 and p["D"]["old_appends"] == 0 and p["D"]["reads"] >= 1
    assert p["B"]["resets"] >= 1 and p["B"]["reads"] == 0      # a non-empty T dropped unread
    assert p["C"]["max_t"] == 70 and p["C"]["reads"] == 70
    assert p["E"]["old_appends"] == p["E"]["batch_appends"] == 0
    assert p["E2"]["batch_appends"] == 1 and p["E2"]["old_appends"] == 0
    for name in ("F1", "F2"):
        assert p[name]["old_appends"] == p[name]["batch_appends"] == 0


def test_planted_cases_catch_the_kernels_they_name():
    """the model with the defect each case is aimed at gives the wrong answer the case predicts"""
    cases = tc.planted()
    for name, wrong_ids in (("A", {3, 1}), ("D", {3, 1})):        # no tie list at all: {z, first of the 5s}
        w = model_of(cases[name], tie_cap=0)
        assert set(w.ids) == wrong_ids and w.scored == 4, name
    w = model_of(cases["C"], tie_cap=64)                            # 64 slots: c79 is lost, t never scored
    assert w.scored == 151 and 151 not in w.ids and w.counters["lost"] == 6


# --------------------------------------------------------------------------------------------------- the random set
@pytest.fixture(scope="module")
def random_runs(oracle):
    """every (form, query, ef) of the random set through the model, unbounded and with 64 slots"""
    runs = {}
    for form in tc.METRICS + ("bits",):
        _, _, ex, d = tc.random_graph(oracle, form)
        for q in range(tc.NQ):
            dq = d[q].tolist()
            for ef in tc.EFS:
                runs[form, q, ef] = tuple(walk(dq.__getitem__, ex["levels"], ex["nbr_start"], ex["nbr"], 8, ex["entry"], ef,
                                               tie_cap=cap) for cap in (None, 64))
    return runs


def test_random_set_reaches_every_branch_of_the_tie_list(random_runs):
    total = {}
    for (form, q, ef), (free, capped) in random_runs.items():
        for key, v in free.counters.items():
            total[form, key] = total.get((form, key), 0) + v
    for form in tc.METRICS + ("bits",):
        for key in ("old_appends", "batch_appends", "resets", "reads"):
            assert total[form, key] >= 1, (form, key)


def test_random_set_sixty_four_slots_against_unbounded(random_runs):
    """how often a T of 64 entries changed a walk: printed for profiles/r22_hnsw_tie_list.md, not asserted.  A T of ef entries
    never does: |T| < ef is asserted inside the unbounded model."""
    differ = {}
    for (form, q, ef), (free, capped) in random_runs.items():
        same = free.ids == capped.ids and free.dist == capped.dist and free.scored == capped.scored
        differ[form, ef] = differ.get((form, ef), 0) + (not same)
        assert same or ef > 64
    print("\n(form, ef): walks of %d that differ with 64 slots" % tc.NQ, {k: v for k, v in differ.items() if v},
          "; largest |T|", max(free.counters["max_t"] for free, _ in random_runs.values()))
