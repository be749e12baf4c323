"""tests/hnsw_link_model.py held to the oracle and to itself, on the CPU: the model is what the device's graph updates are
compared with (tests/test_gpu_hnsw_link_edges.py), so here
  - link_batch's graphs equal the oracle's HnswUpdateConnection (ora_hnsw_update_connections / ora_hnsw_set_neighbors on a
    graph imported empty), tuple for tuple, on every scenario and on a fuzz;
  - the reference's cached form of SelectNeighbors (select_cached) and Algorithm 4 with every flag recomputed
    (select_recompute) give the same list, flags and pruned item after every single update;
  - every scenario crosses the edge it was made for (the conditions of its row in the table of the GPU test's docstring)."""
import numpy as np
import pytest

import hnsw_link_model as hm
from oracle import pyoracle as po


def oracle_tuples(oracle, sc):
    """the scenario through the oracle's update_connection, requests in the reference's order"""
    levels, m = sc["levels"], sc["m"]
    start = np.zeros(len(levels) + 1, np.int64)
    start[1:] = np.cumsum((levels.astype(np.int64) + 2) * m)
    g = po.HnswGraph.from_tuples(oracle, po.OPS_IP if sc["metric"] == hm.IP else po.OPS_L2, po.ORA_F32, sc["rows"], m, levels,
                                 start, np.full(int(start[-1]), -1, np.int32), 0)
    for b in sc["batches"]:
        owner, lc, new, dist = hm.requests_of(b, levels)
        if len(owner):
            g.update_connections(owner, lc, new, dist)
        for q, e in enumerate(b["elements"]):
            if b["linked"][q]:
                for lc in range(min(int(levels[e]), b["lcap"] - 1) + 1):
                    n = int(b["sel_cnt"][q, lc])
                    g.set_neighbors(e, lc, b["sel_ids"][q, lc, :n], b["sel_dist"][q, lc, :n])
    nbr = g.export_tuples()["nbr"]
    g.close()
    return nbr


_RUNS = {}


def run(name):
    if name not in _RUNS:
        sc = hm.all_scenarios()[name]()
        g = hm.Graph(sc["rows"], sc["metric"], sc["m"], sc["levels"])
        st = []
        for k, b in enumerate(sc["batches"]):
            if name == "wide" and k == 3:                 # the crafted lists as the last batch meets them
                g.before_last = {o: (list(g.lists[(o, 0)].elem), list(g.lists[(o, 0)].dist), list(g.lists[(o, 0)].cf),
                                     g.lists[(o, 0)].closer_set) for o in hm.WIDE_SPECIAL}
            st.append(hm.link_batch(g, b))
        _RUNS[name] = (sc, g, st)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(hm.all_scenarios()))
def test_the_model_is_the_oracle_and_both_selections_agree(oracle, name):
    sc, g, st = run(name)
    assert not any(e["mismatch"] for e in g.events)
    np.testing.assert_array_equal(g.tuples()[1], oracle_tuples(oracle, sc))
    # the distances the batches carry are the oracle's
    b = sc["batches"][-1]
    q = int(np.flatnonzero(b["linked"])[0])
    for i in range(int(b["sel_cnt"][q, 0])):
        a, c = sc["rows"][b["elements"][q]], sc["rows"][b["sel_ids"][q, 0, i]]
        want = oracle.lib.ora_index_distance(po.OPS_IP if sc["metric"] == hm.IP else po.OPS_L2, po.ORA_F32, len(a),
                                             po._p(np.ascontiguousarray(a)), po._p(np.ascontiguousarray(c)))
        assert np.float32(want) == b["sel_dist"][q, 0, i]
    assert np.abs(sc["rows"]).max() <= 16 and sc["rows"].shape[1] <= 8 and sc["rows"].shape[0] <= 8000
    assert (sc["rows"] == np.round(sc["rows"])).all()


def test_fuzz_cached_and_recomputed_selection_and_the_oracle(oracle):
    """>= 2 000 overflowing updates over integer grids, m in {2, 4, 16}"""
    total = cached = 0
    for seed, m in enumerate([2, 2, 4, 4, 16, 16]):
        metric = hm.IP if seed % 2 else hm.L2
        n = 260 if m < 16 else 420
        lv = np.minimum(np.random.default_rng(seed).geometric(0.6, n) - 1, 2)
        sc = hm.random_scenario("fuzz", 900 + seed, n, 2 + seed % 3, 3 + seed, m, metric, lv,
                                (n // 5, n // 5, n // 5, n // 5, n - 4 * (n // 5)), ncand=4 * m, dup=20, unlinked=6)
        g, st = hm.run_model(sc)
        assert not any(e["mismatch"] for e in g.events), (seed, m)
        np.testing.assert_array_equal(g.tuples()[1], oracle_tuples(oracle, sc))
        total += len(g.events)
        cached += sum(e["closer_set"] for e in g.events)
    assert total >= 2000 and cached >= 500, (total, cached)


def test_hub_fills_and_overflows_inside_one_batch():
    sc, g, st = run("hub")
    ev = [e for e in g.events if (e["owner"], e["lc"]) == (0, 0)]
    assert len(ev) >= 150
    assert any(e["new_pruned"] for e in ev) and any(not e["new_pruned"] for e in ev)
    # batch 3 (40 newcomers) meets the list with 4 of its 8 places taken
    assert sc["batches"][3]["elements"].size == 40 and any(e["batch"] == 4 for e in ev)
    g2 = hm.Graph(sc["rows"], sc["metric"], sc["m"], sc["levels"])
    for b in sc["batches"][:3]:
        hm.link_batch(g2, b)
    assert 0 < len(g2.lists[(0, 0)].elem) < 8
    assert any((np.diff(b["elements"]) < 0).any() for b in sc["batches"])          # handed over out of heap order


@pytest.mark.parametrize("m", [4, 8])
def test_ties_are_met(m):
    sc, g, st = run("ties_m%d" % m)
    assert sum(e["tie_split"] for e in g.events) >= 50
    assert sum(e["equal_pair"] for e in g.events) >= 50
    assert any((b["linked"] == 0).any() for b in sc["batches"])
    assert len(np.unique(sc["rows"], axis=0)) < len(sc["rows"])


def test_cache_scenario_reuses_flags_and_defers():
    sc, g, st = run("cache")
    assert sum(e["removed_readded"] for e in g.events) >= 30
    assert sum(s["deferred_in_order"] for s in st) >= 10 and sum(s["deferred_any"] for s in st) >= 10
    assert sum(s["deferred_any"] for s in st) > sum(s["deferred_in_order"] for s in st)     # the two verdicts differ somewhere


def test_layers_overflow_on_every_kind_of_list():
    sc, g, st = run("layers")
    assert any(e["lc"] == 0 for e in g.events) and any(e["lc"] > 0 for e in g.events)
    assert max(e["lc"] for e in g.events) >= 2
    assert all(b["lcap"] == 4 for b in sc["batches"]) and (sc["levels"] < 3).any() and sc["levels"].max() == 3
    assert len({int(sc["levels"][e["owner"]]) for e in g.events}) >= 3                      # owners of differing level


@pytest.mark.parametrize("m", [16, 31, 32])
def test_lanes_lists_are_exactly_full_then_overflow(m):
    sc, g, st = run("lanes_m%d" % m)
    assert st[1]["pairs"] == 0 and all(len(g.lists[(o, 0)].elem) == 2 * m for o in range(20))
    assert st[2]["pairs"] == 20 * hm.group_pairs(2 * m + 10, 1) and st[3]["pairs"] == 20 * hm.group_pairs(2 * m + 5, 2 * m)
    assert sum(not e["closer_set"] for e in g.events) >= 20 and sum(e["closer_set"] for e in g.events) >= 20


def test_tri_cap_records_sit_round_1024_pairs():
    got = set()
    for m in (22, 23):
        sc, g, st = run("tri_cap_m%d" % m)
        assert st[2]["pairs"] == 6 * hm.group_pairs(2 * m + 2, 1) + 6 * hm.group_pairs(2 * m + 1, 1)
        got |= {hm.group_pairs(2 * m + 1, 1), hm.group_pairs(2 * m + 2, 1)}
    assert {990, 1035, 1081} <= got


def test_wide_takes_the_synchronous_second_round():
    sc, g, st = run("wide")
    for s in st[2:]:
        assert s["nrec"] > 6744 and s["nrec"] * 19900 * 4 > 512 << 20
    assert st[3]["deferred_in_order"] >= 1
    assert any(e["pruned"] >= 128 and not e["new_pruned"] for e in g.events)


def test_wide_has_lists_whose_pruned_item_is_the_second_rounds_decision():
    """the crafted lists: in the last batch they wait for their member triangle, and the item they drop depends on the
    member-member distances -- read as 0 (a triangle that was never written, or written elsewhere) another item goes"""
    sc, g, st = run("wide")
    last, lm, differ = sc["batches"][3], 200, 0
    for owner in hm.WIDE_SPECIAL:
        l_elem, l_dist, l_cf, l_set = g.before_last[owner]
        assert l_set and len(l_elem) == lm
        q, i = [(q, i) for q in range(36) for i in range(lm) if last["sel_ids"][q, 0, i] == owner][0]
        elem = l_elem + [int(last["elements"][q])]
        dist = np.asarray(l_dist + [float(last["sel_dist"][q, 0, i])], np.float32)
        D = hm.pair_matrix(sc["rows"], sc["metric"], elem)
        true = hm.select_cached(elem, dist, D, lm, l_cf + [0], True, list(range(lm + 1)), lm)
        assert true["wait_in_order"] and true["wait_any"] and true["readded"]
        wrong = D.copy()
        wrong[:lm, :lm] = 0
        other = hm.select_cached(elem, dist, wrong, lm, l_cf + [0], True, list(range(lm + 1)), lm)
        differ += true["pruned"] != other["pruned"]
        # and the model's graph holds the true decision: the newcomer where the pruned item was
        assert g.lists[(owner, 0)].elem[true["pruned"]] == elem[lm] and true["pruned"] != lm
    assert differ == len(hm.WIDE_SPECIAL)


@pytest.mark.parametrize("nlists", [4095, 4096, 4097])
def test_scan_record_counts(nlists):
    sc, g, st = run("scan_%d" % nlists)
    assert st[1]["nrec"] == nlists and st[2]["nrec"] == nlists and st[2]["pairs"] == 8 * hm.group_pairs(10, 1)


@pytest.mark.parametrize("name", ["hub_ip", "cache_ip", "hub_ip_f16", "cache_ip_f16"])
def test_types_mix_signs(name):
    sc, g, st = run(name)
    assert sum(e["mixed_signs"] for e in g.events) >= 30
    d = np.concatenate([b["sel_dist"][b["sel_cnt"] > 0].ravel() for b in sc["batches"] if (b["sel_cnt"] > 0).any()])
    assert (d < 0).any() and (d > 0).any()
