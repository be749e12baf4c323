"""Pins tests/hnsw_repair_model.py -- the plain-Python restatement of hnswvacuum's repair that tests/test_gpu_hnsw_repair.py
compares the device against -- and asserts, on the same seeds, the preconditions those GPU tests rely on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_repair_model as rm  # noqa: E402
from hnsw_walk_model import tuples, walk  # noqa: E402


@pytest.fixture(autouse=True)
def no_ties():
    rm.TIES[0] = 0
    yield
    assert rm.TIES[0] == 0, "a distance tie decided something: the data of this test is not tie-free"


def test_without_dead_elements_the_search_is_the_walk_at_ef_plus_one():
    c = rm.make_case(rm.CASES[0])
    d = rm.sqdist(c["pts"])
    live = np.ones(rm.N, dtype=bool)
    m, efc = c["m"], c["efc"]
    found_self = 0
    for e in c["queries"][:10]:
        got = rm.find_neighbors(d, c["levels"], c["nbr_start"], c["nbr"], m, e, c["entry"], efc, live)
        w = walk(lambda x: d(e, x), c["levels"], c["nbr_start"], c["nbr"], m, c["entry"], efc + 1, qlevel=int(c["levels"][e]))
        assert w.counters["max_t"] == 0
        assert sorted(got) == sorted(w.layers)
        for lc, (ids, dist) in w.layers.items():
            lw = [(dd, x) for x, dd in zip(ids, dist) if x != e]
            found_self += e in ids
            assert got[lc] == rm.select_neighbors(lw, rm.layer_m(m, lc), d)
    assert found_self > 0, "the elements find themselves: that is what the + 1 is for"


@pytest.mark.parametrize("trap", rm.TRAPS, ids=lambda t: t.__name__)
def test_traps_where_truncating_to_ef_is_wrong(trap):
    (pts, live, levels, start, nbr), want = trap()
    d = rm.sqdist(pts)
    st = rm.new_stats()
    got = rm.find_neighbors(d, levels, start, nbr, 4, 0, 1, 4, live, st)
    assert sorted(x for x, _, _ in got[0]) == want
    assert [x for x, _, _ in got[0]] == sorted(want, key=lambda x: -d(0, x)), "<= lm candidates: furthest first"
    assert st["max_w"] > 5, "W grew past ef"
    trunc = rm.truncating_search(lambda x: d(0, x), levels, start, nbr, 4, 1, 5, live)
    assert sorted(x for x in trunc.ids if x != 0 and live[x]) != want, "the truncated merge must get this one wrong"


def line(m, positions, lists, dead=()):
    pts = np.zeros((len(positions), 8), dtype=np.int64)
    pts[:, 0] = positions
    live = np.ones(len(positions), dtype=bool)
    live[list(dead)] = False
    levels, start, nbr = tuples(m, [0] * len(positions), lists)
    return pts, live, levels, start, nbr


def owner_list(start, nbr, owner, lm):
    return nbr[int(start[owner]):int(start[owner]) + lm].tolist()


def test_back_link_takes_a_free_slot():
    pts, live, levels, start, nbr = line(2, [0, 1, 2, -3], {(0, 0): [1, 2]}, dead=[1])
    d = rm.sqdist(pts)
    assert rm.back_link(d, levels, start, nbr, 2, 0, 0, 3, 9, live)
    assert owner_list(start, nbr, 0, 4) == [1, 2, 3, -1], "a free slot wins over a dead member"


def test_back_link_replaces_the_first_dead_member():
    pts, live, levels, start, nbr = line(2, [0, 1, 2, 4, 8, -3], {(0, 0): [1, 2, 3, 4]}, dead=[2, 3])
    d = rm.sqdist(pts)
    assert rm.back_link(d, levels, start, nbr, 2, 0, 0, 5, 9, live)
    assert owner_list(start, nbr, 0, 4) == [1, 5, 3, 4]


def test_back_link_reselects_a_full_live_list():
    # owner at 0, members at 1 2 4 8, the newcomer at -3: the sweep keeps 1 and -3, refills with 2 and 4, prunes 8
    pts, live, levels, start, nbr = line(2, [0, 1, 2, 4, 8, -3, 20], {(0, 0): [1, 2, 3, 4]})
    d = rm.sqdist(pts)
    assert rm.update_index(d, 0, [1, 2, 3, 4], 4, 5, 9, live) == 3
    assert rm.back_link(d, levels, start, nbr, 2, 0, 0, 5, 9, live)
    assert owner_list(start, nbr, 0, 4) == [1, 2, 3, 5]
    # ... and a newcomer at 20 is itself the one pruned: nothing changes
    assert rm.update_index(d, 0, [1, 2, 3, 5], 4, 6, 400, live) == -1
    assert not rm.back_link(d, levels, start, nbr, 2, 0, 0, 6, 400, live)
    assert owner_list(start, nbr, 0, 4) == [1, 2, 3, 5]


def test_back_link_leaves_an_existing_connection():
    pts, live, levels, start, nbr = line(2, [0, 1, 2, 4, 8], {(0, 0): [1, 2, 3, 4]}, dead=[1])
    d = rm.sqdist(pts)
    assert not rm.back_link(d, levels, start, nbr, 2, 0, 0, 3, 16, live)
    assert owner_list(start, nbr, 0, 4) == [1, 2, 3, 4], "the dead member stays: the connection exists"


def small_graph(seed):
    pts = rm.int_points(80, 8, seed, 700)
    levels, start, nbr, entry = rm.knn_graph(pts, 4, seed)
    return pts, levels, start, nbr, entry


def test_a_dead_entry_point_is_replaced_by_the_highest_point():
    pts, levels, start, nbr, entry = small_graph(3)
    live = np.ones(80, dtype=bool)
    live[entry] = False
    live[np.random.RandomState(5).permutation(80)[:15]] = False
    highest, _ = rm.highest_points(levels, live)
    got, new_entry, cnt = rm.repair_graph(rm.sqdist(pts), levels, start, nbr, entry, live, 4, 8, 1)
    assert highest >= 0 and live[new_entry] and levels[new_entry] >= levels[highest]
    rm.check_invariants(levels, start, got, new_entry, live, 4)
    assert cnt["repaired"] > 0


def test_a_live_entry_point_with_a_dead_neighbour_is_repaired_in_place():
    pts, levels, start, nbr, entry = small_graph(4)
    live = np.ones(80, dtype=bool)
    first = int(nbr[int(start[entry])])
    live[first] = False
    got, new_entry, _ = rm.repair_graph(rm.sqdist(pts), levels, start, nbr, entry, live, 4, 8, 1)
    assert new_entry == entry
    assert first not in got[int(start[entry]):int(start[entry + 1])]
    rm.check_invariants(levels, start, got, new_entry, live, 4)


def test_when_the_highest_point_is_the_entry_the_fallback_serves():
    pts, levels, start, nbr, entry = small_graph(6)
    live = np.ones(80, dtype=bool)
    highest, fallback = rm.highest_points(levels, live)
    assert highest == entry and fallback >= 0 and fallback != entry, "knn_graph's entry is the first of the top level"
    victim = int(nbr[int(start[entry]) + int(levels[entry]) * 4])  # a layer-0 neighbour of the entry point
    live[victim] = False
    highest, fallback = rm.highest_points(levels, live)
    got, new_entry, _ = rm.repair_graph(rm.sqdist(pts), levels, start, nbr, entry, live, 4, 8, 1)
    assert new_entry == entry
    # the entry point was searched from the fallback point: its layer-0 list is full again and holds no dead element
    tup = got[int(start[entry]):int(start[entry + 1])]
    assert victim not in tup and tup[-1] >= 0
    rm.check_invariants(levels, start, got, new_entry, live, 4)


def test_everyone_dead_leaves_no_entry_point():
    pts, levels, start, nbr, entry = small_graph(3)
    live = np.zeros(80, dtype=bool)
    got, new_entry, cnt = rm.repair_graph(rm.sqdist(pts), levels, start, nbr, entry, live, 4, 8, 4)
    assert new_entry == -1 and cnt["repaired"] == 0 and (got == nbr).all()


@pytest.mark.parametrize("case", rm.CASES, ids=lambda c: c[0])
def test_preconditions_of_the_gpu_search_cases(case):
    """tie-free walks (the fixture), the plantings are what they claim, and no query needs more than the dead_cap the GPU
    test gives (the number of elements)"""
    c = rm.make_case(case)
    d = rm.sqdist(c["pts"])
    levels, start, nbr, live, m, efc = c["levels"], c["nbr_start"], c["nbr"], c["live"], c["m"], c["efc"]
    assert int(c["pts"].max()) <= 2048 and int(c["pts"].min()) >= -2048, "exact in fp16"
    assert c["dim"] * (2 * int(np.abs(c["pts"]).max())) ** 2 < 2 ** 24, "every distance exact in fp32"
    assert all(live[q] for q in c["queries"]) and live[c["entry"]]
    assert all(x < 0 or not live[x] for x in nbr[int(start[c["lonely"]]):int(start[c["lonely"] + 1])])
    assert levels[c["top"]] == levels.max() and levels[c["top"]] >= 1 and c["top"] != c["entry"]
    need = {q: rm.dead_cap_needed(d, levels, start, nbr, m, q, c["entry"], efc, live) for q in c["queries"]}
    print(case[0], "dead", int((~live).sum()), "needs", sorted(need.values())[-5:])
    assert need[c["centre"]] > 16, "the dead cluster makes W exceed ef by more than 16"
    assert max(need.values()) <= rm.N
    lonely = rm.find_neighbors(d, levels, start, nbr, m, c["lonely"], c["entry"], efc, live)
    assert len(lonely[0]) > 0, "an element all of whose neighbours are dead still finds live ones through them"


def test_preconditions_of_the_planted_overflow():
    c = rm.make_overflow_case()
    d = rm.sqdist(c["pts"])
    need = [rm.dead_cap_needed(d, c["levels"], c["nbr_start"], c["nbr"], c["m"], q, c["entry"], c["efc"], c["live"])
            for q in c["queries"]]
    print("overflow case needs", need)
    assert need[0] > c["dead_cap"], "the planted case really exceeds its dead_cap"
    assert max(need[1:]) <= c["dead_cap"], "no other query needs more than it is given"


@pytest.mark.parametrize("spec", rm.DRIVER_CASES, ids=lambda s: s[0])
@pytest.mark.parametrize("max_batch", [1, 7, 64])
def test_preconditions_of_the_gpu_driver_runs(max_batch, spec):
    """the whole-graph repairs the GPU driver tests compare against: tie-free (the fixture) and sound"""
    c = rm.make_case(spec)
    st = rm.new_stats()
    got, entry, cnt = rm.repair_graph(rm.sqdist(c["pts"]), c["levels"], c["nbr_start"], c["nbr"], c["entry"], c["live"],
                                      c["m"], c["efc"], max_batch, st)
    print("max_batch", max_batch, cnt, st)
    rm.check_invariants(c["levels"], c["nbr_start"], got, entry, c["live"], c["m"])
    assert cnt["repaired"] > 100 and cnt["reselections"] > 0
    assert st["max_over"] > 4, "the forced-small first dead_cap (4) of the redo test is really exceeded"
    if max_batch > 1:
        assert cnt["batches"] < cnt["repaired"]
