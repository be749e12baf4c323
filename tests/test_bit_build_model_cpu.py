"""tests/bit_build_model.py pinned on the CPU: to the oracle's build where the oracle has one (squared L2 on an integer
grid), and on hand-made Jaccard cases to the three things a build under bit_jaccard_ops adds -- W in the float8's order,
lists in floats, `<=` between two floats that two different float8 values rounded to."""
from fractions import Fraction

import numpy as np

import bit_build_model as bm
import jaccard_model as jm
from helpers import gen
from hnsw_walk_model import tuples
from oracle import pyoracle as po


def test_the_model_builds_the_oracles_graph(oracle):
    """the data of test_hnsw_build_serial_is_the_reference_loop (n 1200, dim 8, int10, seed 401, m 6, ef_construction 24,
    oracle seed 11), levels from the oracle: the oracle's entry point, and at least 0.99 of the neighbour tuples identical
    -- the share that test grants the device on this data for the walk's tie order"""
    n, dim, m, efc = 1200, 8, 6, 24
    data = gen(n, dim, seed=401, dist="int10")
    g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, data, m=m, ef_construction=efc, seed=11)
    ex = g.export_tuples()
    assert np.array_equal(ex["rows"], np.arange(n))
    built = bm.build(ex["levels"], m, efc, *bm.l2_functions(data))
    assert built["entry"] == ex["entry"] and built["nelements"] == n and built["mismatches"] == 0
    np.testing.assert_array_equal(built["nbr_start"], ex["nbr_start"])
    st = ex["nbr_start"]
    same = np.array([np.array_equal(built["nbr"][st[e]:st[e + 1]], ex["nbr"][st[e]:st[e + 1]]) for e in range(n)])
    print("identical neighbour tuples: %.4f" % same.mean())
    assert same.mean() >= 0.99, same.mean()


def _merged_pairs(count):
    """Farey neighbours p < q (ratios >= 1 / 2) that round to ONE float: different float8 values, equal floats"""
    found = sorted((pr for pr in jm.farey_pairs(lo=63900, least=Fraction(1, 2))
                    if jm.fp32_key(*pr[0]) == jm.fp32_key(*pr[1]) and jm.fraction(*pr[1]) < Fraction(9, 10)),
                   key=lambda pr: jm.fraction(*pr[0]))
    out = []
    for p, q in found:   # apart from each other: every next pair lies wholly beyond the one before
        if not out or jm.ref_float(*p) > jm.ref_float(*out[-1][1]):
            out.append((p, q))
    assert len(out) >= count
    for p, q in out[:count]:
        assert jm.ref_double(*p) < jm.ref_double(*q) and jm.ref_float(*p) == jm.ref_float(*q)
    return out[:count]


def test_w_is_ordered_by_the_fraction_and_lists_hold_floats():
    """element 4 is inserted into a one-layer graph 0 - 1 - 2 - 3 whose elements are at q, p, q', p' from it (two merged
    pairs, the farther of each met first): W comes back p, q, p', q' -- the Fractions' order, which a walk ranking by floats
    would leave in batch order -- its distances are the floats, equal inside each pair, and the list, taken whole, is W
    backwards"""
    (p, q), (p2, q2) = _merged_pairs(2)
    assert jm.fraction(*q) < jm.fraction(*p2)
    xu = {(0, 4): q, (1, 4): p, (2, 4): q2, (3, 4): p2, (0, 1): (1, 3), (1, 2): (1, 3), (2, 3): (1, 3)}
    key, value, pair, same = bm.table_functions(xu)
    m = 2
    levels, nbr_start, nbr = tuples(m, [0] * 5, {(0, 0): [1, 2, 3], (1, 0): [0, 2], (2, 0): [1, 3], (3, 0): [2]})
    f = bm.find_neighbors(4, 0, levels, nbr_start, nbr, m, 0, 4, key, value, pair)[0]
    assert f["w"] == [1, 0, 3, 2]
    assert f["keys"] == sorted(f["keys"]) and len(set(f["keys"])) == 4
    assert f["dist"].dtype == np.float32 and f["dist"][0] == f["dist"][1] and f["dist"][2] == f["dist"][3]
    assert f["dist"].tolist() == [float(jm.ref_float(*x)) for x in (p, q, p2, q2)]
    assert f["ids"] == [2, 3, 0, 1] and f["closer"] == [0, 0, 0, 0]


def test_selection_compares_floats_with_less_or_equal():
    """CheckElementCloser (src/hnswutils.c:1040-1059) on floats: candidate B is at p from the new element and at q from
    the chosen A, p < q as float8 values and equal as floats -- `distance <= e->distance` holds and B is NOT closer; the
    float8 values would have accepted it.  The other way round (B at q, p from A) is not closer either way."""
    (p, q), = _merged_pairs(1)
    near, far = (1, 4), (63000, 64000)
    # elements: 0 = A, 1 = B, 2 = C, 3..5 fill layer 0 so that the list is thinned (5 candidates > 2 m = 4); 6 is new
    for b_to_new, b_to_a in ((p, q), (q, p)):
        xu = {(0, 6): near, (1, 6): b_to_new, (2, 6): (60000, 64000), (3, 6): far, (4, 6): (63001, 64000),
              (0, 1): b_to_a}
        key, value, pair, same = bm.table_functions(xu)
        m = 2
        levels, nbr_start, nbr = tuples(m, [0] * 7, {(0, 0): [1, 2, 3, 4], (1, 0): [0], (2, 0): [0], (3, 0): [0], (4, 0): [0]})
        f = bm.find_neighbors(6, 0, levels, nbr_start, nbr, m, 0, 8, key, value, pair)[0]
        assert f["w"] == [0, 1, 2, 3, 4]
        # A, C, then 3 and 4 are closer (everything else is disjoint: 1.0 apart); B is rejected and not needed as a filler
        assert f["ids"] == [0, 2, 3, 4] and f["closer"] == [1, 1, 1, 1], (b_to_new, f)
        # ... and by the float8 values B would have been taken in the first case
        wide = [key(1, 0) > key(6, 1)]
        assert wide == [b_to_new == p]


def test_a_serial_jaccard_build_of_the_model_keeps_its_invariants():
    """n 120, nbits 64, m 4, ef_construction 12 with three all-zero rows (1.0 from everything, each other included) and
    five copies of one row: no self loops, no repeats, neighbours linked and at or above the layer, the cached and the
    recomputed SelectNeighbors agree on every update, the copies share one element, the zero rows merge only where the
    loop meets one first in a list"""
    rng = np.random.default_rng(7)
    n, nbits, m, efc = 120, 64, 4, 12
    rows = np.packbits(rng.random((n, nbits)) < rng.uniform(.2, .8, (n, 1)), axis=1)
    rows[[20, 50, 90]] = 0
    rows[[30, 31, 60, 61, 99]] = rows[5]
    levels = np.minimum((-np.log(rng.random(n)) / np.log(m)).astype(np.int32), 3)
    b = bm.build(levels, m, efc, *bm.jaccard_functions(rows))
    assert b["mismatches"] == 0 and b["nelements"] + int((b["dup_of"] >= 0).sum()) == n
    assert (b["dup_of"][[30, 31, 60, 61, 99]] >= 0).all()
    for r in np.flatnonzero(b["dup_of"] >= 0):
        assert np.array_equal(rows[r], rows[b["dup_of"][r]]) and b["dup_of"][b["dup_of"][r]] < 0
    st, nb = b["nbr_start"], b["nbr"]
    for e in range(n):
        for lc in range(levels[e] + 1):
            o = st[e] + (levels[e] - lc) * m
            ids = nb[o:o + (2 * m if lc == 0 else m)]
            ids = ids[ids >= 0]
            assert len(set(ids.tolist())) == len(ids) and e not in ids
            assert (levels[ids] >= lc).all() and (b["dup_of"][ids] < 0).all()
            if b["dup_of"][e] >= 0:
                assert len(ids) == 0
