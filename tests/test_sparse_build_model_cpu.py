"""tests/sparse_build_model.py pinned on the CPU, the way bit_build_model.l2_functions is: over integer-valued sparse rows,
whose sums are exact in fp32 in any order, its functions make bit_build_model.build rebuild the oracle's dense squared-L2
graph of the rows' expansion.  And the two things the helper adds itself: the orientation of a pair and the byte-wise
duplicate check."""
import numpy as np

import bit_build_model as bm
import sparse_build_model as sbm
import sparse_hnsw_model as shm
import sparse_model as sm
from oracle import pyoracle as po


def test_the_sparse_functions_rebuild_the_oracles_dense_l2_graph(oracle):
    """n 600 rows of 4 .. 12 stored integers in -300 .. 300 over 64 dimensions, m 6, ef_construction 24, levels from the oracle: its entry
    point, and at least 0.99 of the neighbour tuples identical -- the share test_the_model_builds_the_oracles_graph grants
    l2_functions for the walk's tie order"""
    n, dim, m, efc = 600, 64, 6, 24
    rng = np.random.default_rng(5)
    csr = shm.rand_csr(rng.integers(4, 13, n), 501, dim=dim, lo=-300, hi=300)   # (sums below 2^24: exact; few equal distances)
    dense = shm.expand_dense(csr, dim)
    assert len(np.unique(dense, axis=0)) == n
    g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, dense, m=m, ef_construction=efc, seed=11)
    ex = g.export_tuples()
    g.close()
    assert np.array_equal(ex["rows"], np.arange(n))
    D = sbm.oriented_matrix(sbm.model_score(sm.L2SQ, csr), n)
    want = ((dense[:, None, :] - dense[None, :, :]) ** 2).sum(-1)
    assert np.array_equal(D, want.astype(np.float32))
    built = bm.build(ex["levels"], m, efc, *sbm.functions(D, csr))
    assert built["entry"] == ex["entry"] and built["nelements"] == n and built["mismatches"] == 0
    np.testing.assert_array_equal(built["nbr_start"], ex["nbr_start"])
    st = ex["nbr_start"]
    same = np.array([np.array_equal(built["nbr"][st[e]:st[e + 1]], ex["nbr"][st[e]:st[e + 1]]) for e in range(n)])
    print("identical neighbour tuples: %.4f" % same.mean())
    assert same.mean() >= 0.99, same.mean()


def test_the_matrix_asks_for_every_pair_once_smaller_slot_first():
    asked = []

    def score(a, b):
        asked.append((a.copy(), b.copy()))
        return (a * 10 + b).astype(np.float32)
    D = sbm.oriented_matrix(score, 5, chunk=4)
    a, b = np.concatenate([x for x, _ in asked]), np.concatenate([y for _, y in asked])
    assert (a <= b).all() and len(a) == 15 and len(set(zip(a.tolist(), b.tolist()))) == 15
    assert D[3, 1] == D[1, 3] == 13.0 and D[4, 4] == 44.0
    lo, hi = sbm.oriented_pairs([3, 1, 2], [1, 3, 2])
    assert lo.tolist() == [1, 1, 2] and hi.tolist() == [3, 3, 2]


def test_duplicates_are_equal_bytes():
    """the same number of stored elements, equal index bytes, equal value bytes: a stored -0.0 is not a stored 0.0, rows of
    different lengths differ whatever they expand to, two empty rows are equal"""
    csr = sm.csr([(np.array([1, 5], np.int32), np.array([1.0, 0.0], np.float32)),
                  (np.array([1, 5], np.int32), np.array([1.0, -0.0], np.float32)),
                  (np.array([1, 5], np.int32), np.array([1.0, 0.0], np.float32)),
                  (np.array([1], np.int32), np.array([1.0], np.float32)),
                  (np.array([1, 6], np.int32), np.array([1.0, 0.0], np.float32)),
                  (np.zeros(0, np.int32), np.zeros(0, np.float32)),
                  (np.zeros(0, np.int32), np.zeros(0, np.float32))])
    same = sbm.same_bytes(csr)
    assert same(0, 2) and same(2, 0) and same(5, 6) and same(3, 3)
    assert not same(0, 1) and not same(0, 3) and not same(0, 4) and not same(3, 5)
