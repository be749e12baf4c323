"""The yardsticks of tests/test_gpu_bit_hnsw.py, checked without a GPU: the oracle's HNSW walk over the 0/1 expansion of
bit strings (squared L2) returns their Hamming distances exactly -- so it is the reference's walk under bit_hamming_ops
(hamming_distance, src/bitvec.c:45-56) -- and the tie-free generator of tests/bit_hnsw_model.py keeps its promise."""
import ctypes

import numpy as np
import pytest

import bit_hnsw_model as bhm
import bit_model as bm
from oracle import pyoracle as po
from pgvector_amd import _lib, api

# the tie-free case of the GPU tests: n, nbits, queries, seed (levels reach 3; the oracle scores 71-83 elements at ef 40)
TIE_FREE = (8, 500, 16000, 5)


@pytest.fixture(scope="module")
def tie_free_case(oracle):
    nq, n, nbits, seed = TIE_FREE
    queries, rows = bhm.tie_free(nq, n, nbits, seed)
    g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, bhm.expand01(rows, nbits), m=8, ef_construction=32, seed=7)
    return queries, rows, nbits, g


@pytest.mark.parametrize("nbits", [1, 7, 64, 100, 129, 1536])
def test_oracle_walk_returns_hamming_distances(oracle, nbits):
    """every result of g.search on the 0/1 floats carries bit_model.hamming of the packed rows (tie-heavy data included)"""
    rows, queries = bhm.rand_bits(400, nbits, 3 + nbits), bhm.rand_bits(6, nbits, 4 + nbits)
    g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, bhm.expand01(rows, nbits), m=8, ef_construction=32, seed=1)
    q01 = bhm.expand01(queries, nbits)
    for i in range(6):
        ids, dist, scored = g.search(q01[i], 40, 10)
        assert len(ids) == 10 and scored >= 10
        assert np.array_equal(dist, bm.hamming(queries[i], rows[ids]).astype(np.float64)), (nbits, i)
        assert (np.diff(dist) >= 0).all()


def test_tie_free_generator_keeps_its_promise(tie_free_case):
    queries, rows, nbits, _ = tie_free_case
    assert rows.shape == (500, 2000) and queries.shape == (8, 2000)
    for q in queries:
        assert len(np.unique(bm.hamming(q, rows))) == len(rows)
    assert not (rows[:, -1] & ((1 << (-nbits % 8)) - 1)).any()


def test_oracle_walk_on_tie_free_data_is_exact(tie_free_case):
    """on the tie-free case the oracle's distances are the Hamming distances, its graph has upper layers, and its walk
    scores far fewer elements than there are: the GPU test compares a real multi-layer walk, not a scan"""
    queries, rows, nbits, g = tie_free_case
    ex = g.export_tuples()
    assert int(ex["levels"].max()) >= 2
    q01 = bhm.expand01(queries, nbits)
    for i in range(len(queries)):
        ids, dist, scored = g.search(q01[i], 40, 10)
        assert np.array_equal(dist, bm.hamming(queries[i], rows[ids]).astype(np.float64))
        assert len(np.unique(dist)) == 10 and 40 <= scored < len(rows) // 2
        ids1, dist1, scored1 = g.search(q01[i], 1, 1)
        assert len(ids1) == 1 and dist1[0] == bm.hamming(queries[i], rows[ids1])[0]


def test_model_helpers():
    n, entry, levels, nbr_start, nbr = bhm.complete_graph(8)
    assert (n, entry) == (17, 0) and nbr_start[-1] == len(nbr) == 17 * 16 and not levels.any()
    for e in range(n):
        assert sorted(nbr[nbr_start[e]:nbr_start[e + 1]].tolist()) == [j for j in range(n) if j != e]
    rows = np.zeros((6, 2), dtype=np.uint8)
    rows[4, 0] = 0x80
    q = np.zeros((1, 2), dtype=np.uint8)
    wd, wi = bm.hamming_topk(q, rows, 3)
    bhm.assert_topk_up_to_ties(np.array([[5, 2, 0]]), wd, q, rows, 3)           # any three of the five zeros
    bhm.assert_topk_up_to_ties(np.array([[5, 2, 0, 1, 3, 4]]), bm.hamming_topk(q, rows, 6)[0], q, rows, 6)
    with pytest.raises(AssertionError):
        bhm.assert_topk_up_to_ties(np.array([[5, 4, 0]]), wd, q, rows, 3)       # row 4 is not at distance 0
    with pytest.raises(AssertionError):
        bhm.assert_topk_up_to_ties(np.array([[5, 5, 0]]), wd, q, rows, 3)       # a repeat
    assert np.array_equal(bhm.expand01(np.array([[0xA0]], dtype=np.uint8), 3), [[1, 0, 1]])


def test_library_and_api_have_the_bit_hnsw_entries():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "pgv_hnsw_upload_bits"), "libpgv_hip.so does not export pgv_hnsw_upload_bits"
    assert "pgv_hnsw_upload_bits" in _lib.SYMBOLS
    for name in ("search", "score", "set_graph", "update_graph", "get_payload", "export", "close"):
        assert callable(getattr(api.BitHnsw, name, None)), "api.BitHnsw has no %s" % name
    assert callable(getattr(api, "binary_search_hnsw", None))
