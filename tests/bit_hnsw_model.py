"""numpy helpers of the bit-HNSW tests (tests/test_bit_hnsw_model_cpu.py, tests/test_gpu_bit_hnsw.py) on top of
tests/bit_model.py: the 0/1 expansion of packed bits, a tie-free data generator, one-layer complete graphs and a
comparison of walk results up to the order inside runs of equal distances."""
import numpy as np

from bit_model import hamming, hamming_topk


# ---------------------------------------------------------------------------------------------- HNSW over bit strings
# (tests/test_bit_hnsw_model_cpu.py, tests/test_gpu_bit_hnsw.py).  The Hamming distance of two bit strings is the squared
# L2 distance of their 0/1 expansions, a sum of at most 64 000 ones: exact in fp32 in any order.  So the oracle's walk over
# the expansion (po.HnswGraph with OPS_L2, ORA_F32) is the reference's walk under bit_hamming_ops.
def expand01(packed, nbits):
    """packed rows [n x (nbits + 7) // 8] uint8 -> their bits as float32 [n x nbits]"""
    return np.unpackbits(np.asarray(packed, dtype=np.uint8), axis=1)[:, :nbits].astype(np.float32)


def rand_bits(n, nbits, seed):
    """n packed bit strings of nbits, density 0.5 (first bit in the top bit of byte 0, pad bits zero)"""
    rng = np.random.default_rng(seed)
    return np.packbits(rng.integers(0, 2, (n, nbits), dtype=np.uint8), axis=1)


def tie_free(nq, n, nbits, seed):
    """(queries [nq x bytes], rows [n x bytes]) such that, for every query, its n distances to the rows are all distinct:
    rows of every density between 0.05 and 0.95 are drawn 64 at a time and a row is kept only if its distance to every
    query is new for that query.  With no two candidates equally far a walk is determined, tie order and all."""
    rng = np.random.default_rng(seed)
    nbytes = (nbits + 7) // 8

    def draw(c):
        p = rng.uniform(.05, .95, (c, 1))
        bits = rng.random((c, 8 * nbytes)) < p
        bits[:, nbits:] = 0
        return np.packbits(bits, axis=1)

    queries = draw(nq)
    seen = np.zeros((nq, 8 * nbytes + 1), dtype=bool)
    rows = []
    while len(rows) < n:
        batch = draw(64)
        d = np.stack([hamming(q, batch) for q in queries])  # [nq x 64]
        for j in range(64):
            if len(rows) < n and not seen[np.arange(nq), d[:, j]].any():
                seen[np.arange(nq), d[:, j]] = True
                rows.append(batch[j])
    return queries, np.stack(rows)


def complete_graph(m):
    """one layer, n = 2 m + 1 elements all at level 0, every tuple lists all the others in its 2 m layer-0 slots, entry 0
    -> (n, entry, levels, nbr_start, nbr) in pgv_hnsw_set_graph's layout"""
    n = 2 * m + 1
    nbr = np.array([[j for j in range(n) if j != e] for e in range(n)], dtype=np.int32)
    return n, 0, np.zeros(n, dtype=np.int32), np.arange(n + 1, dtype=np.int64) * (2 * m), nbr.ravel()


def assert_topk_up_to_ties(elem, dist, queries, rows, k, what=""):
    """elem / dist [nq x k] against hamming_topk(queries, rows, k): the distances equal exactly; the ids agree as SETS
    within each run of equal distances, the last run (cut by k) drawn from its tie class without repeats"""
    wd, _ = hamming_topk(queries, rows, k)
    elem, dist = np.asarray(elem), np.asarray(dist)
    assert np.array_equal(dist, wd), (what, "distances", np.argwhere(dist != wd)[:5].tolist())
    for q in range(queries.shape[0]):
        d_all = hamming(queries[q], rows)
        got = elem[q][elem[q] >= 0]
        assert len(got) == min(k, rows.shape[0]) and len(set(got.tolist())) == len(got), (what, q, "ids repeat or are missing")
        for v in np.unique(wd[q][np.isfinite(wd[q])]):
            mine = set(got[dist[q][:len(got)] == v].tolist())
            tie_class = set(np.flatnonzero(d_all == v).tolist())
            if v < wd[q][np.isfinite(wd[q])].max() or len(tie_class) == len(mine):
                assert mine == tie_class, (what, q, float(v))
            else:
                assert mine < tie_class, (what, q, float(v), "the run cut by k")
