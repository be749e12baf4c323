"""numpy helpers of the sparse-HNSW tests (tests/test_sparse_hnsw_model_cpu.py, tests/test_gpu_sparse_hnsw.py) on top of
tests/sparse_model.py and tests/hnsw_walk_model.py: CSR generators, the dense expansion, a tie-free draw, random and
complete graphs, and a comparison of walk results up to the order inside runs of equal distances.

FUNCTION 1 of the four sparsevec opclasses returns the (double) of an fp32 sum (src/sparsevec.c:899, :965, :1059), and on
integer-valued data whose partial sums stay below 2^24 that sum is exact in any order.  So the oracle's walk over the
dense expansion (po.HnswGraph with OPS_L2 / OPS_IP / OPS_L1, ORA_F32) is the reference's walk under the sparsevec
opclasses, and sparse_model.distances gives the device's keys exactly."""
import numpy as np

import sparse_model as sm
from hnsw_walk_model import tuples

METRICS = (sm.L2SQ, sm.NEG_IP, sm.L1)
HNSW_MAX_NNZ = 1000     # src/hnsw.h:34
SPARSE_MAX_NNZ = 16000  # src/sparsevec.h:9


def draw_indices(rng, nnz, dim=None, pool=None):
    """nnz distinct ascending indices out of `pool` (an array of distinct indices) or out of 0 .. dim - 1"""
    if pool is not None:
        return np.sort(rng.choice(pool, nnz, replace=False)).astype(np.int32)
    if dim <= 1 << 22:
        return np.sort(rng.permutation(dim)[:nnz]).astype(np.int32)
    got = np.zeros(0, dtype=np.int64)
    while len(got) < nnz:
        got = np.unique(np.concatenate([got, rng.integers(0, dim, 2 * nnz)]))
    return np.sort(rng.permutation(got)[:nnz]).astype(np.int32)


def rand_csr(lengths, seed, dim=None, pool=None, floats=False, lo=-8, hi=8):
    """one vector per entry of `lengths`: integer values in lo .. hi without 0 (floats: standard normal) -> CSR"""
    rng = np.random.default_rng(seed)
    vectors = []
    for nnz in lengths:
        idx = draw_indices(rng, int(nnz), dim, pool)
        if floats:
            val = rng.standard_normal(int(nnz)).astype(np.float32)
        else:
            val = rng.integers(lo, hi, int(nnz))  # lo .. hi - 1; shift the non-negative ones up: no stored 0, hi included
            val = np.where(val >= 0, val + 1, val).astype(np.float32)
        vectors.append((idx, val))
    return sm.csr(vectors)


def expand_dense(csr, dim):
    """CSR -> float32 [n x dim]"""
    ptr, idx, val = csr
    out = np.zeros((len(ptr) - 1, dim), dtype=np.float32)
    out[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), idx] = val
    return out


def take(csr, rows):
    """the CSR of the given vectors, in that order"""
    return sm.csr([sm.vector(csr, int(r)) for r in rows])


def all_distances(metric, queries, rows):
    """[nq x n] float32 kernel values by sparse_model"""
    return np.stack([sm.distances(metric, sm.vector(queries, q), rows)[0] for q in range(len(queries[0]) - 1)])


def max_abs_sum(queries, rows):
    """the largest sum of |term| over every pair and metric: below 2^24 every partial sum of integer terms is exact in fp32"""
    worst = 0.0
    for metric in METRICS:
        for q in range(len(queries[0]) - 1):
            worst = max(worst, float(sm.distances(metric, sm.vector(queries, q), rows)[2].max(initial=0.0)))
    return worst


def _dense_int_distances(Q, E):
    """Q [nq x dim], E [c x dim] int64 -> {metric: [nq x c] int64}"""
    ip = Q @ E.T
    l2 = (Q * Q).sum(1)[:, None] + (E * E).sum(1)[None, :] - 2 * ip
    l1 = np.abs(Q[:, None, :] - E[None, :, :]).sum(-1)
    return {sm.L2SQ: l2, sm.NEG_IP: -ip, sm.L1: l1}


TIE_FREE = dict(nq=6, n=400, dim=2048, seed=11)  # the draw both test files use


def tie_free(nq, n, dim, seed):
    """(queries CSR, rows CSR), integer values in -8 .. 8, such that for every query and each of the three metrics its n
    distances to the rows are all distinct: rows of 1 .. 1000 stored elements are drawn 32 at a time and a row is kept only
    if, for every query and metric, its distance is new.  The queries store ~1500 elements (queries are not elements:
    HNSW_MAX_NNZ does not bind them), which spreads the inner products.  With no two candidates equally far a walk is
    determined, tie order and all."""
    rng = np.random.default_rng(seed)
    queries = rand_csr(rng.integers(1400, 1600, nq), seed + 1, dim=dim)
    Q = expand_dense(queries, dim).astype(np.int64)
    seen = {m: [set() for _ in range(nq)] for m in METRICS}
    kept, trip = [], 0
    while len(kept) < n:
        trip += 1
        batch = rand_csr(rng.integers(1, HNSW_MAX_NNZ + 1, 32), seed + 1000 + trip, dim=dim)
        d = _dense_int_distances(Q, expand_dense(batch, dim).astype(np.int64))
        for j in range(32):
            if len(kept) < n and not any(int(d[m][q, j]) in seen[m][q] for m in METRICS for q in range(nq)):
                for m in METRICS:
                    for q in range(nq):
                        seen[m][q].add(int(d[m][q, j]))
                kept.append(sm.vector(batch, j))
    return queries, sm.csr(kept)


TIED = dict(nq=48, n=3000, dim=1536, seed=13)


def tied(nq, n, dim, seed):
    """(queries CSR, rows CSR) on which most distances are shared: 2 .. 6 stored elements in {-1, 1, 2} out of 40 indices
    spread over the dimensions (the first and the last among them)"""
    rng = np.random.default_rng(seed)
    pool = np.unique(np.concatenate([[0, dim - 1], rng.permutation(dim)[:38]])).astype(np.int32)

    def draw(count, lo, hi, s):
        r = np.random.default_rng(s)
        return sm.csr([(draw_indices(r, int(k), pool=pool), r.choice(np.array([-1, 1, 2], dtype=np.float32), int(k)))
                       for k in r.integers(lo, hi + 1, count)])

    return draw(nq, 3, 8, seed + 1), draw(n, 2, 6, seed + 2)


def complete_graph(m):
    """bit_hnsw_model.complete_graph: one layer, n = 2 m + 1 elements, every tuple lists all the others, entry 0"""
    n = 2 * m + 1
    nbr = np.array([[j for j in range(n) if j != e] for e in range(n)], dtype=np.int32)
    return n, 0, np.zeros(n, dtype=np.int32), np.arange(n + 1, dtype=np.int64) * (2 * m), nbr.ravel()


def random_graph(n, m, seed):
    """any graph can be walked: levels geometric in 1 / m, every tuple of layer lc filled with distinct random elements of
    level >= lc, the entry point an element of the top level -> (m, entry, levels, nbr_start, nbr)"""
    rng = np.random.default_rng(seed)
    levels = np.minimum((-np.log(1.0 - rng.random(n)) / np.log(m)).astype(np.int32), 3)
    lists = {}
    for lc in range(int(levels.max()) + 1):
        members = np.flatnonzero(levels >= lc)
        lm = 2 * m if lc == 0 else m
        for e in members:
            others = members[members != e]
            lists[(int(e), lc)] = rng.choice(others, min(lm, len(others)), replace=False).tolist()
    levels, nbr_start, nbr = tuples(m, levels, lists)
    return m, int(np.flatnonzero(levels == levels.max())[0]), levels, nbr_start, nbr


def assert_topk_up_to_ties(elem, dist, d_all, k, what=""):
    """elem / dist [nq x k] against the k smallest of d_all [nq x n]: the distances equal exactly; the ids agree as SETS
    within each run of equal distances, the last run (cut by k) drawn from its tie class without repeats"""
    elem, dist = np.asarray(elem), np.asarray(dist)
    n = d_all.shape[1]
    for q in range(d_all.shape[0]):
        want = np.sort(d_all[q], kind="stable")[:k]
        got = elem[q][elem[q] >= 0]
        assert len(got) == min(k, n) and len(set(got.tolist())) == len(got), (what, q, "ids repeat or are missing")
        assert np.array_equal(dist[q][:len(got)], want), (what, q, "distances", dist[q].tolist(), want.tolist())
        assert np.array_equal(d_all[q][got], dist[q][:len(got)]), (what, q, "an element beside its distance")
        for v in np.unique(want):
            mine = set(got[dist[q][:len(got)] == v].tolist())
            tie_class = set(np.flatnonzero(d_all[q] == v).tolist())
            if v < want.max() or len(tie_class) == len(mine):
                assert mine == tie_class, (what, q, float(v))
            else:
                assert mine < tie_class, (what, q, float(v), "the run cut by k")
