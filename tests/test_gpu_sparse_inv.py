"""Inverted sparsevec rows on the device -- pgv_sparse_rows_upload / pgv_sparse_rows_topk (kernels_sparse_inv.hip) -- against
the float64 model tests/sparse_model.py and against pgv_sparse_topk(PGV_NEG_IP).

INTEGER values in -8 .. 8 (stored zeros among them) over a few dozen dimensions: every partial sum is an integer far below
2^24, so row ids and the BITS of the distances must equal the model's and the pair scan's; such data is full of ties, which
go to the lower row.  (The model negates a float64 sum, so its empty intersection is -0.0 where the library's contract is
+0.0: the model's values are compared as `value + 0.0`.)  The shapes stand at the edges of a row block (R rows) and of a
query tile (QT queries); k = n + 3 is capped at the entry's 4096.
FLOAT values: a distance lies within bound(S, m, 0) = (m + 2) 2^-24 S of the exact sum.  A returned row r outside the exact
top-k displaced a row x inside it, so computed(r) <= computed(x): exact(r) <= exact(k-th) + bound(r) + bound(x), checked
with the largest bound among the exact top-k for x."""
import numpy as np
import pytest

import sparse_model as sm
from pgvector_amd import _lib, api

pytestmark = pytest.mark.gpu

R, QT = _lib.SPARSE_INV_ROWS, _lib.SPARSE_INV_QUERIES
NQ = QT + 1


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def prefix(triple, n):
    ptr, idx, val = triple
    return ptr[:n + 1].copy(), idx[:ptr[n]].copy(), val[:ptr[n]].copy()


def to_device(triple):
    import torch
    return tuple(torch.from_numpy(x).cuda() for x in triple)


def int_case(dim, n):
    """-> (rows, NQ queries).  Dimensions in use: a small pool with 0 and dim - 1 in it, and three apart from it -- `every`
    (stored by every row of one block: the second where there is one), `straddle` (stored by the last row of block 0 and
    the first of block 1 only) and `ghost` (stored by query 0 and by no row).  Rows outside the `every` block store 0 .. 5
    pool dimensions, so some are empty; query 2 is empty"""
    rng = np.random.default_rng(dim % 1000 + n)
    dims = np.arange(dim) if dim == 7 else np.unique(np.concatenate([[0, dim - 1], rng.integers(0, dim, 30)]))
    every, straddle, ghost = (int(d) for d in rng.permutation(dims)[:3])
    pool = np.setdiff1d(dims, [every, straddle, ghost])
    every_block = 1 if n > R else 0

    def vec(extra, most):
        idx = np.concatenate([rng.choice(pool, rng.integers(0, most + 1), replace=False), extra]).astype(np.int32)
        return np.sort(idx), rng.integers(-8, 9, idx.size).astype(np.float32)
    rows = [vec([d for d, on in ((every, r // R == every_block), (straddle, n > R and r in (R - 1, R))) if on],
                min(5, pool.size)) for r in range(n)]
    queries = [vec([every, straddle, ghost] if q == 0 else [every, straddle][:q % 3], pool.size) for q in range(NQ)]
    queries[2] = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    return sm.csr(rows), sm.csr(queries)


@pytest.mark.parametrize("n", [1, R - 1, R, R + 1, 2 * R + 5])
@pytest.mark.parametrize("dim", [7, 30522, 10 ** 9])
def test_integer_data_equals_model_and_pair_scan(ctx, dim, n):
    """nq in {1, QT, QT + 1} x k in {1, 10, min(n + 3, 4096)} on one mirror: heads of fewer queries / smaller k are
    prefixes of the model's stable order, computed once"""
    rows, queries = int_case(dim, n)
    kmax = max(10, min(n + 3, 4096))
    wd, wi = sm.topk(sm.NEG_IP, queries, rows, kmax)[:2]
    pd, pi = api.sparse_topk(ctx, api.PGV_NEG_IP, dim, queries, rows, kmax)
    mirror = api.SparseRows(ctx, dim, rows)
    for nq in (1, QT, NQ):
        for k in (1, 10, min(n + 3, 4096)):
            dist, idx = mirror.topk(prefix(queries, nq), k)
            what = (dim, n, nq, k)
            assert dist.shape == idx.shape == (nq, k) and dist.dtype == np.float32 and idx.dtype == np.int64, what
            assert np.array_equal(idx, wi[:nq, :k]), (what, "rows", np.argwhere(idx != wi[:nq, :k])[:5].tolist())
            assert np.array_equal(bits(dist), bits(wd[:nq, :k] + np.float32(0))), (what, "model bits")
            assert np.array_equal(idx, pi[:nq, :k]) and np.array_equal(bits(dist), bits(pd[:nq, :k])), (what, "pair scan")
    mirror.free()


@pytest.fixture(scope="module")
def split_case(ctx):
    rows, queries = int_case(30522, R + 1)
    mirror = api.SparseRows(ctx, 30522, rows)
    yield rows, queries, mirror, mirror.topk(queries, 10)
    mirror.free()


def test_chunk_split(ctx, split_case, monkeypatch):
    """PGV_SPARSE_MATRIX_FLOATS at a third of the queries' worth of matrix: QT + 1 queries in three chunks, whose query
    tiles are counted from the chunk's first query; the unchunked answer bit for bit"""
    rows, queries, mirror, (dist, idx) = split_case
    per = -(-NQ // 3)
    assert -(-NQ // per) == 3
    monkeypatch.setenv("PGV_SPARSE_MATRIX_FLOATS", str(per * (R + 1)))
    got = mirror.topk(queries, 10)
    assert np.array_equal(got[1], idx) and np.array_equal(bits(got[0]), bits(dist))


def test_device_input_gives_the_same_bytes(ctx, split_case):
    rows, queries, _, (dist, idx) = split_case
    mirror = api.SparseRows(ctx, 30522, to_device(rows))
    got = mirror.topk(to_device(queries), 10)
    assert got[0].is_cuda and got[1].is_cuda
    assert np.array_equal(got[1].cpu().numpy(), idx) and np.array_equal(bits(got[0].cpu().numpy()), bits(dist))
    mirror.free()


def test_float_data_within_the_bound_and_repeatable(ctx):
    """n = 2R + 5 rows of about 40 normal values, QT + 1 queries of about 12, over 500 dimensions, k = 10"""
    rng = np.random.default_rng(7)

    def draw(count, nnz):
        return sm.csr([(np.sort(rng.choice(500, s, replace=False)).astype(np.int32), rng.standard_normal(s).astype(np.float32))
                       for s in rng.integers(nnz - nnz // 4, nnz + nnz // 4 + 1, count)])
    rows, queries, k = draw(2 * R + 5, 40), draw(NQ, 12), 10
    mirror = api.SparseRows(ctx, 500, rows)
    dist, idx = mirror.topk(queries, k)
    again = mirror.topk(queries, k)
    assert np.array_equal(bits(dist), bits(again[0])) and np.array_equal(idx, again[1])
    _, _, exact, S, m = sm.topk(sm.NEG_IP, queries, rows, k)
    tol = sm.bound(S, m, 0)
    for q in range(NQ):
        r = idx[q]
        assert len(set(r.tolist())) == k and (r >= 0).all() and (np.diff(dist[q]) >= 0).all(), q
        err = np.abs(dist[q].astype(np.float64) - exact[q][r])
        assert (err <= tol[q][r]).all(), (q, float(err.max()), float(tol[q][r].min()))
        best = np.argsort(exact[q], kind="stable")[:k]
        assert (exact[q][r] <= exact[q][best[-1]] + tol[q][r] + tol[q][best].max()).all(), q
    mirror.free()


def test_refusals(ctx):
    rows, queries = int_case(7, 5)
    mirror = api.SparseRows(ctx, 7, rows)

    def refused(code, text, call):
        with pytest.raises(api.PgvError) as e:
            call()
        assert e.value.code == code and text in e.value.message, e.value

    refused(api.PGV_ERR_ARG, "k 0", lambda: mirror.topk(queries, 0))
    refused(api.PGV_ERR_ARG, "k 4097", lambda: mirror.topk(queries, 4097))
    bad_ptr = rows[0].copy()
    bad_ptr[1] = bad_ptr[2] + 1
    refused(api.PGV_ERR_ARG, "ptr is not monotone at vector 1", lambda: api.SparseRows(ctx, 7, (bad_ptr, rows[1], rows[2])))
    one = (np.array([0, 1]), np.array([7]), np.array([1.0]))
    refused(api.PGV_ERR_ARG, "index 7 outside 0..6", lambda: mirror.topk(one, 1))
    big = (np.array([0, 16001]), np.arange(16001), np.ones(16001))
    refused(_lib.PGV_ERR_DIMS, "16001 stored elements", lambda: api.SparseRows(ctx, 20000, big))
    refused(_lib.PGV_ERR_DIMS, "16001 stored elements", lambda: mirror.topk(big, 1))
    assert mirror.topk(queries, 1)[1].shape == (NQ, 1)  # nothing was left behind
    mirror.free()
