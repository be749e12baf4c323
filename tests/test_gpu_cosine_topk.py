"""pgv_cosine_topk (cosine_tile_kernel, the float selection over its truncated keys, the refine and finish kernels)
against numpy float64.  The data are small integers, so the three fp32 sums are exact and numpy's
1 - clip(ip / sqrt(na * nb)) IS the reference's float8: indexes are compared as lists, distances by their bit patterns."""
import numpy as np
import pytest

from pgvector_amd import api

pytestmark = pytest.mark.gpu


def distances(queries, rows):
    q, x = queries.astype(np.float64), rows.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1.0 - np.clip((q @ x.T) / np.sqrt(np.outer((q * q).sum(1), (x * x).sum(1))), -1.0, 1.0)


def model(queries, rows, k):
    """each query's rows by (float8, index), NaN behind the numbers (a stable sort does both), +inf / -1 behind those"""
    nq, n = queries.shape[0], rows.shape[0]
    dist, idx = np.full((nq, k), np.inf), np.full((nq, k), -1, dtype=np.int64)
    if n:
        d = distances(queries, rows)
        order = np.argsort(d, axis=1, kind="stable")[:, :k]
        dist[:, :order.shape[1]], idx[:, :order.shape[1]] = np.take_along_axis(d, order, 1), order
    return dist, idx


def check(got, want, what):
    (dist, idx), (wd, wi) = got, want
    assert idx.tolist() == wi.tolist(), (what, "indexes", np.argwhere(idx != wi)[:5].tolist())
    nan = np.isnan(wd)
    assert np.array_equal(np.isnan(dist), nan), (what, "NaN")
    assert np.array_equal(dist[~nan].view(np.uint64), wd[~nan].view(np.uint64)), (what, "distances")


def integers(shape, seed, dtype):
    return np.random.default_rng(seed).integers(-8, 9, shape).astype(dtype)


# every dim (a partial 16-byte vector, a partial 128-byte slice, odd and even slice counts), nq and n (the 128 x 128 tile;
# 1025 rows are nine row tiles, one past a round of the XCDs) appears; k is 1, 10 or n + 3 (the padding).  From six rows
# on there are a zero row, two identical rows and a positive multiple of query 0 (distance exactly 0); the last query is
# zero: NaN sorts behind the numbers in index order and before the padding.  dim 1 has only 0, 2 and NaN: long ties
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype,dim,nq,n,k", [
    (np.float32, 1, 1, 1, 1), (np.float16, 3, 127, 127, 10), (np.float32, 31, 128, 129, 132), (np.float16, 32, 129, 1025, 10),
    (np.float32, 33, 129, 1025, 1028), (np.float16, 64, 1, 129, 1), (np.float32, 257, 128, 127, 10),
    (np.float16, 257, 127, 1025, 1), (np.float32, 64, 129, 1, 4), (np.float16, 1, 129, 1025, 10), (np.float32, 3, 1, 127, 130),
    (np.float16, 31, 128, 129, 10), (np.float32, 32, 127, 1025, 10), (np.float16, 33, 1, 1025, 1028)])
def test_integer_data_bit_for_bit(ctx, dtype, dim, nq, n, k, device):
    rows, queries = integers((n, dim), 100 + dim + n, dtype), integers((nq, dim), 200 + dim + nq, dtype)
    if n >= 6:
        rows[2] = 0
        rows[4] = rows[3]
        rows[5] = 3 * queries[0]
    if nq > 1:
        queries[-1] = 0
    want = model(queries, rows, k)
    if device:
        import torch
        dist, idx = api.cosine_topk(ctx, torch.from_numpy(queries).cuda(), torch.from_numpy(rows).cuda(), k)
        ctx.sync()
        check((dist.cpu().numpy(), idx.cpu().numpy()), want, (dim, nq, n, k))
    else:
        check(api.cosine_topk(ctx, queries, rows, k), want, (dim, nq, n, k))


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_tie_class_at_zero_crosses_the_boundary(ctx, dtype):
    """more than k + 1 rows that are the query or a positive multiple of it: all clamp to exactly 0, the refine path has to
    keep them in index order"""
    rows, queries = integers((400, 24), 1, dtype), integers((3, 24), 2, dtype)
    at = np.random.default_rng(3).permutation(400)[:30]
    rows[at] = queries[1] * np.array([1, 2, 3], dtype=dtype)[np.arange(30) % 3, None]
    want = model(queries, rows, 10)
    assert want[1][1].tolist() == sorted(at)[:10] and not want[0][1].any()
    check(api.cosine_topk(ctx, queries, rows, 10), want, "multiples")


def four_squares(t):
    return next((a, b, c, d) for a in range(7) for b in range(7) for c in range(7) for d in range(7)
                if a * a + b * b + c * c + d * d == t)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_float8_trap(ctx, dtype):
    """query e_0, rows (2000, y) with sum(y^2) = 12 000 000 + t, t = 0 .. 39, shuffled among ordinary rows: the values
    1 - 2000 / sqrt(16 000 000 + t) are distinct doubles near 0.5 (every sum <= 2^24: exact), several to one float.  The
    boundary is put INSIDE a float class of three distinct doubles: ordering by any 32-bit float fails here"""
    n, dim = 300, 8
    rows, query = integers((n, dim), 11, dtype), np.zeros((1, dim), dtype)
    query[0, 0] = 1
    at = np.random.default_rng(12).permutation(n)[:40]
    for t, r in enumerate(at):
        rows[r] = (2000, 2000, 2000, 2000) + four_squares(t)
    d = distances(query, rows)[0]
    order = np.argsort(d, kind="stable")
    keys = d[order].view(np.uint64) >> np.uint64(29)  # the truncated float of a double in [2^-53, 2]
    j = next(j for j in range(n - 2) if keys[j] == keys[j + 2] and d[order[j]] < d[order[j + 1]] < d[order[j + 2]])
    assert sorted(order[j:j + 3]) != order[j:j + 3].tolist()  # ... and ties by index would answer another order
    for k in (j + 2, 4):
        check(api.cosine_topk(ctx, query, rows, k), model(query, rows, k), ("trap", k))


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("n,at", [(3, (0, 2)), (4096, (4093, 4094, 4095))])
def test_selection_of_every_row_still_drops_the_right_one(ctx, dtype, n, at):
    """n == k + 1: the selection of k + 1 holds every row, ordered by its float keys.  Every row is the query (distance 0)
    but the trap rows at `at`, one float class near 0.5 whose doubles FALL as the index grows: the row to drop is the
    class's lowest index, the one a tie by index keeps"""
    rows, query = np.zeros((n, 8), dtype), np.zeros((1, 8), dtype)
    query[0, 0] = rows[:, 0] = 1
    for j, r in enumerate(at):
        rows[r] = (2000, 2000, 2000, 2000) + four_squares(len(at) - j)
    d = distances(query, rows)[0]
    worst, keys = int(np.argmax(d)), d.view(np.uint64) >> np.uint64(29)
    assert worst == at[0] and keys[worst] == keys[at[-1]] and d[worst] > d[at[-1]]
    want = model(query, rows, n - 1)
    assert worst not in want[1][0]
    check(api.cosine_topk(ctx, query, rows, n - 1), want, ("n = k + 1", n))


def test_k_4096_is_never_settled(ctx):
    """k + 1 entries do not fit the selection: every query takes the refine path"""
    rows, queries = integers((5000, 8), 21, np.float32), integers((2, 8), 22, np.float32)
    check(api.cosine_topk(ctx, queries, rows, 4096), model(queries, rows, 4096), "k 4096")


def test_chunk_split(ctx, monkeypatch):
    """chunks of 128 queries (the matrix bound is read at call time): both sides of a split are the unsplit call's bits"""
    rows, queries = integers((129, 40), 31, np.float32), integers((300, 40), 32, np.float32)
    whole = api.cosine_topk(ctx, queries, rows, 10)
    monkeypatch.setenv("PGV_COSINE_MATRIX_FLOATS", str(129 * 128))
    check(api.cosine_topk(ctx, queries, rows, 10), whole, "split")
    check(whole, model(queries, rows, 10), "whole")


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_float_data_within_the_fp32_sum_bound(ctx, dtype):
    """random normal rows.  The bound is derived, not tuned: an fp32 sum of dim products is within gamma_dim ~ dim 2^-24
    of the exact one relative to |q| |x|, which is absolute in cosine units; the factor 4 covers the three sums and the
    division"""
    dim, n, nq, k = 1536, 2048, 130, 10
    rng = np.random.default_rng(41)
    rows, queries = rng.standard_normal((n, dim)).astype(dtype), rng.standard_normal((nq, dim)).astype(dtype)
    dist, idx = api.cosine_topk(ctx, queries, rows, k)
    exact = distances(queries, rows)
    assert ((idx >= 0) & (idx < n)).all() and all(len(set(r)) == k for r in idx.tolist())
    assert np.abs(dist - np.take_along_axis(exact, idx, 1)).max() <= 4 * dim * 2.0 ** -24
    assert (np.diff(dist, axis=1) >= 0).all()  # the answer is ordered as its own values are
    assert np.abs(dist - np.sort(exact, axis=1)[:, :k]).max() <= 4 * dim * 2.0 ** -24
