"""sparsevec on the device -- pgv_sparse_distance_batch, pgv_sparse_cosine_distance_batch and pgv_sparse_topk
(sparse_tile_kernel of kernels_sparse.hip + the top-k selection) -- against the float64 model of tests/sparse_model.py,
which tests/test_sparse_model_cpu.py pins to the reference's recorded results.

Two kinds of data.  INTEGER values in -4 .. 4: every term and every partial sum is an integer below 2^24 (at most 32 000
terms of at most 64), so fp32 arithmetic is exact in any order and distances AND row ids must equal the model's bit for bit
(a stable order by (value, row): such data is full of ties).  FLOAT values (standard normal): a distance must lie within
    (m + 2) 2^-24 S        S = sum |term|, m = the number of terms,
the first-order bound for ANY order of m fp32 additions of terms carrying at most two roundings each, and within RTOL S
where that is larger (m <= 165); row ids go through helpers.assert_topk_equiv with the largest such bound of the query as
atol.  pgv_sparse_topk's heads equal pgv_sparse_distance_batch's values BIT FOR BIT: both run sparse_tile_kernel and a
pair's order of addition depends on the pair alone.

The cosine (left to this file): got = 1 - ip / sqrt(na nb) from three fp32 sums, each within e_x = (m_x + 2) 2^-24 S_x of
the model's (the model rounds the exact sum once, the device m_x + 1 times at most).  To first order
    |d cos| <= e_ip / sqrt(na nb) + |sim| (e_na / (2 na) + e_nb / (2 nb)),
the terms dropped are smaller by a factor e_x / x <= 2e-3 (m <= 32 000), covered by a 1 % margin; three float8 operations
add 4 x 2^-52."""
import contextlib
import ctypes

import numpy as np
import pytest

import sparse_model as sm
from helpers import RTOL, assert_topk_equiv, golden
from pgvector_amd import api

pytestmark = pytest.mark.gpu

TILE_NNZ = 2048      # kSparseTileNnz (kernels_sparse.hip): stored query elements of a shared tile
TILE_QUERIES = 128   # kSparseTileQueries: queries of a tile
REG_ROW = 256        # kSparseRegChunks * 64: rows up to this many elements stay in registers
MAX_NNZ = 16000      # SPARSEVEC_MAX_NNZ
METRICS = (api.PGV_L2SQ, api.PGV_NEG_IP, api.PGV_L1)
SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 192, 193, REG_ROW - 1, REG_ROW, REG_ROW + 1, 1000, TILE_NNZ - 1, TILE_NNZ, TILE_NNZ + 1, MAX_NNZ)


# ------------------------------------------------------------------------------------------------------- data
def index_pool(rng, dim, size):
    """`size` distinct indices of 0 .. dim - 1, ascending, the two ends among them: vectors drawn from one pool share
    indices whatever dim is"""
    size = min(size, dim)
    if dim <= 4 * size:
        return np.sort(rng.permutation(dim)[:size]).astype(np.int64)
    got = np.unique(np.concatenate([[0, dim - 1], rng.integers(0, dim, 2 * size)]))
    inner = rng.choice(got[1:-1], size - 2, replace=False) if size > 2 else got[:0]
    return np.sort(np.concatenate([[0, dim - 1][:size], inner])).astype(np.int64)


def values(rng, nnz, kind):
    if kind == "int":
        return rng.integers(-4, 5, nnz).astype(np.float32)  # stored zeros included: legal
    return rng.standard_normal(nnz).astype(np.float32)


def rand_vec(rng, pool, nnz, kind):
    return np.sort(rng.choice(pool, nnz, replace=False)).astype(np.int32), values(rng, nnz, kind)


def rand_csr(rng, pool, sizes, kind):
    return sm.csr([rand_vec(rng, pool, int(s), kind) for s in sizes])


def to_device(triple):
    import torch
    return tuple(torch.from_numpy(x).cuda() for x in triple)


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------- checks
def check_topk(ctx, metric, dim, queries, rows, k, kind, what, call_with=None, model=None):
    """pgv_sparse_topk against the model -> (dist, idx) as host arrays"""
    cq, cr = call_with if call_with is not None else (queries, rows)
    dist, idx = api.sparse_topk(ctx, metric, dim, cq, cr, k)
    dist, idx = host(dist), host(idx)
    nq = len(queries[0]) - 1
    wd, wi, exact, S, m = model if model is not None else sm.topk(metric, queries, rows, k)
    assert dist.dtype == np.float32 and idx.dtype == np.int64 and dist.shape == idx.shape == (nq, k), what
    if kind == "int":
        assert np.array_equal(idx, wi), (what, "row ids", np.argwhere(idx != wi)[:5].tolist())
        assert np.array_equal(dist, wd), (what, "distances", np.argwhere(dist != wd)[:5].tolist())
        return dist, idx
    tol = sm.bound(S, m, RTOL)
    for q in range(nq):
        real = idx[q] >= 0
        assert real.sum() == min(k, exact.shape[1]) and np.isinf(dist[q][~real]).all(), (what, q)
        err = np.abs(dist[q][real].astype(np.float64) - exact[q][idx[q][real]])
        assert (err <= tol[q][idx[q][real]]).all(), (what, q, float(err.max()), float(tol[q].max()))
        atol = max(float(tol[q].max()) if tol.shape[1] else 0.0, 1e-30)
        assert np.array_equal(wi[q] >= 0, real), (what, q)
        assert_topk_equiv(idx[q][real].tolist(), dist[q][real], wi[q][real].tolist(), wd[q][real], atol=atol,
                          what="%s q%d" % (what, q))
    return dist, idx


def check_distances(ctx, metric, dim, query, rows, kind, what, call_with=None):
    cq, cr = call_with if call_with is not None else (query, rows)
    got = host(api.sparse_distance_batch(ctx, metric, dim, cq, cr))
    value, exact, S, m = sm.distances(metric, query, rows)
    assert got.dtype == np.float32 and got.shape == value.shape, what
    if kind == "int":
        assert np.array_equal(got, value), (what, np.argwhere(got != value)[:5].tolist())
    else:
        err = np.abs(got.astype(np.float64) - exact)
        assert (err <= sm.bound(S, m, RTOL)).all(), (what, float(err.max()))
    return got


def check_cosine(ctx, dim, query, rows, kind, what, call_with=None):
    cq, cr = call_with if call_with is not None else (query, rows)
    got = host(api.sparse_cosine_distance_batch(ctx, dim, cq, cr))
    want = sm.cosine(query, rows)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    tol = np.full(want.shape, 4 * 2.0 ** -52)
    if kind != "int":  # the derivation is in the module docstring
        u = 2.0 ** -24
        _, S_ip, m_ip = sm.sums(sm.NEG_IP, query, rows)
        na = float((np.asarray(query[1], dtype=np.float64) ** 2).sum())
        nb = np.array([(sm.vector(rows, r)[1].astype(np.float64) ** 2).sum() for r in range(len(want))])
        with np.errstate(invalid="ignore", divide="ignore"):
            first = (m_ip + 2) * u * S_ip / np.sqrt(na * nb) + np.abs(1.0 - want) * 0.5 * (
                (len(query[1]) + 2) * u + (np.diff(rows[0]) + 2) * u)
        tol = tol + 1.01 * first
    assert (np.abs(got[ok] - want[ok]) <= tol[ok]).all(), (what, float(np.abs(got[ok] - want[ok]).max()))
    return got


def check_everything(ctx, dim, queries, rows, k, kind, what, call_with=None):
    """the three metrics through pgv_sparse_topk, the first, middle and last query through pgv_sparse_distance_batch
    (bit-equal to the heads), and the cosine of the first and the last query"""
    nq = len(queries[0]) - 1
    cr = None if call_with is None else call_with[1]
    for metric in METRICS:
        dist, idx = check_topk(ctx, metric, dim, queries, rows, k, kind, "%s metric %d" % (what, metric), call_with)
        for q in sorted({0, nq // 2, nq - 1}):
            one = sm.vector(queries, q)
            d = check_distances(ctx, metric, dim, one, rows, kind, "%s metric %d q%d" % (what, metric, q),
                                None if call_with is None else (one, cr))
            real = idx[q] >= 0
            assert np.array_equal(bits(dist[q][real]), bits(d[idx[q][real]])), (what, metric, q, "heads vs single query")
    for q in sorted({0, nq - 1}):
        check_cosine(ctx, dim, sm.vector(queries, q), rows, kind, "%s cosine q%d" % (what, q),
                     None if call_with is None else (sm.vector(queries, q), cr))


# ----------------------------------------------------------------------------------------------------- golden
CASES = golden("sparsevec_known_answers.json")["cases"]


@pytest.mark.parametrize("case", CASES, ids=["%s-%d" % (c["fn"], c["sql_line"]) for c in CASES])
def test_known_answers(ctx, case):
    """every recorded distance of the reference's regression transcript through the three entries at n = 1"""
    def batch(metric, dim, a, b):
        if metric == "cosine":
            return api.sparse_cosine_distance_batch(ctx, dim, a, b)[0]
        return api.sparse_distance_batch(ctx, metric, dim, a, b)[0]

    def head(metric, dim, a, b):
        dist, idx = api.sparse_topk(ctx, metric, dim, sm.csr([a]), b, 2)
        assert idx[0, 1] == -1 and np.isinf(dist[0, 1]) and idx[0, 0] == 0
        return dist[0, 0]
    assert sm.known_answer(case, batch) == case["result"]
    if case["fn"] != "cosine_distance":
        assert sm.known_answer(case, head) == case["result"]


# -------------------------------------------------------------------------------------------------- nnz edges
@pytest.fixture(scope="module")
def edge_rows():
    """one row of every size of SIZES (in a shuffled order), drawn from a pool of 24 000 of 40 000 dimensions"""
    rng = np.random.default_rng(101)
    pool = index_pool(rng, 40000, 24000)
    sizes = rng.permutation(SIZES)
    return pool, {kind: rand_csr(rng, pool, sizes, kind) for kind in ("int", "float")}


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("qnnz", SIZES)
def test_nnz_edges(ctx, edge_rows, qnnz, kind):
    """query nnz x row nnz over {0, 1, 63, 64, 65, 257, 1000, 16000}, the edges of the one to four 64-element chunks a
    register row has (128 +- 1, 192 | 193), the register-row limit 256 +- 1 and the tile limit TILE_NNZ +- 1 on either side: every row size meets every query size.  Three queries (qnnz, 7, qnnz) so that tiles of
    one, two and three queries occur"""
    pool, rows = edge_rows
    rng = np.random.default_rng(200 + qnnz)
    queries = rand_csr(rng, pool, (qnnz, 7, qnnz), kind)
    check_everything(ctx, 40000, queries, rows[kind], 5, kind, "qnnz %d" % qnnz)


@pytest.mark.parametrize("kind", ["int", "float"])
def test_lds_capacity_path(ctx, kind):
    """16 000 x 16 000 stored elements at n = 64, nq = 3: a query tile of 128 000 bytes plus the matched bitmaps, the
    raised dynamic-LDS launch"""
    rng = np.random.default_rng(301)
    pool = index_pool(rng, 10 ** 6, 24000)
    rows = rand_csr(rng, pool, [MAX_NNZ] * 64, kind)
    queries = rand_csr(rng, pool, [MAX_NNZ] * 3, kind)
    check_everything(ctx, 10 ** 6, queries, rows, 10, kind, "16000 x 16000")


@pytest.mark.parametrize("sizes", [(TILE_NNZ - 7, 7, 5), (TILE_NNZ - 6, 7, 5), (TILE_NNZ + 1, TILE_NNZ, 1, TILE_NNZ - 1),
                                   (3,) * (TILE_QUERIES - 1), (3,) * TILE_QUERIES, (3,) * (TILE_QUERIES + 1),
                                   (40,) * 300],
                         ids=["sum-fills-tile", "sum-one-over", "around-tile", "nq-127", "nq-128", "nq-129", "nnz-cut"])
def test_tile_limits(ctx, sizes):
    """where the host plan cuts the queries into tiles: two queries filling a tile exactly / one element over, queries
    around the tile size, one query fewer than / exactly / one more than a tile holds, and 300 queries of 40 elements
    (cut by the element count: TILE_NNZ // 40 queries a tile)"""
    rng = np.random.default_rng(401)
    pool = index_pool(rng, 9000, 6000)
    rows = rand_csr(rng, pool, rng.integers(0, 300, 70), "int")
    queries = rand_csr(rng, pool, sizes, "int")
    for metric in METRICS:
        check_topk(ctx, metric, 9000, queries, rows, 8, "int", "tiles %s metric %d" % (sizes[:3], metric))


# --------------------------------------------------------------------------------------------- index geometry
def geometry(name, kind):
    rng = np.random.default_rng(501)
    v = lambda n: values(rng, n, kind)  # noqa: E731
    ar = lambda lo, hi, step=1: np.arange(lo, hi, step, dtype=np.int32)  # noqa: E731
    if name == "disjoint":
        return 1000, [(ar(0, 400, 2), v(200)), (ar(0, 10, 2), v(5))], [(ar(1, 400, 2), v(200)), (ar(501, 700), v(199))]
    if name == "identical":
        vecs = [(ar(3, 903, 3), v(300)), (ar(0, 70), v(70)), (ar(0, 0), v(0))]
        return 1000, vecs, vecs + [(ar(3, 903, 3), v(300))]
    if name == "query-below":
        return 1000, [(ar(0, 100), v(100)), (ar(0, 1), v(1))], [(ar(100, 400), v(300)), (ar(999, 1000), v(1))]
    if name == "query-above":
        return 1000, [(ar(900, 1000), v(100)), (ar(999, 1000), v(1))], [(ar(0, 300), v(300)), (ar(0, 1), v(1))]
    if name == "interleaved":
        return 1000, [(ar(0, 600, 2), v(300))], [(ar(1, 601, 2), v(300)), (ar(1, 131, 2), v(65)), (ar(0, 600), v(600))]
    if name == "dim-1":
        one = (ar(0, 1), np.array([3 if kind == "int" else 0.3], dtype=np.float32))
        return 1, [one, (ar(0, 0), v(0))], [one, (ar(0, 1), v(1)), (ar(0, 0), v(0))]
    assert name == "dim-1e9"
    dim = 10 ** 9
    pool = index_pool(rng, dim, 3000)
    vecs = [rand_vec(rng, pool, n, kind) for n in (1, 200, 1500, 3000, 0)]
    last = (np.array([dim - 1], dtype=np.int32), v(1))
    return dim, vecs[:3] + [last], vecs + [last, (np.array([0, dim - 1], dtype=np.int32), v(2))]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("name", ["disjoint", "identical", "query-below", "query-above", "interleaved", "dim-1", "dim-1e9"])
def test_index_geometry(ctx, name, kind):
    """no shared index; rows that are the query; every query index below / above every row index; strictly interleaved;
    one dimension; 10^9 dimensions with indices up to dim - 1"""
    dim, queries, rows = geometry(name, kind)
    check_everything(ctx, dim, sm.csr(queries), sm.csr(rows), 4, kind, name)


def test_self_distance_is_exactly_zero(ctx):
    """float data: under L2 and L1 a vector is at exactly 0.0 from itself (every term is (a - a)^2 or |a - a|), at every
    row length the kernel treats differently"""
    rng = np.random.default_rng(601)
    pool = index_pool(rng, 50000, 24000)
    rows = rand_csr(rng, pool, (0, 1, 64, REG_ROW, REG_ROW + 1, 1000, TILE_NNZ + 1, MAX_NNZ), "float")
    for r in range(len(rows[0]) - 1):
        for metric in (api.PGV_L2SQ, api.PGV_L1):
            got = api.sparse_distance_batch(ctx, metric, 50000, sm.vector(rows, r), rows)
            assert got[r] == 0.0 and not np.signbit(got[r]), (r, metric, got[r])
    dist, idx = api.sparse_topk(ctx, api.PGV_L2SQ, 50000, rows, rows, 1)
    assert (dist[1:, 0] == 0.0).all() and idx[1:, 0].tolist() == list(range(1, len(rows[0]) - 1))


# ------------------------------------------------------------------------------------------------------ shapes
@pytest.fixture(scope="module")
def shape_data():
    """1000 rows of 0 .. 80 stored elements and 64 queries of 0 .. 60 over 500 dimensions, and the model's full answer;
    the smaller shapes are prefixes of it"""
    out = {}
    for kind in ("int", "float"):
        rng = np.random.default_rng(701)
        pool = index_pool(rng, 500, 500)
        out[kind] = (rand_csr(rng, pool, rng.integers(0, 81, 1000), kind), rand_csr(rng, pool, rng.integers(0, 61, 64), kind))
    return out


def prefix(triple, n):
    ptr, idx, val = triple
    return ptr[:n + 1].copy(), idx[:ptr[n]].copy(), val[:ptr[n]].copy()


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("n,nq,k,where", [(0, 1, 10, "host"), (1, 31, 1, "host"), (31, 33, 10, "device"),
                                          (32, 64, 40, "rows-device"), (33, 1, 4096, "queries-device"),
                                          (1000, 64, 10, "device"), (1000, 33, 4096, "host")])
def test_shapes(ctx, shape_data, n, nq, k, where, kind):
    """n in {0, 1, 31, 32, 33, 1000} (one row block, its edge, many blocks) x nq in {1, 31, 33, 64} x k in {1, 10, k > n,
    4096}, with host arrays, device tensors (outputs on the device too) and one side each"""
    rows, queries = prefix(shape_data[kind][0], n), prefix(shape_data[kind][1], nq)
    call = None if where == "host" else (to_device(queries) if where != "rows-device" else queries,
                                         to_device(rows) if where != "queries-device" else rows)
    for metric in METRICS:
        check_topk(ctx, metric, 500, queries, rows, k, kind, "n %d nq %d k %d" % (n, nq, k), call)
    if where in ("device", "queries-device"):
        dist, idx = api.sparse_topk(ctx, api.PGV_L2SQ, 500, call[0], call[1], k)
        assert dist.is_cuda and idx.is_cuda
    if n:
        q = sm.vector(queries, nq - 1)
        cr = None if call is None else call[1]
        for metric in METRICS:
            check_distances(ctx, metric, 500, q, rows, kind, "n %d" % n, None if call is None else (q, cr))
        got = check_cosine(ctx, 500, q, rows, kind, "n %d" % n, None if call is None else (q, cr))
        assert got.shape == (n,)
    if where == "device":  # the inputs are left as they were
        assert all(np.array_equal(host(a), b) for a, b in zip(call[0] + call[1], queries + rows))


def test_k_4096_of_5000(ctx):
    """a full head of 4096 from 5000 rows, integer data: the whole stable order"""
    rng = np.random.default_rng(801)
    pool = index_pool(rng, 300, 300)
    rows, queries = rand_csr(rng, pool, rng.integers(0, 40, 5000), "int"), rand_csr(rng, pool, (30, 0), "int")
    check_topk(ctx, api.PGV_L1, 300, queries, rows, 4096, "int", "k 4096", (queries, to_device(rows)))


def test_query_chunks(ctx, shape_data, monkeypatch):
    """nq = 65 x n = 33 served in chunks: the library's rule is min(nq, max(1, F / n)) queries a chunk with F = 2^30
    floats, unreached at any quick shape; PGV_SPARSE_MATRIX_FLOATS (read at every call) puts F at 33 x 16, so the call
    runs five chunks (16, 16, 16, 16, 1) whose tiles are planned chunk by chunk, and at 1: one query a chunk.  Same answer,
    bit for bit, as the unchunked call and as the model"""
    rows = prefix(shape_data["int"][0], 33)
    q64 = shape_data["int"][1]
    queries = sm.csr([sm.vector(q64, q) for q in range(64)] + [sm.vector(q64, 5)])
    whole = check_topk(ctx, api.PGV_L2SQ, 500, queries, rows, 10, "int", "one chunk")
    for floats in (33 * 16, 1):
        monkeypatch.setenv("PGV_SPARSE_MATRIX_FLOATS", str(floats))
        got = check_topk(ctx, api.PGV_L2SQ, 500, queries, rows, 10, "int", "F = %d" % floats)
        assert np.array_equal(bits(got[0]), bits(whole[0])) and np.array_equal(got[1], whole[1])


# ------------------------------------------------------------------------------------------------------ errors
def small():
    rows = sm.csr([(np.array([0, 2, 5], dtype=np.int32), np.array([1, 2, 3], dtype=np.float32)),
                   (np.array([1, 4], dtype=np.int32), np.array([4, 5], dtype=np.float32))])
    return rows, (np.array([2, 3], dtype=np.int32), np.array([1, 1], dtype=np.float32))


@contextlib.contextmanager
def raises(code, *fragments):
    with pytest.raises(api.PgvError) as e:
        yield e
    assert e.value.code == code, e.value
    for f in fragments:
        assert f in e.value.message, (f, e.value.message)


def test_argument_errors(ctx):
    rows, query = small()
    queries = sm.csr([query])
    for dim in (0, 10 ** 9 + 1):
        with raises(api._lib.PGV_ERR_DIMS, "dimensions"):
            api.sparse_topk(ctx, api.PGV_L2SQ, dim, queries, rows, 1)
        with raises(api._lib.PGV_ERR_DIMS, "dimensions"):
            api.sparse_distance_batch(ctx, api.PGV_L2SQ, dim, query, rows)
        with raises(api._lib.PGV_ERR_DIMS, "dimensions"):
            api.sparse_cosine_distance_batch(ctx, dim, query, rows)
    for k in (0, 4097):
        with raises(api.PGV_ERR_ARG, "k %d" % k):
            api.sparse_topk(ctx, api.PGV_L2SQ, 6, queries, rows, k)
    with raises(api.PGV_ERR_ARG, "unknown metric"):
        api.sparse_topk(ctx, 7, 6, queries, rows, 1)
    with raises(api.PGV_ERR_ARG, "unknown metric"):
        api.sparse_distance_batch(ctx, 7, 6, query, rows)
    # NULL outputs
    with raises(api.PGV_ERR_ARG, "NULL"):
        api.sparse_topk(ctx, api.PGV_L2SQ, 6, queries, rows, 1, out=(None, np.zeros((1, 1), dtype=np.int64)))
    with raises(api.PGV_ERR_ARG, "NULL"):
        api.sparse_topk(ctx, api.PGV_L2SQ, 6, queries, rows, 1, out=(np.zeros((1, 1), dtype=np.float32), None))
    p = api.ptr
    with raises(api.PGV_ERR_ARG, "NULL"):
        api.check(api.lib.pgv_sparse_distance_batch(ctx.h, api.PGV_L2SQ, 6, 2, p(query[0]), p(query[1]), p(rows[0]), p(rows[1]),
                                                    p(rows[2]), 2, None))
    with raises(api.PGV_ERR_ARG, "NULL"):
        api.check(api.lib.pgv_sparse_cosine_distance_batch(ctx.h, 6, 2, p(query[0]), p(query[1]), p(rows[0]), p(rows[1]),
                                                           p(rows[2]), 2, ctypes.c_void_p(None)))


def test_data_errors_name_the_vector_and_the_position(ctx):
    """host arrays are validated before any launch, on the row side and on the query side of every entry"""
    rows, query = small()
    queries = sm.csr([query])

    def every_entry(code, bad_rows, *fragments):
        with raises(code, "rows", *fragments):
            api.sparse_topk(ctx, api.PGV_L2SQ, 6, queries, bad_rows, 1)
        with raises(code, "rows", *fragments):
            api.sparse_distance_batch(ctx, api.PGV_L1, 6, query, bad_rows)
        with raises(code, "rows", *fragments):
            api.sparse_cosine_distance_batch(ctx, 6, query, bad_rows)
        with raises(code, "queries", *fragments):  # the same vectors as queries
            api.sparse_topk(ctx, api.PGV_NEG_IP, 6, bad_rows, rows, 1)

    def edit(which, at, value):
        out = [a.copy() for a in rows]
        out[which][at] = value
        return tuple(out)
    every_entry(api.PGV_ERR_ARG, edit(1, 4, 0), "vector 1", "position 1", "ascend")        # unsorted: 1, 0
    every_entry(api.PGV_ERR_ARG, edit(1, 1, 0), "vector 0", "position 1", "ascend")        # a duplicate: 0, 0, 5
    every_entry(api.PGV_ERR_ARG, edit(1, 2, 6), "vector 0", "position 2", "index 6")       # an index equal to dim
    every_entry(api.PGV_ERR_ARG, edit(1, 0, -1), "vector 0", "position 0", "index -1")
    every_entry(api.PGV_ERR_ARG, edit(2, 3, np.nan), "vector 1", "position 0", "finite")
    every_entry(api.PGV_ERR_ARG, edit(2, 2, np.inf), "vector 0", "position 2", "finite")
    every_entry(api.PGV_ERR_ARG, edit(0, 1, 6), "vector 1", "monotone")                    # ptr 0, 6, 5
    every_entry(api.PGV_ERR_ARG, edit(0, 0, 1), "ptr[0]")
    big = sm.csr([(np.arange(MAX_NNZ + 1, dtype=np.int32), np.ones(MAX_NNZ + 1, dtype=np.float32))])
    with raises(api._lib.PGV_ERR_DIMS, "rows", "vector 0", "16001"):
        api.sparse_topk(ctx, api.PGV_L2SQ, 20000, queries, big, 1)
    with raises(api._lib.PGV_ERR_DIMS, "queries", "vector 0", "16001"):
        api.sparse_topk(ctx, api.PGV_L2SQ, 20000, big, rows, 1)
    with raises(api._lib.PGV_ERR_DIMS, "query", "16001"):
        api.sparse_distance_batch(ctx, api.PGV_L2SQ, 20000, (big[1], big[2]), rows)
    with raises(api._lib.PGV_ERR_DIMS, "query", "16001"):
        api.sparse_cosine_distance_batch(ctx, 20000, (big[1], big[2]), rows)
    # a single query's own elements (the entries without a q_ptr)
    with raises(api.PGV_ERR_ARG, "query", "vector 0", "position 1", "ascend"):
        api.sparse_distance_batch(ctx, api.PGV_L2SQ, 6, (np.array([3, 3], dtype=np.int32), query[1]), rows)
    with raises(api.PGV_ERR_ARG, "query", "vector 0", "position 0", "finite"):
        api.sparse_cosine_distance_batch(ctx, 6, (query[0], np.array([np.nan, 1], dtype=np.float32)), rows)
    # nothing was left behind: a good call still works
    assert api.sparse_distance_batch(ctx, api.PGV_L2SQ, 6, query, rows).tolist() == [12.0, 43.0]
