"""Binary-quantized search on the device -- pgv_bit_topk (hamming_tile_kernel + the top-k selection), pgv_binary_quantize,
pgv_rerank and api.binary_search -- against the numpy model of tests/bit_model.py, which tests/test_bit_model_cpu.py pins
to the oracle and to the reference's recorded results.  Hamming distances and quantised bits are integers: every such
comparison is exact equality of both distance and index."""
import numpy as np
import pytest

import bit_model as bm
from helpers import RTOL, assert_topk_equiv, gen, golden
from oracle import pyoracle as po
from pgvector_amd import api

pytestmark = pytest.mark.gpu

ROW_TILE = 256      # kBitThreads (kernels_bit.hip): rows per workgroup
QUERY_TILE = 32     # kBitQueries: queries per workgroup
SLICE_BITS = 1024   # kBitSliceBits: the bits of a row a lane holds in registers at a time
DT = {po.ORA_F32: api.PGV_F32, po.ORA_F16: api.PGV_F16}


def rand_bits(n, nbits, seed):
    """n packed bit strings of nbits (first bit in the top bit of byte 0, pad bits zero, as PostgreSQL keeps them)"""
    rng = np.random.default_rng(seed)
    return np.packbits(rng.integers(0, 2, (n, nbits), dtype=np.uint8), axis=1) if nbits else np.zeros((n, 0), dtype=np.uint8)


def check_topk(ctx, nbits, queries, rows, k, what, model=None):
    dist, idx = api.bit_topk(ctx, nbits, queries, rows, k)
    wd, wi = model if model is not None else bm.hamming_topk(queries, rows, k)
    assert dist.dtype == np.float32 and idx.dtype == np.int64 and dist.shape == idx.shape == (queries.shape[0], k)
    assert np.array_equal(idx, wi), (what, "indexes", np.argwhere(idx != wi)[:5].tolist())
    assert np.array_equal(dist, wd), (what, "distances", np.argwhere(dist != wd)[:5].tolist())


# ------------------------------------------------------------------------------------------------ pgv_bit_topk
@pytest.mark.parametrize("nbits", [1, 7, 8, 9, 127, 128, 129, 136, 1536, SLICE_BITS - 1, SLICE_BITS, SLICE_BITS + 1, 4096 + 8])
def test_bit_topk_every_row_length(ctx, nbits):
    """whole bytes / ragged last byte, the 16-byte vector edge (127 .. 129), a staged row of an odd vector count (136),
    the headline 1536, one below / at / one above the kernel's register slice (kBitSliceBits = 1024) and 4096 + 8 bits,
    where five slices accumulate"""
    rows, queries = rand_bits(300, nbits, 11), rand_bits(5, nbits, 12)
    check_topk(ctx, nbits, queries, rows, 10, "nbits %d" % nbits)


@pytest.fixture(scope="module")
def nq_case():
    rows, queries = rand_bits(1000, 256, 21), rand_bits(65, 256, 22)
    return rows, queries, bm.hamming_topk(queries, rows, 10)


@pytest.mark.parametrize("nq", [1, 2, QUERY_TILE - 1, QUERY_TILE, QUERY_TILE + 1, 65])
def test_bit_topk_query_tile_edges(ctx, nq_case, nq):
    """fewer queries than a tile (the clamped tail queries), exactly one tile, one more, two tiles and one"""
    rows, queries, (wd, wi) = nq_case
    check_topk(ctx, 256, np.ascontiguousarray(queries[:nq]), rows, 10, "nq %d" % nq, model=(wd[:nq], wi[:nq]))


@pytest.mark.parametrize("n,k", [(0, 10), (1, 10), (9, 10), (10, 10), (11, 10), (6, 10), (ROW_TILE - 1, 10), (ROW_TILE, 10),
                                 (ROW_TILE + 1, 10), (3 * ROW_TILE + 77, 10)])
def test_bit_topk_row_counts(ctx, n, k):
    """no rows, fewer rows than k (+inf / -1 padding), k - 1 / k / k + 1 rows, one row tile -1 / exactly / +1 (the
    clamped tail rows), several tiles and a remainder"""
    rows, queries = rand_bits(n, 256, 31 + n), rand_bits(3, 256, 32)
    check_topk(ctx, 256, queries, rows, k, "n %d" % n)
    if n < k:
        dist, idx = api.bit_topk(ctx, 256, queries, rows, k)
        assert np.isinf(dist[:, n:]).all() and (dist[:, n:] > 0).all() and (idx[:, n:] == -1).all()


@pytest.fixture(scope="module")
def k_case():
    rows, queries = rand_bits(5000, 256, 41), rand_bits(2, 256, 42)
    return rows, queries, bm.hamming_topk(queries, rows, 4096)


@pytest.mark.parametrize("k", [1, 256, 257, 4096])
def test_bit_topk_k_sweep(ctx, k_case, k):
    rows, queries, (wd, wi) = k_case
    check_topk(ctx, 256, queries, rows, k, "k %d" % k, model=(wd[:, :k], wi[:, :k]))


def test_bit_topk_rejects_k_above_4096(ctx, k_case):
    rows, queries, _ = k_case
    with pytest.raises(api.PgvError) as e:
        api.bit_topk(ctx, 256, queries, rows, 4097)
    assert e.value.code == api.PGV_ERR_ARG
    with pytest.raises(api.PgvError) as e:
        api.bit_topk(ctx, 256, queries, rows, 0)
    assert e.value.code == api.PGV_ERR_ARG


def test_bit_topk_ties_go_to_the_lower_index(ctx):
    """identical rows: every distance of a query is the same, so the answer is rows 0 .. k - 1; 64-bit rows at
    n = 20 000: hundreds of rows share each distance and equal distances must come in index order"""
    queries = rand_bits(4, 200, 51)
    rows = np.repeat(rand_bits(1, 200, 52), 1000, axis=0)
    dist, idx = api.bit_topk(ctx, 200, queries, rows, 20)
    assert np.array_equal(idx, np.tile(np.arange(20, dtype=np.int64), (4, 1)))
    assert np.array_equal(dist, np.repeat(bm.hamming_topk(queries, rows[:1], 1)[0], 20, axis=1))
    rows, queries = rand_bits(20000, 64, 53), rand_bits(3, 64, 54)
    wd, wi = bm.hamming_topk(queries, rows, 300)
    assert max(np.unique(wd[q], return_counts=True)[1].max() for q in range(3)) >= 100  # the case holds long tie runs
    check_topk(ctx, 64, queries, rows, 300, "64-bit ties", model=(wd, wi))


def test_bit_topk_splits_the_queries_at_the_matrix_limit(ctx):
    """n = 2^20 + 64 rows x 1025 queries exceed 2^30 matrix entries: the call serves the queries in chunks of
    2^30 / n = 1023 rounded down to whole 32-query tiles = 992 (include/pgv_hip.h).  Checked against the model: the
    first query, the last of the first chunk, the first of the second chunk and the last query"""
    import torch
    n, nq, k = (1 << 20) + 64, 1025, 10
    chunk = min(nq, (1 << 30) // n) // 32 * 32
    assert chunk == 992 and chunk * n <= 1 << 30 < nq * n
    rows, queries = rand_bits(n, 64, 61), rand_bits(nq, 64, 62)
    dist, idx = api.bit_topk(ctx, 64, queries, torch.from_numpy(rows).cuda(), k)
    for q in (0, chunk - 1, chunk, nq - 1):
        wd, wi = bm.hamming_topk(queries[q:q + 1], rows, k)
        assert np.array_equal(idx[q], wi[0]) and np.array_equal(dist[q], wd[0]), q


@pytest.mark.parametrize("nbits", [128, 136])
def test_bit_topk_pointer_kinds(ctx, nbits):
    """numpy in and out, torch device in and out, device rows used in place (128 bits = 16 bytes) or staged (136 bits =
    17 bytes) under host queries: the same answer"""
    import torch
    rows, queries = rand_bits(700, nbits, 71), rand_bits(40, nbits, 72)
    wd, wi = bm.hamming_topk(queries, rows, 12)
    check_topk(ctx, nbits, queries, rows, 12, "numpy", model=(wd, wi))
    d_rows, d_queries = torch.from_numpy(rows).cuda(), torch.from_numpy(queries).cuda()
    dist, idx = api.bit_topk(ctx, nbits, d_queries, d_rows, 12)
    assert dist.is_cuda and idx.is_cuda
    assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(dist.cpu().numpy(), wd)
    dist, idx = api.bit_topk(ctx, nbits, queries, d_rows, 12)
    assert np.array_equal(idx, wi) and np.array_equal(dist, wd)
    assert np.array_equal(d_rows.cpu().numpy(), rows) and np.array_equal(d_queries.cpu().numpy(), queries)


def test_bit_topk_degenerate(ctx):
    # empty bit strings: every distance is 0, rows 0 .. min(k, n) - 1
    for n in (20, 3):
        dist, idx = api.bit_topk(ctx, 0, np.zeros((2, 0), dtype=np.uint8), np.zeros((n, 0), dtype=np.uint8), 5)
        m = min(n, 5)
        assert np.array_equal(idx[:, :m], np.tile(np.arange(m), (2, 1))) and (idx[:, m:] == -1).all()
        assert (dist[:, :m] == 0).all() and np.isinf(dist[:, m:]).all()
    # a query that is one of the rows finds it first, at distance 0
    rows = rand_bits(500, 300, 81)
    dist, idx = api.bit_topk(ctx, 300, np.ascontiguousarray(rows[[123, 499]]), rows, 3)
    assert idx[:, 0].tolist() == [123, 499] and (dist[:, 0] == 0).all()
    # all ones against all zeros: nbits
    for nbits in (77, 1536, 2000):
        ones = np.packbits(np.ones((1, nbits), dtype=np.uint8), axis=1)
        dist, idx = api.bit_topk(ctx, nbits, ones, np.zeros((2, ones.shape[1]), dtype=np.uint8), 2)
        assert dist.tolist() == [[nbits, nbits]] and idx.tolist() == [[0, 1]]
    # no queries: nothing to do
    dist, idx = api.bit_topk(ctx, 64, np.zeros((0, 8), dtype=np.uint8), rand_bits(10, 64, 82), 4)
    assert dist.shape == (0, 4)


# ----------------------------------------------------------------------------------------- pgv_binary_quantize
QUANT_CASES = golden("binary_quantize_known_answers.json")["cases"]


@pytest.mark.parametrize("case", QUANT_CASES, ids=["%s-%d" % (c["type"], len(c["input"])) for c in QUANT_CASES])
def test_binary_quantize_known_answers(ctx, case):
    dtype = po.ORA_F32 if case["type"] == "vector" else po.ORA_F16
    x = np.array([case["input"]], dtype=po.NP_OF[dtype])
    got = np.unpackbits(api.binary_quantize(ctx, DT[dtype], x.shape[1], x), axis=1)[0]
    assert "".join(str(b) for b in got[:x.shape[1]]) == case["bits"]
    assert not got[x.shape[1]:].any()


@pytest.mark.parametrize("dtype", [po.ORA_F32, po.ORA_F16])
@pytest.mark.parametrize("dim", [1, 7, 8, 9, 31, 32, 33, 1536, 1537])
def test_binary_quantize_matches_the_model(ctx, dtype, dim):
    """random normal rows through host and device pointers; the unused low bits of every row's last byte are zero"""
    import torch
    x = gen(257, dim, seed=91 + dim, dist="normal", dtype=dtype)
    want = bm.binary_quantize(x)
    got = api.binary_quantize(ctx, DT[dtype], dim, x)
    assert got.dtype == np.uint8 and got.shape == (257, (dim + 7) // 8)
    assert np.array_equal(got, want)
    got_dev = api.binary_quantize(ctx, DT[dtype], dim, torch.from_numpy(x).cuda())
    assert got_dev.is_cuda and np.array_equal(got_dev.cpu().numpy(), want)
    if dim % 8:
        assert not (got[:, -1] & ((1 << (8 - dim % 8)) - 1)).any()


@pytest.mark.parametrize("dtype", [po.ORA_F32, po.ORA_F16])
def test_binary_quantize_is_the_c_comparison(ctx, dtype):
    """x > 0 exactly: zeros of both signs, NaN and negatives give 0; +inf and the smallest subnormal give 1"""
    dt = po.NP_OF[dtype]
    tiny, sub = np.finfo(dt).tiny, np.finfo(dt).smallest_subnormal
    x = np.array([[0.0, -0.0, np.nan, np.inf, -np.inf, sub, tiny, -sub, -tiny, -np.nan, 1.0]], dtype=dt)
    x[0, 9] = np.array([0xffc00000 if dt == np.float32 else 0xfe00], dtype=np.uint32 if dt == np.float32 else np.uint16).view(dt)[0]
    got = np.unpackbits(api.binary_quantize(ctx, DT[dtype], x.shape[1], x), axis=1)[0]
    assert got.tolist() == [0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1] + [0] * 5
    assert np.array_equal(api.binary_quantize(ctx, DT[dtype], x.shape[1], x), bm.binary_quantize(x))


# --------------------------------------------------------------------------------------------------- pgv_rerank
def rand_cand(nq, kc, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(n, kc, replace=False) for _ in range(nq)]).astype(np.int64)


def ip_atol(metric, queries, rows, cand):
    """inner products cancel: the tolerance is relative to the size of the terms (tests/test_gpu_round3.py)"""
    if metric != api.PGV_NEG_IP:
        return 1e-30
    r = np.abs(rows[np.unique(cand[cand >= 0])].astype(np.float64))
    return RTOL * float(np.max(r @ np.abs(queries.astype(np.float64)).T)) if len(r) else 1e-30


@pytest.mark.parametrize("metric", [api.PGV_L2SQ, api.PGV_NEG_IP, api.PGV_L1])
@pytest.mark.parametrize("dtype", [po.ORA_F32, po.ORA_F16])
def test_rerank_exact_arithmetic(ctx, oracle, dtype, metric):
    """dim 8 `int10` data: every value is exact in fp32, so distances AND indexes equal the model's.  kc = 1, k = kc,
    k < kc; -1 in the middle and at the end; a list of all -1; duplicate candidates (ties to the lower position)"""
    half = dtype == po.ORA_F16
    rows = gen(500, 8, seed=101, dist="int10", dtype=dtype)
    queries = gen(4, 8, seed=102, dist="int10", dtype=dtype)
    cand = rand_cand(4, 16, 500, 103)
    cand[0, 5] = cand[0, 15] = -1
    cand[1, :] = -1
    cand[2, 9] = cand[2, 2]
    cand[2, 11] = cand[2, 2]
    for c, k in ((cand[:, :1], 1), (cand, 16), (cand, 5)):
        c = np.ascontiguousarray(c)
        dist, idx = api.rerank(ctx, metric, DT[dtype], 8, queries, rows, c, k)
        wd, wi = bm.rerank(oracle, metric, half, queries, rows, c, k)
        assert np.array_equal(idx, wi), (k, idx.tolist(), wi.tolist())
        assert np.array_equal(dist, wd), (k, dist.tolist(), wd.tolist())
    dist, idx = api.rerank(ctx, metric, DT[dtype], 8, queries, rows, cand, 16)
    assert (idx[1] == -1).all() and np.isinf(dist[1]).all()
    assert idx[0, 14:].tolist() == [-1, -1] and np.isinf(dist[0, 14:]).all()
    pos = [int(np.flatnonzero(idx[2] == cand[2, 2])[i]) for i in range(3)]
    assert pos == list(range(pos[0], pos[0] + 3))  # the three copies tie and stay together


@pytest.mark.parametrize("metric", [api.PGV_L2SQ, api.PGV_NEG_IP, api.PGV_L1])
@pytest.mark.parametrize("dtype", [po.ORA_F32, po.ORA_F16])
def test_rerank_long_rows(ctx, oracle, dtype, metric):
    """dim 1536 normal data against the oracle's per-pair kernels at the project's tolerance; device pointers too"""
    import torch
    half = dtype == po.ORA_F16
    rows = gen(300, 1536, seed=111, dist="normal", dtype=dtype)
    queries = gen(3, 1536, seed=112, dist="normal", dtype=dtype)
    cand = rand_cand(3, 32, 300, 113)
    cand[1, 7] = -1
    wd, wi = bm.rerank(oracle, metric, half, queries, rows, cand, 10)
    atol = ip_atol(metric, queries, rows, cand)
    dist, idx = api.rerank(ctx, metric, DT[dtype], 1536, queries, rows, cand, 10)
    for q in range(3):
        assert_topk_equiv(idx[q].tolist(), dist[q], wi[q].tolist(), wd[q], atol=atol, what="rerank q%d" % q)
    d_dist, d_idx = api.rerank(ctx, metric, DT[dtype], 1536, torch.from_numpy(queries).cuda(), torch.from_numpy(rows).cuda(),
                               torch.from_numpy(cand).cuda(), 10)
    assert np.array_equal(d_idx.cpu().numpy(), idx) and np.array_equal(d_dist.cpu().numpy(), dist)


def test_rerank_argument_errors(ctx):
    rows, queries = gen(50, 8, seed=121, dist="int10"), gen(2, 8, seed=122, dist="int10")
    cand = rand_cand(2, 4, 50, 123)
    for bad in (50, 1 << 40):
        c = cand.copy()
        c[1, 2] = bad
        with pytest.raises(api.PgvError) as e:
            api.rerank(ctx, api.PGV_L2SQ, api.PGV_F32, 8, queries, rows, c, 2)
        assert e.value.code == api.PGV_ERR_ARG
    with pytest.raises(api.PgvError) as e:
        api.rerank(ctx, api.PGV_L2SQ, api.PGV_F32, 8, queries, rows, cand, 5)  # k > kc
    assert e.value.code == api.PGV_ERR_ARG


# ------------------------------------------------------------------------------------------- api.binary_search
def test_binary_search_end_to_end(ctx, oracle):
    """4 000 clustered 256-d rows, 16 queries, kc = 200, k = 10: stage one is the model's Hamming top-kc of the quantised
    queries, stage two the model's rerank of stage one's candidates (recall is the data's property: not asserted)"""
    rows = gen(4000, 256, seed=131, dist="clustered") - np.float32(0.5)
    queries = gen(16, 256, seed=132, dist="clustered") - np.float32(0.5)
    bits = api.binary_quantize(ctx, api.PGV_F32, 256, rows)
    assert np.array_equal(bits, bm.binary_quantize(rows))
    dist, idx, hamming, cand = api.binary_search(ctx, api.PGV_L2SQ, api.PGV_F32, 256, queries, rows, bits, 200, 10,
                                                 want_candidates=True)
    wh, wc = bm.hamming_topk(bm.binary_quantize(queries), bits, 200)
    assert np.array_equal(cand, wc) and np.array_equal(hamming, wh)
    wd, wi = bm.rerank(oracle, api.PGV_L2SQ, False, queries, rows, wc, 10)
    for q in range(16):
        assert_topk_equiv(idx[q].tolist(), dist[q], wi[q].tolist(), wd[q], what="binary_search q%d" % q)
    d2, i2 = api.binary_search(ctx, api.PGV_L2SQ, api.PGV_F32, 256, queries, rows, bits, 200, 10)
    assert np.array_equal(i2, idx) and np.array_equal(d2, dist)
