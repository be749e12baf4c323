"""pgv_bit_jaccard_topk (jaccard_tile_kernel, the top-k selection over its order images, jaccard_values_kernel) against the
exact fractions of tests/jaccard_model.py: each query's rows sorted by (Fraction, row index), the values the reference's
float8 as a float.  Every comparison is equality: indexes as lists, distances by their bit patterns."""
import numpy as np
import pytest

import jaccard_model as jm
from pgvector_amd import _lib, api

pytestmark = pytest.mark.gpu


def model(queries, rows, k):
    n = rows.shape[0]
    dist = np.full((queries.shape[0], k), np.inf, dtype=np.float32)
    idx = np.full((queries.shape[0], k), -1, dtype=np.int64)
    for q, query in enumerate(queries):
        x, u = jm.counts(query, rows) if n else ((), ())
        fr = [jm.fraction(a, b) for a, b in zip(x, u)]
        for j, r in enumerate(sorted(range(n), key=lambda r: (fr[r], r))[:k]):
            dist[q, j], idx[q, j] = jm.ref_float(x[r], u[r]), r
    return dist, idx


def check(got, want, what):
    (dist, idx), (wd, wi) = got, want
    assert idx.tolist() == wi.tolist(), (what, "indexes", np.argwhere(idx != wi)[:5].tolist())
    assert np.array_equal(dist.view(np.uint32), wd.view(np.uint32)), (what, "distances", np.argwhere(dist != wd)[:5].tolist())


def mixed_bits(n, nbits, seed):
    """rows of bit density about 0.02, 0.5 and 0.98 in turn, pad bits zero"""
    rng = np.random.default_rng(seed)
    bits = rng.random((n, nbits)) < np.array([.02, .5, .98])[np.arange(n) % 3, None]
    return np.packbits(bits, axis=1)


# every nbits (the byte, the 16-byte vector, the 1024-bit register slice), n (the 256-row tile) and nq (the 32-query tile)
# appears; k is 1, 10 or n + 3 (the padding)
@pytest.mark.parametrize("nbits,n,nq,k", [(1, 1, 1, 1), (7, 255, 31, 10), (8, 256, 32, 10), (127, 257, 33, 260), (128, 700, 1, 703),
                                          (129, 255, 32, 1), (1023, 256, 33, 10), (1024, 257, 31, 10), (1025, 700, 33, 10),
                                          (2049, 700, 32, 10), (2049, 1, 33, 4)])
def test_random_strings(ctx, nbits, n, nq, k):
    rows, queries = mixed_bits(n, nbits, 100 + nbits), mixed_bits(nq, nbits, 200 + n)
    if n >= 6:
        rows[2] = 0               # an all-zero row: x = u against every query
        rows[4] = rows[3]         # two identical rows tie, the lower index first
        rows[5] = queries[0]      # distance 0
    if nq > 1:
        queries[-1] = 0           # an all-zero query: u = 0 against the zero row, x = u against the rest -- all tie at 1
    check(api.bit_jaccard_topk(ctx, nbits, queries, rows, k), model(queries, rows, k), (nbits, n, nq, k))


def test_farey_neighbours_at_64000_bits(ctx):
    """two neighbouring ratios that round to ONE fp32 value, the larger in the lower row: any float-keyed order takes the
    tie to the lower index and answers q before p"""
    p, q = next(pr for pr in jm.farey_pairs(least=jm.Fraction(1, 2)) if jm.fp32_key(*pr[0]) == jm.fp32_key(*pr[1]))
    assert jm.fraction(*p) < jm.fraction(*q)
    xu = [(63000, 64000), q, p, (16000, 48000), q, (0, 32000), p]
    rows, query = np.stack([jm.planted_row(x, u) for x, u in xu]), jm.planted_query()
    want = model(query, rows, 8)
    assert want[1][0].tolist() == [5, 3, 2, 6, 1, 4, 0, -1]
    check(api.bit_jaccard_topk(ctx, jm.MAX_BITS, query, rows, 8), want, "farey")


def test_two_chunks(ctx):
    """2^20 + 3 rows: the chunk is 2^30 // n = 1023 -> 992 queries, 1056 queries are two chunks.  One byte a string: the
    expected order comes from the 256 x 256 table of fractions, ranked once; a query's k best are among the first k rows
    of each byte value"""
    n, nq, k = (1 << 20) + 3, 1056, 5
    rng = np.random.default_rng(7)
    rows, queries = rng.integers(0, 256, (n, 1), dtype=np.uint8), rng.integers(0, 256, (nq, 1), dtype=np.uint8)
    vals = np.arange(256, dtype=np.uint8)
    fr = [jm.fractions_of(vals[a:a + 1], vals[:, None]) for a in range(256)]
    order = {f: i for i, f in enumerate(sorted({f for row in fr for f in row}))}
    rank = np.array([[order[f] for f in row] for row in fr])
    cand = np.concatenate([np.flatnonzero(rows[:, 0] == b)[:k] for b in range(256)])
    wi = np.stack([cand[np.lexsort((cand, rank[a, rows[cand, 0]]))[:k]] for a in queries[:, 0]])
    x, u = jm.POPCOUNT[rows[wi, 0] ^ queries], jm.POPCOUNT[rows[wi, 0] | queries]
    wd = np.array([[jm.ref_float(a, b) for a, b in zip(xs, us)] for xs, us in zip(x, u)], dtype=np.float32)
    import torch
    dev_rows = torch.from_numpy(rows).cuda()  # (a million one-byte rows pad on the device in no time; from the host it takes seconds)
    check(api.bit_jaccard_topk(ctx, 8, queries, dev_rows, k), (wd, wi), "two chunks")


@pytest.mark.parametrize("nbits", [256, 136])  # rows used in place (32 bytes) and staged (17 bytes)
def test_device_arrays_give_the_host_call(ctx, nbits):
    import torch
    rows, queries = mixed_bits(300, nbits, 5), mixed_bits(33, nbits, 6)
    want = api.bit_jaccard_topk(ctx, nbits, queries, rows, 10)
    out = (torch.empty((33, 10), dtype=torch.float32, device="cuda"), torch.empty((33, 10), dtype=torch.int64, device="cuda"))
    api.bit_jaccard_topk(ctx, nbits, torch.from_numpy(queries).cuda(), torch.from_numpy(rows).cuda(), 10, out=out)
    ctx.sync()
    check((out[0].cpu().numpy(), out[1].cpu().numpy()), want, nbits)


@pytest.mark.parametrize("nbits,k,code", [(64001, 10, _lib.PGV_ERR_DIMS), (64, 0, api.PGV_ERR_ARG), (64, 4097, api.PGV_ERR_ARG)])
def test_refusals(ctx, nbits, k, code):
    nbytes = (nbits + 7) // 8
    with pytest.raises(api.PgvError) as e:
        api.bit_jaccard_topk(ctx, nbits, np.zeros((2, nbytes), np.uint8), np.zeros((20, nbytes), np.uint8), k)
    assert e.value.code == code


@pytest.mark.parametrize("n", [3, 20])
def test_empty_strings(ctx, n):
    dist, idx = api.bit_jaccard_topk(ctx, 0, np.zeros((2, 0), np.uint8), np.zeros((n, 0), np.uint8), 10)
    m = min(n, 10)
    assert idx.tolist() == [list(range(m)) + [-1] * (10 - m)] * 2
    assert dist[:, :m].tolist() == [[1.0] * m] * 2 and np.isposinf(dist[:, m:]).all()
