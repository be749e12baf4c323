"""pgv_search_batch against pgv_rank_lists + pgv_scan_batch on either side of every decision the batched list scan takes
from the batch's shape (scan_batch_impl's route: per query, list-major on the vector ALUs, matrix cores, the 64-query
form; the ranking's own matrix-core threshold).

One fp32 L2 index of 8192 rows x 64-d in 64 lists, created with PGV_SCAN_SHADOW=1 so that an index this small carries
the fp16 row and center shadows: share = nq * probes / 64.  pgv_search_batch tells the ranking ahead of time what the
scan will do (the cast, the pair terms, the counted plan); the two separate calls prepare everything themselves.  Both
must return the same bytes, and both the oracle's answer."""
import numpy as np
import pytest

from helpers import CpuIvf, assert_topk_equiv, gen
from oracle import pyoracle as po
from pgvector_amd import api

pytestmark = pytest.mark.gpu

N, DIM, NLISTS = 8192, 64, 64

# (nq, probes, k): the two sides of each boundary sit next to each other
SHAPES = [
    (4, 6, 10),      # per-query route by nq <= 4
    (5, 6, 10),      # ... nq 5, share 0.47: the list-major plan
    (5, 5, 10),      # per-query route by share 0.39 <= 0.4
    (128, 1, 10),    # share 2: no matrix cores
    (128, 2, 10),    # share 4: fp16 ranking, shadow scan, fused plan
    (128, 2, 192),   # the largest head of the matrix-core scan
    (128, 2, 193),   # ... one past it: no MFMA scan
    (128, 6, 10),    # share 12.0: not the 64-query form
    (128, 7, 10),    # share 14: the 64-query form
    (127, 2, 10),    # below the ranking's 128 queries: no MFMA ranking, the scan casts for itself
]


@pytest.fixture(scope="module")
def case(ctx, oracle):
    data = gen(N, DIM, seed=41, dist="clustered", clusters=NLISTS)
    ivf = CpuIvf(oracle, po.OPS_L2, po.ORA_F32, data, NLISTS)
    rng = np.random.default_rng(42)
    base = data[rng.integers(0, N, 128)]
    queries = np.ascontiguousarray(base + np.float32(0.05) * rng.standard_normal(base.shape).astype(np.float32))
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PGV_SCAN_SHADOW", "1")
        mp.delenv("PGV_RANK_SHADOW", raising=False)
        ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, DIM, ivf.centers, ivf.list_offsets, ivf.vectors, ivf.tids)
        try:
            yield ivf, ix, queries
        finally:
            ix.close()


@pytest.mark.parametrize("nq,probes,k", SHAPES, ids=["nq%d-p%d-k%d" % s for s in SHAPES])
def test_search_batch_equals_rank_then_scan(ctx, oracle, case, nq, probes, k):
    ivf, ix, queries = case
    q = queries[:nq]
    what = "nq %d probes %d k %d" % (nq, probes, k)
    d, s, t = (np.asarray(a).copy() for a in ix.search_batch(q, probes, k, want_tid=True))
    lists, _ = ix.rank_lists(q, probes)
    d2, s2, t2 = (np.asarray(a).copy() for a in ix.scan_batch(q, lists, k, want_tid=True))
    ctx.sync()
    np.testing.assert_array_equal(d.view(np.uint32), d2.view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(s, s2, err_msg=what)
    np.testing.assert_array_equal(t, t2, err_msg=what)
    for i in range(nq):
        wt, wd = oracle.search(ivf.struct, q[i], probes, k)
        n = len(wt)
        assert_topk_equiv(t[i][:n].tolist(), d[i][:n], wt.tolist(), wd, what="%s q%d" % (what, i))
        if n < k:  # fewer rows probed than asked for: INFINITY / -1 padding
            assert np.isinf(d[i][n:]).all() and (s[i][n:] == -1).all(), (what, i)
