"""The single-query path (pgv_query_rank / pgv_query_scan) and the few-queries path of pgv_rank_lists /
pgv_search_batch launch the SAME query_rank / query_lists / query_scan kernels, the first with one grid row, the second
with one grid row per query.  Pinned here: grid row q reads query q and writes row q, and row 0 of a one-row launch
answers like any row of a wider one.  Both sides run the same instantiation over the same rows, so every comparison is
exact: list ids, slots, tids and the bit patterns of the distances."""
import numpy as np
import pytest

from oracle import pyoracle as po
from pgvector_amd import api

from helpers import gen

pytestmark = pytest.mark.gpu

N, LISTS, PROBES, K = 3000, 40, 5, 20
EMPTY = 7  # the list nothing is assigned to; its center is queries[1], so an L2 ranking probes it first
ORA = {api.PGV_F32: po.ORA_F32, api.PGV_F16: po.ORA_F16}


def _np_dist(metric, rows, q):
    rows, q = rows.astype(np.float64), q.astype(np.float64)
    return ((rows - q) ** 2).sum(axis=1) if metric == api.PGV_L2SQ else -(rows @ q)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).tolist()


def _image(metric, dtype, dim):
    """an IVFFlat image laid out list-major (rows go to their nearest center but EMPTY's), three queries, and one row of
    query 0's probed lists overwritten with a copy of its K-th nearest: entries K - 1 and K of its stream tie exactly"""
    data = gen(N, dim, seed=2301, dist="clustered", clusters=LISTS, dtype=ORA[dtype])
    queries = gen(3, dim, seed=2302, dist="clustered", clusters=LISTS, dtype=ORA[dtype])
    centers = np.ascontiguousarray(data[np.random.default_rng(2303).choice(N, LISTS, replace=False)])
    centers[EMPTY] = queries[1]
    x, c = data.astype(np.float32), centers.astype(np.float32)
    d = (x * x).sum(axis=1)[:, None] - 2.0 * (x @ c.T) + (c * c).sum(axis=1)[None, :]
    d[:, EMPTY] = np.inf
    lists = d.argmin(axis=1)
    vectors = np.ascontiguousarray(data[np.argsort(lists, kind="stable")])
    off = np.concatenate([[0], np.cumsum(np.bincount(lists, minlength=LISTS))]).astype(np.int64)
    assert off[EMPTY] == off[EMPTY + 1]
    tids = (np.arange(N, dtype=np.uint64) << np.uint64(16)) | np.uint64(1)
    probed = np.argsort(_np_dist(metric, centers, queries[0]), kind="stable")[:PROBES]
    slots = np.concatenate([np.arange(off[l], off[l + 1]) for l in probed])
    by = slots[np.argsort(_np_dist(metric, vectors[slots], queries[0]), kind="stable")]
    vectors[by[-1]] = vectors[by[K - 1]]
    return centers, off, vectors, tids, queries


@pytest.mark.parametrize("metric,dtype,dim", [
    (api.PGV_L2SQ, api.PGV_F32, 256),    # whole 1 KiB rows, one slice (NCH 1)
    (api.PGV_NEG_IP, api.PGV_F32, 256),
    (api.PGV_L2SQ, api.PGV_F32, 1536),   # six slices (NCH 6)
    (api.PGV_L2SQ, api.PGV_F16, 512),    # fp16, one slice
    (api.PGV_L2SQ, api.PGV_F32, 100),    # the generic loop, 32 lanes per row
    (api.PGV_L2SQ, api.PGV_F32, 5),      # the generic loop, 2 lanes per row
])
def test_grid_row_q_answers_like_query_q_alone(ctx, metric, dtype, dim):
    centers, off, vectors, tids, queries = _image(metric, dtype, dim)
    ix = api.IvfIndex(ctx, metric, dtype, dim, centers, off, vectors, tids)
    blists, _ = ix.rank_lists(queries, PROBES)                           # nq = 3 <= 24: one grid row per query
    bdist, bslot, btid = ix.search_batch(queries, PROBES, K, want_tid=True)  # nq = 3 <= 4: likewise
    qh = api.Query(ix)
    for i in range(3):
        qh.rank(queries[i], PROBES)
        lists = qh.lists(PROBES)
        assert lists.tolist() == blists[i].tolist(), i
        d, s, t, total = qh.scan(0, PROBES, K)
        assert total == sum(int(off[l + 1] - off[l]) for l in lists) and len(s) == K, i
        assert s.tolist() == bslot[i].tolist() and t.tolist() == btid[i].tolist(), i
        assert _bits(d) == _bits(bdist[i]), i
        if i == 0:  # the planted tie crosses the head: entry K of the stream has entry K - 1's distance
            nxt, nslot, _ = qh.more(K, 1)
            assert _bits(nxt) == _bits(d[K - 1:]) and nslot[0] != s[K - 1]
    if metric == api.PGV_L2SQ:
        assert blists[1][0] == EMPTY  # an empty list among the probed
    assert len({tuple(_bits(r)) for r in bdist}) == 3  # three answers: no row was computed from another row's query
    qh.close()
    ix.close()


def test_rank_kernel_over_contiguous_rows_is_the_center_ranking(ctx):
    """pgv_distance_batch (one query over rows, dense_scan's nq == 1 path) and the center ranking are one launcher over
    one kernel: the same rows as centers give the same bits"""
    dim, n = 256, 64
    rows = gen(n, dim, seed=2311, dist="normal")
    q = gen(1, dim, seed=2312, dist="normal")
    got = api.distance_batch(ctx, api.PGV_L2SQ, api.PGV_F32, dim, q[0], rows)
    ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, dim, rows, np.arange(n + 1), rows)  # every row its own list
    lists, dist = ix.rank_lists(q, n)
    assert sorted(lists[0].tolist()) == list(range(n))
    assert _bits(got[lists[0]]) == _bits(dist[0])
    ix.close()
