"""Run by tests/test_gpu_shadow_edges.py in a process of its own, under PGV_SCAN_SHADOW=1 and the PGV_SCAN_WIDE /
PGV_SCAN_DEEP the parent chose (the library reads those two once per process): the fp16 shadow scan in whichever form
they select, with tasks of <= 16 queries (the 16-wide path), 17 .. 32 and 33 .. 64 (the 64-query form's upper half),
ragged last tasks, and an index of ~2.2 GB of fp32 rows whose shadow (>= 1 GiB) streams past the caches (the NT forms).
Every answer against a reference and against the same index without the shadow.  Prints
'SHADOW-FORMS-OK <cases> <shadow queries>' on success."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import assert_topk_equiv  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from pgvector_amd import api  # noqa: E402

PER_LIST = (10, 25, 50)  # queries probing list 0, 1, 2: the three widths of a task


def _tids(n):
    return np.arange(n, dtype=np.uint64) * 7 + 3


def _data(dim, sizes, seed):
    """rows around one center per list, every row distinct: a block of Gaussian noise, rotated by one element per block
    of rows (generating 2 GB of fresh noise would take longer than the GPU work)"""
    rng = np.random.default_rng(seed)
    nlists = len(sizes)
    centers = rng.random((nlists, dim), dtype=np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    noise = np.float32(0.1) * rng.standard_normal((1024, dim)).astype(np.float32)
    rows = np.empty((n, dim), dtype=np.float32)
    for b in range(0, n, 1024):
        e = min(n, b + 1024)
        rows[b:e] = np.roll(noise, b // 1024, axis=1)[:e - b]
    lst = np.repeat(np.arange(nlists), sizes)
    for l in range(nlists):
        rows[off[l]:off[l + 1]] += centers[l]
    lists = np.concatenate([np.full(c, l, dtype=np.int32) for l, c in enumerate(PER_LIST)])[:, None]
    pick = np.concatenate([rng.integers(off[l], off[l + 1], c) for l, c in enumerate(PER_LIST)])
    queries = rows[pick] + np.float32(0.05) * rng.standard_normal((len(pick), dim)).astype(np.float32)
    assert (lst[pick] == lists[:, 0]).all()
    return rows, centers, off, np.ascontiguousarray(queries, dtype=np.float32), np.ascontiguousarray(lists)


def _run(ctx, env, dim, rows, centers, off, queries, lists, k):
    os.environ["PGV_SCAN_SHADOW"] = env
    ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, dim, centers, off, rows, _tids(rows.shape[0]))
    ctx.reset_stats()
    d, s, t = ix.scan_batch(queries, lists, k, want_tid=True)
    ctx.sync()
    st = ctx.stats()
    ix.close()
    return (np.asarray(d).copy(), np.asarray(s).copy(), np.asarray(t).copy()), st


def _reference_fp64(rows, off, queries, lists, k):
    """top k of every query over its probed lists, distances in float64 (chunks of rows)"""
    part = [([], []) for _ in range(lists.shape[0])]
    for l in np.unique(lists):
        qi = np.flatnonzero((lists == l).any(axis=1))
        q = queries[qi].astype(np.float64)
        a, b = int(off[l]), int(off[l + 1])
        d = np.empty((len(qi), b - a))
        for c in range(a, b, 2048):
            x = rows[c:min(b, c + 2048)].astype(np.float64)
            d[:, c - a:c - a + x.shape[0]] = (x * x).sum(1)[None, :] + (q * q).sum(1)[:, None] - 2.0 * q @ x.T
        for j, i in enumerate(qi):
            o = np.argsort(d[j], kind="stable")[:k]
            part[i][0].append(a + o)
            part[i][1].append(d[j][o])
    out = []
    for ws, wd in part:
        ws, wd = np.concatenate(ws), np.concatenate(wd)
        o = np.lexsort((ws, wd))[:k]
        out.append((ws[o], wd[o]))
    return out


def main():
    assert os.environ.get("PGV_SCAN_SHADOW") == "1"
    oracle = po.Oracle()
    ctx = api.Context(0)
    ctx.set_profiling(True)
    cases, shadow_queries = 0, 0.0
    # (dim, list sizes, k): a small index (plain loads) and one whose shadow is >= 1 GiB (streaming loads); 16000
    # dimensions keep the big index's task bound under two per CU, so that the three-stage form can take it too
    # each index twice: every query on its own list (tasks of 10, 25 and 50 queries), then on all three lists (85 a
    # list: a query's rows in different lists carry different pair terms t)
    for dim, sizes, k, every in ((256, (300, 457, 611), 10, False), (200, (129, 1000, 77), 64, False),
                                 (200, (129, 1000, 77), 10, True), (16000, (11000, 11500, 11600), 10, False),
                                 (16000, (11000, 11500, 11600), 10, True)):
        rows, centers, off, queries, lists = _data(dim, sizes, seed=dim)
        if every:
            lists = np.ascontiguousarray(np.tile(np.arange(3, dtype=np.int32), (queries.shape[0], 1)))
        big = rows.nbytes >= 2 << 30
        a, sa = _run(ctx, "1", dim, rows, centers, off, queries, lists, k)
        assert sa["scan_shadow_queries"] == queries.shape[0], sa
        shadow_queries += sa["scan_shadow_queries"]
        b, sb = _run(ctx, "0", dim, rows, centers, off, queries, lists, k)
        assert sb["scan_shadow_queries"] == 0, sb
        np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[2], b[2])
        tids = _tids(rows.shape[0])
        if big:
            want = _reference_fp64(rows, off, queries, lists, k)
        else:
            ixs = oracle.index_struct(po.OPS_L2, po.ORA_F32, centers, off, rows, tids)
            want = []
            for i in range(queries.shape[0]):
                wd, ws = oracle.get_scan_items(ixs, queries[i], lists[i])
                o = np.lexsort((ws, wd))[:k]
                want.append((ws[o], wd[o]))
        for i in range(queries.shape[0]):
            ws, wd = want[i]
            assert_topk_equiv(a[2][i].astype(np.uint64).tolist(), a[0][i], tids[ws].tolist(), wd,
                              what="dim %d q %d" % (dim, i))
        cases += 1
        del rows
    ctx.close()
    print("SHADOW-FORMS-OK %d %d wide=%s deep=%s" % (cases, shadow_queries, os.environ.get("PGV_SCAN_WIDE"),
                                                     os.environ.get("PGV_SCAN_DEEP")))


if __name__ == "__main__":
    main()
