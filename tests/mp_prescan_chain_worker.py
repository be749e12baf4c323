"""Run by tests/test_gpu_prescan_chain.py in a process of its own with PGV_SCAN_SHADOW=1 (read when the library loads):
every case of prescan_cases() through pgv_search_batch -- the ranking over the center shadow counts the plan's lists where
it emits them, DESIGN.md 4.1 -- and through the unfused composition pgv_rank_lists + pgv_scan_batch (memset,
plan_count_kernel, shadow_pair_kernel), with profiling on; then the query cast alone (pgv_index_shadow_cast) for every row
length of cast_cases().  Answers and counters go to the .npz named on the command line.  Prints 'PRESCAN-OK <cases>'."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pgvector_amd import api  # noqa: E402
from pgvector_amd import _lib  # noqa: E402

K, LISTS = 10, 64
CAST_DIMS = (1, 63, 64, 65, 255, 257, 1536, 2000, 2100)  # (2100: past the rows the cast keeps in registers)
STAT_KEYS = ("scan_pairs", "scan_rows", "scan_unique_rows", "scan_launches", "scan_shadow_queries", "scan_widened_queries",
             "scan_redo_queries")


def tids_of(n):
    return np.arange(n, dtype=np.uint64) * 5 + 11


def _index(dim, seed, huge=False):
    """64 lists: list 0 empty, list 1 one row, list 2 longer than one task of 128 rows, ~6 000 rows in all; rows round
    their list's center.  huge: one coordinate of 4096 sets the fp16 centers' scale, and the ranking's band swallows
    its candidates (tests/mp_rank_shadow_worker.py, `huge`)"""
    rng = np.random.default_rng(seed)
    centers = rng.random((LISTS, dim), dtype=np.float32)
    if huge:
        centers[:, 5] += np.float32(4096.0)
    lens = np.full(LISTS, 92, dtype=np.int64)
    lens[0], lens[1], lens[2] = 0, 1, 300
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.repeat(centers, lens, axis=0) + np.float32(0.1) * rng.standard_normal((int(off[-1]), dim)).astype(np.float32)
    return np.ascontiguousarray(centers), off, np.ascontiguousarray(rows.astype(np.float32))


def _queries(centers, off, rows, nq, seed):
    """40 queries round list 2's center (two query groups of 32 on that list), the others near rows anywhere"""
    rng = np.random.default_rng(seed)
    dim = rows.shape[1]
    q = rows[rng.integers(0, rows.shape[0], nq)] + np.float32(0.05) * rng.standard_normal((nq, dim)).astype(np.float32)
    q[:40] = centers[2] + np.float32(0.05) * rng.standard_normal((40, dim)).astype(np.float32)
    q[40] = centers[0]  # the empty list is probed
    q[41] = centers[1]  # ... and the list of one row
    return np.ascontiguousarray(q.astype(np.float32))


def prescan_cases():
    """name -> (centers, offsets, rows, [(queries, probes), ...]): the calls run one after the other on ONE context"""
    out = {}
    for dim, nq in ((64, 144), (100, 131), (1536, 128)):
        c, off, rows = _index(dim, dim)
        out["d%d" % dim] = (c, off, rows, [(_queries(c, off, rows, nq, dim + 1), 4)])
    # consecutive calls with other nq and fewer and fewer lists: a counter the first call left must not survive
    c, off, rows = _index(100, 7)
    out["repeat"] = (c, off, rows, [(_queries(c, off, rows, 160, 8), 8), (_queries(c, off, rows, 128, 9), 4),
                                    (_queries(c, off, rows, 136, 10), 2)])
    # fewer centers than probes + 54 (the ranking takes all 64 as candidates), and every list probed
    c, off, rows = _index(64, 11)
    out["allcand"] = (c, off, rows, [(_queries(c, off, rows, 130, 12), 16), (_queries(c, off, rows, 128, 13), LISTS)])
    # flagged ranking queries: batch_fix_kernel replaces the lists the recheck emitted and counted
    c, off, rows = _index(256, 14, huge=True)
    out["flagged"] = (c, off, rows, [(_queries(c, off, rows, 144, 15), 4)])
    return out


def cast_cases():
    """dim -> (centers, offsets, rows, queries): queries of mixed magnitude, one all zero, one subnormal, one with a NaN"""
    out = {}
    for dim in CAST_DIMS:
        rng = np.random.default_rng(1000 + dim)
        centers = rng.random((8, dim), dtype=np.float32)
        off = (np.arange(9) * 12).astype(np.int64)
        rows = np.repeat(centers, 12, axis=0) + np.float32(0.1) * rng.standard_normal((96, dim)).astype(np.float32)
        q = rng.standard_normal((12, dim)).astype(np.float32) * (np.float32(2.0) ** rng.integers(-6, 7, (12, 1))).astype(np.float32)
        q[9] = 0.0
        q[10] = np.float32(1e-41) * rng.integers(1, 9, dim).astype(np.float32)
        q[11, dim // 2] = np.nan
        out[dim] = (np.ascontiguousarray(centers), off, np.ascontiguousarray(rows.astype(np.float32)), np.ascontiguousarray(q))
    return out


def _stats(ctx):
    st = ctx.stats()
    return np.array([float(st[key]) for key in STAT_KEYS])


def main():
    assert os.environ.get("PGV_SCAN_SHADOW") == "1" and os.environ.get("PGV_RANK_SHADOW", "1") == "1"
    ctx = api.Context(0)
    ctx.set_profiling(True)
    res = {}
    cases = prescan_cases()
    for name, (centers, off, rows, calls) in cases.items():
        ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, rows.shape[1], centers, off, rows, tids_of(rows.shape[0]))
        for i, (q, probes) in enumerate(calls):  # the fused calls back to back: nothing else touches the context between
            ctx.reset_stats()
            d, s, t = ix.search_batch(q, probes, K, want_tid=True)
            ctx.sync()
            key = "%s.%d" % (name, i)
            res[key + ".d"], res[key + ".s"], res[key + ".t"] = (np.asarray(x).copy() for x in (d, s, t))
            res[key + ".stats"] = _stats(ctx)
        for i, (q, probes) in enumerate(calls):
            key = "%s.%d" % (name, i)
            ctx.reset_stats()
            lists, _ = ix.rank_lists(q, probes)
            ctx.sync()
            res[key + ".rank_stats"] = _stats(ctx)
            ctx.reset_stats()
            d, s, t = ix.scan_batch(q, np.ascontiguousarray(lists, dtype=np.int32), K, want_tid=True)
            ctx.sync()
            res[key + ".lists"] = np.asarray(lists).copy()
            res[key + ".d2"], res[key + ".s2"], res[key + ".t2"] = (np.asarray(x).copy() for x in (d, s, t))
            res[key + ".stats2"] = _stats(ctx)
        ix.close()
    for dim, (centers, off, rows, q) in cast_cases().items():
        ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, dim, centers, off, rows, tids_of(rows.shape[0]))
        nq, ld16 = q.shape[0], (dim + 7) // 8 * 8
        qcast = np.full((nq, ld16), 0x7e00, dtype=np.uint16)
        terms = [np.full(nq, np.nan, dtype=np.float32) for _ in range(4)]
        api.check(_lib.lib.pgv_index_shadow_cast(ix.h, api.ptr(q), nq, api.ptr(qcast), *[api.ptr(x) for x in terms]))
        res["cast%d.qcast" % dim] = qcast
        for key, x in zip(("qscale", "qeps", "cscale", "ceps"), terms):
            res["cast%d.%s" % (dim, key)] = x
        ix.close()
    ctx.close()
    np.savez(sys.argv[1], **res)
    print("PRESCAN-OK %d" % (len(cases) + len(CAST_DIMS)))


if __name__ == "__main__":
    main()
