"""Run by tests/test_gpu_probe_prune.py in a process of its own with PGV_SCAN_SHADOW=1: every call of prune_cases() with
PGV_PROBE_PRUNE=1 and =0 (read at every batch), through pgv_search_batch (the fused route: the ranking's recheck and
batch_fix_kernel prune where they emit) and through pgv_rank_lists + pgv_scan_batch (the unfused route: probe_prune_kernel in
front of the plan), profiling on.  Answers and counters go to the .npz named on the command line.  Prints 'PRUNE-OK <calls>'.

The cases are built here so that the CPU tests can check, with the host model, that they reach what they are for."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mp_prescan_chain_worker import _index, _queries, tids_of  # noqa: E402

LISTS = 64
STAT_KEYS = ("scan_pairs", "scan_rows", "scan_unique_rows", "scan_pruned_probes", "scan_shadow_queries", "scan_widened_queries",
             "scan_redo_queries")
PLANTED_DIM = 16
# planted queries, by row of the `planted` query set
Q_OUTLIER, Q_SHORT, Q_STARVED, Q_EMPTY_MID, Q_NAN, Q_INF, Q_TINY = range(7)
OUTLIER_LIST = 7


def planted_index():
    """Integer coordinates: every difference, square and sum stays below 2^24 and is exact in fp32 in any order.  Center l
    sits at 64 * (the six bits of l) in the first six coordinates, so its nearest neighbours are the six lists one bit
    away, exactly 64 from it; rows are their center plus integer offsets in [-2, 2] in coordinates 6 .. 15 (R <= 6.4).
    Lists of 40 rows, except
        list 7          one more row, an outlier one step from list 5's center: R_7 ~ 64.008
        list 1          3 rows  (Q_SHORT: the nearest list holds fewer than k rows)
        lists 48, 16, 32, 49   2, 0, 1, 3 rows  (Q_STARVED probes exactly these: 6 rows in all, an empty list second)
        list 8          empty  (Q_EMPTY_MID: second in the probe order of center 40, behind a full list)
        list 4          1 row"""
    rng = np.random.default_rng(22)
    dim = PLANTED_DIM
    centers = np.zeros((LISTS, dim), dtype=np.float32)
    for l in range(LISTS):
        for b in range(6):
            centers[l, b] = 64.0 * ((l >> b) & 1)
    lens = np.full(LISTS, 40, dtype=np.int64)
    for l, n in ((1, 3), (4, 1), (OUTLIER_LIST, 41), (48, 2), (16, 0), (32, 1), (49, 3), (8, 0)):
        lens[l] = n
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.repeat(centers, lens, axis=0)
    rows[:, 6:] += rng.integers(-2, 3, (rows.shape[0], dim - 6)).astype(np.float32)
    rows[off[OUTLIER_LIST + 1] - 1] = centers[5]
    rows[off[OUTLIER_LIST + 1] - 1, 6] += 1.0
    return np.ascontiguousarray(centers), off, np.ascontiguousarray(rows.astype(np.float32))


def planted_queries(centers, off, rows, nq=128):
    """the planted rows first (Q_*), then integer queries near rows anywhere"""
    rng = np.random.default_rng(23)
    dim = centers.shape[1]
    q = rows[rng.integers(0, rows.shape[0], nq)] + rng.integers(-1, 2, (nq, dim)).astype(np.float32)
    q[Q_OUTLIER] = centers[5]     # probes 5, 1, 4, 7: list 7 is 64 away and holds the row one step from the query
    q[Q_SHORT] = centers[1]       # probes 1 (3 rows), 0, 3, 5
    q[Q_STARVED] = centers[48]    # probes 48, 16, 32, 49
    q[Q_EMPTY_MID] = centers[40]  # probes 40, 8 (empty), 32, 41
    q[Q_NAN] = q[20]
    q[Q_NAN, 3] = np.nan
    q[Q_INF] = q[21]
    q[Q_INF, 4] = np.inf
    q[Q_TINY] = np.float32(1e-41) * rng.integers(1, 9, dim).astype(np.float32)
    return np.ascontiguousarray(q.astype(np.float32))


def equal_case():
    """sqrt(d_j) - R_j exactly equal to tau, and its twin beyond it.  Lists 0 and 1: every row of list 0 is 5 from its
    center (3, 4), center 1 is 13 from center 0 (5, 12) and every row of list 1 is 8 from it: for a query AT center 0,
    tau = 0 + 5 and list 1 has 13 - 8 = 5 -- kept.  Lists 2 and 3 alike with center 3 at 15 (9, 12) from center 2: for a
    query at center 2, 15 - 8 = 7 > 5 -- dropped.  The other centers lie thousands away: always dropped.  Even queries
    sit at center 0, odd ones at center 2"""
    dim = PLANTED_DIM
    centers = np.zeros((LISTS, dim), dtype=np.float32)
    centers[:, 0] = 1000.0 * (np.arange(LISTS) // 2)
    centers[1, 1], centers[1, 2] = 5.0, 12.0
    centers[3, 1], centers[3, 2] = 9.0, 12.0
    lens = np.full(LISTS, 40, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.repeat(centers, lens, axis=0)
    for l in (0, 2):
        rows[off[l]:off[l + 1], 3] += 3.0
        rows[off[l]:off[l + 1], 4] += 4.0
    for l in (1, 3):
        rows[off[l]:off[l + 1], 5] += 8.0
    q = np.zeros((128, dim), dtype=np.float32)
    q[1::2] = centers[2]
    return np.ascontiguousarray(centers), off, np.ascontiguousarray(rows), np.ascontiguousarray(q)


def prune_cases():
    """name -> (centers, offsets, rows, [(queries, probes, k), ...])"""
    out = {}
    for dim, nq in ((64, 144), (1536, 128)):
        c, off, rows = _index(dim, dim)
        out["d%d" % dim] = (c, off, rows, [(_queries(c, off, rows, nq, dim + 1), 4, 10)])
    c, off, rows = _index(256, 14, huge=True)  # flagged ranking queries: batch_fix_kernel's emit prunes
    out["flagged"] = (c, off, rows, [(_queries(c, off, rows, 144, 15), 4, 10)])
    c, off, rows = planted_index()
    q = planted_queries(c, off, rows)
    out["planted"] = (c, off, rows, [(q, 4, 10), (q, 8, 1), (q, 1, 100), (q, 4, 100)])
    c, off, rows, q = equal_case()
    out["equal"] = (c, off, rows, [(q, 4, 10)])
    rng = np.random.default_rng(25)  # U[0, 1)^d: nothing can be dropped
    c = rng.random((LISTS, 64), dtype=np.float32)
    lens = np.full(LISTS, 90, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = rng.random((int(off[-1]), 64), dtype=np.float32)
    from prune_model import rank_lists
    assign = np.array([rank_lists(x, c, 1)[0] for x in rows])
    order = np.argsort(assign, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=LISTS))]).astype(np.int64)
    out["uniform"] = (c, off, np.ascontiguousarray(rows[order]), [(rng.random((128, 64), dtype=np.float32), 4, 10)])
    return out


def _stats(ctx):
    st = ctx.stats()
    return np.array([float(st[key]) for key in STAT_KEYS])


def main():
    from pgvector_amd import api
    assert os.environ.get("PGV_SCAN_SHADOW") == "1"
    ctx = api.Context(0)
    ctx.set_profiling(True)
    res = {}
    ncalls = 0
    for name, (centers, off, rows, calls) in prune_cases().items():
        ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, rows.shape[1], centers, off, rows, tids_of(rows.shape[0]))
        for i, (q, probes, k) in enumerate(calls):
            for mode in ("1", "0"):
                os.environ["PGV_PROBE_PRUNE"] = mode
                key = "%s.%d.p%s" % (name, i, mode)
                ctx.reset_stats()
                d, s, t = ix.search_batch(q, probes, k, want_tid=True)
                ctx.sync()
                res[key + ".d"], res[key + ".s"], res[key + ".t"] = (np.asarray(x).copy() for x in (d, s, t))
                res[key + ".stats"] = _stats(ctx)
                lists, _ = ix.rank_lists(q, probes)
                ctx.sync()
                ctx.reset_stats()
                d, s, t = ix.scan_batch(q, np.ascontiguousarray(lists, dtype=np.int32), k, want_tid=True)
                ctx.sync()
                res[key + ".lists"] = np.asarray(lists).copy()
                res[key + ".d2"], res[key + ".s2"], res[key + ".t2"] = (np.asarray(x).copy() for x in (d, s, t))
                res[key + ".stats2"] = _stats(ctx)
                ncalls += 1
        ix.close()
    ctx.close()
    np.savez(sys.argv[1], **res)
    print("PRUNE-OK %d" % ncalls)


if __name__ == "__main__":
    main()
