"""Run by tests/test_gpu_rank_shadow.py in a process of its own under one PGV_RANK_SHADOW setting (0: fp32 ranking and
shadow_pair_kernel, 1: fp16 center-shadow ranking whose recheck hands the pair terms on, 2: fp16 ranking and
shadow_pair_kernel) with PGV_SCAN_SHADOW=1: every case of rank_shadow_cases() through pgv_rank_lists, pgv_search_batch and
pgv_rank_lists + pgv_scan_batch, the answers and the counters written to the .npz named on the command line.  The parent
compares the settings with each other and with the oracle.  Prints 'RANK-SHADOW-OK <cases>'."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pgvector_amd import api  # noqa: E402

PROBES, K = 10, 10


def _tids(n):
    return np.arange(n, dtype=np.uint64) * 7 + 3


def _index_arrays(centers, nq, per_list, seed, sigma):
    """rows list-major round their centers (every list per_list rows), queries near rows"""
    rng = np.random.default_rng(seed)
    nlists, dim = centers.shape
    off = (np.arange(nlists + 1) * per_list).astype(np.int64)
    rows = np.repeat(centers, per_list, axis=0) + np.float32(sigma) * rng.standard_normal((nlists * per_list, dim)).astype(np.float32)
    q = rows[rng.integers(0, rows.shape[0], nq)] + np.float32(sigma / 2) * rng.standard_normal((nq, dim)).astype(np.float32)
    return np.ascontiguousarray(rows.astype(np.float32)), off, np.ascontiguousarray(q.astype(np.float32))


def near_tie_centers(seed, k, dim):
    """the construction of tests/test_gpu_round6.py: integer centers in groups of two that differ by 1 in one coordinate
    (every fourth group: in two), queries = a center of the group + integer noise with those coordinates set on purpose, so
    that the squared distances to the two centers are exact in fp32 and 0, 1 or 2 ulp apart at 2^23 .. 2^24"""
    rng = np.random.default_rng(seed)
    amp = int(np.sqrt(3 * 1.15e7 / dim))
    base = rng.integers(400, 1600, (k // 2, dim)).astype(np.float32)
    centers = np.repeat(base, 2, axis=0)
    jj = rng.integers(0, dim, k // 2)
    ll = (jj + 1 + rng.integers(0, dim - 1, k // 2)) % dim
    two = (np.arange(k // 2) % 4) == 0
    for g in range(k // 2):
        centers[2 * g + 1, jj[g]] += 1.0
        if two[g]:
            centers[2 * g + 1, ll[g]] -= 1.0

    def rows_near(n, seed2):
        r2 = np.random.default_rng(seed2)
        grp = r2.integers(0, k // 2, n)
        rows = base[grp] + r2.integers(-amp, amp + 1, (n, dim)).astype(np.float32)
        r = np.arange(n)
        rows[r, jj[grp]] = base[grp, jj[grp]] + r2.integers(0, 2, n)
        rows[r, ll[grp]] = np.where(two[grp], base[grp, ll[grp]] + r2.integers(0, 2, n), rows[r, ll[grp]])
        return np.ascontiguousarray(rows)
    return np.ascontiguousarray(centers), rows_near


def rank_shadow_cases():
    """name -> (centers, list offsets, rows, queries); seeded, the same in every process"""
    out = {}
    rng = np.random.default_rng(41)
    # the clustered mixture: 50 components, four lists each
    means = rng.random((50, 256), dtype=np.float32)
    centers = means[np.arange(200) % 50] + np.float32(0.02) * rng.standard_normal((200, 256)).astype(np.float32)
    rows, off, q = _index_arrays(np.ascontiguousarray(centers), 256, 60, 1, 0.1)
    out["mixture"] = (np.ascontiguousarray(centers), off, rows, q)
    # uniform data, a row length with a partial last slice
    centers = rng.random((128, 100), dtype=np.float32)
    rows, off, q = _index_arrays(centers, 256, 80, 2, 0.3)
    out["uniform"] = (centers, off, rows, q)
    # centers 0 / 1 / 2 ulp apart
    centers, rows_near = near_tie_centers(263, 256, 256)
    rows = rows_near(256 * 40, 5)
    # rows list-major by their nearest center (float64 on integer data: exact; ties to the lower id)
    lst = np.empty(rows.shape[0], dtype=np.int64)
    c64 = centers.astype(np.float64)
    for a in range(0, rows.shape[0], 1024):
        x = rows[a:a + 1024].astype(np.float64)
        dd = (x * x).sum(1)[:, None] + (c64 * c64).sum(1)[None, :] - 2.0 * x @ c64.T
        lst[a:a + 1024] = np.argmin(dd, axis=1)
    order = np.argsort(lst, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(lst, minlength=256))]).astype(np.int64)
    out["ulp"] = (centers, off, np.ascontiguousarray(rows[order]), rows_near(256, 6))
    # centers (and rows, queries) with one huge coordinate: the one scale of the fp16 copy leaves the others ~2^-12 each
    centers = rng.random((200, 256), dtype=np.float32)
    centers[:, 5] += np.float32(4096.0)
    rows, off, q = _index_arrays(centers, 256, 60, 3, 0.1)
    out["huge"] = (centers, off, rows, q)
    # NaN in a center: no shadow at all, the fp32 paths answer
    centers = rng.random((160, 128), dtype=np.float32)
    rows, off, q = _index_arrays(centers, 256, 50, 4, 0.1)
    centers = centers.copy()
    centers[7, 9] = np.nan
    out["nan"] = (centers, off, rows, q)
    return out


def main():
    assert os.environ.get("PGV_SCAN_SHADOW") == "1" and os.environ.get("PGV_RANK_SHADOW") in ("0", "1", "2")
    ctx = api.Context(0)
    ctx.set_profiling(True)
    res = {}
    cases = rank_shadow_cases()
    for name, (centers, off, rows, q) in cases.items():
        dim = rows.shape[1]
        ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, dim, centers, off, rows, _tids(rows.shape[0]))
        ctx.reset_stats()
        lists, ldist = ix.rank_lists(q, PROBES)
        ctx.sync()
        st = ctx.stats()
        res[name + ".rank_ids"], res[name + ".rank_dist"] = np.asarray(lists).copy(), np.asarray(ldist).copy()
        res[name + ".rank_flagged"] = np.array([st["scan_widened_queries"], st["scan_redo_queries"]])
        ctx.reset_stats()
        d, s, t = ix.search_batch(q, PROBES, K, want_tid=True)
        ctx.sync()
        st = ctx.stats()
        res[name + ".d"], res[name + ".s"], res[name + ".t"] = (np.asarray(x).copy() for x in (d, s, t))
        res[name + ".shadow_queries"] = np.array([st["scan_shadow_queries"]])
        # the lists through the caller: pgv_scan_batch casts for itself and runs shadow_pair_kernel
        d2, s2, t2 = ix.scan_batch(q, np.ascontiguousarray(lists, dtype=np.int32), K, want_tid=True)
        ctx.sync()
        res[name + ".d2"], res[name + ".s2"], res[name + ".t2"] = (np.asarray(x).copy() for x in (d2, s2, t2))
        ix.close()
    ctx.close()
    np.savez(sys.argv[1], **res)
    print("RANK-SHADOW-OK %d" % len(cases))


if __name__ == "__main__":
    main()
