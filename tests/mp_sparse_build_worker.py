"""Shared by tests/test_gpu_sparse_hnsw_build.py and its child process: the inputs of the pgv_hnsw_score_groups cases over
sparse rows, and the job that needs a process of its own --

  mp_sparse_build_worker.py groups OUT.npz   every groups case on the device, with whatever PGV_HNSW_PAIRS_GATHER the
                                             parent set (the variable is read once per process).  Prints 'GROUPS-OK <n>'.

Nothing here looks at a model's results: the parent compares."""
import sys

import numpy as np

import sparse_hnsw_model as shm
import sparse_model as sm
from pgvector_amd import api

# 0 twice (a pair of empty rows), the ends of the register chunks, 256 = the last register row, 257 = the first
# row_side_mem row, 1000 = HNSW_MAX_NNZ
GROUP_LENGTHS = (0, 0, 1, 63, 64, 65, 256, 257, 1000)
GROUP_SIZES = (1, 2, 4, 5, 9, 33, 80)
GROUP_ROWS = 96
GROUP_DIM = 3000
DATA = ("float", "int")
METRICS = (api.PGV_L2SQ, api.PGV_NEG_IP, api.PGV_L1)
MODEL_METRIC = {api.PGV_L2SQ: sm.L2SQ, api.PGV_NEG_IP: sm.NEG_IP, api.PGV_L1: sm.L1}


def group_pairs(n, frm):
    frm = max(frm, 1)
    return (n * (n - 1) - frm * (frm - 1)) // 2 if n > frm else 0


def groups_rows(data):
    """96 rows over 3000 dimensions: the special lengths three times over (slots 0 .. 26), then lengths 2 .. 400.  Rows share
    indices in plenty (a 1000-element row holds a third of the dimensions), so hits, row-side misses and query-side
    misses all occur in a pair"""
    rng = np.random.default_rng(31)
    lengths = list(GROUP_LENGTHS) * 3 + rng.integers(2, 401, GROUP_ROWS - 3 * len(GROUP_LENGTHS)).tolist()
    return shm.rand_csr(lengths, 9100, dim=GROUP_DIM, floats=(data == "float"))


def groups_input():
    """every size with from = 1, 3, n - 1, n, n + 2 (the last two, and whatever is past the size, want no pairs: empty groups
    between full ones).  A group is distinct slots in random order, so both orientations occur under every local order;
    the first group of every size holds the two empty rows and the 256 / 257 / 1000-element ones
    -> ids, ids_start, from, pair_start, and the pairs expanded (a[i], b[i]) in the order the values are written"""
    rng = np.random.default_rng(77)
    ids, start, frm, pstart, a, b = [], [0], [], [0], [], []
    for n in GROUP_SIZES:
        for k, f in enumerate((1, 3, n - 1, n, n + 2)):
            g = rng.permutation(GROUP_ROWS)[:n].tolist()
            if k == 0:
                special = [0, 1, 6, 7, 8][:n]
                g = special + [x for x in g if x not in special][:n - len(special)]
                g = [g[i] for i in rng.permutation(n)]
            ids += g
            start.append(len(ids))
            frm.append(f)
            for u in range(max(f, 1), n):
                a += [g[u]] * u
                b += g[:u]
            pstart.append(pstart[-1] + group_pairs(n, f))
    assert pstart[-1] == len(a)
    return (np.asarray(ids, np.int32), np.asarray(start, np.int64), np.asarray(frm, np.int32), np.asarray(pstart, np.int64),
            np.asarray(a, np.int32), np.asarray(b, np.int32))


def groups_on_device(ctx):
    """-> {"groups/<data>/<metric>": pgv_hnsw_score_groups' values, "pairs/..": pgv_hnsw_score_pairs(min slot, max slot) over
    the same pairs, "swapped/..": pgv_hnsw_score_pairs(max slot, min slot)}"""
    ids, ids_start, frm, pair_start, a, b = groups_input()
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    res = {}
    for data in DATA:
        rows = groups_rows(data)
        for metric in METRICS:
            h = api.SparseHnsw(ctx, metric, GROUP_DIM, rows, buildable=True)
            try:
                got = np.full(len(a), np.nan, np.float32)
                api.check(api.lib.pgv_hnsw_score_groups(h.h, api.ptr(ids), api.ptr(ids_start), api.ptr(frm), api.ptr(pair_start),
                                                        len(frm), len(ids), len(a), api.ptr(got)))
                key = "%s/%d" % (data, metric)
                res["groups/" + key], res["pairs/" + key], res["swapped/" + key] = got, h.score_pairs(lo, hi), h.score_pairs(hi, lo)
            finally:
                h.close()
    return res


if __name__ == "__main__":
    assert sys.argv[1] == "groups"
    c = api.Context(0)
    out = groups_on_device(c)
    np.savez(sys.argv[2], **out)
    c.close()
    print("GROUPS-OK %d" % (len(out) // 3))
