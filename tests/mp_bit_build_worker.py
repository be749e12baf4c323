"""Shared by tests/test_gpu_bit_hnsw_build.py and its child processes: the inputs of the pgv_hnsw_score_groups cases over
bit rows, and two jobs that need a process of their own --

  mp_bit_build_worker.py groups OUT.npz      every groups case on the device, with whatever PGV_HNSW_PAIRS_GATHER the
                                             parent set (the variable is read once per process).  Prints 'GROUPS-OK <n>'.
  mp_bit_build_worker.py import JOB.npz OUT.npz
                                             imports a buildable mirror's export: its search, and the codes the build-side
                                             entries and pgv_hnsw_buildable_bits give an importer.

Nothing here looks at a model's results: the parent compares."""
import ctypes as C
import sys

import numpy as np

from pgvector_amd import api

GROUP_NBITS = (1, 8, 100, 128, 129, 1536, 64000)
GROUP_SIZES = (1, 2, 4, 5, 9, 33)
GROUP_ROWS = 48
METRICS = (api.PGV_BIT_HAMMING, api.PGV_BIT_JACCARD)


def group_pairs(n, frm):
    frm = max(frm, 1)
    return (n * (n - 1) - frm * (frm - 1)) // 2 if n > frm else 0


def groups_rows(nbits):
    """48 packed rows of every density; 0 and 1 all-zero, 3 a copy of 2, 5 the complement of 4 inside nbits"""
    rng = np.random.default_rng(9000 + nbits)
    nbytes = (nbits + 7) // 8
    bits = rng.random((GROUP_ROWS, 8 * nbytes)) < rng.uniform(.1, .9, (GROUP_ROWS, 1))
    bits[:, nbits:] = False
    bits[0] = bits[1] = False
    bits[3] = bits[2]
    bits[5, :nbits] = ~bits[4, :nbits]
    return np.packbits(bits, axis=1)


def groups_input():
    """every size with from = 1, 3, 6, n - 1, n, n + 2 (the last two, and whatever is past the size, want no pairs: empty
    groups between full ones); the first group of every size starts with the special rows
    -> ids, ids_start, from, pair_start, and the pairs expanded (a[i], b[i]) in the order the values are written"""
    rng = np.random.default_rng(77)
    ids, start, frm, pstart, a, b = [], [0], [], [0], [], []
    for n in GROUP_SIZES:
        for k, f in enumerate((1, 3, 6, n - 1, n, n + 2)):
            g = rng.integers(0, GROUP_ROWS, n).tolist()
            if k == 0:
                g[:6] = [0, 1, 2, 3, 4, 5][:n]
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
    """-> {"groups/<metric>/<nbits>": pgv_hnsw_score_groups' values, "pairs/<metric>/<nbits>": pgv_hnsw_score_pairs' over the
    same pairs}"""
    ids, ids_start, frm, pair_start, a, b = groups_input()
    res = {}
    for metric in METRICS:
        for nbits in GROUP_NBITS:
            h = api.BitHnsw(ctx, nbits, groups_rows(nbits), metric=metric, buildable=True)
            try:
                got = np.full(len(a), np.nan, np.float32)
                api.check(api.lib.pgv_hnsw_score_groups(h.h, api.ptr(ids), api.ptr(ids_start), api.ptr(frm), api.ptr(pair_start),
                                                        len(frm), len(ids), len(a), api.ptr(got)))
                res["groups/%d/%d" % (metric, nbits)], res["pairs/%d/%d" % (metric, nbits)] = got, h.score_pairs(a, b)
            finally:
                h.close()
    return res


def importer(job_path, out_path):
    job = np.load(job_path)
    ctx = api.Context(0)
    h = api.BitHnsw.from_handle(ctx, job["handle"].tobytes())
    elem, dist, scored = h.search(job["queries"], int(job["ef"]), int(job["k"]))
    i32 = np.zeros(4096, np.int32)
    f32, u8, i64 = np.zeros(4096, np.float32), np.zeros(4096, np.uint8), np.zeros(8, np.int64)
    codes = [
        api.lib.pgv_hnsw_build_search(h.h, api.ptr(i32), api.ptr(i32), 2, 8, 1, api.ptr(i32), api.ptr(f32), api.ptr(i32)),
        api.lib.pgv_hnsw_build_neighbors(h.h, api.ptr(i32), api.ptr(i32), 2, 8, 1, api.ptr(i32), api.ptr(f32), api.ptr(u8),
                                         api.ptr(i32), api.ptr(i64)),
        api.lib.pgv_hnsw_score_groups(h.h, api.ptr(i32), api.ptr(i64), api.ptr(i32), api.ptr(i64), 1, 2, 1, api.ptr(f32)),
        C.CDLL(api._lib.LIB_PATH).pgv_hnsw_link_begin(h.h),
    ]
    text = api.lib.pgv_last_error().decode()
    np.savez(out_path, elem=np.asarray(elem), dist=np.asarray(dist), scored=np.asarray(scored), codes=np.asarray(codes),
             text=np.frombuffer(text.encode(), dtype=np.uint8), buildable=int(api.lib.pgv_hnsw_buildable_bits(h.h)))
    h.close()
    ctx.close()


if __name__ == "__main__":
    if sys.argv[1] == "groups":
        c = api.Context(0)
        out = groups_on_device(c)
        np.savez(sys.argv[2], **out)
        c.close()
        print("GROUPS-OK %d" % (len(out) // 2))
    else:
        importer(sys.argv[2], sys.argv[3])
