"""Run by tests/test_gpu_hnsw_link_edges.py in a process of its own under one setting of PGV_HNSW_LINK_SERIAL /
PGV_HNSW_PAIRS_GATHER / PGV_HNSW_SELECT_SERIAL (each read once per process).

  mp_hnsw_link_worker.py link OUT.npz [scenario ...]   every scenario of tests/hnsw_link_model.py (or the ones named)
      through pgv_hnsw_link_begin / _prepare / _apply / _end on an empty graph; per scenario the tuples, each batch's
      first-round pair count, the deferred-list count and the second round's pair count go into OUT.npz; for the small
      scenarios also the tuples and counts after every batch (each prefix of the batches run on its own: only
      pgv_hnsw_link_end reads the state back, and it ends the build).  Prints 'LINK-OK <scenarios>'.
  mp_hnsw_link_worker.py select                         select_cases() below.  Prints 'SELECT-OK <lists thinned>'.
  mp_hnsw_link_worker.py groups OUT.npz                 groups_on_device() below: pgv_hnsw_score_groups' and
      pgv_hnsw_score_pairs' values of every groups_cases() case go into OUT.npz.  Prints 'GROUPS-OK <cases>'.

The parent compares; nothing here looks at the model's results."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hnsw_link_model as hm  # noqa: E402
from pgvector_amd import api  # noqa: E402

P, I, I64 = C.c_void_p, C.c_int, C.c_int64
api.lib.pgv_hnsw_link_begin.argtypes = [P]
api.lib.pgv_hnsw_link_prepare.argtypes = [P, P, P, I, I, P, P, P, P, C.POINTER(I64)]
api.lib.pgv_hnsw_link_apply.argtypes = [P, C.c_int32]
api.lib.pgv_hnsw_link_end.argtypes = [P, P, C.POINTER(I64), C.POINTER(I64)]
api.lib.pgv_hnsw_score_groups.argtypes = [P, P, P, P, P, I, I64, I64, P]


def link_on_device(ctx, sc, nbatches=None):
    """the scenario's (first nbatches) batches linked into an empty graph -> (tuples, pairs per batch, deferred lists,
    second-round pairs)"""
    metric = api.PGV_NEG_IP if sc["metric"] == hm.IP else api.PGV_L2SQ
    dtype = api.PGV_F16 if sc["f16"] else api.PGV_F32
    rows = sc["rows"].astype(np.float16) if sc["f16"] else sc["rows"]
    levels, m = sc["levels"], sc["m"]
    mirror = api.Hnsw(ctx, metric, dtype, rows.shape[1], rows)
    start = np.zeros(len(levels) + 1, np.int64)
    start[1:] = np.cumsum((levels.astype(np.int64) + 2) * m)
    nbr = np.full(int(start[-1]), -1, np.int32)
    try:
        mirror.set_graph(m, 0, levels, start, nbr)
        api.check(api.lib.pgv_hnsw_link_begin(mirror.h))
        pairs = []
        for b in sc["batches"][:nbatches]:
            arrs = [np.ascontiguousarray(b[k]) for k in ("elements", "linked", "sel_ids", "sel_dist", "sel_closer", "sel_cnt")]
            assert [a.dtype for a in arrs] == [np.int32, np.uint8, np.int32, np.float32, np.uint8, np.int32]
            np_ = I64(-1)
            api.check(api.lib.pgv_hnsw_link_prepare(mirror.h, api.ptr(arrs[0]), api.ptr(arrs[1]), len(arrs[0]), b["lcap"],
                                                    api.ptr(arrs[2]), api.ptr(arrs[3]), api.ptr(arrs[4]), api.ptr(arrs[5]),
                                                    C.byref(np_)))
            api.check(api.lib.pgv_hnsw_link_apply(mirror.h, 0))
            pairs.append(np_.value)
        pairs2, deferred = I64(-1), I64(-1)
        api.check(api.lib.pgv_hnsw_link_end(mirror.h, api.ptr(nbr), C.byref(pairs2), C.byref(deferred)))   # OK: nothing left waiting
    finally:
        mirror.close()
    return nbr, np.asarray(pairs, np.int64), deferred.value, pairs2.value


def run_link(out, names):
    ctx = api.Context(0)
    res = {}
    todo = names or list(hm.all_scenarios())
    for name in todo:
        sc = hm.all_scenarios()[name]()
        t0 = time.time()
        nbr, pairs, deferred, pairs2 = link_on_device(ctx, sc)
        res[name + "/nbr"], res[name + "/pairs"] = nbr, pairs
        res[name + "/deferred"], res[name + "/pairs2"] = np.int64(deferred), np.int64(pairs2)
        # the state after every batch: pgv_hnsw_link_end is the one search-free way to read the tuples and the counts, and
        # it ends the build, so every prefix of a small scenario is a run of its own
        if len(sc["rows"]) <= hm.PREFIX_ROWS:
            for k in range(1, len(sc["batches"])):
                nbr_k, _, deferred_k, pairs2_k = link_on_device(ctx, sc, k)
                res["%s/nbr@%d" % (name, k)] = nbr_k
                res["%s/deferred@%d" % (name, k)], res["%s/pairs2@%d" % (name, k)] = np.int64(deferred_k), np.int64(pairs2_k)
        print("%-14s m=%-3d device %.2fs pairs %s deferred %d pairs2 %d" % (name, sc["m"], time.time() - t0, pairs.tolist(),
                                                                          deferred, pairs2), flush=True)
    ctx.close()
    np.savez(out, **res)
    print("LINK-OK %d" % len(todo))


# ------------------------------------------------------------------ the new elements' own selection at its switch
SELECT_CASES = [(m, efc) for m in (4, 31, 32) for efc in (64, 65)]


def knn_graph(rows, levels, m):
    """a graph to search: every element's list on layer lc = its lm nearest elements of level >= lc (ties by id)"""
    n = len(rows)
    start = np.zeros(len(levels) + 1, np.int64)
    start[1:] = np.cumsum((levels.astype(np.int64) + 2) * m)
    nbr = np.full(int(start[-1]), -1, np.int32)
    for lc in range(int(levels[:n].max()) + 1):
        pool = np.flatnonzero(levels[:n] >= lc)
        D = hm.pair_matrix(rows, hm.L2, pool)
        lm = 2 * m if lc == 0 else m
        for i, e in enumerate(pool):
            d = D[i].copy()
            d[i] = np.inf
            o = np.lexsort((pool, d))[:min(lm, len(pool) - 1)]
            at = int(start[e]) + (int(levels[e]) - lc) * m
            nbr[at:at + len(o)] = pool[o]
    return start, nbr


def select_cases(ctx):
    """pgv_hnsw_build_neighbors against the plain sweep (hm.host_select) over the lists and pair distances that
    pgv_hnsw_build_search / pgv_hnsw_score_pairs return, on a 600-row integer grid: ef_construction 64 and 65 (the two
    sides of launch_hnsw_select's ef <= 64 switch), m 4 / 31 / 32.  -> {(m, efc): lists with more than lm candidates}"""
    rng = np.random.default_rng(600)
    n, head, dim = 600, 400, 4
    data = rng.integers(-6, 7, (n, dim)).astype(np.float32)
    levels = np.zeros(n, np.int32)
    levels[:head:2] = 1                       # 200 elements on layer 1: lists of more than m = 32 candidates there
    levels[0] = 2
    new_levels = np.ones(n - head, np.int32)
    levels[head:] = new_levels
    elems = np.arange(head, n, dtype=np.int32)
    thinned_of = {}
    for m, efc in SELECT_CASES:
        mirror = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, dim, data)
        start, nbr = knn_graph(data[:head], levels, m)
        mirror.set_graph(m, 0, levels, start, nbr)
        lcap = 2
        per = len(elems) * lcap
        ids = np.empty((per, efc), np.int32)
        dist = np.empty((per, efc), np.float32)
        cnt = np.empty(per, np.int32)
        api.check(api.lib.pgv_hnsw_build_search(mirror.h, api.ptr(elems), api.ptr(new_levels), len(elems), efc, lcap,
                                                api.ptr(ids), api.ptr(dist), api.ptr(cnt)))
        oi = np.empty((per, 2 * m), np.int32)
        od = np.empty((per, 2 * m), np.float32)
        oc = np.empty((per, 2 * m), np.uint8)
        on = np.empty(per, np.int32)
        pairs = I64()
        api.check(api.lib.pgv_hnsw_build_neighbors(mirror.h, api.ptr(elems), api.ptr(new_levels), len(elems), efc, lcap,
                                                   api.ptr(oi), api.ptr(od), api.ptr(oc), api.ptr(on), C.byref(pairs)))
        mirror.close()
        thinned = want_pairs = 0
        for g in range(per):
            q, lc = divmod(g, lcap)
            lm = 2 * m if lc == 0 else m
            nw = int(cnt[g])
            gi, gd = ids[g, :nw], dist[g, :nw]
            # the search's list is what the sweep assumes: nearest first, the true (exact) distances
            assert (np.diff(gd) >= 0).all() and (gd == hm.distances_to(data, hm.L2, int(elems[q]), gi)).all(), (m, efc, g)
            tri = None
            if nw > lm:
                thinned += 1
                want_pairs += nw * (nw - 1) // 2
                D = hm.pair_matrix(data, hm.L2, gi)
                tri = np.concatenate([D[u, :u] for u in range(1, nw)])
            wi, wd, wc = hm.host_select(gi, gd, tri, lm)
            assert on[g] == len(wi), (m, efc, g, on[g], len(wi))
            assert oi[g, :on[g]].tolist() == wi, (m, efc, g, lc, nw)
            assert od[g, :on[g]].tolist() == wd, (m, efc, g)
            assert oc[g, :on[g]].tolist() == wc, (m, efc, g)
        assert pairs.value == want_pairs, (m, efc, pairs.value, want_pairs)
        thinned_of[(m, efc)] = thinned
    return thinned_of


# ------------------------------------------------------------------ pair distances inside groups of rows
GROUP_SIZES = (1, 2, 5, 64, 65, 257, 300)    # across the expand loop's 64 lanes and 256 threads, score_groups' 4 x 4 tiles
GROUP_ROWS = 320
GROUP_CASES = [(metric, dtype) for metric in (api.PGV_L2SQ, api.PGV_NEG_IP, api.PGV_L1) for dtype in (api.PGV_F32, api.PGV_F16)]


def groups_input():
    """One call's groups: every size of GROUP_SIZES with from = 0, 1, 3, n - 1 and n (n: no pairs wanted), ids drawn from
    320 rows with repeats inside a group.  -> ids, ids_start, from, pair_start and the slot pairs (a, b) the call asks for:
    per group (u, v < u) for u >= max(from, 1), u ascending then v."""
    rng = np.random.default_rng(1605)
    ids, frm, a, b = [], [], [], []
    for n in GROUP_SIZES:
        for f in (0, 1, 3, n - 1, n):
            gi = rng.integers(0, GROUP_ROWS, n).astype(np.int32)
            gi[-1] = gi[0]                    # (a repeated id whatever the draw; a group of one is its own repeat)
            u, v = np.tril_indices(n, -1)     # row-major: u ascending then v
            keep = u >= max(f, 1)
            ids.append(gi)
            frm.append(f)
            a.append(gi[u[keep]])
            b.append(gi[v[keep]])
    ids_start = np.concatenate([[0], np.cumsum([len(g) for g in ids])]).astype(np.int64)
    pair_start = np.concatenate([[0], np.cumsum([len(x) for x in a])]).astype(np.int64)
    return (np.concatenate(ids), ids_start, np.asarray(frm, np.int32), pair_start, np.concatenate(a).astype(np.int32),
            np.concatenate(b).astype(np.int32))


def groups_rows(dtype):
    """320 rows on an integer grid in [-6, 6]: 4-d fp32, 5-d fp16 (both padded to a 16-byte vector and past one)"""
    rng = np.random.default_rng(1606)
    dim = 4 if dtype == api.PGV_F32 else 5
    return rng.integers(-6, 7, (GROUP_ROWS, dim)).astype(np.float32 if dtype == api.PGV_F32 else np.float16)


def groups_on_device(ctx):
    """-> {"groups/<metric>/<dtype>": pgv_hnsw_score_groups' values, "pairs/<metric>/<dtype>": pgv_hnsw_score_pairs' over
    the same pairs} for every case"""
    ids, ids_start, frm, pair_start, a, b = groups_input()
    res = {}
    for metric, dtype in GROUP_CASES:
        rows = groups_rows(dtype)
        mirror = api.Hnsw(ctx, metric, dtype, rows.shape[1], rows)
        try:
            got = np.full(len(a), np.nan, np.float32)
            api.check(api.lib.pgv_hnsw_score_groups(mirror.h, api.ptr(ids), api.ptr(ids_start), api.ptr(frm), api.ptr(pair_start),
                                                    len(frm), len(ids), len(a), api.ptr(got)))
            want = np.full(len(a), np.nan, np.float32)
            api.check(api.lib.pgv_hnsw_score_pairs(mirror.h, api.ptr(a), api.ptr(b), len(a), api.ptr(want)))
        finally:
            mirror.close()
        res["groups/%d/%d" % (metric, dtype)], res["pairs/%d/%d" % (metric, dtype)] = got, want
    return res


if __name__ == "__main__":
    if sys.argv[1] == "link":
        run_link(sys.argv[2], sys.argv[3:])
    elif sys.argv[1] == "groups":
        c = api.Context(0)
        r = groups_on_device(c)
        c.close()
        np.savez(sys.argv[2], **r)
        print("GROUPS-OK %d" % len(GROUP_CASES))
    else:
        c = api.Context(0)
        t = select_cases(c)
        c.close()
        assert min(t.values()) >= 100, t
        print("SELECT-OK %s" % sorted(t.items()))
