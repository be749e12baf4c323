"""The checks of tests/test_gpu_scan_band.py, and a program that runs them in a process of its own under the
PGV_SCAN_WIDE / PGV_SCAN_DEEP / PGV_NO_DENSE128 the parent chose (the library reads those once per process).

Raw values: inner product is not rechecked, so -acc of every kernel form is observable.  fp32: bit for bit the chain
model's (tests/chain_model.py) on swamping and random inputs, the swamped error at least what the builder claims and at
most the bound.  fp16: the error within the charged bound, the largest attained fraction reported.
Answers: every adversarial set through scan_batch (fp32 without the shadow, fp16), rank_lists and exact_topk against the
oracle's exact form and the float64 order, id for id; the swamped center set through assign.  The callers set
PGV_SCAN_SHADOW=0 (the test's fixture, main() here): nothing below changes the environment.
scan_widened_queries / scan_redo_queries are counted for list scans only (batch_fix_kernel gets its stats pointer only
with probe lists): rank_lists and exact_topk have no counter to show that the band did the work, so those cases assert
ids alone and lean on the model's margins (tests/test_chain_model_cpu.py) for the rest.

Prints 'SCAN-BAND-OK <checks>' on success and one 'FRACTION ...' line per fp16 measurement."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chain_model as cm  # noqa: E402

DIMS = (64, 100, 256, 1536, 1600, 2000)
CHANGED = ("the accumulator chain structure of the kernel changed: restate it in tests/chain_model.py and revisit "
           "scan_bound / scan_chain_length (pgv_internal.h, kernels_mfma.hip) -- the band is computed from it")


def _api():
    from pgvector_amd import api
    return api


def _np_t(dtype):
    return np.float32 if dtype == cm.F32 else np.float16


def _pgv_t(dtype):
    return _api().PGV_F32 if dtype == cm.F32 else _api().PGV_F16


def is_wide(nq, wide_env):
    """whether nq queries probing ONE list run on the 64-query kernel: PGV_SCAN_WIDE when set (True / False), else the
    library's own rule, more than 12 queries per list on average (pgv_abi_ivf.hip, scan_batch_dev)"""
    return nq > 12 if wide_env is None else bool(wide_env)


def scan_form(nq, wide):
    """the form that takes a task of nq queries probing one list"""
    if nq <= 16:
        return "scan16"
    return "scan64" if (wide and nq > 32) else "scan32"


def ip_values(ctx, dtype, rows, queries):
    """q.x of every (query, row) pair as mfma_scan_kernel computes it: an inner-product index of one list"""
    api = _api()
    n, dim = rows.shape
    ix = api.IvfIndex(ctx, api.PGV_NEG_IP, _pgv_t(dtype), dim, rows[:1].copy(), np.array([0, n], dtype=np.int64), rows,
                      np.arange(n, dtype=np.uint64))
    dist, slot, _ = ix.search_batch(queries, 1, n)
    ix.close()
    out = np.zeros((queries.shape[0], n), dtype=np.float32)
    for i in range(queries.shape[0]):
        out[i, slot[i]] = dist[i]
    return -out


def topk_ip_values(ctx, dtype, rows, queries):
    """the same through pgv_exact_topk (mfma_dense_kernel from 128 queries x 128 rows on, else the 32-query kernel)"""
    api = _api()
    n, dim = rows.shape
    dist, idx = api.exact_topk(ctx, api.PGV_NEG_IP, _pgv_t(dtype), dim, queries, rows, n)
    out = np.zeros((queries.shape[0], n), dtype=np.float32)
    for i in range(queries.shape[0]):
        out[i, idx[i]] = dist[i]
    return -out


def raw_inputs(form, dtype, dim, nq, n, seed):
    """rows 0 / 1 and query 0: swamped down / up; the rest Gaussian"""
    rng = np.random.default_rng(seed)
    t = _np_t(dtype)
    rows = rng.standard_normal((n, dim)).astype(t)
    queries = rng.standard_normal((nq, dim)).astype(t)
    down, q = cm.swamp(form, dtype, dim, -1)
    up, _ = cm.swamp(form, dtype, dim, +1)
    rows[0], rows[1], queries[0] = down[0], up[0], q
    return np.ascontiguousarray(rows), np.ascontiguousarray(queries)


def check_raw(values, form, dtype, dim, rows, queries, chain, check_queries, what):
    """values [nq x n] from the GPU against the model (fp32) and the bound; returns the largest attained fraction"""
    worst = 0.0
    for qi in check_queries:
        v = values[qi]
        frac = cm.attained_fraction(v, rows, queries[qi], chain)
        worst = max(worst, float(frac.max()))
        assert (frac <= 1.0).all(), "%s q%d: error %.3f of the charged bound (chain %d). %s" % (what, qi, frac.max(), chain, CHANGED)
        if dtype == cm.F32:
            want = cm.chain_dot(form, rows, queries[qi])
            bad = np.flatnonzero(v.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, "%s q%d: %d of %d values differ from the %s chain model (row %d: %r != %r). %s" % (
                what, qi, bad.size, v.size, form, bad[0], float(v[bad[0]]), float(want[bad[0]]), CHANGED)
    if dtype == cm.F32:
        claim = cm.claimed_fraction(form, dtype, dim, chain)
        f = cm.attained_fraction(values[0][:2], rows[:2], queries[0], chain)
        assert (f >= claim).all(), "%s: swamped rows attain %r < %.4f claimed. %s" % (what, f, claim, CHANGED)
        true = rows[:2].astype(np.float64) @ queries[0].astype(np.float64)
        assert values[0][0] < true[0] and values[0][1] > true[1], what
    else:
        print("FRACTION %s dim %d: %.4f of the charged bound (chain %d; swamped rows %.4f / %.4f)" % (
            what, dim, worst, chain, *cm.attained_fraction(values[0][:2], rows[:2], queries[0], chain)))
    return worst


def raw_scan_checks(ctx, wide_env, dims=DIMS, sizes=(8, 24, 48)):
    """the list scan's forms: tasks of <= 16, 17 .. 32 and 33 .. 64 queries (the last: scan64 when wide, else 32 + 16)"""
    done = 0
    for dtype in (cm.F32, cm.F16):
        for dim in dims:
            for nq in sizes:
                wide = is_wide(nq, wide_env)
                form = scan_form(nq, wide)
                chain = cm.scan_chain_length(dim, dtype, wide)
                rows, queries = raw_inputs(form, dtype, dim, nq, 40, seed=dim + nq)
                v = ip_values(ctx, dtype, rows, queries)
                # (not wide, nq 48: queries 32 .. 47 are a 16-wide task; fp32: the same chains)
                check_raw(v, form, dtype, dim, rows, queries, chain, (0, 1, nq - 1), "scan %s %s nq %d" % (dtype, form, nq))
                done += 1
    return done


def raw_topk_checks(ctx, no_dense, dims=DIMS):
    done = 0
    for dtype in (cm.F32, cm.F16):
        for dim in dims:
            for nq in (64, 128):
                dense = nq >= 128 and not no_dense
                form = "dense" if dense else "scan32"
                chain = cm.dense_chain_length(dim, dtype) if dense else cm.scan_chain_length(dim, dtype, False)
                rows, queries = raw_inputs(form, dtype, dim, nq, 130, seed=7 * dim + nq)
                v = topk_ip_values(ctx, dtype, rows, queries)
                check_raw(v, form, dtype, dim, rows, queries, chain, (0, 33, nq - 1), "exact_topk %s %s nq %d" % (dtype, form, nq))
                done += 1
    return done


# ------------------------------------------------------------------------------------------------- answers
def _others(s, n, seed):
    """n benign queries near the set's query (they probe the same list, so that the attacked query sits in a task of
    the wanted width)"""
    rng = np.random.default_rng(seed)
    q = s.query.astype(np.float32)[None, :] + np.float32(2.0 ** -6) * rng.standard_normal((n, s.dim)).astype(np.float32)
    return q.astype(_np_t(s.dtype))


def _far_rows(s, n):
    """n distinct rows of the set's norm on the far side of the origin (they change neither the band nor the head)"""
    hd = cm.heads(s.form, s.dtype, s.dim)
    far = np.tile(-s.query.astype(np.float64), (n, 1))
    far[:, hd[-1]] -= (1 + np.arange(n) % 64) * 2.0 ** -9
    far[:, hd[0]] -= (np.arange(n) // 64) * 2.0 ** -9
    return far.astype(_np_t(s.dtype))


def _oracle_order(oracle, s, rows, q):
    """the oracle's exact distances of `rows` to q (one list holding them all) -> the first k row indices"""
    from oracle import pyoracle as po
    dt = po.ORA_F32 if s.dtype == cm.F32 else po.ORA_F16
    ixs = oracle.index_struct(po.OPS_L2, dt, rows[:1], np.array([0, rows.shape[0]], dtype=np.int64), rows,
                              np.arange(rows.shape[0], dtype=np.uint64))
    wd, ws = oracle.get_scan_items(ixs, q, np.array([0], dtype=np.int32))
    o = np.lexsort((ws, wd))[:s.k]
    return ws[o]


def _expect(oracle, s, rows, got_ids, what):
    want64 = np.lexsort((np.arange(rows.shape[0]),
                         np.sum((rows.astype(np.float64) - s.query.astype(np.float64)) ** 2, axis=1)))[:s.k]
    want_ora = _oracle_order(oracle, s, rows, s.query)
    assert list(want_ora) == list(want64), what
    assert list(np.asarray(got_ids)) == list(want64), "%s: got %r, want %r (T = row %d)" % (
        what, list(np.asarray(got_ids)), list(want64), want64[0])


def answer_scan(ctx, oracle, s, nq, worst_case=True):
    """the set as one list of an index; the attacked query among nq - 1 others in one task"""
    api = _api()
    n = s.rows.shape[0]
    ix = api.IvfIndex(ctx, api.PGV_L2SQ, _pgv_t(s.dtype), s.dim, s.query[None, :].copy(), np.array([0, n], dtype=np.int64),
                      s.rows, np.arange(n, dtype=np.uint64))
    at = nq // 2
    queries = _others(s, nq, seed=nq)
    queries[at] = s.query
    lists = np.zeros((nq, 1), dtype=np.int32)
    ctx.set_profiling(True)
    if worst_case is not None:      # (None: the context's own bound mode, untouched)
        ctx.set_bound(worst_case)
    try:
        ctx.reset_stats()
        dist, slot, _ = ix.scan_batch(np.ascontiguousarray(queries), lists, s.k)
        ctx.sync()
        st = ctx.stats()
    finally:
        ctx.set_profiling(False)
        if worst_case is not None:
            ctx.set_bound(True)
        ix.close()
    if worst_case is False:
        return st      # the statistical bound is EXPECTED to lose T on these rows: nothing asserted
    what = "scan_batch %s %s dim %d nq %d" % (s.dtype, s.form, s.dim, nq)
    _expect(oracle, s, s.rows, slot[at], what)
    assert st["scan_widened_queries"] + st["scan_redo_queries"] >= 1, (what, st)
    assert st["scan_shadow_queries"] == 0, (what, st)
    return st


def answer_rank(ctx, oracle, s):
    """the set as the CENTERS of an index (>= 64 of them), 128 queries: rank_lists_dev's MFMA ranking"""
    api = _api()
    centers = s.rows
    n = centers.shape[0]
    assert n >= 64
    ix = api.IvfIndex(ctx, api.PGV_L2SQ, _pgv_t(s.dtype), s.dim, centers, np.arange(n + 1, dtype=np.int64), centers.copy(),
                      np.arange(n, dtype=np.uint64))
    queries = _others(s, 128, seed=3)
    queries[5] = s.query
    lists, _ = ix.rank_lists(np.ascontiguousarray(queries), s.k)
    ix.close()
    _expect(oracle, s, centers, lists[5], "rank_lists %s dim %d" % (s.dtype, s.dim))


def answer_topk(ctx, oracle, s, nq):
    api = _api()
    rows = np.ascontiguousarray(np.concatenate([s.rows, _far_rows(s, 200)]))
    queries = _others(s, nq, seed=nq)
    queries[nq - 3] = s.query
    _, idx = api.exact_topk(ctx, api.PGV_L2SQ, _pgv_t(s.dtype), s.dim, np.ascontiguousarray(queries), rows, s.k)
    _expect(oracle, s, rows, idx[nq - 3], "exact_topk %s %s dim %d nq %d" % (s.dtype, s.form, s.dim, nq))


def answer_assign(ctx, oracle, dtype, dim):
    """chain_model.assign_set through api.assign (mfma_argmin_kernel: >= 64 centers, >= 256 rows): the oracle's and the
    float64 center for every row, and the rows went through the exact recheck or the redo"""
    from oracle import pyoracle as po
    api = _api()
    rows, centers, t = cm.assign_set(dim, dtype)
    ctx.set_profiling(True)
    try:
        ctx.reset_stats()
        got, _ = api.assign(ctx, api.PGV_L2SQ, _pgv_t(dtype), dim, centers, rows)
        ctx.sync()
        st = ctx.stats()
    finally:
        ctx.set_profiling(False)
    want, _ = oracle.assign(po.OPS_L2, po.ORA_F32 if dtype == cm.F32 else po.ORA_F16, centers, rows)
    d = np.sum((centers.astype(np.float64) - rows[0].astype(np.float64)) ** 2, axis=1)
    assert int(np.argmin(d)) == t and (np.asarray(want) == t).all()
    assert (np.asarray(got) == t).all(), ("assign %s dim %d" % (dtype, dim), np.unique(np.asarray(got)), t)
    assert st["assign_recheck_rows"] + st["assign_redo_rows"] >= 1, st
    return st


def answer_large(ctx, oracle, dtype, wide_env, dim=2048):
    """the adversarial group inside ONE list of an index of >= 1 GiB of rows (the non-temporal instantiations of
    mfma_scan_kernel): the other rows are a block of Gaussian noise of |x|^2 = 3.5 (below the set's, so the band is the
    set's own), rotated by one element per block, all ~7.5 from the query.  10, 25 and 50 queries on the list."""
    api = _api()
    rng = np.random.default_rng(11)
    t = _np_t(dtype)
    n = ((1 << 30) // (dim * np.dtype(t).itemsize)) + 1200
    noise = rng.standard_normal((1024, dim))
    noise *= np.sqrt(3.5) / np.linalg.norm(noise, axis=1, keepdims=True)
    noise = noise.astype(t)
    rows = np.empty((n, dim), dtype=t)
    for b in range(0, n, 1024):
        e = min(n, b + 1024)
        rows[b:e] = np.roll(noise, b // 1024, axis=1)[:e - b]
    done = 0
    for nq in (10, 25, 50):
        wide = is_wide(nq, wide_env)
        s = cm.band_set(scan_form(nq, wide), dtype, dim, chain=cm.scan_chain_length(dim, dtype, wide))
        at = np.sort(rng.choice(n, s.rows.shape[0], replace=False))
        rows[at] = s.rows
        assert cm.row_norms(noise[:8], dtype).max() < cm.row_norms(s.rows, dtype).max()
        ix = api.IvfIndex(ctx, api.PGV_L2SQ, _pgv_t(dtype), dim, s.query[None, :].copy(), np.array([0, n], dtype=np.int64),
                          rows, np.arange(n, dtype=np.uint64))
        queries = _others(s, nq, seed=nq)
        queries[nq // 2] = s.query
        ctx.set_profiling(True)
        try:
            ctx.reset_stats()
            _, slot, _ = ix.scan_batch(np.ascontiguousarray(queries), np.zeros((nq, 1), dtype=np.int32), s.k)
            ctx.sync()
            st = ctx.stats()
        finally:
            ctx.set_profiling(False)
            ix.close()
        want, _ = s.want()
        assert list(_oracle_order(oracle, s, s.rows, s.query)) == list(want)
        what = "large index %s %s nq %d" % (dtype, s.form, nq)
        assert list(np.asarray(slot[nq // 2])) == list(at[want]), (what, list(np.asarray(slot[nq // 2])), list(at[want]))
        assert st["scan_widened_queries"] + st["scan_redo_queries"] >= 1 and st["scan_shadow_queries"] == 0, (what, st)
        rows[at] = np.roll(noise, 3, axis=1)[:at.size]     # (the next set goes elsewhere)
        done += 1
    return done


def answer_checks(ctx, oracle, wide_env, no_dense, dims=(256, 1600)):
    done = 0
    for dtype in (cm.F32, cm.F16):
        for dim in dims:
            for nq in (10, 25, 50):
                wide = is_wide(nq, wide_env)
                s = cm.band_set(scan_form(nq, wide), dtype, dim, chain=cm.scan_chain_length(dim, dtype, wide))
                answer_scan(ctx, oracle, s, nq)
                done += 1
            s = cm.band_set("scan32", dtype, dim, chain=cm.scan_chain_length(dim, dtype, False))
            answer_rank(ctx, oracle, s)
            answer_topk(ctx, oracle, s, 64)
            if not no_dense:
                s = cm.band_set("dense", dtype, dim, chain=cm.dense_chain_length(dim, dtype))
            answer_topk(ctx, oracle, s, 128)
            answer_assign(ctx, oracle, dtype, dim)
            done += 4
    return done


def main():
    from oracle import pyoracle as po
    wide = {None: None, "0": False, "1": True}[os.environ.get("PGV_SCAN_WIDE")]
    no_dense = os.environ.get("PGV_NO_DENSE128", "0") not in ("", "0")
    os.environ["PGV_SCAN_SHADOW"] = "0"
    api = _api()
    ctx = api.Context(0)
    oracle = po.Oracle()
    done = raw_scan_checks(ctx, wide)
    done += raw_topk_checks(ctx, no_dense)
    done += answer_checks(ctx, oracle, wide, no_dense)
    if not no_dense:     # (PGV_NO_DENSE128 does not touch the list scan: its child leaves the large indexes out)
        for dtype in (cm.F32, cm.F16):
            done += answer_large(ctx, oracle, dtype, wide)
    ctx.close()
    print("SCAN-BAND-OK %d wide=%s deep=%s no_dense=%s" % (done, os.environ.get("PGV_SCAN_WIDE"),
                                                           os.environ.get("PGV_SCAN_DEEP"), no_dense))


if __name__ == "__main__":
    main()
