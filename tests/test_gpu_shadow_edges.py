"""The fp16 residual shadow scan (kernels_shadow.hip) at the edges of its rounding band, against the CPU oracle.

Every case builds the index with PGV_SCAN_SHADOW=1 and checks that the shadow ran (scan_shadow_queries > 0, or == 0
where it must be dropped), compares ids and distances with the oracle's GetScanItems over the same probe lists
(tie-tolerant), and compares with the same index built with PGV_SCAN_SHADOW=0: distance bit patterns, slots and tids
equal.  The adversarial sets come from tests/shadow_model.py, whose margins test_shadow_model_cpu.py checks on the
host: there a band too narrow by half, or without its row or query representation term, answers the decoys."""
import os
import subprocess
import sys

import numpy as np
import pytest

import shadow_model as sm
from helpers import assert_topk_equiv
from oracle import pyoracle as po
from pgvector_amd import api

pytestmark = pytest.mark.gpu


def _tids(n):
    return np.arange(n, dtype=np.uint64) * 7 + 3


def _nearest_lists(centers, queries, probes):
    c = centers.astype(np.float64)
    q = queries.astype(np.float64)
    d = (q * q).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * q @ c.T
    return np.ascontiguousarray(np.argsort(d, axis=1, kind="stable")[:, :probes].astype(np.int32))


def _run(ctx, monkeypatch, env, dim, rows, centers, off, queries, lists, k):
    monkeypatch.setenv("PGV_SCAN_SHADOW", env)
    ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, dim, centers, off, rows, _tids(rows.shape[0]))
    try:
        ctx.set_profiling(True)
        ctx.reset_stats()
        d, s, t = ix.scan_batch(queries, lists, k, want_tid=True)
        ctx.sync()
        st = ctx.stats()
    finally:
        ctx.set_profiling(False)
        ix.close()
    return (np.asarray(d).copy(), np.asarray(s).copy(), np.asarray(t).copy()), st


def check(ctx, monkeypatch, oracle, rows, centers, off, queries, k, lists=None, probes=None, shadow=True, vs_oracle=True,
          what=""):
    """shadow side against the oracle and against the plain scan; returns the shadow side's stats and answers"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    centers = np.ascontiguousarray(centers, dtype=np.float32)
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    off = np.ascontiguousarray(off, dtype=np.int64)
    dim = rows.shape[1]
    if lists is None:
        lists = _nearest_lists(centers, queries, probes)
    lists = np.ascontiguousarray(lists, dtype=np.int32)
    a, sa = _run(ctx, monkeypatch, "1", dim, rows, centers, off, queries, lists, k)
    b, sb = _run(ctx, monkeypatch, "0", dim, rows, centers, off, queries, lists, k)
    if shadow:
        assert sa["scan_shadow_queries"] == queries.shape[0], (what, sa)
    else:
        assert sa["scan_shadow_queries"] == 0, (what, sa)
    assert sb["scan_shadow_queries"] == 0, (what, sb)
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(a[1], b[1], err_msg=what)
    np.testing.assert_array_equal(a[2], b[2], err_msg=what)
    if vs_oracle:
        ixs = oracle.index_struct(po.OPS_L2, po.ORA_F32, centers, off, rows, _tids(rows.shape[0]))
        tids = _tids(rows.shape[0])
        for i in range(queries.shape[0]):
            wd, ws = oracle.get_scan_items(ixs, queries[i], lists[i])
            order = np.lexsort((ws, wd))[:k]
            n = len(order)
            got_t, got_d = a[2][i], a[0][i]
            assert_topk_equiv(got_t[:n].astype(np.uint64).tolist(), got_d[:n], tids[ws[order]].tolist(), wd[order],
                              what="%s q%d" % (what, i))
            if n < k:  # fewer rows probed than asked for: INFINITY / -1 padding
                assert np.isinf(got_d[n:]).all() and (a[1][i][n:] == -1).all(), (what, i)
    return sa, a


def _mixture(n, dim, nlists, seed, sigma=0.1, scale=1.0, sizes=None):
    """rows list-major around per-list centers (uniform means, Gaussian spread); `sizes` fixes the list lengths"""
    rng = np.random.default_rng(seed)
    centers = rng.random((nlists, dim), dtype=np.float32)
    if sizes is None:
        sizes = np.bincount(rng.integers(0, nlists, n), minlength=nlists)
    sizes = np.asarray(sizes, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    lst = np.repeat(np.arange(nlists), sizes)
    rows = centers[lst] + np.float32(sigma) * rng.standard_normal((int(off[-1]), dim)).astype(np.float32)
    return (rows * np.float32(scale)).astype(np.float32), (centers * np.float32(scale)).astype(np.float32), off


def _queries_near(rows, nq, seed, sigma=0.05):
    rng = np.random.default_rng(seed + 100)
    base = rows[rng.integers(0, rows.shape[0], nq)]
    return (base + np.float32(sigma) * rng.standard_normal(base.shape).astype(np.float32)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the adversarial band cases (tests/shadow_model.py)

@pytest.mark.parametrize("name", ["rows", "query"])
@pytest.mark.parametrize("k", [10, 16])
def test_adversarial_band_answers_the_true_neighbours(ctx, monkeypatch, oracle, name, k):
    st = (sm.row_inversion_set if name == "rows" else sm.query_inversion_set)()
    nq = 16  # a list-major batch (16 queries on one list: the matrix-core scan), one cast query repeated
    queries = np.tile(st.query, (nq, 1))
    lists = np.zeros((nq, 1), dtype=np.int32)
    stats, (_, s, _) = check(ctx, monkeypatch, oracle, st.rows, st.centers, st.list_offsets, queries, k, lists=lists,
                             what="adversarial %s k %d" % (name, k))
    assert stats["scan_redo_queries"] + stats["scan_widened_queries"] > 0, stats
    # the true rows are in every answer (the decoys are exactly farther, beyond the tie tolerance)
    for i in range(nq):
        assert set(st.groups["true"].tolist()) <= set(s[i].tolist()), (name, k, i)


# ---------------------------------------------------------------------------------------------------------------------
# value edges

def test_rows_equal_to_their_centers(ctx, monkeypatch, oracle):
    """rho = 0 everywhere: s = 0, an all-zero shadow, E = P = 0; the pair term alone orders the lists"""
    dim, nlists = 64, 12
    centers = np.random.default_rng(1).random((nlists, dim), dtype=np.float32)
    sizes = np.full(nlists, 40)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = np.repeat(centers, sizes, axis=0)
    queries = _queries_near(rows, 64, 1, sigma=0.2)
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=4, what="rows = centers")


def test_rows_equal_to_their_centers_in_some_lists(ctx, monkeypatch, oracle):
    dim, nlists = 96, 10
    rows, centers, off = _mixture(3000, dim, nlists, seed=2)
    for l in range(0, nlists, 2):
        rows[off[l]:off[l + 1]] = centers[l]
    queries = _queries_near(rows, 64, 2)
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=3, what="rows = centers (half)")


def _scaled_case(scale_log2, dim=32, nlists=8, nq=48, seed=3):
    rows, centers, off = _mixture(2000, dim, nlists, seed=seed)
    queries = _queries_near(rows, nq, seed)
    f = np.float32(2.0 ** scale_log2)
    return rows * f, centers * f, off, queries * f


def _exponent(rows, centers, off, queries):
    s, _, _, _ = sm.shadow_rows(rows, centers, off)
    return [1 + s + sm.cast_query(q)[0] for q in queries]


def _cut_case(e, scale_log2):
    """rows scaled by 2^scale_log2, and every query's element 0 set to the one value of the binade that makes
    1 + s + s_q = e for all of them (it is the query's largest element)"""
    rows, centers, off, queries = _scaled_case(scale_log2)
    s = sm.shadow_rows(rows, centers, off)[0]
    v = np.float32(1.5 * 2.0 ** (e - 1 - s + 13))
    assert v >= np.abs(queries).max() and v <= 4 * np.abs(queries).max()
    queries[:, 0] = v
    assert _exponent(rows, centers, off, queries) == [e] * queries.shape[0]
    return rows, centers, off, queries


def test_exponent_cut_just_inside(ctx, monkeypatch, oracle):
    """1 + s + s_q = -125 for every query (the smallest exponent whose factor 2^(1 + s + s_q) is a normal fp32): the
    shadow answers the oracle's rows.  (The other end, +125, needs |q| |x - c| > 2^150: |x|^2 or |q|^2 overflows fp32
    first, and that makes the band infinite anyway.)"""
    rows, centers, off, queries = _cut_case(-125, -49)
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=3, what="exponent -125")


def test_exponent_cut_just_outside_takes_the_exact_pass(ctx, monkeypatch, oracle):
    rows, centers, off, queries = _cut_case(-126, -50)
    d = ((rows[:1].astype(np.float32) - queries[:1]) ** 2).sum()
    assert np.isfinite(d) and d > 0
    stats, _ = check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=3, what="exponent -126")
    assert stats["scan_redo_queries"] == queries.shape[0], stats


def test_large_values_with_finite_distances(ctx, monkeypatch, oracle):
    """values near 2^60: |x|^2 stays finite at 32 dimensions, 1 + s + s_q ~ 95"""
    rows, centers, off, queries = _scaled_case(60)
    assert np.isfinite((rows.astype(np.float32) ** 2).sum(1)).all()
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=3, what="2^60")


def test_zero_query_and_a_query_with_one_huge_element(ctx, monkeypatch, oracle):
    """q = 0: s_q = 0, q^ = 0; q with one element of 2^10 and the rest tiny: after its scale the rest are fp16
    subnormals or zero, the query term 2 |q - q^| P covers what they lose"""
    dim = 64
    rows, centers, off = _mixture(3000, dim, 8, seed=4)
    queries = _queries_near(rows, 32, 4)
    queries[0] = 0.0
    queries[1] = 1e-6
    queries[1, 5] = 1024.0
    queries[2, 7] = 1024.0
    queries[3] = np.float32(2.0 ** -30) * np.arange(dim, dtype=np.float32)
    queries[3, 0] = 4.0
    for i in (1, 3):
        qh = np.abs(sm.cast_query(queries[i])[1].astype(np.float64))
        assert ((qh > 0) & (qh < 2.0 ** -14)).sum() >= 30, i
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=3, what="query edges")


def test_lists_of_very_different_spread_share_one_scale(ctx, monkeypatch, oracle):
    """one list spread ~1, others ~2^-28 of that: the one index-wide scale makes the tight lists' shadow rows fp16
    subnormals or zero; E charges it"""
    dim = 48
    rows, centers, off = _mixture(4000, dim, 8, seed=5)
    f = np.float32(2.0 ** -28)
    rows[off[1]:] *= f  # lists 1 .. 7, centers and rows: the same shapes 2^28 smaller
    centers[1:] *= f
    s, sh, E, P = sm.shadow_rows(rows, centers, off)
    tight = np.abs(sh[off[1]:].astype(np.float64))
    assert (tight < 2.0 ** -14).all() and (tight == 0).any() and (tight > 0).mean() > 0.9
    queries = np.concatenate([_queries_near(rows[off[1]:], 48, 5, sigma=0.05 * f), _queries_near(rows[:off[1]], 16, 6)])
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=2, what="spread 2^28")


@pytest.mark.parametrize("where", ["nan row", "inf row", "nan center"])
def test_non_finite_data_drops_the_shadow(ctx, monkeypatch, oracle, where):
    dim = 64
    rows, centers, off = _mixture(3000, dim, 8, seed=6)
    queries = _queries_near(rows, 48, 6)
    if where == "nan row":
        rows[int(off[3]) + 2, 5] = np.nan
    elif where == "inf row":
        rows[int(off[5]), 0] = np.inf
    else:
        centers[2, 9] = np.nan
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=3, shadow=False, vs_oracle=False, what=where)


# ---------------------------------------------------------------------------------------------------------------------
# list shapes

@pytest.mark.parametrize("empty", [(0,), (5,), (11,), (0, 1, 6, 10, 11)])
def test_empty_lists(ctx, monkeypatch, oracle, empty):
    """list_of_row and shadow_pair_kernel's pair_start search with lists that share an offset (first, middle, last)"""
    dim, nlists = 40, 12
    sizes = np.random.default_rng(7).integers(30, 90, nlists)
    sizes[list(empty)] = 0
    rows, centers, off = _mixture(0, dim, nlists, seed=7, sizes=sizes)
    queries = _queries_near(rows, 64, 7, sigma=0.3)
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, lists=np.tile(np.arange(nlists, dtype=np.int32), (64, 1)),
          what="empty %s" % (empty,))
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=3, what="empty %s probes 3" % (empty,))


def test_single_row_lists_and_short_ragged_lists(ctx, monkeypatch, oracle):
    """lists of one row, and lists shorter than one 128-row task and not a multiple of 16"""
    dim, nlists = 72, 16
    sizes = np.array([1, 1, 3, 17, 1, 95, 33, 127, 1, 129, 255, 1, 7, 49, 1, 300])
    rows, centers, off = _mixture(0, dim, nlists, seed=8, sizes=sizes)
    queries = _queries_near(rows, 96, 8, sigma=0.3)
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=5, what="short lists")


def test_one_list_of_100k_rows(ctx, monkeypatch, oracle):
    dim = 64
    rows, centers, off = _mixture(0, dim, 3, seed=9, sizes=[100_000, 500, 700])
    queries = _queries_near(rows[:100_000], 40, 9)
    lists = np.zeros((40, 1), dtype=np.int32)
    lists[::4] = 2
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, lists=lists, what="100k list")


def test_probes_equal_to_lists(ctx, monkeypatch, oracle):
    dim, nlists = 56, 20
    rows, centers, off = _mixture(4000, dim, nlists, seed=10)
    queries = _queries_near(rows, 64, 10, sigma=0.2)
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=nlists, what="probes = nlists")


# ---------------------------------------------------------------------------------------------------------------------
# shapes

@pytest.mark.parametrize("dim", [1, 7, 8, 65, 100, 2000])
def test_dimensions(ctx, monkeypatch, oracle, dim):
    nlists = 12
    n = 1500 if dim == 2000 else 4000
    rows, centers, off = _mixture(n, dim, nlists, seed=dim, sigma=0.2)
    queries = _queries_near(rows, 64, dim, sigma=0.1)
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, probes=3, what="dim %d" % dim)


@pytest.mark.parametrize("k", [1, 16, 17, 64, 65, 192])
def test_head_sizes(ctx, monkeypatch, oracle, k):
    """k across the k' steps of approx_candidates (32, 64, 128, 256, k + 64) up to the largest matrix-core head"""
    dim, nlists = 80, 10
    rows, centers, off = _mixture(5000, dim, nlists, seed=11)
    queries = _queries_near(rows, 48, 11)
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, k, probes=3, what="k %d" % k)


def test_k_larger_than_the_rows_probed(ctx, monkeypatch, oracle):
    dim, nlists = 24, 16
    sizes = np.array([5, 9, 0, 12, 3, 30, 7, 1, 22, 4, 16, 2, 8, 11, 6, 10])
    rows, centers, off = _mixture(0, dim, nlists, seed=12, sizes=sizes)
    queries = _queries_near(rows, 64, 12, sigma=0.3)
    check(ctx, monkeypatch, oracle, rows, centers, off, queries, 40, probes=2, what="k > rows")


# ---------------------------------------------------------------------------------------------------------------------
# views

def test_shared_view_outlives_the_original(ctx, monkeypatch, oracle):
    """a pgv_index_share view on a second context: search after the original is closed, then close the view -- the
    shadow goes with the last handle, once"""
    dim, nlists = 128, 16
    rows, centers, off = _mixture(6000, dim, nlists, seed=13)
    queries = _queries_near(rows, 64, 13)
    lists = _nearest_lists(centers, queries, 4)
    _, (d0, s0, t0) = check(ctx, monkeypatch, oracle, rows, centers, off, queries, 10, lists=lists, what="view: original")
    monkeypatch.setenv("PGV_SCAN_SHADOW", "1")
    ctx2 = api.Context(0)
    try:
        ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, dim, centers, off, rows, _tids(rows.shape[0]))
        view = ix.share(ctx2)
        ix.close()
        ctx2.reset_stats()
        d, s, t = view.scan_batch(queries, lists, 10, want_tid=True)
        ctx2.sync()
        assert ctx2.stats()["scan_shadow_queries"] == queries.shape[0]
        np.testing.assert_array_equal(np.asarray(d).view(np.uint32), d0.view(np.uint32))
        np.testing.assert_array_equal(s, s0)
        np.testing.assert_array_equal(t, t0)
        view.close()
    finally:
        ctx2.close()
    ctx.sync()


# ---------------------------------------------------------------------------------------------------------------------
# the kernel forms: PGV_SCAN_WIDE / PGV_SCAN_DEEP are read once per process

@pytest.mark.parametrize("env", [{"PGV_SCAN_WIDE": "0", "PGV_SCAN_DEEP": "0"}, {"PGV_SCAN_WIDE": "0"},
                                 {"PGV_SCAN_WIDE": "1"}], ids=["plain", "deep", "wide"])
def test_every_scan_form_in_a_process_that_forces_it(env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ, PGV_SCAN_SHADOW="1", **env)
    if "PGV_SCAN_DEEP" not in env:
        e.pop("PGV_SCAN_DEEP", None)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "mp_shadow_forms_worker.py")], capture_output=True,
                       text=True, timeout=600, env=e)
    assert r.returncode == 0 and "SHADOW-FORMS-OK 5 " in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    print(r.stdout.strip().splitlines()[-1])
