"""The fp16 residual shadow of fp32 L2 indexes (kernels_shadow.hip): the batched list scan streams fp16 (x - c_l) 2^-s
instead of the fp32 rows, the exact recheck keeps the answers.  Every case compares an index built with the shadow
(PGV_SCAN_SHADOW=1) against the same index without it (PGV_SCAN_SHADOW=0): distances as bit patterns, slots and tids
equal."""
import numpy as np
import pytest

from pgvector_amd import api

pytestmark = pytest.mark.gpu


def _mixture(n, dim, nlists, seed, comps=None, sigma=0.1, scale=1.0):
    """bench.py's headline kind of data: uniform means, Gaussian components of spread sigma; `nlists` lists, each the
    rows of one component near a center of its own (a component holds nlists / comps lists).  Rows list-major."""
    rng = np.random.default_rng(seed)
    comps = comps or max(1, nlists // 4)
    means = rng.random((comps, dim), dtype=np.float32)
    centers = means[np.arange(nlists) % comps] + 0.02 * rng.standard_normal((nlists, dim)).astype(np.float32)
    lst = np.sort(rng.integers(0, nlists, n))
    rows = means[lst % comps] + sigma * rng.standard_normal((n, dim)).astype(np.float32)
    off = np.zeros(nlists + 1, dtype=np.int64)
    np.add.at(off, lst + 1, 1)
    off = np.cumsum(off)
    return (np.ascontiguousarray(rows * np.float32(scale)), np.ascontiguousarray(centers * np.float32(scale)), off,
            means * np.float32(scale))


def _queries(means, nq, sigma, seed, scale=1.0):
    rng = np.random.default_rng(seed + 1)
    q = means[rng.integers(0, means.shape[0], nq)] + np.float32(sigma * scale) * rng.standard_normal(
        (nq, means.shape[1])).astype(np.float32)
    return np.ascontiguousarray(q.astype(np.float32))


def _both(ctx, monkeypatch, dim, rows, centers, off, queries, probes, k, lanes=1, batches=1):
    """(shadow, plain) answers of the same batches, and the shadow side's redo count"""
    tids = np.arange(rows.shape[0], dtype=np.uint64) * 7 + 3
    out = []
    redo = 0
    for env in ("1", "0"):
        monkeypatch.setenv("PGV_SCAN_SHADOW", env)
        ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, dim, centers, off, rows, tids)
        try:
            if lanes > 1:
                ix.set_overlap(lanes)
            ctx.set_profiling(True)
            ctx.reset_stats()
            res = []
            for b in range(batches):
                d, s, t = ix.search_batch(queries[b::batches], probes, k, want_tid=True)
                res.append((d, s, t))
            ctx.sync()
            st = ctx.stats()
            if env == "1":
                redo = st["scan_redo_queries"]
                assert st["scan_shadow_queries"] > 0, st  # the shadow ran: no silent fall-back to the fp32 scan
            else:
                assert st["scan_shadow_queries"] == 0, st
            out.append([(np.asarray(d).copy(), np.asarray(s).copy(), np.asarray(t).copy()) for d, s, t in res])
        finally:
            ctx.set_profiling(False)
            ix.close()
    return out[0], out[1], redo


def _assert_same(a, b):
    for (da, sa, ta), (db, sb, tb) in zip(a, b):
        np.testing.assert_array_equal(da.view(np.uint32), db.view(np.uint32))
        np.testing.assert_array_equal(sa, sb)
        np.testing.assert_array_equal(ta, tb)


def test_headline_like_mixture_same_answers(ctx, monkeypatch):
    dim, nlists = 1536, 1000
    rows, centers, off, means = _mixture(200_000, dim, nlists, seed=11, comps=250)
    q = _queries(means, 1024, 0.1, seed=11)
    a, b, _ = _both(ctx, monkeypatch, dim, rows, centers, off, q, probes=10, k=10)
    _assert_same(a, b)
    assert np.isfinite(a[0][0]).all()


@pytest.mark.parametrize("dim", [768, 777])
def test_other_dimensions_same_answers(ctx, monkeypatch, dim):
    rows, centers, off, means = _mixture(40_000, dim, 200, seed=dim)
    q = _queries(means, 256, 0.1, seed=dim)
    a, b, _ = _both(ctx, monkeypatch, dim, rows, centers, off, q, probes=8, k=10)
    _assert_same(a, b)


def test_near_duplicates_collapse_to_one_fp16_row(ctx, monkeypatch):
    """rows that differ from each other below fp16's resolution of their residual (and exact copies): the shadow values
    tie, the exact distances order them (ties by stream position)"""
    dim = 256
    rows, centers, off, means = _mixture(30_000, dim, 200, seed=5)
    rng = np.random.default_rng(5)
    for l in range(0, 200, 3):
        a, e = int(off[l]), int(off[l + 1])
        if e - a < 40:
            continue
        base = rows[a].copy()
        rows[a:a + 30] = base
        rows[a + 15:a + 30, rng.integers(0, dim, 15)] += np.float32(1e-6)
    q = _queries(means, 256, 0.1, seed=5)
    q[:64] = rows[off[:64 * 3:3][:64]] + np.float32(1e-3)
    a, b, _ = _both(ctx, monkeypatch, dim, rows, centers, off, q, probes=8, k=10)
    _assert_same(a, b)


@pytest.mark.parametrize("scale", [1e6, 1e-6])
def test_large_and_tiny_values(ctx, monkeypatch, scale):
    dim = 512
    rows, centers, off, means = _mixture(30_000, dim, 200, seed=9, scale=scale)
    q = _queries(means, 256, 0.1, seed=9, scale=scale)
    a, b, _ = _both(ctx, monkeypatch, dim, rows, centers, off, q, probes=8, k=10)
    _assert_same(a, b)


def test_band_overflow_takes_the_exact_pass(ctx, monkeypatch):
    """300 copies of one row in a list: every query next to it has more tied candidates than k' and the widening can
    hold, so it is scored exactly -- and still answers what the fp32 scan answers"""
    dim = 256
    rows, centers, off, means = _mixture(30_000, dim, 20, seed=3)
    l = int(np.argmax(np.diff(off)))
    a0 = int(off[l])
    assert off[l + 1] - a0 >= 300
    rows[a0:a0 + 300] = rows[a0]
    q = _queries(means, 256, 0.1, seed=3)
    q[:16] = rows[a0] + np.float32(0.01) * np.random.default_rng(3).standard_normal((16, dim)).astype(np.float32)
    a, b, redo = _both(ctx, monkeypatch, dim, rows, centers, off, q, probes=4, k=10)
    _assert_same(a, b)
    assert redo > 0


def test_lanes_share_the_shadow(ctx, monkeypatch):
    dim = 768
    rows, centers, off, means = _mixture(40_000, dim, 200, seed=21)
    q = _queries(means, 768, 0.1, seed=21)
    a, b, _ = _both(ctx, monkeypatch, dim, rows, centers, off, q, probes=8, k=10, lanes=3, batches=3)
    _assert_same(a, b)
