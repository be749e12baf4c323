"""Probe pruning's rule (pgvector_amd/csrc/pgv_internal.h beside ScanBound; tests/prune_model.py is its host model) against
brute force, and the shapes of tests/test_gpu_probe_prune.py against what they are for.  No GPU.

The property: for every query, no row of a dropped list is within the k-th smallest distance of the rows of the lists that
are kept -- in float64 and in the fp32 sum((q - x)^2) the search orders by, strictly, so ties cannot matter."""
import numpy as np
import pytest

import mp_probe_prune_worker as w
import prune_model as pm


def _clustered(seed, dim, lists, per, sigma, spread):
    rng = np.random.default_rng(seed)
    centers = (spread * rng.standard_normal((lists, dim))).astype(np.float32)
    lens = rng.integers(0, 2 * per, lists)
    lens[rng.integers(0, lists)] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.repeat(centers, lens, axis=0) + (sigma * rng.standard_normal((int(off[-1]), dim))).astype(np.float32)
    rows = rows.astype(np.float32)
    # the lists are an ARBITRARY partition for the rule (rows need not sit in their nearest center's list): move a few
    for i in rng.integers(0, rows.shape[0], 8):
        rows[i] = centers[rng.integers(0, lists)] + np.float32(sigma)
    q = rows[rng.integers(0, rows.shape[0], 48)] + (sigma * rng.standard_normal((48, dim))).astype(np.float32)
    return centers, off, rows, q.astype(np.float32)


def _check_never_loses_an_answer(centers, off, rows, queries, probes, k, what):
    R = pm.radii(centers, off, rows)
    ndropped = 0
    for qi, q in enumerate(queries):
        lists = pm.rank_lists(q, centers, probes)
        drop = pm.dropped_for(q, centers, off, R, lists, k)
        ndropped += int(drop.sum())
        if not drop.any():
            continue
        kept = np.concatenate([np.arange(off[l], off[l + 1]) for l in lists[~drop]])
        gone = np.concatenate([np.arange(off[l], off[l + 1]) for l in lists[drop]])
        assert kept.size >= k, (what, qi)
        if gone.size == 0:
            continue
        for dt in (np.float64, np.float32):
            dk = np.sort(np.sum((rows[kept].astype(dt) - q.astype(dt)) ** 2, axis=1, dtype=dt))[k - 1]
            dg = np.min(np.sum((rows[gone].astype(dt) - q.astype(dt)) ** 2, axis=1, dtype=dt))
            assert dg > dk, (what, qi, dt, dg, dk)
    return ndropped


@pytest.mark.parametrize("seed,dim,sigma,spread,probes,k", [
    (1, 8, 0.1, 1.0, 6, 10), (2, 32, 0.1, 0.3, 8, 10), (3, 64, 0.3, 0.2, 8, 1), (4, 100, 0.05, 0.1, 12, 40),
    (5, 16, 1.0, 1.0, 8, 10), (6, 257, 0.1, 0.05, 5, 3)])
def test_rule_never_drops_a_list_that_holds_an_answer(seed, dim, sigma, spread, probes, k):
    centers, off, rows, q = _clustered(seed, dim, 40, 30, sigma, spread)
    n = _check_never_loses_an_answer(centers, off, rows, q, probes, k, "seed %d" % seed)
    print("seed %d: %d of %d probes dropped" % (seed, n, q.shape[0] * probes))


def test_clustered_sets_are_pruned_and_overlapping_ones_less():
    tight = _check_never_loses_an_answer(*_clustered(1, 8, 40, 30, 0.1, 1.0), 6, 10, "tight")
    loose = _check_never_loses_an_answer(*_clustered(5, 16, 40, 30, 1.0, 1.0), 8, 10, "loose")
    assert tight > 0 and loose < tight


def test_uniform_data_drops_nothing():
    c, off, rows, calls = w.prune_cases()["uniform"]
    q, probes, k = calls[0]
    R = pm.radii(c, off, rows)
    assert sum(int(pm.dropped_for(x, c, off, R, pm.rank_lists(x, c, probes), k).sum()) for x in q) == 0
    assert q.shape[0] * probes / c.shape[0] > 3.0  # the list-major MFMA plan


def _drops(case, call=0):
    c, off, rows, calls = case
    q, probes, k = calls[call]
    R = pm.radii(c, off, rows)
    lists = [pm.rank_lists(x, c, probes) for x in q]
    return lists, [pm.dropped_for(x, c, off, R, l, k) for x, l in zip(q, lists)], R


def test_the_gpu_cases_prune_where_they_should():
    cases = w.prune_cases()
    for name in ("d64", "d1536", "flagged", "planted", "equal"):
        _, drops, _ = _drops(cases[name])
        n = sum(int(d.sum()) for d in drops)
        print("%s: the model drops %d probes" % (name, n))
        assert n > 0, name
    for name, (c, off, rows, calls) in cases.items():
        assert c.shape[0] == 64 and rows.shape[0] <= 6500, name
        for q, probes, k in calls:
            assert 128 <= q.shape[0] <= 160, name


def test_planted_edges_reach_their_branches():
    c, off, rows, calls = w.prune_cases()["planted"]
    q, probes, k = calls[0]
    lens = np.diff(off)
    lists, drops, R = _drops((c, off, rows, calls))
    # the outlier: list 7 is probed last, is as far as the dropped lists 1 and 4, holds a top-k answer; its radius saves it
    i = w.Q_OUTLIER
    assert lists[i].tolist() == [5, 1, 4, 7] and drops[i].tolist() == [False, True, True, False]
    d = np.sum((rows.astype(np.float64) - q[i].astype(np.float64)) ** 2, axis=1)
    outlier = int(off[w.OUTLIER_LIST + 1] - 1)
    probed = np.concatenate([np.arange(off[l], off[l + 1]) for l in lists[i]])
    assert outlier in probed[np.argsort(d[probed], kind="stable")[:k]]
    assert R[w.OUTLIER_LIST] > 64.0 and np.delete(R, w.OUTLIER_LIST).max() < 7.0
    # the nearest list holds fewer than k rows: m = 2, and the far side of the others is inside tau
    i = w.Q_SHORT
    assert lists[i][0] == 1 and lens[1] < k and not drops[i].any()
    # fewer than k rows in all probes together, an empty list second
    i = w.Q_STARVED
    assert lists[i].tolist() == [48, 16, 32, 49] and lens[lists[i]].sum() < k and lens[16] == 0 and not drops[i].any()
    # an empty list in the middle of the probe order behind a full one
    i = w.Q_EMPTY_MID
    assert lists[i].tolist() == [40, 8, 32, 41] and lens[8] == 0 and drops[i].tolist() == [False, True, True, True]
    # NaN / inf queries: nothing is dropped; the subnormal query is an ordinary one (its distances are the centers' norms)
    assert not drops[w.Q_NAN].any() and not drops[w.Q_INF].any()
    # k = 1 (call 1) and k = 100 with one probe (call 2): one probe can drop nothing
    assert calls[1][2] == 1 and calls[2][1:] == (1, 100)
    assert sum(int(x.sum()) for x in _drops((c, off, rows, calls), 1)[1]) > 0
    assert sum(int(x.sum()) for x in _drops((c, off, rows, calls), 2)[1]) == 0


def test_equality_keeps_and_its_twin_beyond_is_dropped():
    c, off, rows, calls = w.prune_cases()["equal"]
    q, probes, k = calls[0]
    lists, drops, R = _drops((c, off, rows, calls))
    assert float(R[0]) >= 5.0 and float(R[0]) < 5.00001 and float(R[1]) >= 8.0 and float(R[1]) < 8.00001
    assert lists[0].tolist() == [0, 1, 2, 3] and drops[0].tolist() == [False, False, True, True]   # 13 - 8 = 0 + 5: kept
    assert lists[1].tolist() == [2, 3, 0, 4] and drops[1].tolist() == [False, True, True, True]    # 15 - 8 > 0 + 5
    # the rule with NO margins keeps at equality too: strict >
    assert not pm.dropped(np.float32([0, 169]), np.float32([5, 8]), [40, 40], 10, 16)[1]
    assert pm.dropped(np.float32([0, 225]), np.float32([5, 8]), [40, 40], 10, 16)[1]


def test_non_finite_and_degenerate_inputs_drop_nothing():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    far = np.float32(1e6)
    assert pm.dropped(np.float32([0, far]), np.float32([1, 1]), [40, 40], 10, 16).tolist() == [False, True]
    assert not pm.dropped(np.float32([nan, far]), np.float32([1, 1]), [40, 40], 10, 16).any()
    assert not pm.dropped(np.float32([0, far]), np.float32([inf, 1]), [40, 40], 10, 16).any()
    assert not pm.dropped(np.float32([0, far]), np.float32([1, inf]), [40, 40], 10, 16).any()
    assert not pm.dropped(np.float32([0, inf]), np.float32([1, 1]), [40, 40], 10, 16).any()
    assert not pm.dropped(np.float32([0, nan]), np.float32([1, 1]), [40, 40], 10, 16).any()
    assert not pm.dropped(np.float32([0, far]), np.float32([1, 1]), [4, 40], 10, 16).any()       # m = 2: no probe behind it
    assert not pm.dropped(np.float32([0, far, far]), np.float32([1, 1, 1]), [4, 3, 2], 10, 16).any()  # fewer than k rows
    assert not pm.dropped(np.float32([3e38, 3.3e38]), np.float32([1, 1]), [40, 40], 10, 16).any()
    # a kept side whose rows' distances may overflow fp32: nothing is dropped behind it
    assert not pm.dropped(np.float32([1e38, 3.4e38]), np.float32([1.5e19, 0]), [40, 40], 10, 16).any()
