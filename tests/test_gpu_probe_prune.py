"""Probe pruning on the device (the rule: pgv_internal.h beside ScanBound, tests/prune_model.py).  A batch
over the fp16 residual shadow drops the probed lists that provably hold none of a query's k nearest rows -- in the
ranking's recheck and batch_fix_kernel where pgv_search_batch emits the lists, in probe_prune_kernel where
pgv_scan_batch is given them.  tests/mp_probe_prune_worker.py runs every case with PGV_PROBE_PRUNE=1 and =0 through both
routes in one child process (PGV_SCAN_SHADOW=1); tests/test_probe_prune_cpu.py checks on the host that the cases reach
the branches they are for.

Pruning must not change a bit of the answers: distances, slots and tids with it on equal those with it off byte for byte,
and both are what the CPU oracle's search returns.  The pruned counts of the two routes are equal, zero with the switch
off, and on the planted integer cases (every distance exact in fp32) equal to the host model's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import prune_model as pm
from helpers import assert_topk_equiv
from mp_probe_prune_worker import Q_INF, Q_NAN, STAT_KEYS, prune_cases, tids_of
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CALLS = [("d64", 0), ("d1536", 0), ("flagged", 0), ("planted", 0), ("planted", 1), ("planted", 2), ("planted", 3), ("equal", 0),
         ("uniform", 0)]
SHADOW_CALLS = [c for c in CALLS if c != ("planted", 2)]  # (one probe of 128 queries over 64 lists: not a list-major MFMA batch)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path_factory.mktemp("prune") / "out.npz")
    e = dict(os.environ, PGV_SCAN_SHADOW="1", PGV_RANK_SHADOW="1")
    e.pop("PGV_PROBE_PRUNE", None)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "mp_probe_prune_worker.py"), path],
                       capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0 and "PRUNE-OK %d" % (2 * len(CALLS)) in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return dict(np.load(path))


@pytest.fixture(scope="module")
def cases():
    return prune_cases()


def _stat(run, key, which, name):
    return run[key + which][STAT_KEYS.index(name)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name,i", CALLS)
def test_pruning_changes_no_bit_of_the_answers(run, name, i):
    on, off = "%s.%d.p1" % (name, i), "%s.%d.p0" % (name, i)
    for a, b in ((on + ".d", off + ".d"), (on + ".d2", off + ".d2"), (on + ".d", on + ".d2")):
        np.testing.assert_array_equal(_bits(run[a]), _bits(run[b]), err_msg=a)
    for suffix in (".s", ".t"):
        np.testing.assert_array_equal(run[on + suffix], run[off + suffix], err_msg=on + suffix)
        np.testing.assert_array_equal(run[on + suffix + "2"], run[off + suffix + "2"], err_msg=on + suffix)
        np.testing.assert_array_equal(run[on + suffix], run[on + suffix + "2"], err_msg=on + suffix)
    np.testing.assert_array_equal(run[on + ".lists"], run[off + ".lists"])  # pgv_rank_lists returns the true nearest lists
    assert (run[on + ".lists"] >= 0).all()


@pytest.mark.parametrize("name,i", CALLS)
def test_both_routes_answer_what_the_oracle_answers(run, cases, oracle, name, i):
    centers, off, rows, calls = cases[name]
    q, probes, k = calls[i]
    key = "%s.%d.p1" % (name, i)
    ixs = oracle.index_struct(po.OPS_L2, po.ORA_F32, centers, off, rows, tids_of(rows.shape[0]))
    for suffix in ("", "2"):
        d, t = run[key + ".d" + suffix], run[key + ".t" + suffix]
        for j in range(q.shape[0]):
            if not np.isfinite(q[j]).all():  # (every distance NaN: the order among them is the sort's; on == off above)
                continue
            wt, wd = oracle.search(ixs, q[j], probes, k)
            n = len(wt)
            assert_topk_equiv(t[j][:n].astype(np.uint64).tolist(), d[j][:n], wt.tolist(), wd, what="%s q%d" % (key, j))
            assert np.isinf(d[j][n:]).all(), (key, j)


@pytest.mark.parametrize("name,i", SHADOW_CALLS)
def test_pruned_counts_on_off_and_between_the_routes(run, cases, name, i):
    q, probes, k = cases[name][3][i]
    on, off = "%s.%d.p1" % (name, i), "%s.%d.p0" % (name, i)
    for key in (on, off):  # no silent fallback: both routes scanned the shadow
        assert _stat(run, key, ".stats", "scan_shadow_queries") == q.shape[0], key
        assert _stat(run, key, ".stats2", "scan_shadow_queries") == q.shape[0], key
    fused, unfused = _stat(run, on, ".stats", "scan_pruned_probes"), _stat(run, on, ".stats2", "scan_pruned_probes")
    print("%s.%d: %g of %d probes pruned; pairs %g -> %g, rows streamed %g -> %g" % (
        name, i, fused, q.shape[0] * probes, _stat(run, off, ".stats", "scan_pairs"), _stat(run, on, ".stats", "scan_pairs"),
        _stat(run, off, ".stats", "scan_rows"), _stat(run, on, ".stats", "scan_rows")))
    assert fused == unfused
    assert _stat(run, off, ".stats", "scan_pruned_probes") == 0 and _stat(run, off, ".stats2", "scan_pruned_probes") == 0
    for stat in ("scan_pairs", "scan_rows", "scan_unique_rows"):
        assert _stat(run, on, ".stats", stat) == _stat(run, on, ".stats2", stat), stat
        assert _stat(run, on, ".stats", stat) <= _stat(run, off, ".stats", stat), stat
    if name == "uniform":
        assert fused == 0
    elif (name, i) != ("planted", 3):  # (k = 100 takes three of the four lists to fill: the model's count decides below)
        assert fused > 0
        assert _stat(run, on, ".stats", "scan_pairs") < _stat(run, off, ".stats", "scan_pairs")


@pytest.mark.parametrize("name,i", [("planted", 0), ("planted", 1), ("planted", 3), ("equal", 0)])
def test_planted_cases_prune_exactly_what_the_host_model_prunes(run, cases, name, i):
    """integer coordinates: the center distances and the radii have the same bits on both sides"""
    centers, off, rows, calls = cases[name]
    q, probes, k = calls[i]
    R = pm.radii(centers, off, rows)
    lists = run["%s.%d.p1.lists" % (name, i)]
    want = 0
    for j in range(q.shape[0]):
        if j in (Q_NAN, Q_INF) and name == "planted":
            continue  # (nothing is dropped for them, whatever lists the ranking names)
        np.testing.assert_array_equal(lists[j], pm.rank_lists(q[j], centers, probes), err_msg="q%d" % j)
        want += int(pm.dropped_for(q[j], centers, off, R, lists[j], k).sum())
    assert _stat(run, "%s.%d.p1" % (name, i), ".stats", "scan_pruned_probes") == want
    assert _stat(run, "%s.%d.p1" % (name, i), ".stats2", "scan_pruned_probes") == want


def test_flagged_ranking_queries_occurred(run):
    """`flagged`: batch_fix_kernel decides those queries' lists and prunes them where it emits"""
    key = "flagged.0.p1"
    assert _stat(run, key, ".stats", "scan_widened_queries") + _stat(run, key, ".stats", "scan_redo_queries") >= 1
