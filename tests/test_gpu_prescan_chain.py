"""The launches in front of the batched list scan.  When pgv_search_batch ranks on the center shadow
and a list-major shadow scan follows, the ranking's kernels do part of the plan: topk_kernel clears the list counters,
batch_recheck_kernel counts the lists where it emits them and writes probe_off / seg_len, batch_fix_kernel moves the
counts of the queries it redoes; the plan is then plan_scan_kernel (with the profiling totals) and one launch for pairs
and tasks.  The yardstick is the unfused composition on the same index and queries, pgv_rank_lists + pgv_scan_batch
(memset, plan_count_kernel, shadow_pair_kernel, plan_stats_kernel): distances, slots and tids byte for byte, the
profiling counters equal, and both against the CPU oracle.  tests/mp_prescan_chain_worker.py runs everything in one child
process (PGV_SCAN_SHADOW is read when the library loads).

The query cast (shadow_query_kernel) is compared with a numpy restatement: cast row and power-of-two scales bit for bit;
the band terms are upper bounds formed in fp64, inflated by 2^-20 and rounded to fp32 (relative 2^-24), so each must be
>= the model's fp64 value and within 1e-5 relative of it (2^-20 + 2^-24 + the few 1e-9 the host adds to E and P are
~1e-6)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rank_shadow_model as rm
import shadow_model as sm
from helpers import assert_topk_equiv
from mp_prescan_chain_worker import CAST_DIMS, K, STAT_KEYS, cast_cases, prescan_cases, tids_of
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CALLS = [("d64", 0), ("d100", 0), ("d1536", 0), ("repeat", 0), ("repeat", 1), ("repeat", 2), ("allcand", 0), ("allcand", 1),
         ("flagged", 0)]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path_factory.mktemp("prescan") / "out.npz")
    e = dict(os.environ, PGV_SCAN_SHADOW="1", PGV_RANK_SHADOW="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "mp_prescan_chain_worker.py"), path],
                       capture_output=True, text=True, timeout=600, env=e)
    want = "PRESCAN-OK %d" % (len(prescan_cases()) + len(CAST_DIMS))
    assert r.returncode == 0 and want in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return dict(np.load(path))


@pytest.fixture(scope="module")
def cases():
    return prescan_cases()


def _stat(run, key, which, name):
    return run[key + which][STAT_KEYS.index(name)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_shapes_reach_what_they_are_for(cases):
    c, off, rows, calls = cases["d64"]
    lens = np.diff(off)
    assert lens[0] == 0 and lens[1] == 1 and lens[2] > 128 and 5500 <= rows.shape[0] <= 6500
    for name, (c, off, rows, calls) in cases.items():
        for q, probes in calls:
            assert 128 <= q.shape[0] <= 160 and q.shape[0] * probes / c.shape[0] > 3.0, name  # the list-major MFMA plan


@pytest.mark.parametrize("name,i", CALLS)
def test_fused_chain_equals_the_unfused_composition_byte_for_byte(run, cases, name, i):
    key = "%s.%d" % (name, i)
    nq = cases[name][3][i][0].shape[0]
    # no silent fallback: both paths scanned the fp16 residual shadow for every query
    assert _stat(run, key, ".stats", "scan_shadow_queries") == nq, run[key + ".stats"]
    assert _stat(run, key, ".stats2", "scan_shadow_queries") == nq, run[key + ".stats2"]
    np.testing.assert_array_equal(_bits(run[key + ".d"]), _bits(run[key + ".d2"]), err_msg=key)
    np.testing.assert_array_equal(run[key + ".s"], run[key + ".s2"], err_msg=key)
    np.testing.assert_array_equal(run[key + ".t"], run[key + ".t2"], err_msg=key)


@pytest.mark.parametrize("name,i", CALLS)
def test_profiling_totals_from_plan_scan_kernel_equal_plan_stats_kernels(run, name, i):
    key = "%s.%d" % (name, i)
    for stat in ("scan_pairs", "scan_rows", "scan_unique_rows", "scan_launches"):
        a, b = _stat(run, key, ".stats", stat), _stat(run, key, ".stats2", stat)
        assert a == b and a > 0, (key, stat, a, b)


@pytest.mark.parametrize("name,i", CALLS)
def test_both_paths_answer_what_the_oracle_answers(run, cases, oracle, name, i):
    centers, off, rows, calls = cases[name]
    q, probes = calls[i]
    key = "%s.%d" % (name, i)
    ixs = oracle.index_struct(po.OPS_L2, po.ORA_F32, centers, off, rows, tids_of(rows.shape[0]))
    for suffix in ("", "2"):
        d, t = run[key + ".d" + suffix], run[key + ".t" + suffix]
        for j in range(q.shape[0]):
            wt, wd = oracle.search(ixs, q[j], probes, K)
            n = len(wt)
            assert_topk_equiv(t[j][:n].astype(np.uint64).tolist(), d[j][:n], wt.tolist(), wd, what="%s q%d" % (key, j))
            assert np.isinf(d[j][n:]).all(), (key, j)


def test_lists_probed_by_two_query_groups_and_the_edge_lists_are_probed(run):
    lists = run["d64.0.lists"]
    per_list = np.bincount(lists.ravel(), minlength=64)
    assert per_list[2] > 32 and per_list[0] >= 1 and per_list[1] >= 1, per_list[:3]


def test_flagged_ranking_queries_occurred_and_their_lists_were_replaced_in_the_plan(run, cases):
    """`flagged`: the ranking's band swallows its candidates, batch_fix_kernel decides those queries' lists after the
    recheck has counted the ones it emitted.  The counters of the fused call hold the ranking's and the scan's flagged
    queries; the ranking alone (pgv_rank_lists) flagged too.  The answers are compared in the tests above."""
    rank = _stat(run, "flagged.0", ".rank_stats", "scan_widened_queries") + _stat(run, "flagged.0", ".rank_stats", "scan_redo_queries")
    fused = _stat(run, "flagged.0", ".stats", "scan_widened_queries") + _stat(run, "flagged.0", ".stats", "scan_redo_queries")
    print("flagged: ranking alone %g, fused call %g" % (rank, fused))
    assert rank >= 1 and fused >= rank
    assert _stat(run, "d64.0", ".rank_stats", "scan_widened_queries") + _stat(run, "d64.0", ".rank_stats", "scan_redo_queries") == 0


def _model_terms(centers, off, rows, q):
    """shadow_query_kernel's qeps and ceps in float64 WITHOUT the final inflation: what the fp32 values must bound"""
    dim = rows.shape[1]
    u = rm.U
    s, _, E, P = sm.shadow_rows(rows, centers, off)
    s_c, _, E_c, P_c = rm.cast_centers(centers)
    cn_max = float(np.max(rm.center_norms_f32(centers)))
    rn_max = float(np.max(rm.center_norms_f32(rows)))
    ld = (dim + 3) // 4 * 4
    g_dot, g_cn, g_pair = rm.gamma(sm.chain_length(dim) + 4.0), rm.gamma(ld / 64.0 + 10.0), rm.gamma(rm.pair_chain_length(dim)[0])
    qeps, ceps, qexp, cexp = [], [], [], []
    for x in q:
        x64 = x.astype(np.float64)
        sq, qh = sm.cast_query(x)
        back = np.ldexp(qh.astype(np.float64), sq)
        qn, dq, qhn = np.linalg.norm(x64), np.linalg.norm(x64 - back), np.linalg.norm(back)
        tmax = 2.0 * qn * np.sqrt(cn_max * (1.0 + g_cn))
        a = 2.0 * (qn * E + dq * P) + g_dot * 2.0 * qhn * P + g_pair * tmax + \
            4.0 * u * (rn_max * (1.0 + g_cn) + tmax * (1.0 + g_pair) + 2.0 * qhn * P * (1.0 + g_dot))
        b = 2.0 * (qn * E_c + dq * P_c) + g_dot * 2.0 * qhn * P_c + 4.0 * u * (cn_max * (1.0 + g_cn) + 2.0 * qhn * P_c * (1.0 + g_dot))
        for val, e, vals, exps in ((a, 1 + s + sq, qeps, qexp), (b, 1 + s_c + sq, ceps, cexp)):
            bad = e < -125 or e > 125 or not val < 1e30
            vals.append(np.inf if bad else val)
            exps.append(0 if (e < -125 or e > 125) else e)
    return np.array(qeps), np.array(ceps), np.array(qexp), np.array(cexp)


@pytest.mark.parametrize("dim", CAST_DIMS)
def test_query_cast_rows_and_scales_bit_for_bit_and_band_terms_bound_the_model(run, dim):
    centers, off, rows, q = cast_cases()[dim]
    ld16 = (dim + 7) // 8 * 8
    want = np.zeros((q.shape[0], ld16), dtype=np.float16)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i, x in enumerate(q):
            want[i, :dim] = sm.cast_query(x)[1]
        qeps, ceps, qexp, cexp = _model_terms(centers, off, rows, q)
    got = run["cast%d.qcast" % dim]
    ok = ~np.isnan(q).any(axis=1)  # (a NaN query: its scale is 0 and the NaN's payload is the hardware's)
    np.testing.assert_array_equal(got[ok], want.view(np.uint16)[ok], err_msg="dim %d" % dim)
    assert np.isnan(got[11].view(np.float16)[dim // 2])
    np.testing.assert_array_equal(_bits(run["cast%d.qscale" % dim]), _bits(np.ldexp(np.float32(1.0), qexp).astype(np.float32)))
    np.testing.assert_array_equal(_bits(run["cast%d.cscale" % dim]), _bits(np.ldexp(np.float32(1.0), cexp).astype(np.float32)))
    for name, model in (("qeps", qeps), ("ceps", ceps)):
        g = run["cast%d.%s" % (dim, name)].astype(np.float64)
        print("dim %d %s: got / model - 1 in [%g, %g]" % (dim, name, np.nanmin(g[:9] / model[:9] - 1), np.nanmax(g[:9] / model[:9] - 1)))
        assert np.isinf(g[11]) and g[11] > 0, (dim, name, g[11])       # the NaN query: an infinite band
        assert np.isinf(model[10]) and np.isinf(g[10]), (dim, name)     # the subnormal query: its scale leaves fp32's range
        fin = np.isfinite(model)
        assert fin[:10].all() and np.isfinite(g[:10]).all(), (dim, name)  # (row 9: the zero query)
        assert (g[fin] >= model[fin]).all(), (dim, name, g[fin] / model[fin] - 1)
        assert (g[fin] - model[fin] <= 1e-5 * model[fin] + 8 * rm.FLT_MIN).all(), (dim, name, g[fin] / model[fin] - 1)
