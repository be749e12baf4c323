"""The batch ranking over the fp16 center shadow and the pair terms its exact recheck hands to the shadow
scan, through the C ABI.  tests/mp_rank_shadow_worker.py runs every case under PGV_RANK_SHADOW = 0 (fp32 ranking,
shadow_pair_kernel: the path before the center shadow), 1 (the default) and 2 (fp16 ranking, shadow_pair_kernel) in a
process each; here the three are compared bit for bit -- list ids, list distances, and the heads of pgv_search_batch and
of pgv_rank_lists + pgv_scan_batch -- and every query's lists and head are compared with the CPU oracle: ids exact
wherever the reference's own order is a fact (_same_ids_where_the_order_is_a_fact), distances to helpers.RTOL."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import RTOL, assert_close, assert_topk_equiv
from mp_rank_shadow_worker import K, PROBES, _tids, rank_shadow_cases
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CASES = ["mixture", "uniform", "ulp", "huge", "nan"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for mode in ("0", "1", "2"):
        path = str(tmp_path_factory.mktemp("rank_shadow") / ("mode%s.npz" % mode))
        e = dict(os.environ, PGV_SCAN_SHADOW="1", PGV_RANK_SHADOW=mode)
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "mp_rank_shadow_worker.py"), path],
                           capture_output=True, text=True, timeout=900, env=e)
        assert r.returncode == 0 and "RANK-SHADOW-OK %d" % len(CASES) in r.stdout, (mode, r.stdout[-2000:], r.stderr[-3000:])
        out[mode] = dict(np.load(path))
    return out


@pytest.fixture(scope="module")
def cases():
    return rank_shadow_cases()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_ids_where_the_order_is_a_fact(got, want, wd, dim, exact_below, what):
    """ids exact wherever the reference's own order is a fact.  Two neighbours are not ordered by fact when their oracle
    distances are EQUAL, or when they lie closer than the reference's own summation error: sum((q - c)^2) in fp32 is within
    gamma_(dim + 2) of the true value, relative (Higham 3.5, all terms positive), in whatever order its compiler adds --
    except that integer data with sums below `exact_below` = 2^24 is exact in any order, so there only equality is a tie.
    (A run cut by the end of the list: its members come from the tie class.)"""
    g = (dim + 2) * 2.0 ** -24
    g = 2.0 * g / (1.0 - g)

    def tied(a, b):
        if a == b:
            return True
        return not (a < exact_below and b < exact_below) and abs(a - b) <= g * max(abs(a), abs(b))
    i, n = 0, len(want)
    assert len(got) == n, what
    while i < n:
        j = i + 1
        while j < n and tied(wd[j - 1], wd[j]):
            j += 1
        if j == n and j - i > 1:
            assert set(got[:i]) == set(want[:i]), (what, got, want)
            break
        assert sorted(got[i:j]) == sorted(want[i:j]), (what, i, j, got, want)
        i = j


@pytest.mark.parametrize("name", CASES)
def test_fp16_ranking_returns_the_fp32_rankings_lists_bit_for_bit(runs, name):
    a, b, c = runs["0"], runs["1"], runs["2"]
    for other in (b, c):
        np.testing.assert_array_equal(a[name + ".rank_ids"], other[name + ".rank_ids"], err_msg=name)
        np.testing.assert_array_equal(_bits(a[name + ".rank_dist"]), _bits(other[name + ".rank_dist"]), err_msg=name)


@pytest.mark.parametrize("name", CASES)
def test_lists_are_the_oracles(runs, cases, oracle, name):
    centers, off, rows, q = cases[name]
    if name == "nan":
        # a NaN distance has no place in the reference's pairing heap (every comparison with it is false: where it lands,
        # and what it displaces, is an accident of the insertion order); the float8 order the library sorts by puts NaN
        # last.  The oracle therefore ranks the same centers with the NaN center moved far away: the same ten lists.
        nan_rows = np.flatnonzero(np.isnan(centers).any(axis=1))
        assert nan_rows.tolist() == [7]
        centers = centers.copy()
        centers[7] = 1000.0
    ixs = oracle.index_struct(po.OPS_L2, po.ORA_F32, centers, off, rows, _tids(rows.shape[0]))
    ids, dist = runs["1"][name + ".rank_ids"], runs["1"][name + ".rank_dist"]
    for i in range(q.shape[0]):
        wl, wd = oracle.get_scan_lists(ixs, q[i], PROBES)
        n = len(wl)
        assert n == PROBES and np.isfinite(wd).all(), (name, i)
        assert_close(dist[i][:n], wd, rtol=RTOL, what="%s q%d list distances" % (name, i))
        _same_ids_where_the_order_is_a_fact(ids[i][:n].tolist(), wl.tolist(), wd, q.shape[1],
                                            2.0 ** 24 if name == "ulp" else 0.0, "%s q%d" % (name, i))


@pytest.mark.parametrize("name", CASES)
def test_pair_terms_from_the_ranking_and_from_the_pair_kernel_give_one_head(runs, cases, oracle, name):
    """mode 1: t from batch_recheck_kernel (batch_fix_kernel for flagged queries); modes 0 / 2 and every mode's
    pgv_rank_lists + pgv_scan_batch: t from shadow_pair_kernel.  Both land in the band: the heads are the exact
    recheck's, bit for bit; and they are the oracle's."""
    nq = cases[name][3].shape[0]
    ref = runs["0"]
    for mode in ("0", "1", "2"):
        r = runs[mode]
        want_shadow = 0 if name == "nan" else nq  # NaN in a center: the shadow is dropped, the fp32 scan answers
        assert r[name + ".shadow_queries"][0] == want_shadow, (name, mode, r[name + ".shadow_queries"])
        for suffix in ("", "2"):
            np.testing.assert_array_equal(_bits(ref[name + ".d"]), _bits(r[name + ".d" + suffix]), err_msg="%s mode %s" % (name, mode))
            np.testing.assert_array_equal(ref[name + ".s"], r[name + ".s" + suffix], err_msg="%s mode %s" % (name, mode))
            np.testing.assert_array_equal(ref[name + ".t"], r[name + ".t" + suffix], err_msg="%s mode %s" % (name, mode))
    if name == "nan":
        return  # (the reference's list choice with a NaN center is its heap's accident: the lists test compares the rest)
    centers, off, rows, q = cases[name]
    ixs = oracle.index_struct(po.OPS_L2, po.ORA_F32, centers, off, rows, _tids(rows.shape[0]))
    d, t = runs["1"][name + ".d"], runs["1"][name + ".t"]
    for i in range(nq):
        wt, wd = oracle.search(ixs, q[i], PROBES, K)
        assert_topk_equiv(t[i].astype(np.uint64).tolist(), d[i], wt.tolist(), wd, what="%s q%d" % (name, i))


def test_a_flagged_ranking_fills_the_pair_terms_end_to_end(runs, cases):
    """`huge`: one coordinate of 4096 sets the scale of the fp16 centers, the other 255 keep ~2^-12 each, so 2 |q| E_c is
    tens of units against center gaps of a few: the band swallows the candidates, batch_fix_kernel decides the lists
    and fills their pair terms, and the shadow scan that follows still returns the fp32 path's head (the test above).
    Here: the ranking did flag (the fp32 ranking's own band flags on this data too: |c|^2 ~ 1.7e7)."""
    nq = cases["huge"][3].shape[0]
    assert runs["1"]["huge.rank_flagged"].sum() >= 1, runs["1"]["huge.rank_flagged"]
    assert runs["2"]["huge.rank_flagged"].sum() >= 1
    assert runs["1"]["huge.shadow_queries"][0] == nq
    print("huge: ranking widened / exact-pass queries, fp32", runs["0"]["huge.rank_flagged"], "fp16", runs["1"]["huge.rank_flagged"])
    for name in ("mixture", "uniform"):  # benign data: nobody is flagged
        assert runs["1"][name + ".rank_flagged"].sum() == 0, (name, runs["1"][name + ".rank_flagged"])
