"""pgv_hnsw_score_groups against pgv_hnsw_score_pairs: the pair distances inside groups of rows, by score_groups_kernel's
4 x 4 tiles (the default) and by expand_groups_kernel + score_gather_kernel (PGV_HNSW_PAIRS_GATHER=1, read once per
process: a child, tests/mp_hnsw_link_worker.py groups).

One call (the worker's groups_input): groups of 1, 2, 5, 64, 65, 257 and 300 ids -- across the 64 lanes and the 256
threads of the expand loop and the 4 x 4 tiles -- each with from = 0, 1, 3, n - 1 and n (n: no pairs wanted), ids repeated
inside a group, over 320 rows on an integer grid in [-6, 6]: every distance is exact in fp32 and fp16.  4-d fp32 and 5-d
fp16 rows (the row padding in play), PGV_L2SQ / PGV_NEG_IP / PGV_L1.  The values must be, bit for bit,
pgv_hnsw_score_pairs' over the pairs (u, v < u, u >= max(from, 1)) enumerated in numpy, and equal the float32 numpy
distances of those pairs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mp_hnsw_link_worker as w
from pgvector_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 60      # the child scores 6 x 236 k pairs twice: seconds, start-up included
_WANT = {}


def numpy_distances(metric, dtype):
    """the float32 distances of the call's pairs, computed once per case"""
    if (metric, dtype) not in _WANT:
        _, _, _, _, a, b = w.groups_input()
        rows = w.groups_rows(dtype).astype(np.float32)
        x, y = rows[a], rows[b]
        if metric == api.PGV_L2SQ:
            d = ((x - y) ** 2).sum(1, dtype=np.float32)
        elif metric == api.PGV_NEG_IP:
            d = -(x * y).sum(1, dtype=np.float32)
        else:
            d = np.abs(x - y).sum(1, dtype=np.float32)
        _WANT[(metric, dtype)] = d
    return _WANT[(metric, dtype)]


def check(res):
    ids, ids_start, frm, pair_start, a, b = w.groups_input()
    sizes = np.diff(ids_start)
    assert sorted(set(sizes.tolist())) == list(w.GROUP_SIZES) and len(a) == pair_start[-1] > 200000
    assert (np.diff(pair_start)[frm >= sizes] == 0).all() and (np.diff(pair_start)[(frm < sizes) & (sizes > 1)] > 0).all()
    for metric, dtype in w.GROUP_CASES:
        got, pairs = res["groups/%d/%d" % (metric, dtype)], res["pairs/%d/%d" % (metric, dtype)]
        print(metric, dtype, len(got), "pairs; differing from score_pairs:", int((got.view(np.uint32) != pairs.view(np.uint32)).sum()),
              "from numpy:", int((got != numpy_distances(metric, dtype)).sum()))
        np.testing.assert_array_equal(got.view(np.uint32), pairs.view(np.uint32), err_msg="metric %d dtype %d" % (metric, dtype))
        np.testing.assert_array_equal(got, numpy_distances(metric, dtype), err_msg="metric %d dtype %d" % (metric, dtype))


def test_score_groups_is_score_pairs_over_the_enumerated_pairs(ctx):
    check(w.groups_on_device(ctx))


def test_score_groups_is_score_pairs_over_the_enumerated_pairs_gathered(tmp_path):
    """the same in a child with PGV_HNSW_PAIRS_GATHER=1; one child, never restarted"""
    path = str(tmp_path / "groups.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mp_hnsw_link_worker.py"), "groups", path], capture_output=True,
                       text=True, timeout=CHILD_SECONDS, env=dict(os.environ, PGV_HNSW_PAIRS_GATHER="1"))
    print(r.stdout)
    assert r.returncode == 0 and "GROUPS-OK %d" % len(w.GROUP_CASES) in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    check(dict(np.load(path)))
