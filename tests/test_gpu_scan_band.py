"""The deterministic rounding band of the MFMA L2 paths under attack (tests/chain_model.py builds the data,
tests/mp_scan_band_worker.py holds the checks).

fp32: every kernel form's raw values equal the chain model bit for bit, and rows whose rounding error reaches 0.67 ..
0.99 of the g_dot term in either direction -- a true neighbour pushed up, k decoys pushed down, more than k' honest
rows in between -- still get the oracle's answer, id for id, because the band flags the query; tests/
test_chain_model_cpu.py shows the same sets defeat a band of half the width.
fp16: the matrix instructions are not an fmaf chain, so the raw values are only held to the charged bound (one u per
product); the largest fraction of it seen on an MI355X is in profiles/r08_scan_band.md.

The statistical bound is the WIDER band below ~4100 dimensions, so it loses the true neighbour only on the 8192-d set
(its stated failure probability is about sums that behave randomly; these do not): it is run there, nothing is
asserted about its answers, and the default is pinned to the deterministic one on a context nobody called set_bound
on."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_model as cm
import mp_scan_band_worker as w

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_shadow(monkeypatch):
    monkeypatch.setenv("PGV_SCAN_SHADOW", "0")


WIDE = {None: None, "": None, "0": False, "1": True}[os.environ.get("PGV_SCAN_WIDE")]   # (the suite runs without it)


@pytest.mark.parametrize("dim", w.DIMS)
def test_scan_raw_values_match_the_chain_model(ctx, dim):
    """a list probed by 8, 24 and 48 queries: the 16-wide path, the four-chain 32-query form, and the 64-query form (more
    than 12 queries on the one list: the library picks the 64-query kernel by itself)"""
    assert w.raw_scan_checks(ctx, WIDE, dims=(dim,), sizes=(8, 24, 48)) == 6


@pytest.mark.parametrize("dim", w.DIMS)
def test_exact_topk_raw_values_match_the_chain_model(ctx, dim):
    assert w.raw_topk_checks(ctx, False, dims=(dim,)) == 4


@pytest.mark.parametrize("dtype", (cm.F32, cm.F16))
@pytest.mark.parametrize("dim", (256, 1536, 1600))
def test_adversarial_sets_get_the_oracles_answer(ctx, oracle, dtype, dim):
    for nq in (10, 25, 50):     # (25 and 50 queries on one list: the 64-query kernel, its four-chain and quarter forms)
        wide = w.is_wide(nq, WIDE)
        s = cm.band_set(w.scan_form(nq, wide), dtype, dim, chain=cm.scan_chain_length(dim, dtype, wide))
        w.answer_scan(ctx, oracle, s, nq)
    s = cm.band_set("scan32", dtype, dim, chain=cm.scan_chain_length(dim, dtype, False))
    w.answer_rank(ctx, oracle, s)
    w.answer_topk(ctx, oracle, s, 64)
    w.answer_topk(ctx, oracle, cm.band_set("dense", dtype, dim, chain=cm.dense_chain_length(dim, dtype)), 128)


def test_statistical_bound_is_run_and_the_default_is_deterministic(oracle):
    """8192 dimensions, where the statistical band (32 sqrt(d) u |q||x|) is narrower than the deterministic one
    ((d / 2 + 8) u |q||x|; below ~4100-d it is the wider of the two and loses nothing): the set's last candidate lies
    beyond twice the statistical eps, so that bound does not flag the query and loses the true neighbour -- checked on
    the model first.  A context of its own, set_bound never called on it: the DEFAULT bound returns the oracle's ids
    and flags the query, which the statistical one cannot.  Then the statistical bound is run on the same context;
    nothing is asserted about its answer."""
    dim = 8192
    s = cm.band_set("scan16", cm.F32, dim, chain=cm.scan_chain_length(dim, cm.F32, False))
    m = s.margins()
    qn, rn = cm.row_norms(s.query[None, :])[0], cm.row_norms(s.rows).max()
    assert m["last_candidate"] * m["eps"] > 2.02 * float(cm.stat_eps(dim, cm.F32, qn, rn)), m
    fresh = w._api().Context(0)
    try:
        st = w.answer_scan(fresh, oracle, s, 10, worst_case=None)           # (None: set_bound is not called)
        assert st["scan_widened_queries"] + st["scan_redo_queries"] >= 1, st
        st = w.answer_scan(fresh, oracle, s, 10, worst_case=False)
        print("statistical bound: widened %d, redo %d" % (st["scan_widened_queries"], st["scan_redo_queries"]))
    finally:
        fresh.close()


@pytest.mark.parametrize("dtype", (cm.F32, cm.F16))
@pytest.mark.parametrize("dim", (256, 1536, 1600))
def test_swamped_centers_get_the_oracles_assignment(ctx, oracle, dtype, dim):
    """the rounding attack on the ONE-chain kernel (mfma_argmin_kernel, 96 centers x 256 rows): the true center's value
    pushed up, three decoys' pushed down, by a third of the band's term each -- all the model allows
    (chain_model.argmin_reach; test_chain_model_cpu.py shows that no input defeats that band at half width).  Every row
    gets the oracle's center and is rechecked or redone."""
    w.answer_assign(ctx, oracle, dtype, dim)


SETTINGS = [("plain", {"PGV_SCAN_WIDE": "0", "PGV_SCAN_DEEP": "0"}), ("deep", {"PGV_SCAN_WIDE": "0"}),
            ("wide", {"PGV_SCAN_WIDE": "1"}), ("no-dense128", {"PGV_NO_DENSE128": "1"})]


def test_every_form_in_a_process_that_forces_it():
    """one child process per setting, each under its own time limit; the first child that fails (a wrong value, a fault,
    a time-out) ends the test: nothing more is started on the card after it.  The children also run the adversarial
    group inside an index of >= 1 GiB of rows, fp32 and fp16 (the non-temporal instantiations)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, env in SETTINGS:
        e = dict(os.environ, **env)
        for var in ("PGV_SCAN_WIDE", "PGV_SCAN_DEEP", "PGV_NO_DENSE128"):
            if var not in env:
                e.pop(var, None)
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "mp_scan_band_worker.py")], capture_output=True,
                           text=True, timeout=420, env=e)
        assert r.returncode == 0 and "SCAN-BAND-OK" in r.stdout, (name, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
        print("\n".join(l for l in r.stdout.splitlines() if l.startswith(("FRACTION", "SCAN-BAND-OK"))))
