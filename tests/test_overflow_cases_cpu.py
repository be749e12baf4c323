"""tests/overflow_cases.py on the CPU: the data rule (every planted case's distances are the same bits in three orders of
summation), the model pinned to the oracle's IVFFlat search, check_head's teeth, and the HNSW models' handling of +-inf.
The device side is tests/test_gpu_overflow_order.py."""
import numpy as np
import pytest

import hnsw_tie_cases as tc
import overflow_cases as oc
from hnsw_scan_model import model_scan
from hnsw_walk_model import walk
from oracle import pyoracle as po

OPS = {oc.L2: po.OPS_L2, oc.NEG_IP: po.OPS_IP, oc.L1: po.OPS_L1}


def order_free(metric, queries, rows, what):
    """the precondition: forward, reversed and pairwise fp32 sums give identical bits, and so do chains of fused
    multiply-adds in both directions -- except on the ambiguous pairs (unfused NaN), where every order gives NaN, +inf or
    -inf and the fused chains, which cannot produce NaN, give one infinity each way -> the forward table"""
    f = oc.distances(metric, queries, rows, "forward")
    amb = oc.ambiguous(f)
    assert metric == oc.NEG_IP or not amb.any(), what
    for order in oc.ORDERS[1:]:
        o = oc.distances(metric, queries, rows, order)
        if order.startswith("fused"):
            assert np.isinf(o[amb]).all(), (what, order, "a fused chain gave NaN")
            o = np.where(amb, f, o)
        assert np.array_equal(oc.bits(f), oc.bits(o)), (what, order, np.argwhere(oc.bits(f) != oc.bits(o))[:5].tolist())
    if amb.any():    # the two directions of the chain disagree: the first infinity wins
        a, b = oc.distances(metric, queries, rows, "fused")[amb], oc.distances(metric, queries, rows, "fused_reversed")[amb]
        assert (a == -b).all(), what
    fin = f[np.isfinite(f)]
    big = float(oc.huge_of(metric))
    small = np.abs(fin) < 2 ** 24
    assert (fin[small] == np.round(fin[small])).all(), what
    # what is finite and not a small integer is an L1 distance over one huge coordinate: exactly HUGE_L1 (the small terms
    # vanish below its ulp)
    assert metric == oc.L1 or small.all(), (what, fin[~small][:5])
    assert (np.abs(fin[~small]) == big).all(), (what, fin[~small][:5])
    return f


# ------------------------------------------------------------------------------------------------------- the data rule
@pytest.mark.parametrize("mix", sorted(oc.ivf_mixes()))
def test_ivf_cases_are_order_free_and_hold_what_they_claim(mix):
    metric, which, _ = oc.ivf_mixes()[mix]
    case = oc.ivf_case(metric)
    q = oc.ivf_queries(case, which)
    d = order_free(metric, q, case["rows"], "ivf %s rows" % mix)
    order_free(metric, q, case["centers"], "ivf %s centers" % mix)
    cl = oc.classes(d)
    if mix in ("a", "b"):
        assert cl["pinf"] == 128 * (3 * len(oc.PLANTED_LISTS) + 2 * len(oc.HUGE_LISTS)) and cl["nan"] == cl["ninf"] == 0
    elif mix == "c":
        assert cl["pinf"] > 0 and cl["ninf"] > 0 and cl["nan"] > 0
    else:
        assert cl["finite"] == 128 * (3 * len(oc.PLANTED_LISTS) + 2 * len(oc.HUGE_LISTS)) and cl["nan"] == 0
    # the heads cross finite -> +inf (-> NaN) -> padding inside k = 10 for some query of every shape
    for nq, probes, k in oc.SHAPES:
        lists, _ = oc.ivf_probes(case, q[:nq], probes)
        crossing = all_classes = 0
        for i in range(nq):
            slots, cd = oc.ivf_candidates(case, lists[i], d[i])
            head = oc.expected_head(cd, k)[1]
            crossing += len(slots) < k and np.isfinite(head).any() and np.isposinf(head).any()
            all_classes += len(slots) < k and all(v > 0 for v in oc.classes(head).values())
        if k == 10 and mix != "d":
            assert crossing > 0, (mix, nq, probes, k)
        if mix == "d":     # the k-th key is not finite for every query: at most 8 finite rows among the probed ones
            for i in range(nq):
                slots, cd = oc.ivf_candidates(case, lists[i], d[i])
                assert np.isfinite(cd).sum() <= 8 < k and len(slots) > k, (mix, nq, probes, i)
        elif mix == "c" and k == 10:   # -inf, finite, +inf, NaN and padding in one head
            assert all_classes > 0, (mix, nq, probes, k)


@pytest.mark.parametrize("huge_queries", (False, True))
@pytest.mark.parametrize("m", oc.SEL_M)
def test_selection_cases_are_order_free(m, huge_queries):
    case = oc.selection_case(m, huge_queries)
    d = order_free(oc.L2, case["queries"], case["rows"], "selection %d" % m)
    assert (np.isfinite(d).sum(1) == oc.SEL_FINITE).all() and (np.isposinf(d).sum(1) == m - oc.SEL_FINITE).all()


@pytest.mark.parametrize("metric", (oc.L2, oc.NEG_IP))
def test_rank_cases_are_order_free(metric):
    case = oc.rank_case(metric)
    d = order_free(metric, case["huge_first"], case["centers"], "rank")
    huge = np.arange(128) % 7 == 0
    if metric == oc.L2:
        assert (np.isposinf(d[~huge]).sum(1) == 6).all() and (np.isfinite(d[huge]).sum(1) == 4).all()
    else:
        assert np.isfinite(d[~huge]).all()
        assert (np.isneginf(d[huge]).sum(1) == 33).all() and (np.isposinf(d[huge]).sum(1) == 33).all()
    assert not np.isnan(d).any()


@pytest.mark.parametrize("metric", (oc.L2, oc.NEG_IP, oc.L1))
def test_exact_rerank_and_sparse_cases_are_order_free(metric):
    seen = dict(ninf=0, finite=0, pinf=0, nan=0)
    for nq in oc.EXACT_NQ:
        for n in oc.EXACT_N:
            for hq in (False, True):
                queries, rows = oc.exact_case(metric, nq, n, hq)
                cl = oc.classes(order_free(metric, queries, rows, ("exact", nq, n, hq)))
                seen = {c: seen[c] + cl[c] for c in seen}
                assert cl["pinf"] > 0 or (metric != oc.L2 and not hq), (metric, nq, n, hq)
    queries, rows, cand = oc.rerank_case(metric)
    d = order_free(metric, queries, rows, "rerank")
    for q in range(oc.RERANK_NQ):
        real = cand[q][cand[q] >= 0]
        assert len(set(real.tolist())) == len(real)
        cl = oc.classes(d[q][real])
        assert cl["pinf"] > 0, (metric, q)
        assert metric != oc.NEG_IP or cl["ninf"] > 0
        assert metric != oc.NEG_IP or q % 2 == 0 or cl["nan"] > 0
    assert cand[1, 0] == -1 and not np.isfinite(d[2][cand[2][cand[2] >= 0]]).any() and (cand[3] >= 0).all()
    assert cand[0, 1] == -1 and np.isposinf(d[0][cand[0, 5]]) or metric == oc.NEG_IP
    for nq in (1, 40):
        _, _, dq, dr = oc.sparse_case(metric, nq)
        cl = oc.classes(order_free(metric, dq, dr, ("sparse", nq)))
        seen = {c: seen[c] + cl[c] for c in seen}
        assert cl["pinf"] > 0
    assert seen["finite"] > 0 and seen["pinf"] > 0
    assert (seen["ninf"] > 0 and seen["nan"] > 0) == (metric == oc.NEG_IP)


def test_sparse_csr_is_its_dense_twin():
    for metric in (oc.L2, oc.NEG_IP, oc.L1):
        (qp, qi, qv), (rp, ri, rv), dq, dr = oc.sparse_case(metric, 40)
        assert qi.max(initial=0) < oc.SPARSE_DIM and ri.max() == oc.SPARSE_DIM - 1 and np.diff(rp).max() <= 8
        for ptr, idx, val, dense in ((qp, qi, qv, dq), (rp, ri, rv, dr)):
            assert len(ptr) == len(dense) + 1 and ptr[-1] == len(idx) == len(val) == np.count_nonzero(dense)
            for v in range(len(dense)):
                assert (np.diff(idx[ptr[v]:ptr[v + 1]]) > 0).all()
                assert np.array_equal(val[ptr[v]:ptr[v + 1]], dense[v][dense[v] != 0])


# ------------------------------------------------------------------------------------------- the model and the oracle
@pytest.mark.parametrize("mix", sorted(oc.ivf_mixes()))
def test_model_is_the_oracles_search(oracle, mix):
    """GetScanLists and the sorted stream of the reference's scan (oracle/oracle_ivf.c) against expected_head: lists
    element for element (its heap's strict `<` keeps the lower id), the stream as tie-class sets with equal bits"""
    metric, which, _ = oc.ivf_mixes()[mix]
    case = oc.ivf_case(metric)
    q = oc.ivf_queries(case, which)
    ix = oracle.index_struct(OPS[metric], po.ORA_F32, case["centers"], case["offsets"], case["rows"], case["tids"])
    slot_of = {int(t): s for s, t in enumerate(case["tids"])}
    d = oc.distances(metric, q, case["rows"])
    for nq, probes, k in oc.SHAPES:
        lists, dc = oc.ivf_probes(case, q[:nq], probes)
        for i in sorted({0, nq // 2, nq - 1}):
            what = (mix, nq, probes, k, i)
            wl, wld = oracle.get_scan_lists(ix, q[i], probes)
            assert wl.tolist() == lists[i].tolist(), what
            assert np.array_equal(oc.bits(wld.astype(np.float32)), oc.bits(dc[i][lists[i]])), what
            wt, wd = oracle.search(ix, q[i], probes, k)
            slots, cd = oc.ivf_candidates(case, lists[i], d[i])
            assert len(wt) == min(k, len(slots)), what     # the reference returns every probed row before it runs out
            gd, gi = oc.pad_stream(wd.astype(np.float32), [slot_of[int(t)] for t in wt], k)
            oc.check_head(gd, gi, slots, cd, k, False, what)


def test_model_orders_like_float8():
    d = np.array([np.nan, np.inf, 3, -np.inf, np.inf, -0.0, 0.0, np.nan, -5], dtype=np.float32)
    order, head = oc.expected_head(d, 9)
    assert order.tolist() == [3, 8, 5, 6, 2, 1, 4, 0, 7]
    assert oc.expected_head(d, 3)[0].tolist() == [3, 8, 5]
    assert np.array_equal(oc.bits(head[:2]), oc.bits(np.array([-np.inf, -5], np.float32)))


# ---------------------------------------------------------------------------------------------------- check_head's teeth
def _good():
    cand_ids = np.array([40, 41, 42, 43, 44, 45, 46], dtype=np.int64)
    cand_dist = np.array([np.inf, 2, np.nan, np.inf, 1, np.nan, 2], dtype=np.float32)
    k = 9
    order, head = oc.expected_head(cand_dist, k)
    gd, gi = oc.pad_stream(head, cand_ids[order], k)
    return gd, gi, cand_ids, cand_dist, k


def test_check_head_accepts_the_models_answer_and_a_permuted_tie_class():
    gd, gi, ids, dist, k = _good()
    assert gi.tolist() == [44, 41, 46, 40, 43, 42, 45, -1, -1]
    oc.check_head(gd, gi, ids, dist, k, True)
    swapped = gi.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    oc.check_head(gd, swapped, ids, dist, k, False)
    with pytest.raises(AssertionError):
        oc.check_head(gd, swapped, ids, dist, k, True)
    # k inside the +inf class: either member may close the head, as a set; by position only the first
    oc.check_head(gd[:4], np.array([44, 41, 46, 43]), ids, dist, 4, False)
    with pytest.raises(AssertionError):
        oc.check_head(gd[:4], np.array([44, 41, 46, 43]), ids, dist, 4, True)


def test_check_head_rejects_real_inf_rows_reported_as_none():
    gd, gi, ids, dist, k = _good()
    gi = gi.copy()
    gi[[3, 4]] = -1          # the distances are right: +inf looks like padding
    with pytest.raises(AssertionError, match="none"):
        oc.check_head(gd, gi, ids, dist, k, False)


def test_check_head_rejects_nan_before_inf():
    gd, gi, ids, dist, k = _good()
    gd, gi = gd.copy(), gi.copy()
    gd[[3, 4, 5, 6]] = gd[[5, 6, 3, 4]]
    gi[[3, 4, 5, 6]] = gi[[5, 6, 3, 4]]
    with pytest.raises(AssertionError, match="distances"):
        oc.check_head(gd, gi, ids, dist, k, False)


def test_check_head_rejects_a_none_ahead_of_a_real_row():
    gd, gi, ids, dist, k = _good()
    # what a selection by (value, position) gives when a "none" at +inf sits in front of the real +inf rows and of NaN
    gd2 = np.array([1, 2, 2, np.inf, np.inf, np.inf, np.nan, np.nan, np.inf], dtype=np.float32)
    gi2 = np.array([44, 41, 46, -1, 40, 43, 42, 45, -1], dtype=np.int64)
    with pytest.raises(AssertionError):
        oc.check_head(gd2, gi2, ids, dist, k, False)
    # ... and with k below the real rows: the last real +inf row pushed out by the "none"
    with pytest.raises(AssertionError, match="none"):
        oc.check_head(gd2[:5], np.array([44, 41, 46, -1, 40]), ids, dist, 5, False)
    # a row twice, a foreign row, a row under another's distance
    for bad in ([44, 41, 41, 40, 43, 42, 45, -1, -1], [44, 41, 46, 40, 99, 42, 45, -1, -1],
                [41, 44, 46, 40, 43, 42, 45, -1, -1]):
        with pytest.raises(AssertionError):
            oc.check_head(gd, np.array(bad), ids, dist, k, False)
    # negative padding
    neg = gd.copy()
    neg[-1] = -np.inf
    with pytest.raises(AssertionError, match="padding"):
        oc.check_head(neg, gi, ids, dist, k, False)


# ------------------------------------------------------------------------------------------------------- HNSW models
def test_hnsw_models_order_inf_as_the_references_comparisons_do():
    """hnsw_walk_model / hnsw_scan_model compare Python floats with `<`, `>`, `==` and sorted(): +inf == +inf is a tie
    (`eDistance < f->distance` is false: not admitted into a full W), -inf < finite < +inf.  A planted check: a chain
    e0(+inf) -> a(+inf), b(+inf), c(5) with ef 2 keeps c and one +inf, and the +inf pushed out at W's furthest distance
    is still expanded (d(-inf) behind it is found)"""
    inf = float("inf")
    e0, a, b, c, d = range(5)
    levels, start, nbr = __import__("hnsw_walk_model").tuples(2, [0] * 5, {(e0, 0): [a, b, c], (b, 0): [d], (a, 0): [d]})
    dist = [inf, inf, inf, 5.0, -inf]
    w = walk(dist.__getitem__, levels, start, nbr, 2, 0, 2, tie_cap=2)
    assert w.ids == [d, c] and w.dist == [-inf, 5.0] and w.scored == 5 and w.counters["lost"] == 0
    ms = model_scan(dist.__getitem__, levels, start, nbr, 2, 0, 2)
    ids, ds, tuples = ms.next()
    assert ids == [d, c] and tuples == 5 and sorted(ms.pool) == [(inf, e0), (inf, a), (inf, b)]
    assert ms.next()[0] == [a, b] and ms.pool == [(inf, e0)]     # the pool comes back in (distance, pool position) order


@pytest.mark.parametrize("form", oc.HNSW_FORMS)
def test_hnsw_overflow_cases(oracle, form):
    """the data rule on the planted elements, what the cases claim, and lost == 0 for every walk the device test compares"""
    elements, queries, ex = tc.random_graph(oracle, form)[:3]
    e, q, planted = oc.hnsw_overflow(form, elements, queries)
    metric = oc.HNSW_METRIC[form]
    d = order_free(metric, q, e, "hnsw " + form)
    assert not np.isnan(d).any() and len(planted) >= 30
    huge = np.arange(tc.NQ) % 6 == 0
    assert huge.sum() == 8
    other = np.setdiff1d(np.arange(len(e)), planted)
    if form == "l2":
        assert np.isposinf(d[~huge][:, planted]).all() and np.isfinite(d[~huge][:, other]).all()
        assert np.isposinf(d[huge][:, other]).all() and np.isfinite(d[huge][:, planted]).all()
    elif form == "l1":
        assert np.isfinite(d[~huge]).all()
        assert np.isposinf(d[huge][:, planted[1::2]]).all() and np.isfinite(d[huge][:, planted[0::2]]).all()
    else:
        assert np.isfinite(d[~huge]).all() and np.isfinite(d[huge][:, other]).all()
        assert np.isneginf(d[huge][:, planted[0::2]]).all() and np.isposinf(d[huge][:, planted[1::2]]).all()
    for qi in range(tc.NQ):
        dq = d[qi].tolist()
        for ef in tc.EFS:
            w = walk(dq.__getitem__, ex["levels"], ex["nbr_start"], ex["nbr"], 8, ex["entry"], ef, tie_cap=ef)
            assert w.counters["lost"] == 0, (form, qi, ef)
            assert w.dist == sorted(w.dist)
