"""Where overflowed distances sort in every top-k path of the device: a real row whose distance is +inf, -inf or NaN is a
row like any other (float8 order: -inf < finite < +inf < NaN) and comes out before anything that is only padding.  Inputs,
model and the one comparison function (check_head) are tests/overflow_cases.py's; tests/test_overflow_cases_cpu.py proves
that every distance here is the same bits in any order of summation, that the model is the oracle's, and that check_head
rejects the wrong answers this file is about.  Every comparison below is equality of bits or of sets.  The one value
that is NOT a fact is the NEG_IP NaN: a chain of fused multiply-adds gives +inf or -inf where separate partial sums give
NaN (overflow_cases' docstring), the vector-ALU kernels and the matrix-core kernels differ on it as the reference's own
builds do, and check_head takes the entry's own choice among the three for such a row before it compares.

  1  pgv_search_batch == pgv_rank_lists + pgv_scan_batch, pgv_scan_lists, over the route table of
     tests/test_gpu_scan_path_edges.py on four cases (L2 with / without the fp16 row shadow, NEG_IP with -inf / +inf / NaN,
     L2 with huge queries: the k-th key is never finite); the three topk_kernel classes with 5 finite values, and the
     same lists through pgv_query_scan
  2  pgv_rank_lists / pgv_query_rank over centers that overflow
  3  pgv_exact_topk   4  pgv_rerank   5  pgv_sparse_topk
  6  pgv_hnsw_search, pgv_hnsw_scan_* and the filtered scan over fp32 elements with overflow planted under an old graph

Shapes the rule cannot reach (see overflow_cases' docstring): an inner product overflows only for a huge query, so NEG_IP
has no "ordinary query against an overflowing center / row" class; L1 needs 3e38 instead of 3e19 to overflow at all."""
import numpy as np
import pytest

import hnsw_tie_cases as tc
import overflow_cases as oc
from hnsw_scan_model import model_scan
from hnsw_walk_model import walk
from oracle import pyoracle as po
from pgvector_amd import api

pytestmark = pytest.mark.gpu

METRIC = {oc.L2: api.PGV_L2SQ, oc.NEG_IP: api.PGV_NEG_IP, oc.L1: api.PGV_L1}
OPS = {oc.L2: po.OPS_L2, oc.NEG_IP: po.OPS_IP, oc.L1: po.OPS_L1}
NONE_TID = np.uint64(0xffffffffffffffff)


def host(x):
    return x.copy() if isinstance(x, np.ndarray) else x.cpu().numpy()


def index_of(ctx, case):
    return api.IvfIndex(ctx, METRIC[case["metric"]], api.PGV_F32, case["centers"].shape[1], case["centers"], case["offsets"],
                        case["rows"], case["tids"])


# ------------------------------------------------------------------------------------------------ 1. IVFFlat batches
class Mix:
    def __init__(self, ctx, oracle, name):
        self.metric, which, self.shadow = oc.ivf_mixes()[name]
        self.case = oc.ivf_case(self.metric)
        self.queries = oc.ivf_queries(self.case, which)
        self.dist = oc.distances(self.metric, self.queries, self.case["rows"])     # computed once, never changed
        self.dist.setflags(write=False)
        with pytest.MonkeyPatch.context() as mp:
            self.env(mp)
            self.ix = index_of(ctx, self.case)
        self.struct = oracle.index_struct(OPS[self.metric], po.ORA_F32, self.case["centers"], self.case["offsets"],
                                          self.case["rows"], self.case["tids"])

    def env(self, mp):
        mp.setenv("PGV_SCAN_SHADOW", self.shadow)
        mp.delenv("PGV_RANK_SHADOW", raising=False)


@pytest.fixture(scope="module")
def mixes(ctx, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Mix(ctx, oracle, name)
        return made[name]
    yield get
    for m in made.values():
        m.ix.close()


@pytest.mark.parametrize("nq,probes,k", oc.SHAPES, ids=["nq%d-p%d-k%d" % s for s in oc.SHAPES])
@pytest.mark.parametrize("mix", sorted(oc.ivf_mixes()))
def test_ivf_batch_heads(ctx, oracle, monkeypatch, mixes, mix, nq, probes, k):
    m = mixes(mix)
    m.env(monkeypatch)
    case, q = m.case, m.queries[:nq]
    what = "mix %s nq %d probes %d k %d" % (mix, nq, probes, k)
    d, s, t = (host(a) for a in m.ix.search_batch(q, probes, k, want_tid=True))
    lists, ld = m.ix.rank_lists(q, probes)
    lists, ld = host(lists), host(ld)
    d2, s2, t2 = (host(a) for a in m.ix.scan_batch(q, lists, k, want_tid=True))
    ctx.sync()
    np.testing.assert_array_equal(d.view(np.uint32), d2.view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(s, s2, err_msg=what)
    np.testing.assert_array_equal(t, t2, err_msg=what)
    want_lists, dc = oc.ivf_probes(case, q, probes)
    np.testing.assert_array_equal(lists, want_lists, err_msg=what + " lists")
    np.testing.assert_array_equal(oc.bits(ld), oc.bits(np.take_along_axis(dc, want_lists.astype(np.int64), 1)), err_msg=what)
    for i in range(nq):
        slots, cd = oc.ivf_candidates(case, want_lists[i], m.dist[i])
        oc.check_head(d[i], s[i], slots, cd, k, False, "%s q%d" % (what, i))
        n = min(k, len(slots))
        assert np.array_equal(t[i][:n], case["tids"][s[i][:n]]) and (t[i][n:] == NONE_TID).all(), (what, i, "tids")
    for i in sorted({0, nq // 2, nq - 1}):
        wt, wd = oracle.search(m.struct, q[i], probes, k)
        n = len(wt)
        assert n == min(k, sum(case["offsets"][l + 1] - case["offsets"][l] for l in want_lists[i])), (what, i)
        gb = oc.bits(d[i][:n])
        if not oc.ambiguous(m.dist[i][s[i][:n]]).any():      # (the oracle's value of such a row is one of three as well)
            assert np.array_equal(gb, oc.bits(wd.astype(np.float32))), (what, i, "oracle distances")
            for b in np.unique(gb[gb != gb[-1]] if n == k else gb):      # every class the head holds whole: the oracle's rows
                assert set(t[i][:n][gb == b].tolist()) == set(wt[gb == b].tolist()), (what, i, "oracle rows at", hex(int(b)))
        # pgv_scan_lists: every probed row of the query with its distance, nothing dropped
        sd, ss = m.ix.scan_lists(q[i], want_lists[i])
        slots, cd = oc.ivf_candidates(case, want_lists[i], m.dist[i])
        order = np.argsort(ss, kind="stable")
        assert np.array_equal(np.sort(slots), ss[order]), (what, i, "scan_lists rows")
        want = oc.settle_ambiguous(sd[order], ss[order], ss[order], m.dist[i][ss[order]], what)
        assert np.array_equal(oc.bits(sd[order]), oc.bits(want)), (what, i, "scan_lists distances")


@pytest.mark.parametrize("huge_queries", (False, True), ids=("huge-rows", "huge-queries"))
@pytest.mark.parametrize("m", oc.SEL_M)
def test_selection_classes_with_five_finite_values(ctx, m, huge_queries):
    """one probed list of 1000 / 4000 / 20 000 rows (the small / medium / long topk_kernel class) of which five are
    finite, 40 queries, k below, at and above five: the register-resident forms' threshold is not finite above five and
    they must fall back; the same list through the single-query head (position order: element for element)"""
    case = oc.selection_case(m, huge_queries)
    dist = oc.distances(oc.L2, case["queries"], case["rows"])
    ix = index_of(ctx, case)
    slots = np.arange(m)
    for k in oc.SEL_K:
        d, s, _ = ix.search_batch(case["queries"], 1, k)
        d, s = host(d), host(s)
        for i in range(oc.SEL_NQ):
            oc.check_head(d[i], s[i], slots, dist[i], k, False, "m %d k %d q%d" % (m, k, i))
    qh = api.Query(ix)
    for i in (0, oc.SEL_NQ // 2, oc.SEL_NQ - 1):
        qh.rank(case["queries"][i], 1)
        assert qh.lists(1).tolist() == [0]
        for k in oc.SEL_K:
            d, s, t, total = qh.scan(0, 1, k)
            assert total == m and len(s) == k
            oc.check_head(d, s, slots, dist[i], k, True, "single query m %d k %d q%d" % (m, k, i))
            assert np.array_equal(t, case["tids"][s])
    qh.close()
    ix.close()


# ------------------------------------------------------------------------------------------------ 2. center ranking
@pytest.mark.parametrize("rank_shadow", ("1", "0"))
@pytest.mark.parametrize("metric", (oc.L2, oc.NEG_IP))
def test_rank_lists_over_overflowing_centers(ctx, monkeypatch, metric, rank_shadow):
    """lists AND distances element for element: the lower list id wins a tie (GetScanLists' strict `<`), +inf centers come
    after every finite one and before nothing -- with maxprobes = 64 and 70 a huge query's list is mostly +inf"""
    monkeypatch.setenv("PGV_SCAN_SHADOW", "1")      # (an index this small carries the fp16 center shadow only when asked)
    monkeypatch.setenv("PGV_RANK_SHADOW", rank_shadow)
    case = oc.rank_case(metric)
    ix = index_of(ctx, case)
    qh = api.Query(ix)
    for pool in ("huge_first", "ordinary_first"):
        queries = case[pool]
        dc = oc.distances(metric, queries, case["centers"])
        for nq in oc.RANK_NQ:
            for maxprobes in oc.RANK_MAXPROBES:
                what = "metric %d shadow %s %s nq %d maxprobes %d" % (metric, rank_shadow, pool, nq, maxprobes)
                lists, dist = ix.rank_lists(queries[:nq], maxprobes)
                lists, dist = host(lists), host(dist)
                for i in range(nq):
                    oc.check_head(dist[i], lists[i], np.arange(oc.RANK_NLISTS), dc[i], maxprobes, True, "%s q%d" % (what, i))
        for i in (0, 1, 7):      # the single-query entry
            for maxprobes in oc.RANK_MAXPROBES:
                qh.rank(queries[i], maxprobes)
                want = oc.expected_head(dc[i], maxprobes)[0]
                assert qh.lists(maxprobes).tolist() == want.tolist(), (metric, pool, i, maxprobes)
    qh.close()
    ix.close()


# --------------------------------------------------------------------------------------------------- 3. pgv_exact_topk
@pytest.mark.parametrize("n", oc.EXACT_N)
@pytest.mark.parametrize("nq", oc.EXACT_NQ)
@pytest.mark.parametrize("metric", (oc.L2, oc.NEG_IP, oc.L1))
def test_exact_topk(ctx, metric, nq, n):
    """3 / 64 / 128 queries (vector ALUs, the 32-query matrix-core scan, the dense 128 form) against 63 / 64 / 200 rows
    (either side of n >= 64), k = 10, n, n + 5, ordinary and huge queries, host and device buffers: ties by lower row"""
    import torch
    for hq in (False, True):
        queries, rows = oc.exact_case(metric, nq, n, hq)
        dist = oc.distances(metric, queries, rows)
        for k in (10, n, n + 5):
            for where in ("host", "device"):
                a, b = (queries, rows) if where == "host" else (torch.from_numpy(queries).cuda(), torch.from_numpy(rows).cuda())
                d, idx = api.exact_topk(ctx, METRIC[metric], api.PGV_F32, oc.EXACT_DIM, a, b, k)
                d, idx = host(d), host(idx)
                for i in range(nq):
                    oc.check_head(d[i], idx[i], np.arange(n), dist[i], k, True,
                                  "metric %d nq %d n %d huge %s k %d %s q%d" % (metric, nq, n, hq, k, where, i))


# ------------------------------------------------------------------------------------------------------- 4. pgv_rerank
@pytest.mark.parametrize("metric", (oc.L2, oc.NEG_IP, oc.L1))
def test_rerank_puts_every_real_candidate_before_any_none(ctx, metric):
    """the contract of include/pgv_hip.h: every real candidate in float8 order, ties by lower candidate position, before
    any -1; -1 only pads.  k = 1, each query's number of real candidates, kc.
    (Before the fix a "none" took part in the selection at +inf and won its ties by position: under L2 and L1, query 2 --
    cand [-1, 3, -1, 4, ..], every real candidate at +inf -- with k = 1 came back as +inf / -1, no row at all.)"""
    queries, rows, cand = oc.rerank_case(metric)
    dist = oc.distances(metric, queries, rows)
    real = [cand[q][cand[q] >= 0] for q in range(oc.RERANK_NQ)]
    ks = sorted({1, oc.RERANK_KC} | {len(r) for r in real})
    assert len(ks) >= 4
    for k in ks:
        d, idx = api.rerank(ctx, METRIC[metric], api.PGV_F32, oc.RERANK_DIM, queries, rows, cand, k)
        d, idx = host(d), host(idx)
        print("metric", metric, "k", k, "q0", d[0].tolist(), idx[0].tolist())
        for q in range(oc.RERANK_NQ):
            oc.check_head(d[q], idx[q], real[q], dist[q][real[q]], k, True, "metric %d k %d q%d" % (metric, k, q))


# -------------------------------------------------------------------------------------------------- 5. pgv_sparse_topk
@pytest.mark.parametrize("nq", (1, 40))
@pytest.mark.parametrize("metric", (oc.L2, oc.NEG_IP, oc.L1))
def test_sparse_topk(ctx, metric, nq):
    queries, rows, dq, dr = oc.sparse_case(metric, nq)
    dist = oc.distances(metric, dq, dr)
    for k in (10, oc.SPARSE_N + 5):
        d, idx = api.sparse_topk(ctx, METRIC[metric], oc.SPARSE_DIM, queries, rows, k)
        d, idx = host(d), host(idx)
        for i in range(nq):
            oc.check_head(d[i], idx[i], np.arange(oc.SPARSE_N), dist[i], k, True, "metric %d nq %d k %d q%d" % (metric, nq, k, i))


# ------------------------------------------------------------------------------------------------------------- 6. HNSW
_hnsw = {}
SCAN_QUERIES = np.arange(0, tc.NQ, 3)      # 16 queries, 8 of them huge


def hnsw_case(ctx, oracle, form):
    """the oracle's graph over tie_cases' elements, then overflow planted in the rows: modified rows under the OLD graph"""
    if form not in _hnsw:
        elements, queries, ex = tc.random_graph(oracle, form)[:3]
        e, q, planted = oc.hnsw_overflow(form, elements, queries)
        metric = oc.HNSW_METRIC[form]
        graph = (8, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"])
        h = api.Hnsw(ctx, METRIC[metric], api.PGV_F32, tc.RDIM, e)
        h.set_graph(*graph)
        d = oc.distances(metric, q, e)
        n = len(e)
        got = np.asarray(h.score(q, np.tile(np.arange(n, dtype=np.int32), tc.NQ), np.repeat(np.arange(tc.NQ, dtype=np.int32), n)))
        assert not oc.ambiguous(d).any()
        assert np.array_equal(oc.bits(got.reshape(tc.NQ, n)), oc.bits(d)), (form, "pgv_hnsw_score")
        _hnsw[form] = h, q, graph, d, planted
    return _hnsw[form]


def fbits(x):
    return oc.bits(np.asarray(x, dtype=np.float32)).tolist()


@pytest.mark.parametrize("form", oc.HNSW_FORMS)
def test_hnsw_walk_on_ties_at_inf(ctx, oracle, form):
    """element order, distance bits and scored of hnsw_walk_model.walk (T of ef entries, nothing lost)"""
    h, q, graph, d, _ = hnsw_case(ctx, oracle, form)
    m, entry, levels, start, nbr = graph
    runs = {}
    for ef, k in tc.ef_k():
        elem, dist, scored = h.search(q, ef, k)
        for qi in range(tc.NQ):
            if (qi, ef) not in runs:
                runs[qi, ef] = walk(d[qi].tolist().__getitem__, levels, start, nbr, m, entry, ef, tie_cap=ef)
                assert runs[qi, ef].counters["lost"] == 0
            w = runs[qi, ef]
            n = min(k, len(w.ids))
            what = (form, ef, k, qi)
            assert elem[qi].tolist() == w.ids[:n] + [-1] * (k - n), (what, "elements")
            assert fbits(dist[qi]) == fbits(w.dist[:n] + [np.inf] * (k - n)), (what, "distances")
            assert int(scored[qi]) == w.scored, (what, "scored")


def device_stream(scan):
    """every batch of every query until all are exhausted -> per query [(ids, distance bits, scored)]"""
    out = [[] for _ in range(scan.nq)]
    live = np.ones(scan.nq, dtype=bool)
    for _ in range(100000):
        if not live.any():
            return out
        e, d, c, s, left = scan.next(None if live.all() else live.copy())
        for qi in np.flatnonzero(live):
            n = int(c[qi])
            assert (e[qi, n:] == -1).all() and (oc.bits(d[qi, n:]) == oc.PINF_BITS).all()
            if n == 0:
                live[qi] = False
            else:
                out[qi].append((e[qi, :n].tolist(), fbits(d[qi, :n]), int(s[qi])))
    raise AssertionError("the scan did not end")


@pytest.mark.parametrize("ef", (10, 40))
@pytest.mark.parametrize("form", oc.HNSW_FORMS)
def test_hnsw_scan_stream_with_inf(ctx, oracle, form, ef):
    """the whole stream to exhaustion, batch by batch, against hnsw_scan_model.model_scan"""
    h, q, graph, d, _ = hnsw_case(ctx, oracle, form)
    m, entry, levels, start, nbr = graph
    with h.scan(q[SCAN_QUERIES], ef) as s:
        got = device_stream(s)
    for j, qi in enumerate(SCAN_QUERIES):
        want = [(ids, fbits(ds), t) for ids, ds, t in model_scan(d[qi].tolist().__getitem__, levels, start, nbr, m, entry, ef).run()]
        assert got[j] == want, (form, ef, int(qi))
        assert len(want) > 1 and any(oc.PINF_BITS in b[1] for b in want) == bool(np.isposinf(d[qi]).any())


@pytest.mark.parametrize("ef", (10, 40))
@pytest.mark.parametrize("form", oc.HNSW_FORMS)
def test_hnsw_filtered_scan_keeps_only_the_overflow_elements(ctx, oracle, form, ef):
    """a bitmap that keeps exactly the planted elements: an ordinary L2 query is served by rows at +inf alone"""
    h, q, graph, d, planted = hnsw_case(ctx, oracle, form)
    m, entry, levels, start, nbr = graph
    keep = np.zeros(d.shape[1], dtype=bool)
    keep[planted] = True
    k = 10
    for strict in (False, True):
        with h.scan(q[SCAN_QUERIES], ef) as s:
            e, ds, cnt, sco, _, left = (api._host_array(x) for x in s.filtered(k, keep, 20000, strict))
        served_by_inf = 0
        for j, qi in enumerate(SCAN_QUERIES):
            ms = model_scan(d[qi].tolist().__getitem__, levels, start, nbr, m, entry, ef)
            ids, wd, t = ms.iterative_search(k, keep, max_scan_tuples=20000, strict=strict)
            n = int(cnt[j])
            what = (form, ef, strict, int(qi))
            assert (e[j, :n].tolist(), fbits(ds[j, :n]), int(sco[j]), int(left[j])) == (ids, fbits(wd), t, len(ms.pool)), what
            assert (e[j, n:] == -1).all() and (oc.bits(ds[j, n:]) == oc.PINF_BITS).all(), (what, "padding")
            served_by_inf += n > 0 and bool(np.isposinf(wd).all())
        assert served_by_inf > 0 or form != "l2"
