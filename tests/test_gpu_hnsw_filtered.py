"""pgv_hnsw_scan_filtered -- hnswgettuple's loop under a filter in one launch -- against its specification,
model_scan.iterative_search (tests/hnsw_scan_model.py), on every mirror kind: the loop over selectivities, limits and
strict_order, integer tie data, the edges of k and of the pool, the scan's state before and after the call, the forms of
`keep`, a workgroup's later queries, an empty index, the overflow of a pool and the argument errors.

As in tests/test_gpu_hnsw_scan.py the model is fed the DEVICE's distance table (pgv_hnsw_score, pgv_hnsw_score_sparse); on
a Jaccard mirror it is fed exact Fractions (tests/jaccard_model.py) as in tests/test_gpu_jaccard_hnsw.py.  Every
comparison is equality: element slots, distance bits, so->tuples, batches and the pool left.  The shapes, seeds, filters
and the named edge cases are tests/hnsw_filtered_cases.py's; tests/test_hnsw_filtered_cpu.py shows on the same seeds
that every edge case takes the branch it is named after."""

import numpy as np
import pytest

import bit_hnsw_model as bhm
import hnsw_filtered_cases as fc
import hnsw_scan_cases as sc
import hnsw_tie_cases as tc
import jaccard_model as jm
import sparse_hnsw_model as shm
from hnsw_scan_model import model_scan
from pgvector_amd import _lib, api

pytestmark = pytest.mark.gpu

METRIC = {"l2": api.PGV_L2SQ, "negip": api.PGV_NEG_IP, "l1": api.PGV_L1}
DTYPE = {"f32": api.PGV_F32, "f16": api.PGV_F16}
FORMS = ([(m, t) for m in ("l2", "negip", "l1") for t in ("f32", "f16")] + [("hamming", "bits"), ("jaccard", "bits")] +
         [(m, "sparse") for m in ("l2", "negip", "l1")])


def bits(x):
    return (np.asarray(x, dtype=np.float32) + np.float32(0)).view(np.uint32).tolist()  # (-0 has key +0)


def nq_of(queries):
    return len(queries[0]) - 1 if isinstance(queries, tuple) else len(queries)


class Case:
    """a mirror with its graph, its queries as the mirror takes them, per query what the model ranks by (`rank`: a list
    over the elements) and the float32 distances the device hands back (`dist`)"""

    def __init__(self, h, queries, graph, rank, dist):
        self.h, self.queries, self.graph, self.rank, self.dist = h, queries, graph, rank, dist
        self.n, self.nq = len(rank[0]), nq_of(queries)
        self._recorded = {}

    def scan(self, ef, discard_cap=0, queries=None):
        begin = self.h.scan_sparse if getattr(self.h, "sparse", False) else self.h.scan
        return begin(self.queries if queries is None else queries, ef, discard_cap)

    def model(self, q, ef):
        m, entry, levels, start, nbr = self.graph
        return model_scan(self.rank[q].__getitem__, levels, start, nbr, m, entry, ef)

    def recorded(self, q, ef, limit):
        key = (q, ef, limit)
        if key not in self._recorded:
            self._recorded[key] = fc.recorded(lambda: self.model(q, ef), limit)
        return self._recorded[key]

    def want(self, q, ids):
        """the distance bits the device must hand back for these elements of query q"""
        return bits(self.dist[q][ids]) if len(ids) else []


def table(h, queries, n):
    nq = nq_of(queries)
    d = h.score(queries, np.tile(np.arange(n, dtype=np.int32), nq), np.repeat(np.arange(nq, dtype=np.int32), n))
    return np.asarray(d).reshape(nq, n)


def from_table(h, queries, graph, n):
    d = table(h, queries, n)
    return Case(h, queries, graph, [d[q].tolist() for q in range(len(d))], d)


def fraction_ranks(query, rows):
    """the exact Jaccard distances of a query to the rows, each Fraction replaced by its position among the query's
    distinct Fractions: the same order and the same ties (the model only compares), without a thousand Fraction
    comparisons per batch"""
    fr = jm.fractions_of(query, rows)
    position = {f: i for i, f in enumerate(sorted(set(fr)))}
    return [position[f] for f in fr]


_cases = {}


def case(ctx, metric, kind):
    """the shape of hnsw_filtered_cases (n 600, dim 48, m 16, two upper layers, 64 queries) as each mirror kind, once per
    session"""
    key = (metric, kind)
    if key in _cases:
        return _cases[key]
    if kind in DTYPE:
        if "float" not in _cases:
            _cases["float"] = fc.float_case()
        rows, queries, graph = _cases["float"]
        c = from_table(api.Hnsw(ctx, METRIC[metric], DTYPE[kind], fc.DIM, rows), queries, graph, fc.N)
    elif kind == "bits":
        if "bits" not in _cases:
            rows, queries = bhm.rand_bits(fc.N, fc.DIM, fc.SEED + 2), bhm.rand_bits(fc.NQ, fc.DIM, fc.SEED + 3)
            _cases["bits"] = rows, queries, sc.knn_graph(bhm.expand01(rows, fc.DIM), fc.M, fc.SEED + 4, top=fc.TOP)
        rows, queries, graph = _cases["bits"]
        if metric == "hamming":
            c = from_table(api.BitHnsw(ctx, fc.DIM, rows), queries, graph, fc.N)
        else:
            c = Case(api.JaccardHnsw(ctx, fc.DIM, rows), queries, graph, [fraction_ranks(q, rows) for q in queries],
                     np.stack([jm.ref_floats(q, rows) for q in queries]))
    else:
        if "sparse" not in _cases:
            lengths = np.random.default_rng(fc.SEED + 5).integers(1, 13, fc.N).tolist()
            lengths[:3] = [0, 1, fc.DIM]  # an empty element, a single pair, a full row
            rows = shm.rand_csr(lengths, fc.SEED + 6, dim=fc.DIM, floats=True)
            queries = shm.rand_csr([0, 1, fc.DIM] + [8] * (fc.NQ - 3), fc.SEED + 7, dim=fc.DIM, floats=True)
            _cases["sparse"] = rows, queries, sc.knn_graph(shm.expand_dense(rows, fc.DIM), fc.M, fc.SEED + 8, top=fc.TOP)
        rows, queries, graph = _cases["sparse"]
        c = from_table(api.SparseHnsw(ctx, METRIC[metric], fc.DIM, rows), queries, graph, fc.N)
    c.h.set_graph(*c.graph)
    _cases[key] = c
    return c


def check_call(c, got, ef, k, keep, limit, strict, what, queries=None):
    """one filtered call on a fresh scan against the loop of the model: ids, distance bits, so->tuples, batches, left.
    keep: [n] or [nq x n] booleans.  -> the tags of the branches the queries took"""
    elem, dist, count, scored, batches, left = (api._host_array(x) for x in got)
    assert elem.shape == dist.shape == (len(count), k)
    seen = set()
    for q in (range(c.nq) if queries is None else queries):
        kq = keep if keep.ndim == 1 else keep[q]
        ids, _, tuples, nb, pool, rp = fc.run_loop(c.recorded(q, ef, limit), k, kq, strict)
        cnt = int(count[q])
        assert (elem[q, :cnt].tolist(), int(scored[q]), int(batches[q]), int(left[q])) == (ids, tuples, nb, pool), (what, q)
        assert bits(dist[q, :cnt]) == c.want(q, ids), (what, q, "distance bits")
        assert (elem[q, cnt:] == -1).all() and np.isinf(dist[q, cnt:]).all() and (dist[q, cnt:] > 0).all(), (what, q, "padding")
        if not strict:
            seen |= fc.tags(rp, ids, k, kq)
    return seen


# ------------------------------------------------------------------------------------------- 1. the loop against the model
@pytest.mark.parametrize("limit", fc.LIMITS)
@pytest.mark.parametrize("ef", fc.EFS)
@pytest.mark.parametrize("metric,kind", FORMS)
def test_loop_is_the_models(ctx, metric, kind, ef, limit):
    """every selectivity, with and without strict_order: the rows, so->tuples, the batches taken and the pool left are
    model_scan.iterative_search's, and the host loop (api.hnsw_iterative_search) over the same mirror agrees"""
    c = case(ctx, metric, kind)
    for selectivity in fc.SELECTIVITIES:
        keep = fc.keep_mask(selectivity, c.n)
        for strict in (False, True):
            what = (metric, kind, ef, limit, selectivity, strict)
            with c.scan(ef) as s:
                got = s.filtered(fc.K, keep, limit, strict)
            check_call(c, got, ef, fc.K, keep, limit, strict, what)
            elem, dist, count = got[0], got[1], got[2]
            ids, ds, scored = api.hnsw_iterative_search(c.h, c.queries, fc.K, keep, ef, max_scan_tuples=limit, strict=strict)
            for q in range(c.nq):
                assert (ids[q], bits(ds[q]), int(scored[q])) == (elem[q, :count[q]].tolist(), bits(dist[q, :count[q]]),
                                                                 int(got[3][q])), (what, q, "the host loop")
            if selectivity == 0.3 and strict:  # the Python face of the whole search: the host loop's return shape
                ids2, ds2, scored2 = api.hnsw_filtered_search(c.h, c.queries, fc.K, keep, ef, max_scan_tuples=limit, strict=True)
                assert ids2 == ids and [bits(x) for x in ds2] == [bits(x) for x in ds] and np.array_equal(scored2, scored)


# ---------------------------------------------------------------------------------------------------- 2. integer tie data
_tie = {}


def tie_case(ctx, oracle, form):
    if form not in _tie:
        elements, queries, ex, _ = tc.random_graph(oracle, form)
        graph = (8, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"])
        if form == "bits":
            h, q = api.BitHnsw(ctx, tc.NBITS, np.packbits(elements.astype(np.uint8), axis=1)), np.packbits(queries.astype(np.uint8), axis=1)
        else:
            h, q = api.Hnsw(ctx, METRIC[form], api.PGV_F32, tc.RDIM, elements), queries
        h.set_graph(*graph)
        _tie[form] = from_table(h, q[:16], graph, len(elements))
    return _tie[form]


@pytest.mark.parametrize("ef", (5, 16))
@pytest.mark.parametrize("form", tc.METRICS + ("bits",))
def test_tie_data_follows_the_models_tie_order(ctx, oracle, form, ef):
    """small-integer data, most distances shared: the rows come out in the array form's tie order ((key, pool position)),
    strict_order passes equal keys, and a drain cuts inside runs of equal keys as the model does"""
    c = tie_case(ctx, oracle, form)
    assert all(len(set(r)) < len(r) // 4 for r in c.rank)
    keep = fc.keep_mask(0.3, c.n)
    for limit in (20000, 150):
        for strict in (False, True):
            with c.scan(ef) as s:
                check_call(c, s.filtered(fc.K, keep, limit, strict), ef, fc.K, keep, limit, strict, (form, ef, limit, strict))


# --------------------------------------------------------------------------------------- 3. the edges of k and of the pool
@pytest.mark.parametrize("name", list(fc.EDGES))
def test_edges_of_k_and_of_the_pool(ctx, name):
    """k reached in the middle of a batch (the tail dropped), at the end of one, k = 1, k beyond what the filter keeps,
    the drain after one walk and after several, both ends in one call, drains from a pool below / at / above ef and above
    256 entries -- each case must take its branch on the device's own distances as well"""
    ef, k, selectivity, limit, branches = fc.EDGES[name]
    c = case(ctx, "l2", "f32")
    keep = fc.keep_mask(selectivity, c.n)
    for strict in (False, True):
        with c.scan(ef) as s:
            seen = check_call(c, s.filtered(k, keep, limit, strict), ef, k, keep, limit, strict, (name, strict))
        assert strict or branches <= seen, (name, sorted(branches - seen))


# ------------------------------------------------------------------------------------------------------------ 4. state
def one_model_per_query(c, ef, queries):
    return {q: c.model(q, ef) for q in queries}


def check_next(c, models, got, what):
    e, d, cnt, sco, left = got
    for q, ms in models.items():
        ids, _, t = ms.next()
        assert (e[q, :cnt[q]].tolist(), bits(d[q, :cnt[q]]), int(sco[q]), int(left[q])) == (ids, c.want(q, ids), t, len(ms.pool)), (what, q)


def check_filtered(c, models, got, k, keep, limit, strict, what):
    e, d, cnt, sco, _, left = got
    for q, ms in models.items():
        ids, _, t = ms.iterative_search(k, keep, max_scan_tuples=limit, strict=strict)
        assert (e[q, :cnt[q]].tolist(), bits(d[q, :cnt[q]]), int(sco[q]), int(left[q])) == (ids, c.want(q, ids), t, len(ms.pool)), (what, q)


@pytest.mark.parametrize("metric,kind", [("l2", "f32"), ("jaccard", "bits"), ("l1", "sparse")])
def test_state_carries_over_between_calls(ctx, metric, kind):
    """next, next, filtered, next -- and filtered twice in a row, the second past max_scan_tuples -- against ONE model_scan
    per query: the call starts from the scan's state and leaves the state after the last batch it took"""
    c = case(ctx, metric, kind)
    queries = range(0, c.nq, 4)
    keep = fc.keep_mask(0.05, c.n)
    models = one_model_per_query(c, 5, queries)
    with c.scan(5) as s:
        check_next(c, models, s.next(), "first")
        check_next(c, models, s.next(), "second")
        check_filtered(c, models, s.filtered(3, keep, 20000, True), 3, keep, 20000, True, "filtered")
        check_next(c, models, s.next(), "after")
        check_filtered(c, models, s.filtered(3, keep, 20000, False), 3, keep, 20000, False, "again")
        check_filtered(c, models, s.filtered(fc.K, keep, 1, False), fc.K, keep, 1, False, "past the limit")
        e, d, cnt = s.drain(7)
        for q, ms in models.items():
            ids, _ = ms.drain(7)
            assert (e[q, :cnt[q]].tolist(), bits(d[q, :cnt[q]])) == (ids, c.want(q, ids)), ("drain", q)


def test_want_leaves_the_other_queries_alone(ctx):
    c = case(ctx, "l2", "f32")
    keep = fc.keep_mask(0.3, c.n)
    want = np.arange(c.nq) % 2 == 0
    models = one_model_per_query(c, 5, range(c.nq))
    with c.scan(5) as s:
        check_next(c, models, s.next(), "first")
        e, d, cnt, sco, batches, left = s.filtered(fc.K, keep, 20000, False, want=want)
        wanted = {q: ms for q, ms in models.items() if want[q]}
        check_filtered(c, wanted, (e, d, cnt, sco, batches, left), fc.K, keep, 20000, False, "wanted")
        for q in np.flatnonzero(~want):  # padding, the current so->tuples and pool, no batch
            assert cnt[q] == 0 and (e[q] == -1).all() and np.isinf(d[q]).all() and batches[q] == 0
            assert (int(sco[q]), int(left[q])) == (models[q].tuples, len(models[q].pool))
        for step in range(3):  # the others' streams go on as the untouched model's, the wanted ones' from where the call left them
            check_next(c, models, s.next(), "after %d" % step)


# ------------------------------------------------------------------------------------------------------ 5. forms of keep
def test_keep_per_query_shared_on_the_device_and_absent(ctx):
    torch = pytest.importorskip("torch")
    c = case(ctx, "negip", "f16")
    masks = np.stack([fc.keep_mask(sel, c.n, seed) for seed, sel in enumerate((0.3, 0.05, 1.0, 0.0))])
    per_query = masks[np.arange(c.nq) % 4]
    with c.scan(5) as s:
        mixed = s.filtered(fc.K, per_query, 150, True)
    check_call(c, mixed, 5, fc.K, per_query, 150, True, "per query")
    for i in range(4):  # a query's own filter gives what the same filter shared by all gives it
        with c.scan(5) as s:
            shared = s.filtered(fc.K, masks[i], 150, True)
        for q in range(i, c.nq, 4):
            assert all(np.array_equal(a[q], b[q]) for a, b in zip(mixed, shared)), (i, q)
    # the same filters from device memory: booleans packed where they live, and words passed through; device outputs
    dev = torch.device("cuda", 0)
    for keep in (torch.from_numpy(per_query).to(dev), torch.from_numpy(api.pack_keep(per_query).view(np.int32)).to(dev)):
        with c.scan(5) as s:
            got = s.filtered(fc.K, keep, 150, True)
        assert all(np.array_equal(a, b) for a, b in zip(mixed, got))
    with c.scan(5, queries=torch.from_numpy(c.queries.astype(np.float16)).to(dev)) as s:
        got = s.filtered(fc.K, torch.from_numpy(masks[0]).to(dev), 150, True)
        assert all(x.is_cuda for x in got)
    with c.scan(5) as s:
        shared = s.filtered(fc.K, masks[0], 150, True)
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(shared, got))
    # keep = NULL keeps everything
    with c.scan(5) as s:
        none = s.filtered(fc.K, None, 150, True)
    with c.scan(5) as s:
        ones = s.filtered(fc.K, np.ones(c.n, dtype=bool), 150, True)
    assert all(np.array_equal(a, b) for a, b in zip(none, ones)) and (none[2] == fc.K).all()
    # a stride wider than the bitmap
    wide = np.zeros((c.nq, (c.n + 31) // 32 + 3), dtype=np.uint32)
    wide[:, :(c.n + 31) // 32] = api.pack_keep(per_query)
    wide[:, (c.n + 31) // 32:] = 0xffffffff
    with c.scan(5) as s:
        got = s.filtered(fc.K, torch.from_numpy(wide.view(np.int32)), 150, True)
    assert all(np.array_equal(a, b) for a, b in zip(mixed, got))
    # words in a numpy array pass through as well (they are not taken for booleans)
    with c.scan(5) as s:
        got = s.filtered(fc.K, wide, 150, True)
    assert all(np.array_equal(a, b) for a, b in zip(mixed, got))
    with c.scan(5) as s:
        got = s.filtered(fc.K, api.pack_keep(masks[0]), 150, True)
    assert all(np.array_equal(a, b) for a, b in zip(shared, got))


def test_keep_of_another_length_is_refused(ctx):
    """a filter is over the mirror's n elements: a shorter or longer boolean filter, too few words, or a per-query filter
    for another number of queries never reaches the library, which would read (n + 31) / 32 words of it"""
    torch = pytest.importorskip("torch")
    c = case(ctx, "l2", "f32")
    words = (c.n + 31) // 32
    bad = [np.ones(c.n - 1, dtype=bool), np.ones(c.n + 1, dtype=bool), np.ones((c.nq, c.n - 32), dtype=bool),
           np.ones((c.nq + 1, c.n), dtype=bool), np.zeros(words - 1, dtype=np.uint32), np.zeros((c.nq, words - 1), dtype=np.uint32),
           torch.zeros(words - 1, dtype=torch.int32), torch.ones(c.n - 1, dtype=torch.bool), np.ones((2, c.nq, c.n), dtype=bool)]
    with c.scan(5) as s:
        for keep in bad:
            with pytest.raises(api.PgvError) as err:
                s.filtered(fc.K, keep)
            assert err.value.code == _lib.PGV_ERR_ARG and "keep" in err.value.message
        first = s.next()  # nothing above touched the scan
    plain = c.h.search(c.queries, 5, 5)
    assert np.array_equal(first[0], plain[0])


# ------------------------------------------------------------ 5b. batches wider than a wavefront, rows wider than 16 bytes
_wide = {}


def wide_case(ctx, name):
    """ef and k above 64, so that the filter step compacts a batch in several chunks of 64 and all four wavefronts write
    rows out; the Jaccard mirror over 512 bits (four 16-byte vectors a row), so that its survivors' distances are scored
    again by several lane groups of every wavefront"""
    if name not in _wide:
        if name == "jaccard":
            nbits = 512
            rows, queries = bhm.rand_bits(fc.N, nbits, fc.SEED + 9), bhm.rand_bits(16, nbits, fc.SEED + 10)
            graph = sc.knn_graph(bhm.expand01(rows, nbits), fc.M, fc.SEED + 12, top=fc.TOP)
            c = Case(api.JaccardHnsw(ctx, nbits, rows), queries, graph, [fraction_ranks(q, rows) for q in queries],
                     np.stack([jm.ref_floats(q, rows) for q in queries]))
            c.h.set_graph(*graph)
        else:
            metric, kind = name
            base = case(ctx, metric, kind)
            queries = base.queries[:16] if not isinstance(base.queries, tuple) else shm.take(base.queries, range(16))
            c = Case(base.h, queries, base.graph, base.rank[:16], base.dist[:16])
        _wide[name] = c
    return _wide[name]


@pytest.mark.parametrize("ef,k", [(200, 150), (65, 130), (128, 128)])
@pytest.mark.parametrize("name", [("l2", "f32"), ("negip", "f16"), ("hamming", "bits"), ("l1", "sparse"), "jaccard"])
def test_batches_wider_than_a_wavefront(ctx, name, ef, k):
    """more than 64 survivors in one batch and k above 64: every row of every batch is written, whichever wavefront
    writes it, with everything kept (a batch's whole W goes out), under a filter, and through a drain"""
    c = wide_case(ctx, name)
    for selectivity, limit in ((1.0, 20000), (0.3, 20000), (1.0, 150), (0.3, 1)):
        keep = fc.keep_mask(selectivity, c.n)
        for strict in (False, True):
            with c.scan(ef) as s:
                got = s.filtered(k, keep, limit, strict)
            check_call(c, got, ef, k, keep, limit, strict, (name, ef, k, selectivity, limit, strict))
            if selectivity == 1.0:
                assert (got[2] == k).all() and (got[4] >= 2 if ef < k else got[4] >= 1).all()


# ------------------------------------------------------------------------------------ 6. a workgroup's later queries
def test_a_workgroups_next_query_starts_clean(ctx):
    """more queries than the launch has workgroups (8 per compute unit): every workgroup serves several in turn, and each
    query's rows, so->tuples, batches and pool are those of the same query scanned alone"""
    torch = pytest.importorskip("torch")
    n, dim, base = 200, 8, 4
    nq = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 100
    rows, queries = sc.rows_and_queries(21, n, dim, base, False)
    graph = sc.knn_graph(rows, 4, 22)
    h = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, dim, rows)
    h.set_graph(*graph)
    keep = fc.keep_mask(0.1, n)
    # four queries that end differently: k rows early, k rows after drains, exhausted
    alone = []
    for q in range(base):
        with h.scan(queries[q:q + 1], 5) as s:
            alone.append([x[0] for x in s.filtered(fc.K, keep, 60, True)])
    assert len({int(a[4]) for a in alone}) > 1  # (they take different numbers of batches)
    order = np.random.default_rng(23).integers(0, base, nq)
    with h.scan(np.ascontiguousarray(queries[order]), 5) as s:
        got = s.filtered(fc.K, keep, 60, True)
    for j, want in enumerate(zip(*[np.stack([alone[q][f] for q in order]) for f in range(6)])):
        assert all(np.array_equal(np.asarray(w).view(np.uint32) if f == 1 else w, g[j].view(np.uint32) if f == 1 else g[j])
                   for f, (w, g) in enumerate(zip(want, got))), j
    h.close()


# -------------------------------------------------------------------------------------- 7. empty index, overflow, errors
def test_empty_index(ctx):
    rows, queries, graph = fc.float_case()
    h = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, fc.DIM, rows)
    h.set_graph(graph[0], -1, graph[2], graph[3], graph[4])
    with h.scan(queries[:8], 5) as s:
        for _ in range(2):
            e, d, cnt, sco, batches, left = s.filtered(fc.K, None, 20000, False)
            assert (cnt == 0).all() and (e == -1).all() and np.isinf(d).all()
            assert (sco == 0).all() and (batches == 0).all() and (left == 0).all()
    h.close()


def test_pool_overflow_ends_the_scan_and_nothing_else(ctx):
    c = case(ctx, "l2", "f32")
    keep = fc.keep_mask(0.0, c.n)
    before = c.h.search(c.queries, 5, 5)
    peaks = []
    for q in range(c.nq):
        rec = c.recorded(q, 5, 20000)
        fc.run_loop(rec, fc.K, keep, False)
        peaks.append(rec.ms.max_pool)
    cap = max(peaks) - 1  # some query's pool outgrows it, in the middle of its scan
    assert cap > 5 * 16
    over = [q for q in range(c.nq) if peaks[q] > cap]
    with c.scan(5, discard_cap=cap) as s:
        for _ in range(2):
            with pytest.raises(api.PgvError) as err:
                s.filtered(fc.K, keep, 20000, False)
            assert err.value.code == _lib.PGV_ERR_NOMEM and "%d entries" % cap in err.value.message
            assert any("query %d " % q in err.value.message for q in over), err.value.message
        with pytest.raises(api.PgvError) as err:
            s.next()
        assert err.value.code == _lib.PGV_ERR_NOMEM
    with c.scan(5, discard_cap=max(peaks)) as s:  # the capacity that is just enough
        check_call(c, s.filtered(fc.K, keep, 20000, False), 5, fc.K, keep, 20000, False, "cap = peak")
    assert all(np.array_equal(x, y) for x, y in zip(c.h.search(c.queries, 5, 5), before))


def test_argument_errors_are_refused_before_any_launch(ctx):
    c = case(ctx, "l2", "f32")
    lib = _lib.lib
    nq, k = c.nq, fc.K
    e, d, cnt = np.zeros((nq, k), np.int64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)
    keep = api.pack_keep(np.ones((nq, c.n), dtype=bool))
    words = (c.n + 31) // 32

    def fails(rc, *text):
        assert rc == _lib.PGV_ERR_ARG, rc
        message = lib.pgv_last_error().decode()
        assert all(t in message for t in text), message

    def call(s, keep=None, stride=0, k=k, limit=20000, e=e, d=d, cnt=cnt):
        return lib.pgv_hnsw_scan_filtered(s, None, api.ptr(keep), stride, k, limit, 0, api.ptr(e), api.ptr(d), api.ptr(cnt),
                                          None, None, None)

    fails(call(None), "NULL")
    with c.scan(5) as s:
        fails(call(s.s, e=None), "NULL")
        fails(call(s.s, d=None), "NULL")
        fails(call(s.s, cnt=None), "NULL")
        for bad in (0, -1, 4097):
            fails(call(s.s, k=bad), "k must be 1..4096", str(bad))
        for bad in (0, -5):
            fails(call(s.s, limit=bad), "max_scan_tuples", str(bad))
        for bad in (1, words - 1, -words):
            fails(call(s.s, keep=keep, stride=bad), "keep_stride", str(bad))
        # nothing above touched the scan: its first batch is still to come; scored / batches / left are optional
        api.check(call(s.s, keep=keep, stride=words))
        first = c.h.search(c.queries, 5, 5)
        assert np.array_equal(e[:, :5], first[0]) and (cnt == k).all()
    with c.scan(5, queries=c.queries[:0]) as s:
        assert s.filtered(k)[0].shape == (0, k)
    big = 4096  # the widest row: k far beyond ef, every reachable element comes out
    with c.scan(16, queries=c.queries[:2]) as s:
        got = s.filtered(big, None, 20000, False)
    check_call(c, got, 16, big, np.ones(c.n, dtype=bool), 20000, False, "k 4096", queries=range(2))
    assert (got[2] > 256).all() and (got[5] == 0).all()
