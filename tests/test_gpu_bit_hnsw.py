"""HNSW over bit strings on the device -- pgv_hnsw_upload_bits, the bit instantiation of hnsw_search_kernel and of
score_gather_kernel, api.BitHnsw and api.binary_search_hnsw.  Hamming distances are integers, so every comparison of
distances, elements and scored counts is exact equality.  The yardsticks are the numpy models (tests/bit_model.py, tests/bit_hnsw_model.py), the
compiled oracle's walk over the 0/1 expansion, and the existing fp32 walk of the same graph over that expansion -- which
computes the same integers (tests/test_bit_hnsw_model_cpu.py) and is itself pinned to the oracle by the existing suite."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bit_hnsw_model as bhm
import bit_model as bm
from helpers import assert_topk_equiv, gen
from oracle import pyoracle as po
from pgvector_amd import _lib, api

pytestmark = pytest.mark.gpu

# 16-byte vector edges, partial last bytes, every lane-split switch of bit_row_geom (1 / 2 / 4 / ... / 64 lanes a row at
# 128 / 256 / 512 / 1024 / 2048 / 4096 bits, two trips past 8192) and the maximum
NBITS = [1, 7, 8, 64, 127, 128, 129, 136, 256, 257, 512, 513, 1023, 1024, 1025, 1536, 2048, 2049, 4096, 4097, 4104, 8192,
         8193, 16000, 64000]


def bit_mirror(ctx, nbits, rows, graph=None, payload=None):
    h = api.BitHnsw(ctx, nbits, rows, payload=payload)
    if graph is not None:
        m, entry, levels, nbr_start, nbr = graph
        h.set_graph(m, entry, levels, nbr_start, nbr)
    return h


# ------------------------------------------------------------------------------------------------------- 1. scores
@pytest.mark.parametrize("nbits", NBITS)
def test_score_is_the_hamming_distance(ctx, nbits):
    n = 64 if nbits == 64000 else 300
    rows, queries = bhm.rand_bits(n, nbits, 1000 + nbits), bhm.rand_bits(7, nbits, 2000 + nbits)
    rng = np.random.default_rng(nbits)
    slot, query_of = rng.integers(0, n, 999).astype(np.int32), rng.integers(0, 7, 999).astype(np.int32)
    h = bit_mirror(ctx, nbits, rows)
    got = h.score(queries, slot, query_of)
    want = np.array([bm.hamming(queries[q], rows[s:s + 1])[0] for s, q in zip(slot, query_of)], dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    assert np.array_equal(h.score(queries[3:4], slot[:10]), np.array([bm.hamming(queries[3], rows[s:s + 1])[0] for s in slot[:10]]))
    b = rng.integers(0, n, 999).astype(np.int32)
    want = np.array([bm.hamming(rows[y], rows[x:x + 1])[0] for x, y in zip(slot, b)], dtype=np.float32)
    assert np.array_equal(h.score_pairs(slot, b), want)
    h.close()


# ------------------------------------------------------------------- 2. the walk's scorer, independent of tie order
@pytest.mark.parametrize("m", [8, 32])
@pytest.mark.parametrize("nbits", [b for b in NBITS if b <= 16000])
def test_walk_scores_a_complete_graph(ctx, nbits, m):
    """whatever the tie order, the walk over a one-layer complete graph scores everything: the entry, then one batch of
    2 m (m = 32: a full 64-row batch)"""
    n, entry, levels, nbr_start, nbr = bhm.complete_graph(m)
    rows, queries = bhm.rand_bits(n, nbits, 3000 + nbits + m), bhm.rand_bits(6, nbits, 4000 + nbits + m)
    h = bit_mirror(ctx, nbits, rows, (m, entry, levels, nbr_start, nbr))
    for ef, k in ((n, n), (n, 5), (5, 5)):
        elem, dist, scored = h.search(queries, ef, k)
        assert (scored == n).all(), (ef, k, scored.tolist())
        bhm.assert_topk_up_to_ties(elem, dist, queries, rows, k, what="nbits %d m %d ef %d k %d" % (nbits, m, ef, k))
    h.close()


# --------------------------------------------------------------------------------------- 3. the oracle's walk, tie-free
@pytest.fixture(scope="module")
def tie_free_case(oracle):
    nq, n, nbits, seed = 8, 500, 16000, 5  # tests/test_bit_hnsw_model_cpu.py checks the precondition on the same draw
    queries, rows = bhm.tie_free(nq, n, nbits, seed)
    g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, bhm.expand01(rows, nbits), m=8, ef_construction=32, seed=7)
    return queries, rows, nbits, g, g.export_tuples()


@pytest.mark.parametrize("ef,k", [(40, 10), (1, 1)])
def test_walk_equals_the_oracle_on_tie_free_data(ctx, tie_free_case, ef, k):
    """no two candidates equally far: the walk is determined, so elements, distances and so->tuples equal the oracle's"""
    queries, rows, nbits, g, ex = tie_free_case
    h = bit_mirror(ctx, nbits, rows[ex["rows"]], (8, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"]))
    elem, dist, scored = h.search(queries, ef, k)
    q01 = bhm.expand01(queries, nbits)
    for i in range(len(queries)):
        want_rows, want_dist, want_scored = g.search(q01[i], ef, k)
        assert len(want_rows) == k
        assert ex["rows"][elem[i]].tolist() == want_rows.tolist(), i
        assert dist[i].astype(np.float64).tolist() == want_dist.tolist(), i
        assert int(scored[i]) == want_scored, i
    h.close()


# -------------------------------------------------------------------------------------- 4. the fp32 twin, ties and all
@pytest.fixture(scope="module", params=[64, 100, 1536])
def twin_case(request, oracle):
    nbits = request.param
    rows, queries = bhm.rand_bits(3000, nbits, 5000 + nbits), bhm.rand_bits(48, nbits, 6000 + nbits)
    g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, bhm.expand01(rows, nbits), m=16, ef_construction=32, seed=9)
    ex = g.export_tuples()
    g.close()
    return nbits, np.ascontiguousarray(rows[ex["rows"]]), queries, ex


def test_walk_equals_the_fp32_twin(ctx, twin_case):
    """density-0.5 bits: ties everywhere.  The same graph over the same elements as a bit mirror and as their 0/1 fp32
    expansion under PGV_L2SQ: the keys are the same integers and the walk code is shared"""
    nbits, elements, queries, ex = twin_case
    graph = (16, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"])
    h = bit_mirror(ctx, nbits, elements, graph)
    twin = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, nbits, bhm.expand01(elements, nbits))
    twin.set_graph(*graph)
    q01 = bhm.expand01(queries, nbits)
    elem, dist, scored = h.search(queries, 64, 10)
    t_elem, t_dist, t_scored = twin.search(q01, 64, 10)
    assert int(ex["levels"].max()) >= 1 and (scored < 3000).all()
    assert np.array_equal(elem, t_elem) and np.array_equal(dist, t_dist) and np.array_equal(scored, t_scored)
    assert max(np.unique(dist[q], return_counts=True)[1].max() for q in range(48)) >= 2  # the case holds ties
    for q in range(48):
        assert np.array_equal(dist[q], bm.hamming(queries[q], elements[elem[q]]))
    rng = np.random.default_rng(nbits)
    slot, query_of = rng.integers(0, 3000, 999).astype(np.int32), rng.integers(0, 48, 999).astype(np.int32)
    assert np.array_equal(h.score(queries, slot, query_of), twin.score(q01, slot, query_of))
    twin.close()
    h.close()


# ---------------------------------------------------------------------------------------------- 5. views and importers
@pytest.fixture(scope="module")
def small_case():
    nbits, m = 200, 8
    n, entry, levels, nbr_start, nbr = bhm.complete_graph(m)
    rows, queries = bhm.rand_bits(n, nbits, 71), bhm.rand_bits(5, nbits, 72)
    payload = (np.arange(n, dtype=np.uint32)[:, None] * 31 + np.arange(3, dtype=np.uint32)[None, :]).astype(np.uint32)
    return nbits, rows, queries, (m, entry, levels, nbr_start, nbr), payload


def test_share_view_returns_the_owners_answers(ctx, small_case):
    nbits, rows, queries, graph, payload = small_case
    h = bit_mirror(ctx, nbits, rows, graph, payload)
    own = h.search(queries, 10, 10)
    ctx2 = api.Context(0)
    view = h.share(ctx2)
    got = view.search(queries, 10, 10)
    for a, b in zip(own, got):
        assert np.array_equal(a, b)
    slot = np.arange(len(rows), dtype=np.int32)
    assert np.array_equal(view.score(queries[:1], slot), bm.hamming(queries[0], rows))
    assert np.array_equal(view.get_payload(np.array([3, -1])), np.stack([payload[3], np.zeros(3, np.uint32)]))
    view.close()
    ctx2.close()
    h.close()


def test_bit_mirror_across_processes(ctx, small_case, tmp_path):
    """pgv_hnsw_export / pgv_hnsw_import carry the element type and nbits: a fresh child process searches and scores the
    owner's rows and reads the payload of its results"""
    nbits, rows, queries, graph, payload = small_case
    h = bit_mirror(ctx, nbits, rows, graph, payload)
    own_elem, own_dist, own_scored = h.search(queries, 10, 10)
    job, res = str(tmp_path / "job.npz"), str(tmp_path / "res.npz")
    np.savez(job, handle=np.frombuffer(h.export(), dtype=np.uint8), queries=queries, ef=10, k=10, words=3)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "mp_bit_hnsw_import_worker.py"), job, res], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(res)
    assert np.array_equal(out["elem"], own_elem) and np.array_equal(out["dist"], own_dist)
    assert np.array_equal(out["scored"], own_scored)
    assert np.array_equal(out["score"], [bm.hamming(queries[i], rows[i:i + 1])[0] for i in range(len(queries))])
    assert np.array_equal(out["payload"], payload[own_elem.ravel()])
    h.close()


def test_payload_round_trip(ctx, small_case):
    nbits, rows, _, _, payload = small_case
    h = bit_mirror(ctx, nbits, rows, payload=payload)
    ids = np.array([0, 16, -1, 5, 5], dtype=np.int64)
    want = np.where(ids[:, None] >= 0, payload[np.clip(ids, 0, None)], 0)
    assert np.array_equal(h.get_payload(ids), want)
    h.close()
    h = bit_mirror(ctx, nbits, rows)
    with pytest.raises(api.PgvError) as e:
        h.get_payload(ids, words=3)
    assert e.value.code == api.PGV_ERR_STATE
    h.close()


def test_update_graph_is_seen_by_the_next_search(ctx, small_case):
    nbits, rows, queries, (m, entry, levels, nbr_start, nbr), _ = small_case
    n = len(rows)
    h = bit_mirror(ctx, nbits, rows, (m, entry, levels, nbr_start, np.full_like(nbr, -1)))
    elem, dist, scored = h.search(queries, n, n)
    assert (elem[:, 0] == 0).all() and (elem[:, 1:] == -1).all() and (scored == 1).all()  # nothing but the entry point
    # element 3 becomes the entry point and gets its full tuple: everything is one hop away
    h.update_graph(3, np.array([3], dtype=np.int32), np.array([0, 2 * m], dtype=np.int64), nbr[nbr_start[3]:nbr_start[4]])
    elem, dist, scored = h.search(queries, n, n)
    assert (scored == n).all()
    bhm.assert_topk_up_to_ties(elem, dist, queries, rows, n, what="patched")
    h.close()


# ------------------------------------------------------------------------------------------------------------ 6. edges
def test_empty_index_and_one_element(ctx):
    queries = bhm.rand_bits(3, 100, 81)
    for rows in (bhm.rand_bits(4, 100, 82), np.zeros((0, 13), dtype=np.uint8)):
        n = len(rows)
        h = bit_mirror(ctx, 100, rows, (8, -1, np.zeros(n, np.int32), np.arange(n + 1, dtype=np.int64) * 16,
                                        np.full(max(16 * n, 1), -1, np.int32)))
        elem, dist, scored = h.search(queries, 5, 5)
        assert (elem == -1).all() and np.isinf(dist).all() and (dist > 0).all() and (scored == 0).all()
        h.close()
    rows = bhm.rand_bits(1, 100, 83)
    h = bit_mirror(ctx, 100, rows, (8, 0, np.zeros(1, np.int32), np.array([0, 16], np.int64), np.full(16, -1, np.int32)))
    elem, dist, scored = h.search(queries, 3, 3)
    assert elem.tolist() == [[0, -1, -1]] * 3 and scored.tolist() == [1] * 3
    assert dist[:, 0].tolist() == [bm.hamming(q, rows)[0] for q in queries] and np.isinf(dist[:, 1:]).all()
    h.close()


def test_argument_errors(ctx, small_case):
    nbits, rows, queries, graph, _ = small_case
    h = bit_mirror(ctx, nbits, rows, graph)
    for ef, k in ((5, 6), (1001, 10), (0, 1), (5, 0)):
        with pytest.raises(api.PgvError) as e:
            h.search(queries, ef, k)
        assert e.value.code == api.PGV_ERR_ARG, (ef, k)
    h.close()
    for bad in (0, 64001, -1):
        with pytest.raises(api.PgvError) as e:
            api.BitHnsw(ctx, bad, np.zeros((2, max((bad + 7) // 8, 1)), dtype=np.uint8))
        assert e.value.code == _lib.PGV_ERR_DIMS, bad
    with pytest.raises(api.PgvError) as e:
        api.BitHnsw(ctx, nbits, rows, metric=api.PGV_BIT_JACCARD)
    assert e.value.code == api.PGV_ERR_ARG and "jaccard" in e.value.message
    with pytest.raises(api.PgvError) as e:
        api.BitHnsw(ctx, nbits, rows, metric=2)
    assert e.value.code == api.PGV_ERR_ARG
    h = api.BitHnsw(ctx, nbits, rows)
    with pytest.raises(api.PgvError) as e:  # no graph yet
        h.search(queries, 5, 5)
    assert e.value.code == api.PGV_ERR_ARG
    h.close()


def test_build_side_entries_reject_a_bit_mirror(ctx, small_case):
    """every pgv_hnsw_build_* / pgv_hnsw_link_* entry and pgv_hnsw_score_groups: PGV_ERR_ARG before any launch, and the
    mirror searches as before afterwards"""
    nbits, rows, queries, graph, _ = small_case
    h = bit_mirror(ctx, nbits, rows, graph)
    before = h.search(queries, 10, 10)
    L = C.CDLL(_lib.LIB_PATH)  # a handle of its own: the prototypes other modules declare on _lib.lib do not apply
    L.pgv_last_error.restype = C.c_char_p
    i32 = lambda c: np.zeros(c, dtype=np.int32)  # noqa: E731
    f32, u8, i64 = np.zeros(4096, np.float32), np.zeros(4096, np.uint8), np.zeros(8, np.int64)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    el, lv, big, cnt = i32(2), i32(2), i32(4096), i32(2)
    calls = {
        "pgv_hnsw_build_search": lambda: L.pgv_hnsw_build_search(h.h, P(el), P(lv), C.c_int(2), C.c_int(8), C.c_int(1), P(big),
                                                                 P(f32), P(cnt)),
        "pgv_hnsw_build_neighbors": lambda: L.pgv_hnsw_build_neighbors(h.h, P(el), P(lv), C.c_int(2), C.c_int(8), C.c_int(1),
                                                                       P(big), P(f32), P(u8), P(cnt), P(i64)),
        "pgv_hnsw_build_search_keep": lambda: L.pgv_hnsw_build_search_keep(h.h, P(el), P(lv), C.c_int(2), C.c_int(8),
                                                                           C.c_int(1), C.c_int(0)),
        "pgv_hnsw_build_select_kept": lambda: L.pgv_hnsw_build_select_kept(h.h, C.c_int(0), P(big), P(f32), P(u8), P(cnt),
                                                                           P(i64)),
        "pgv_hnsw_link_begin": lambda: L.pgv_hnsw_link_begin(h.h),
        "pgv_hnsw_link_prepare": lambda: L.pgv_hnsw_link_prepare(h.h, P(el), P(u8), C.c_int(2), C.c_int(1), P(big), P(f32),
                                                                 P(u8), P(cnt), P(i64)),
        "pgv_hnsw_link_apply": lambda: L.pgv_hnsw_link_apply(h.h, C.c_int32(0)),
        "pgv_hnsw_link_end": lambda: L.pgv_hnsw_link_end(h.h, P(big), P(i64), P(i64)),
        "pgv_hnsw_score_groups": lambda: L.pgv_hnsw_score_groups(h.h, P(el), P(i64), P(cnt), P(i64), C.c_int(1),
                                                                 C.c_int64(2), C.c_int64(1), P(f32)),
    }
    declared = [s for s in _lib.SYMBOLS if s.startswith(("pgv_hnsw_build_", "pgv_hnsw_link_"))] + ["pgv_hnsw_score_groups"]
    assert sorted(calls) == sorted(declared)
    for name, call in calls.items():
        assert call() == api.PGV_ERR_ARG, name
        assert "bit mirror" in L.pgv_last_error().decode(), name
    after = h.search(queries, 10, 10)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    h.close()


def test_device_resident_inputs(ctx, small_case):
    import torch
    nbits, rows, queries, (m, entry, levels, nbr_start, nbr), _ = small_case
    h = bit_mirror(ctx, nbits, rows, (m, entry, levels, nbr_start, nbr))
    want = h.search(queries, 10, 10)
    slot = np.arange(len(rows), dtype=np.int32)
    want_score = h.score(queries[:1], slot)
    d = bit_mirror(ctx, nbits, torch.from_numpy(rows).cuda(), (m, entry, levels, nbr_start, nbr))
    got = d.search(torch.from_numpy(queries).cuda(), 10, 10)
    assert all(g.is_cuda for g in got)
    for a, b in zip(want, got):
        assert np.array_equal(a, b.cpu().numpy())
    assert np.array_equal(d.score(torch.from_numpy(queries[:1].copy()).cuda(), slot), want_score)
    # 128 bits = 16 bytes: device rows and queries are read in place
    rows16, q16 = bhm.rand_bits(len(rows), 128, 91), bhm.rand_bits(4, 128, 92)
    a = bit_mirror(ctx, 128, rows16, (m, entry, levels, nbr_start, nbr))
    b = bit_mirror(ctx, 128, torch.from_numpy(rows16).cuda(), (m, entry, levels, nbr_start, nbr))
    for x, y in zip(a.search(q16, 10, 10), b.search(torch.from_numpy(q16).cuda(), 10, 10)):
        assert np.array_equal(x, y.cpu().numpy())
    for x in (h, d, a, b):
        x.close()


# ------------------------------------------------------------------------------------ 7. the README query end to end
def test_binary_search_hnsw_over_a_complete_graph(ctx, oracle):
    """65 x 200-d normal rows, their binary_quantize image in a complete one-layer graph, ef = kc = 65: stage one hands
    every row over, so the answer is the model's rerank over all rows (continuous data: no ties in the outer metric)"""
    rows, queries = gen(65, 200, seed=141, dist="normal"), gen(16, 200, seed=142, dist="normal")
    bits = api.binary_quantize(ctx, api.PGV_F32, 200, rows)
    assert np.array_equal(bits, bm.binary_quantize(rows))
    n, entry, levels, nbr_start, nbr = bhm.complete_graph(32)
    h = bit_mirror(ctx, 200, bits, (32, entry, levels, nbr_start, nbr))
    dist, idx, hamming, cand, scored = api.binary_search_hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, 200, queries, rows, h, 65, 65, 5,
                                                              want_candidates=True)
    assert (scored == 65).all()
    bhm.assert_topk_up_to_ties(cand, hamming, bm.binary_quantize(queries), bits, 65, what="stage one")
    wd, wi = bm.rerank(oracle, api.PGV_L2SQ, False, queries, rows, np.tile(np.arange(65, dtype=np.int64), (16, 1)), 5)
    assert np.array_equal(idx, wi)
    for q in range(16):
        assert_topk_equiv(idx[q].tolist(), dist[q], wi[q].tolist(), wd[q], what="binary_search_hnsw q%d" % q)
    d2, i2 = api.binary_search_hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, 200, queries, rows, h, 65, 65, 5)
    assert np.array_equal(i2, idx) and np.array_equal(d2, dist)
    h.close()


def test_binary_search_hnsw_over_a_real_graph(ctx, oracle, twin_case):
    """the multi-layer, tie-ridden graphs of test_walk_equals_the_fp32_twin under fp32 rows of as many dimensions as the
    elements have bits, kc = 20: the walk's candidates equal the fp32 twin's, and the outer result is the model's rerank
    of the walk's own candidates"""
    nbits, elements, _, ex = twin_case
    graph = (16, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"])
    rows, queries = gen(3000, nbits, seed=151, dist="normal"), gen(16, nbits, seed=152, dist="normal")
    h = bit_mirror(ctx, nbits, elements, graph)
    dist, idx, hamming, cand, scored = api.binary_search_hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, nbits, queries, rows, h, 64, 20, 5,
                                                              want_candidates=True)
    twin = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F32, nbits, bhm.expand01(elements, nbits))
    twin.set_graph(*graph)
    t_elem, t_dist, t_scored = twin.search(bhm.expand01(bm.binary_quantize(queries), nbits), 64, 20)
    assert np.array_equal(cand, t_elem) and np.array_equal(hamming, t_dist) and np.array_equal(scored, t_scored)
    wd, wi = bm.rerank(oracle, api.PGV_L2SQ, False, queries, rows, cand, 5)
    assert np.array_equal(idx, wi)
    for q in range(16):
        assert_topk_equiv(idx[q].tolist(), dist[q], wi[q].tolist(), wd[q], what="binary_search_hnsw q%d" % q)
    twin.close()
    h.close()
