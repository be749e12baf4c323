"""Round 6: the L2 assignment's completeness bound is deterministic by default."""
import numpy as np
import pytest

from pgvector_amd import api

from helpers import gen  # noqa: F401
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def _near_tie_case(seed, n, k, dim):
    """Integer data: a row's squared distances to the two centers of ITS group are exact in fp32 in any summation order
    (sums of integer squares below 2^24), so the reference's argmin between them is a fact, not a property of its
    compiler's vectorisation -- and they are 0, 1 or 2 apart at magnitudes 2^23 .. 2^24, where fp32 has ulp 1.
    Centers come in groups of two: the odd one is its left neighbour with coordinate j moved up by 1 (every fourth group:
    coordinate l moved down by 1 as well).  A row is a center of its group + noise of amplitude A (dim A^2 / 3 ~ 1.15e7),
    with its coordinates j (and l) set on purpose: distance to the odd center minus distance to the even one is then
    -1 or +1 (two-coordinate groups: 0, 2 or 4) -- exact ties included, which the LOWER id must win
    (src/ivfbuild.c:187-191).  Every other group is ~6e7 away."""
    rng = np.random.default_rng(seed)
    amp = int(np.sqrt(3 * 1.15e7 / dim))
    base = rng.integers(400, 1600, (k // 2, dim)).astype(np.float32)
    centers = np.repeat(base, 2, axis=0)
    jj = rng.integers(0, dim, k // 2)
    ll = (jj + 1 + rng.integers(0, dim - 1, k // 2)) % dim
    two = (np.arange(k // 2) % 4) == 0
    for g in range(k // 2):
        centers[2 * g + 1, jj[g]] += 1.0
        if two[g]:
            centers[2 * g + 1, ll[g]] -= 1.0
    grp = rng.integers(0, k // 2, n)
    rows = base[grp] + rng.integers(-amp, amp + 1, (n, dim)).astype(np.float32)
    r = np.arange(n)
    rows[r, jj[grp]] = base[grp, jj[grp]] + rng.integers(0, 2, n)
    rows[r, ll[grp]] = np.where(two[grp], base[grp, ll[grp]] + rng.integers(0, 2, n), rows[r, ll[grp]])
    assert rows.min() >= 0 and rows.max() < 2048
    return np.ascontiguousarray(rows), np.ascontiguousarray(centers), grp


@pytest.mark.parametrize("tname", ["f32", "f16"])
@pytest.mark.parametrize("n,k,dim", [(40_000, 256, 256), (20_000, 1024, 1024), (6_000, 40, 1536)])
def test_adversarial_near_tie_centers_get_the_oracles_list_ids_exactly(ctx, oracle, tname, n, k, dim):
    rows, centers, grp = _near_tie_case(7 + dim, n, k, dim)
    dt, odt, npdt = (api.PGV_F32, po.ORA_F32, np.float32) if tname == "f32" else (api.PGV_F16, po.ORA_F16, np.float16)
    rows, centers = rows.astype(npdt), centers.astype(npdt)       # (integers below 2048: exact in fp16 too)
    want, wd = oracle.assign(po.OPS_L2, odt, centers, rows)
    got, gd = api.assign(ctx, api.PGV_L2SQ, dt, dim, centers, rows, want_dist=True)
    got, gd = np.asarray(got), np.asarray(gd)
    # how adversarial it is: the two centers of a row's group, in float64 (exact here)
    r64 = rows[:4000].astype(np.float64)
    d0 = ((r64 - centers[2 * grp[:4000]].astype(np.float64)) ** 2).sum(-1)
    d1 = ((r64 - centers[2 * grp[:4000] + 1].astype(np.float64)) ** 2).sum(-1)
    assert d0.max() < 2 ** 24 and d1.max() < 2 ** 24 and np.median(d0) > 2 ** 23
    gap_ulp = np.abs(d1 - d0) / np.spacing(np.minimum(d0, d1).astype(np.float32))
    assert (gap_ulp <= 4).all() and (gap_ulp == 0).mean() > 0.03 and (gap_ulp == 1).mean() > 0.3
    assert (np.asarray(want)[:4000] // 2 == grp[:4000]).all()         # the nearest center IS one of the two
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(gd, wd)        # exact data: the distances are the reference's bit for bit


def test_both_bounds_choose_alike_and_the_default_is_the_deterministic_one(ctx, oracle):
    """real-valued data (the oracle's own summation order is one of many): ids equal the oracle's wherever its two best
    distances differ by more than the float tolerance, under the default AND under the statistical bound; the counters say
    which rows were rechecked / redone"""
    n, k, dim = 30_000, 500, 768
    rows = gen(n, dim, seed=61, dist="clustered", clusters=125)
    centers = rows[np.random.default_rng(62).choice(n, k, replace=False)].copy()
    want, wd = oracle.assign(po.OPS_L2, po.ORA_F32, centers, rows)
    res = {}
    for mode in ("default", "statistical", "worst"):
        if mode != "default":
            ctx.set_bound(mode == "worst")
        ctx.set_profiling(True)
        ctx.reset_stats()
        got, gd = api.assign(ctx, api.PGV_L2SQ, api.PGV_F32, dim, centers, rows, want_dist=True)
        st = ctx.stats()
        ctx.set_profiling(False)
        res[mode] = (np.asarray(got), st["assign_recheck_rows"], st["assign_redo_rows"])
        diff = np.nonzero(res[mode][0] != want)[0]
        for r in diff:       # a float-level tie on the oracle's side: both centers as near as each other to 1e-5
            d = ((rows[r].astype(np.float64) - centers[[res[mode][0][r], want[r]]].astype(np.float64)) ** 2).sum(-1)
            assert abs(d[0] - d[1]) <= 1e-5 * d[1], (mode, r, d)
        assert len(diff) <= n // 1000
    ctx.set_bound(True)      # back to the library's default for the rest of the session
    np.testing.assert_array_equal(res["default"][0], res["worst"][0])
    assert res["default"][1] == res["worst"][1] and res["default"][1] >= res["statistical"][1]


def test_bench_n_gpu_code_path_with_one_rccl_rank(tmp_path):
    """bench.py --sharded-path: the code a --gpus N run takes -- torch.distributed over RCCL, the library's own
    communicator (pgv_comm_create through librccl), pgv_kmeans_sharded, the row exchange to the lists' owners,
    pgv_search_batch_sharded and its device merge -- with the one rank a one-GPU box can give it.  Not a scaling number:
    the closest rehearsal of the multi-GPU run that this pool allows."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k_ in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k_, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--sharded-path", "--workload", "small", "--steps", "3",
                        "--warmup", "1", "--settle-ms", "0", "--full"], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["recall_at_10"] >= 0.99 and line["value"] > 0
    detail = json.load(open(os.path.join(root, "bench_detail.json")))
    mg = detail["multi_gpu"]
    assert mg["communicator"] == "rccl" and mg["comm_size"] == 1 and mg["backend"] == "nccl"


def test_hard_data_set_at_the_headline_shape_answers_like_the_oracle(ctx, oracle):
    """bench.py's mid-difficulty data set (gen_hard: overlapping Zipf-weighted mixture, power-law spectrum) at the
    headline's shape: it must BE mid-difficulty (recall@10 between 0.8 and 0.95 at probes 10 against float64 brute force,
    unbalanced lists, Lloyd running for dozens of iterations) and the GPU's answers must be the oracle's row for row, at
    probes 10 and 32 -- lists probed by hundreds of queries, re-streamed once per 32-query group, k' candidates under the
    deterministic bound with something to decide."""
    import os
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench
    finally:
        sys.argv = argv
    from helpers import assert_topk_equiv
    dev = torch.device("cuda", 0)
    n, dim, lists, k = 1_000_000, 1536, 1000, 10
    data, means = bench.gen_hard(n, dim, lists // 4, 50, dev)
    centers, offsets, vectors, tids, iters, bt, index = bench.build_index(ctx, data, lists, 0, 1, 0, api.PGV_F32, api.PGV_OPS_L2,
                                                                          api.PGV_L2SQ)
    del data
    assert iters >= 10
    sizes = (offsets[1:] - offsets[:-1]).double()
    assert float(sizes.max() / sizes.mean()) > 3.0
    nq = 512
    queries, _ = bench.gen_hard(nq, dim, lists // 4, 150, dev, means=means)
    exact_d, _ = bench.exact_topk_fp64(vectors, queries[:128].contiguous(), k, api.PGV_L2SQ)
    ix = oracle.index_struct(po.OPS_L2, po.ORA_F32, centers.cpu().numpy(), offsets.cpu().numpy(), vectors.cpu().numpy(),
                             tids.cpu().numpy().astype(np.uint64))
    qh = queries.cpu().numpy()
    for probes in (10, 32):
        ctx.set_profiling(True)
        ctx.reset_stats()
        gd, gs, gt = index.search_batch(queries, probes, k, want_tid=True)
        st = ctx.stats()
        ctx.set_profiling(False)
        assert st["scan_launches"] >= 1
        recall = bench.recall_at_k(gd[:128], exact_d, k)
        if probes == 10:
            assert 0.8 < recall < 0.95, recall
        else:
            assert recall > 0.9, recall
        gdh, gth = gd.cpu().numpy(), gt.cpu().numpy()
        for i in range(0, nq, 8):
            wt, wd = oracle.search(ix, qh[i], probes, k)
            assert_topk_equiv(gth[i][:len(wt)].astype(np.uint64).tolist(), gdh[i][:len(wt)], wt.tolist(), wd,
                              what="hard probes %d q%d" % (probes, i))
    index.close()


_QUERY_STREAM = r'''
import hashlib, sys, os
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
from pgvector_amd import api
from helpers import gen
from oracle import pyoracle as po
from helpers import CpuIvf
dim, lists = int(sys.argv[1]), 40
oracle = po.Oracle()
data = gen(9000, dim, seed=611, dist="clustered", clusters=lists)
ivf = CpuIvf(oracle, po.OPS_L2, po.ORA_F32, data, lists)
ctx = api.Context(0)
ix = api.IvfIndex(ctx, ivf.metric, api.PGV_F32, dim, ivf.centers, ivf.list_offsets, ivf.vectors, ivf.tids)
qh = api.Query(ix)
h = hashlib.sha256()
queries = gen(400, dim, seed=612, dist="clustered", clusters=lists)
for i, q in enumerate(queries):
    qh.rank(q, 6)
    if i % 7 == 3:
        qh.rank(queries[(i * 5) % 400], 6)   # a rank no scan followed: the row is rewritten under a pending kernel
        qh.rank(q, 6)
    d, s, t, total = qh.scan(0, 3, 16)
    h.update(np.asarray(d).tobytes()); h.update(np.asarray(s).tobytes()); h.update(np.asarray(t).tobytes())
    h.update(np.asarray(qh.lists(6)).tobytes())
qh.close(); ix.close(); ctx.close()
print("DIGEST", h.hexdigest())
'''


@pytest.mark.parametrize("dim", [256, 100])
def test_query_rows_written_through_the_bar_answer_like_staged_ones(dim):
    """pgv_query_rank writes the query into a fine-grained device row from the host (no staging kernel) where the
    device is behind a large BAR; PGV_QUERY_DIRECT=0 keeps the pinned row + query_stage_kernel.  400 back-to-back
    queries (with ranks that no scan follows in between) must answer bit for bit alike both ways: a stale or torn
    query row would change distances."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    digests = []
    for direct in ("1", "0"):
        env = dict(os.environ, PGV_QUERY_DIRECT=direct)
        r = subprocess.run([sys.executable, "-c", _QUERY_STREAM, str(dim)], cwd=root, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        digests.append([ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][-1])
    assert digests[0] == digests[1]


@pytest.mark.parametrize("m", [5, 1000, 1024, 1025, 4096, 4097, 12288, 12289, 20480, 20481, 30000])
def test_selection_edges_of_the_single_query_head(ctx, m):
    """query_head_kernel's selection at every size class of block_topk_auto (1 / 4 / 12 / 20 vectors per thread, the
    general path past 20 480) and at the k that switch its threshold form (<= 16: per-wavefront extraction; above: the
    256-way rank): integer coordinates make every distance exact, most of them tied, a few rows are NaN and +inf.
    The stream is (distance, position) ascending, NaN last -- compared element for element, ties included."""
    rng = np.random.default_rng(900 + m)
    vec = rng.integers(-3, 4, (m, 2)).astype(np.float32)
    if m > 10:
        vec[rng.integers(0, m, 3)] = np.nan
        vec[rng.integers(0, m, 3), 0] = 3e19           # squares to +inf in fp32
    centers = np.array([[0, 0], [50, 50]], dtype=np.float32)
    off = np.array([0, m, m], dtype=np.int64)
    ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, 2, centers, off, vec, np.arange(m, dtype=np.uint64))
    qh = api.Query(ix)
    q = np.array([1, -1], dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        want_d = ((vec - q) ** 2).sum(axis=1, dtype=np.float32)
    key = np.where(np.isnan(want_d), np.inf, want_d)
    order = np.lexsort((np.arange(m), np.isnan(want_d), key))   # distance, NaN after +inf, then position
    qh.rank(q, 2)
    for head in (1, 2, 3, 15, 16, 17, 33, 64, 128, 129, 500, 1024):
        d, s, t, total = qh.scan(0, 1, head)
        n = min(head, m)
        assert total == m and len(s) == n
        np.testing.assert_array_equal(s, order[:n], err_msg="m %d head %d" % (m, head))
        np.testing.assert_array_equal(np.asarray(d), want_d[order[:n]])
        np.testing.assert_array_equal(t, order[:n].astype(np.uint64))
    qh.close()
    ix.close()


@pytest.mark.parametrize("m", [40, 1025, 4097, 12289, 20481])
@pytest.mark.parametrize("nq", [3, 300])
def test_selection_edges_of_the_batched_heads(ctx, m, nq):
    """the same stream through pgv_search_batch: 3 queries take the few-queries path (mq_head_kernel's selection), 300
    the list-major path (mfma scan + topk_kernel + exact recheck); k below, at and above the extraction limit.
    Distances are exact; inside a run of equal distances any member may close the head (tuplesort's tie order is
    unspecified), so ties are compared as sets."""
    rng = np.random.default_rng(950 + m)
    vec = rng.integers(-3, 4, (m, 2)).astype(np.float32)
    centers = np.array([[0, 0], [50, 50]], dtype=np.float32)
    off = np.array([0, m, m], dtype=np.int64)
    ix = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, 2, centers, off, vec, np.arange(m, dtype=np.uint64))
    queries = rng.integers(-2, 3, (nq, 2)).astype(np.float32)
    for k in (1, 10, 16, 17, 40):
        dist, slot, _ = ix.search_batch(queries, 1, k)
        for qi in (0, nq // 2, nq - 1):
            want_d = ((vec - queries[qi]) ** 2).sum(axis=1, dtype=np.float32)
            order = np.lexsort((np.arange(m), want_d))[:k]
            np.testing.assert_array_equal(np.asarray(dist[qi]), want_d[order], err_msg="m %d nq %d k %d" % (m, nq, k))
            got = np.asarray(slot[qi])
            np.testing.assert_array_equal(want_d[got], want_d[order])       # every slot carries the distance it claims
            last = want_d[order[-1]]
            assert set(got[want_d[got] < last]) == set(order[want_d[order] < last])   # below the last tie class: exact
            assert len(set(got.tolist())) == k
    ix.close()
