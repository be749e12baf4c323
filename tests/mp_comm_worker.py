"""Two ranks on ONE GPU (functional run of the library's multi-GPU path): the collectives of pgv_comm
are host callbacks over gloo, everything else is the real C path.  Launched by test_gpu_round2.py
through torch.distributed.run; rank 0 prints 'COMM-OK' when every check passed."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_model as km  # noqa: E402
from pgvector_amd import api  # noqa: E402


def exact_shards_equal_single(ctx, comm, rank, shards, k, what, script=None):
    """integer data (tests/kmeans_model.py: sums, counts and weight totals below 2^24 are exact under any association):
    the sharded run must equal the single-rank run on the concatenation -- centers, this rank's closest, iterations.
    script = (u32, doubles): both runs replay it (and 0.5 beyond it) instead of the library's generator"""
    whole = np.ascontiguousarray(np.concatenate(shards))
    dim = whole.shape[1]
    lo = sum(len(s) for s in shards[:rank])
    mine = np.ascontiguousarray(shards[rank])
    rngs = [km.ScriptedRng(*script) for _ in range(2)] if script else None
    c, cl, it = comm.kmeans(api.PGV_OPS_L2, api.PGV_F32, dim, mine, k, rngs[0].rng if script else api.make_rng(seed=9))
    sc, scl, sit = api.kmeans(ctx, api.PGV_OPS_L2, api.PGV_F32, dim, whole, k,
                              rngs[1].rng if script else api.make_rng(seed=9))
    assert np.array_equal(c, sc), (what, "centers", int((c != sc).any(axis=1).sum()))
    assert it == sit, (what, "iterations", it, sit)
    if len(mine):
        assert np.array_equal(cl, scl[lo:lo + len(mine)]), (what, "closest", int((cl != scl[lo:lo + len(mine)]).sum()))
    else:
        assert cl is None, what


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    ctx = api.Context(0, stream=0)
    comm = api.Comm(ctx, backend="host")
    rng = np.random.default_rng(5)
    n, dim, k = 6000, 48, 40
    means = rng.random((k, dim), dtype=np.float32)
    data = (means[rng.integers(0, k, n)] + 0.05 * rng.standard_normal((n, dim))).astype(np.float32)
    per = (n + world - 1) // world
    mine = np.ascontiguousarray(data[rank * per:(rank + 1) * per])

    # k-means: sharded samples, same centers on every rank, as good as the single-GPU run
    centers, closest, iters = comm.kmeans(api.PGV_OPS_L2, api.PGV_F32, dim, mine, k, api.make_rng(seed=9))
    allc = [torch.empty(k, dim) for _ in range(world)]
    dist.all_gather(allc, torch.from_numpy(centers))
    assert all(torch.equal(allc[0], c) for c in allc), "centers differ between the ranks"
    single, sc, siters = api.kmeans(ctx, api.PGV_OPS_L2, api.PGV_F32, dim, data, k, api.make_rng(seed=9))

    def inertia(c):
        d = ((data[:, None, :].astype(np.float64) - c[None, :, :].astype(np.float64)) ** 2).sum(-1)
        return float(d.min(axis=1).sum())
    assert inertia(centers) <= 1.03 * inertia(single), (inertia(centers), inertia(single))
    assert 1 <= iters <= 500
    # the local assignment is the argmin under the final centers
    want, _ = api.assign(ctx, api.PGV_L2SQ, api.PGV_F32, dim, centers, mine)
    assert (want != closest).mean() < 0.01

    # spherical opclass, one rank without samples
    unit = data / np.linalg.norm(data, axis=1, keepdims=True)
    part = np.ascontiguousarray(unit) if rank == 0 else np.zeros((0, dim), np.float32)
    c2, _, it2 = comm.kmeans(api.PGV_OPS_IP, api.PGV_F32, dim, part, k, api.make_rng(seed=3))
    np.testing.assert_allclose(np.linalg.norm(c2.astype(np.float64), axis=1), 1.0, rtol=1e-5)

    # exact data: the sharded run IS the single-rank run, whatever the shards look like
    exact = km.exact_rows(4501, 8, seed=601)
    exact_shards_equal_single(ctx, comm, rank, [exact[:3001], exact[3001:]], 20, "uneven shards")
    exact_shards_equal_single(ctx, comm, rank, [exact, exact[:0]], 20, "rank 1 without samples")
    # a leading shard of 300 copies of one row, which the scripted stream picks first: its total is 0 from then on
    dup = np.ascontiguousarray(np.tile(exact[4000:4001], (300, 1)))
    exact_shards_equal_single(ctx, comm, rank, [dup, exact[:1500]], 12, "leading shard with total 0",
                              script=(5, [0.31, 0.77, 0.05, 0.93, 0.5, 0.18, 0.64, 0.999, 0.42, 0.26, 0.85]))
    # more lists than distinct rows: every weight reaches 0 and the reference's walk ends on global sample 0 -- a
    # rank ends the walk because it holds a sample, not because it holds weight, and an empty last rank never does
    few = np.ascontiguousarray(np.tile(km.exact_rows(12, 8, seed=511), (25, 1)))
    exact_shards_equal_single(ctx, comm, rank, [few[:200], few[200:]], 40, "k > distinct rows")
    exact_shards_equal_single(ctx, comm, rank, [few, few[:0]], 40, "k > distinct rows, rank 1 without samples")
    # a draw of 0.0 while the leading shard holds samples but no weight: the walk ends on ITS first sample (a copy of
    # a center, refilled later), not on the first sample that has weight -- which would be a new row of the next rank
    exact_shards_equal_single(ctx, comm, rank, [dup, exact[:1500]], 12, "a draw of 0.0 over a shard with total 0",
                              script=(5, [0.31, 0.0, 0.77, 0.0, 0.5]))

    # list scan: lists sharded l % world, same answers as the unsharded index
    lists, _ = api.assign(ctx, api.PGV_L2SQ, api.PGV_F32, dim, single, data)
    order = np.argsort(lists, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(lists, minlength=k))]).astype(np.int64)
    tids = order.astype(np.uint64)
    whole = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, dim, single, off, data[order], tids)
    own = (lists[order] % world) == rank
    lens = np.where(np.arange(k) % world == rank, np.diff(off), 0)
    loff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    local = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, dim, single, loff, np.ascontiguousarray(data[order][own]),
                         np.ascontiguousarray(tids[own]))
    queries = (means[rng.integers(0, k, 37)] + 0.05 * rng.standard_normal((37, dim))).astype(np.float32)
    for probes in (1, 4, k):
        gd, gt = comm.search_batch(local, queries, probes, 10)
        wd, _, wt = whole.search_batch(queries, probes, 10, want_tid=True)
        np.testing.assert_allclose(gd, wd, rtol=1e-6)
        for i in range(len(queries)):
            assert sorted(gt[i].tolist()) == sorted(wt[i].tolist()), (probes, i)
    whole.close()
    local.close()
    comm.close()
    ctx.close()
    dist.barrier()
    if rank == 0:
        print("COMM-OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
