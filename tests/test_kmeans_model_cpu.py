"""The host model of the k-means build (tests/kmeans_model.py) against the oracle, and the conditions its data builders
promise -- the GPU edge tests (test_gpu_kmeans_edges.py) lean on both.  No GPU here."""
import math

import numpy as np
import pytest

import kmeans_model as km
from oracle import pyoracle as po


def _oracle_stream(oracle, seed, n, k):
    """what InitCenters draws from pg_prng(seed): RandomInt() % n, then k - 1 RandomDouble()"""
    st = oracle.prng(seed)
    first = oracle.lib.ora_prng_u32(st) % n
    return first, [oracle.lib.ora_prng_double(st) for _ in range(k - 1)]


def _model_centers(oracle, samples, k, seed, spherical=False):
    first, draws = _oracle_stream(oracle, seed, samples.shape[0], k)
    picked, _, _ = km.init_centers(samples, k, first, draws, spherical)
    return samples[picked], picked


@pytest.mark.parametrize("n,k", [(70001, 24), (1, 1), (1, 3), (255, 9), (256, 9), (257, 9)])
def test_init_centers_is_the_oracles_on_integer_data(oracle, n, k):
    """the model's walk, fed the oracle's own stream, picks what ora_kmeans_init_centers picks (n = 70 001: 274 blocks,
    two batches of the block walk)"""
    samples = km.exact_rows(n, 8, seed=500 + n)
    got, _ = _model_centers(oracle, samples, k, 17)
    want = oracle.kmeans_init_centers(po.OPS_L2, po.ORA_F32, samples, k, oracle.prng(17))
    np.testing.assert_array_equal(got, want)


def test_init_centers_more_centers_than_distinct_rows(oracle):
    """12 distinct rows, k = 40: once every row is a center all weights are 0, the total is 0 and the walk ends at
    sample 0 (0 - 0 <= 0) whatever the draw"""
    samples = np.ascontiguousarray(np.tile(km.exact_rows(12, 8, seed=511), (25, 1)))
    got, picked = _model_centers(oracle, samples, 40, 23)
    want = oracle.kmeans_init_centers(po.OPS_L2, po.ORA_F32, samples, 40, oracle.prng(23))
    np.testing.assert_array_equal(got, want)
    assert np.unique(got, axis=0).shape[0] == 12
    exhausted = int(np.flatnonzero([np.unique(samples[picked[:i]], axis=0).shape[0] == 12 for i in range(41)])[0])
    assert exhausted < 40 and (picked[exhausted:] == 0).all()


@pytest.mark.parametrize("ops", [po.OPS_IP, po.OPS_COSINE])
def test_init_centers_is_the_oracles_on_the_unit_lattice(oracle, ops):
    samples = km.unit_lattice(1200, 16, seed=351)
    got, _ = _model_centers(oracle, samples, 30, 77, spherical=True)
    want = oracle.kmeans_init_centers(ops, po.ORA_F32, samples, 30, oracle.prng(77))
    np.testing.assert_array_equal(got, want)


def test_draw_for_hits_every_kind_of_target():
    """the scripted run of the GPU test: each aimed draw exists, its product with the total is exactly the running sum
    at the target, and the model's walk ends there"""
    samples, first, draws, targets = km.kmpp_script()
    n = samples.shape[0]
    picked, weights, used = km.init_centers(samples, len(targets) + 1, first, draws)
    assert picked.tolist() == [first] + targets
    head, length = km.KMPP_RUN
    assert targets[:2] == [255, 65536] and targets[5:] == [0, n - 1] and used[5] == 0.0
    for i, (t, u) in enumerate(zip(targets, used)):
        run = km.running_sums(weights[i])
        assert 0.0 <= u < 1.0
        if t not in (0, n - 1):
            assert run[-1] * u == run[t] and (t == 0 or run[t - 1] < run[t]), (i, t)   # exactly 0 left, first at t
    # the zero run: in place from the round after its head was picked, >= 300 long, across two block edges
    assert (weights[3][head:head + length] == 0).all() and length >= 300 and weights[3][head - 1] > 0
    assert (weights[4][head:head + length] == 0).all() and weights[4][head + length] > 0
    assert head // km.BLOCK < (head + length) // km.BLOCK - 1
    # the fall-through really passes sample n - 2
    assert km.running_sums(weights[6])[-1] * used[6] > km.running_sums(weights[6])[n - 2]
    # every weight and every total is an integer below 2^53: exact in every association
    assert (weights[:, :] == np.floor(weights)).all() and float(km.running_sums(weights[0])[-1]) < 2.0 ** 53


def test_draw_for_refuses_what_the_walk_cannot_do():
    w = np.array([4, 0, 0, 3, 5], dtype=np.float32)
    assert km.draw_for(w, 1) is None and km.draw_for(w, 2) is None      # the walk already ended at sample 0
    for t in (0, 3):
        u = km.draw_for(w, t)
        assert u is not None and km.walk(w, float(w.sum()) * u) == t
    assert km.walk(w, 0.0) == 0 and km.walk(w, 11.9) == 4 and km.walk(w, 12.0) == 4
    assert km.draw_for(np.zeros(5, np.float32), 2) is None and km.walk(np.zeros(5, np.float32), 0.0) == 0


def test_exact_builders_keep_their_bounds():
    x = km.exact_rows(5000, 8, seed=1)
    assert np.unique(x, axis=0).shape[0] == 5000
    d = ((x[:200, None, :].astype(np.float64) - x[None, :200, :]) ** 2).sum(-1)
    assert d.max() < km.EXACT and x.sum(axis=0).max() < km.EXACT
    for k in (1, 63, 64, 1024, 1025, 2049):
        empty = tuple(c for c in (0, 1023, 1024, k - 1) if 0 <= c < k) if k > 1 else ()
        s, c, labels = km.forced_step(k, 4 * k + 37, 8, empty=empty, seed=k)
        assert (np.abs(s) == np.floor(np.abs(s))).all() and not set(labels.tolist()) & set(empty)
        sums = np.zeros((k, 8))
        np.add.at(sums, labels, s.astype(np.float64))
        assert sums.max() < km.EXACT
        far = ((s[:64, None, :].astype(np.float64) - c[None, :, :]) ** 2).sum(-1)
        assert far.max() < km.EXACT
        np.testing.assert_array_equal(far.argmin(1), labels[:64])
    for dim in (1, 3, 100, 1028, 2000, 2056, 4000):
        s, c, labels = km.forced_step(5, 57, dim, seed=dim)
        far = ((s[:, None, :].astype(np.float64) - c[None, :, :]) ** 2).sum(-1)
        assert far.max() < km.EXACT and float(s.max()) < 2048          # exact in fp16 as well
        np.testing.assert_array_equal(far.argmin(1), labels)


def test_long_chain_is_order_sensitive():
    x = km.long_chain()
    assert x.shape[0] >= 50000 and x.dtype == np.float32 and (x != np.floor(x)).all()
    seq = km.sequential_sum(x)
    acc = np.zeros(x.shape[1], dtype=np.float32)
    for row in x[:2000]:
        acc += row
    np.testing.assert_array_equal(km.sequential_sum(x[:2000]), acc)      # the accumulate really is one add at a time
    assert (seq != km.pairwise_sum(x)).all() and (seq != km.sequential_sum(x[::-1])).all()


@pytest.mark.parametrize("k", sorted(km.WHOLE_RUNS))
def test_separated_sets_leave_no_close_call(oracle, k):
    """the whole-run sets: the smallest relative gap between best and second-best distance over all iterations is
    >= 1e-3, four orders above fp32 rounding of these distances, so every correct argmin agrees with the model's.

    The reference's own Elkan run from the same stream reaches the same closest and centers: the bounds only skip
    distance computations whose outcome they prove, and with gaps this wide no fp32 bound is on the edge."""
    samples, stream = km.whole_run_samples(k)
    d = ((samples[:300, None, :].astype(np.float64) - samples[None, :300, :]) ** 2).sum(-1)
    assert d.max() < km.EXACT and samples.max() < 2048
    centers, closest, iterations, gaps = km.lloyd_model(oracle, po.OPS_L2, po.ORA_F32, samples, k, stream)
    print("k = %d: %d iterations, smallest gap %.6f" % (k, iterations, min(gaps)))
    assert min(gaps) >= km.GAP_FLOOR and 2 <= iterations < 500
    ec, ecl, eit = oracle.kmeans(po.OPS_L2, po.ORA_F32, samples, k, oracle.prng(stream))
    np.testing.assert_array_equal(ecl, closest)
    np.testing.assert_array_equal(ec, centers)
    assert eit == iterations
    if k == 80:
        h16 = samples.astype(np.float16)
        np.testing.assert_array_equal(h16.astype(np.float32), samples)
        _, _, it16, gaps16 = km.lloyd_model(oracle, po.OPS_L2, po.ORA_F16, h16, k, stream)
        print("k = %d fp16: %d iterations, smallest gap %.6f" % (k, it16, min(gaps16)))
        assert min(gaps16) >= km.GAP_FLOOR


def test_lattice_whole_run_gap(oracle):
    """the spherical whole run: a lattice in clusters, inner products exact, the same gap condition as the L2 sets"""
    k, per, seed, stream = km.LATTICE_RUN
    samples = km.clustered_lattice(k, per, seed)
    np.testing.assert_array_equal(np.abs(samples).sum(axis=1), 2.0)
    ip = samples @ samples.T
    np.testing.assert_array_equal(ip * 4, np.round(ip * 4))
    _, _, iterations, gaps = km.lloyd_model(oracle, po.OPS_IP, po.ORA_F32, samples, k, stream)
    print("lattice: %d iterations, smallest gap %.6f" % (iterations, min(gaps)))
    assert min(gaps) >= km.GAP_FLOOR


def test_draw_for_hits_the_lattice_boundaries():
    """the spherical weights (acos(ip) / pi)^2 are not integers, but few and close in exponent: their double running
    sums are exact (equal to math.fsum's correctly rounded sum of the same terms), and the aimed draws exist"""
    samples = km.unit_lattice(1200, 16, seed=351)
    targets = km.LATTICE_TARGETS
    picked, weights, used = km.init_centers(samples, len(targets) + 1, 600, [km.aim(t) for t in targets], spherical=True)
    assert picked.tolist() == [600] + targets
    for w in weights:
        run = km.running_sums(w)
        for cut in (256, 512, 1200):
            assert run[cut - 1] == math.fsum(w[:cut].astype(np.float64).tolist())


def test_iterating_set_moves_members_for_several_iterations(oracle):
    """the whole-run set that its first step does not settle: at least 4 iterations, members changing center after
    the first, and still no close call; the k-means++ weights stay exact"""
    samples, stream = km.whole_run_samples("iterating")
    k = km.ITERATING_RUN[0]
    d = ((samples[:, None, :].astype(np.float64) - samples[None, :, :]) ** 2).sum(-1)
    assert d.max() < km.EXACT
    _, closest, iterations, gaps = km.lloyd_model(oracle, po.OPS_L2, po.ORA_F32, samples, k, stream)
    print("iterating: %d iterations, smallest gap %.6f" % (iterations, min(gaps)))
    assert iterations >= 4 and min(gaps) >= km.GAP_FLOOR
    first, _ = oracle.lloyd_assign(po.OPS_L2, po.ORA_F32, samples,
                                   oracle.kmeans_init_centers(po.OPS_L2, po.ORA_F32, samples, k, oracle.prng(stream)))
    assert (first != closest).sum() > 0
