"""The k-means build kernels (kernels_kmeans.hip, driven by pgv_abi_build.hip / pgv_abi_comm.hip) pinned bit for bit to
the reference's algorithm at their edges: the k-means++ walk across blocks and batches of blocks and exactly on their
boundaries, the offsets carry, the member compaction, the sample-order sums, the finish step's clamp, rounding and
refill draws, the spherical renormalisation and the three verdicts of CheckCenters.

The inputs come from tests/kmeans_model.py: integer data on which fp32 arithmetic is exact, so that any difference
from the oracle is a wrong index and never rounding, and one long non-integer chain on which only the reference's
order of additions gives the reference's bits.  test_kmeans_model_cpu.py checks the model and those conditions."""
import numpy as np
import pytest

import kmeans_model as km
from oracle import pyoracle as po
from pgvector_amd import api
from pgvector_amd._lib import PGV_ERR_DATA, PgvError

pytestmark = pytest.mark.gpu

DT = {po.ORA_F32: api.PGV_F32, po.ORA_F16: api.PGV_F16}
POPS = {po.OPS_L2: api.PGV_OPS_L2, po.OPS_IP: api.PGV_OPS_IP, po.OPS_COSINE: api.PGV_OPS_COSINE}
BOTH = [po.ORA_F32, po.ORA_F16]


def _as(x, dtype):
    return np.ascontiguousarray(np.asarray(x).astype(po.NP_OF[dtype]))


def _kmpp_vs_oracle(ctx, oracle, ops, dtype, samples, k, seed):
    rng, keep = km.oracle_rng(oracle, seed)
    got = api.kmeanspp_init(ctx, POPS[ops], DT[dtype], samples.shape[1], samples, k, rng)
    want = oracle.kmeans_init_centers(ops, dtype, samples, k, oracle.prng(seed))
    np.testing.assert_array_equal(got, want)
    return got


# ------------------------------------------------------------------------------------------ k-means++
def test_kmpp_oracle_stream_over_two_batches_of_blocks(ctx, oracle):
    """n = 70 001: 274 block sums, so the total and the block walk both take a second batch of 256"""
    samples = km.exact_rows(70001, 8, seed=500 + 70001)
    _kmpp_vs_oracle(ctx, oracle, po.OPS_L2, po.ORA_F32, samples, 24, 17)


@pytest.fixture(scope="module")
def script():
    samples, first, draws, targets = km.kmpp_script()
    picked, _, used = km.init_centers(samples, len(targets) + 1, first, draws)
    assert picked.tolist() == [first] + targets
    return samples, first, used, targets


@pytest.mark.parametrize("dtype", BOTH)
def test_kmpp_scripted_draws_land_on_their_targets(ctx, script, dtype):
    """n = 131 073, the walk aimed to end with exactly 0 left at: the last sample of block 0, the first sample of
    block 256 (the first entry of the walk's second batch: the f == 0 carry), the head of a 400-row duplicate run,
    the sample before that run (a `< 0` walk would cross 400 zero weights), the sample after it, sample 0 by a draw of
    0.0, and the fall-through n - 1 (alone in block 512).  Rows are distinct, so a center names its sample."""
    samples, first, used, targets = script
    rng = km.ScriptedRng(first, used)
    got = api.kmeanspp_init(ctx, api.PGV_OPS_L2, DT[dtype], 8, _as(samples, dtype), len(targets) + 1, rng.rng)
    assert (rng.u32_calls, rng.left, rng.overrun) == (1, 0, 0)
    want = samples[[first] + targets]
    for i in range(len(want)):
        hit = np.flatnonzero((samples == got[i].astype(np.float32)).all(axis=1))
        assert (got[i].astype(np.float32) == want[i]).all(), \
            "center %d: wanted sample %d, got sample(s) %s" % (i, ([first] + targets)[i], hit[:3].tolist())


@pytest.mark.parametrize("n,k", [(1, 1), (1, 3), (255, 9), (256, 9), (257, 9), (65537, 6)])
def test_kmpp_small_and_ragged_sizes(ctx, oracle, n, k):
    """one sample; one block less one, exactly one, one more; one batch of blocks plus one sample"""
    _kmpp_vs_oracle(ctx, oracle, po.OPS_L2, po.ORA_F32, km.exact_rows(n, 8, seed=500 + n), k, 17)


def test_kmpp_more_centers_than_distinct_rows(ctx, oracle):
    """k = 40 over 12 distinct rows: all weights reach 0, the total is 0, and every later pick is sample 0"""
    samples = np.ascontiguousarray(np.tile(km.exact_rows(12, 8, seed=511), (25, 1)))
    got = _kmpp_vs_oracle(ctx, oracle, po.OPS_L2, po.ORA_F32, samples, 40, 23)
    seen = [np.unique(got[:i], axis=0).shape[0] for i in range(41)]
    exhausted = seen.index(12)
    assert exhausted < 40
    np.testing.assert_array_equal(got[exhausted:], np.tile(samples[0], (40 - exhausted, 1)))


@pytest.mark.parametrize("ops", [po.OPS_IP, po.OPS_COSINE])
def test_kmpp_spherical_lattice_on_its_boundaries(ctx, oracle, ops):
    """the unit lattice: inner products exact, the weights (acos(ip) / pi)^2 few enough distinct values that their
    double sums are exact too; the oracle's stream, then draws aimed at block edges"""
    samples = km.unit_lattice(1200, 16, seed=351)
    _kmpp_vs_oracle(ctx, oracle, ops, po.ORA_F32, samples, 30, 77)
    targets, first = km.LATTICE_TARGETS, 600
    picked, _, used = km.init_centers(samples, len(targets) + 1, first, [km.aim(t) for t in targets], spherical=True)
    assert picked.tolist() == [first] + targets
    rng = km.ScriptedRng(first, used)
    got = api.kmeanspp_init(ctx, POPS[ops], api.PGV_F32, 16, samples, len(targets) + 1, rng.rng)
    assert (rng.u32_calls, rng.left, rng.overrun) == (1, 0, 0)
    np.testing.assert_array_equal(got, samples[picked])


@pytest.mark.parametrize("dim", [3, 2000])
def test_kmpp_row_copy_of_one_and_of_500_vectors(ctx, oracle, dim):
    samples = km.exact_rows(700, dim, seed=520 + dim, high=64, distinct=False)
    _kmpp_vs_oracle(ctx, oracle, po.OPS_L2, po.ORA_F32, samples, 6, 29)


# ------------------------------------------------------------------------------------------ one Lloyd step
def _exact_sums(samples, closest, k):
    """per-cluster sums of exact data: below 2^24 every order of additions gives these bits"""
    sums = np.zeros((k, samples.shape[1]), dtype=np.float64)
    np.add.at(sums, closest, np.asarray(samples).astype(np.float64))
    assert np.abs(sums).max() < km.EXACT
    return sums.astype(np.float32)


def _step(ctx, oracle, ops, dtype, samples, centers, want_sums=None):
    """lloyd_partial from closest = -1, checked against the oracle's assignment -> (closest, sums, counts)"""
    samples, centers = _as(samples, dtype), _as(centers, dtype)
    n, dim = samples.shape
    k = centers.shape[0]
    closest = np.full(n, -1, dtype=np.int32)
    sums, counts, changes = api.lloyd_partial(ctx, POPS[ops], DT[dtype], dim, samples, centers, closest)
    want, _ = oracle.lloyd_assign(ops, dtype, samples, centers)
    np.testing.assert_array_equal(closest, want)
    np.testing.assert_array_equal(counts, np.bincount(want, minlength=k))
    assert int(changes[0]) == n
    np.testing.assert_array_equal(sums, _exact_sums(samples, want, k) if want_sums is None else want_sums)
    return closest, sums, counts


def _finish_vs_oracle(ctx, oracle, ops, dtype, samples, closest, sums, counts, seed=41):
    """lloyd_finish on the oracle's stream against ComputeNewCenters on the same stream"""
    samples = _as(samples, dtype)
    k = counts.shape[0]
    rng, keep = km.oracle_rng(oracle, seed)
    got = api.lloyd_finish(ctx, POPS[ops], DT[dtype], samples.shape[1], sums, counts, rng)
    want, want_counts = oracle.kmeans_compute_new_centers(ops, dtype, samples, closest, k, oracle.prng(seed))
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(got.view(np.uint16 if dtype == po.ORA_F16 else np.uint32),
                                  want.view(np.uint16 if dtype == po.ORA_F16 else np.uint32))
    return got


@pytest.mark.parametrize("k", [1, 63, 64, 1024, 1025, 2049])
def test_lloyd_step_offsets_members_and_refill(ctx, oracle, k):
    """n = 4 k + 37 (never a multiple of 64), the assignment forced, clusters 0, 1023, 1024 and k - 1 empty where they
    exist: the offsets carry over 1024-wide chunks, the compaction's ballot edges, and the refill draws in center
    order -- dim draws per empty cluster -- from a scripted and from the oracle's stream"""
    n, dim = 4 * k + 37, 8
    empty = sorted(set(c for c in (0, 1023, 1024, k - 1) if 0 <= c < k)) if k > 1 else []
    samples, centers, labels = km.forced_step(k, n, dim, empty=empty, seed=k)
    for dtype in BOTH:
        closest, sums, counts = _step(ctx, oracle, po.OPS_L2, dtype, samples, centers)
        np.testing.assert_array_equal(closest, labels)
        assert [c for c in range(k) if counts[c] == 0] == empty
        s16 = _as(samples, dtype)
        # nothing changes on a second call; exactly m change after m entries were spoilt
        again = closest.copy()
        sums2, counts2, changes = api.lloyd_partial(ctx, api.PGV_OPS_L2, DT[dtype], dim, s16, _as(centers, dtype), again)
        assert int(changes[0]) == 0
        np.testing.assert_array_equal(again, closest)
        np.testing.assert_array_equal(sums2, sums)
        if k > 1:
            spoilt = closest.copy()
            where = np.array([0, 63, 64, n // 2, n - 1])
            spoilt[where] = (spoilt[where] + 1) % k
            _, counts3, changes = api.lloyd_partial(ctx, api.PGV_OPS_L2, DT[dtype], dim, s16, _as(centers, dtype), spoilt)
            assert int(changes[0]) == len(where)
            np.testing.assert_array_equal(spoilt, closest)
            np.testing.assert_array_equal(counts3, counts)
        _finish_vs_oracle(ctx, oracle, po.OPS_L2, dtype, samples, closest, sums, counts)
        # scripted refill: draw i goes to dimension i % dim of the (i // dim)-th empty cluster
        draws = (np.arange(len(empty) * dim) + 1.0) / (len(empty) * dim + 2.0)
        rng = km.ScriptedRng(0, draws)
        got = api.lloyd_finish(ctx, api.PGV_OPS_L2, DT[dtype], dim, sums, counts, rng.rng)
        assert (rng.u32_calls, rng.left, rng.overrun) == (0, 0, 0)
        want = draws.astype(np.float32).reshape(len(empty), dim).astype(po.NP_OF[dtype])
        np.testing.assert_array_equal(got[empty], want)


@pytest.mark.parametrize("dtype", BOTH)
def test_lloyd_step_long_chain_in_sample_order(ctx, oracle, dtype):
    """all 60 037 non-integer rows in cluster 0 of 2: the fp32 sums must be the sequential ones -- the pairwise and
    the reversed sum differ in every column (kmeans_model.long_chain asserts it) -- and cluster 1 is refilled"""
    rows = _as(km.long_chain(), dtype)
    centers = np.array([[0.75] * 3, [1000.0] * 3], dtype=np.float32)
    want_sums = np.stack([km.sequential_sum(rows.astype(np.float32)), np.zeros(3, np.float32)])
    if dtype == po.ORA_F32:
        assert (want_sums[0] != km.pairwise_sum(rows)).all()
    closest, sums, counts = _step(ctx, oracle, po.OPS_L2, dtype, rows, centers, want_sums=want_sums)
    assert counts.tolist() == [rows.shape[0], 0]
    _finish_vs_oracle(ctx, oracle, po.OPS_L2, dtype, rows, closest, sums, counts)


@pytest.mark.parametrize("dtype,dim", [(po.ORA_F32, 1), (po.ORA_F32, 3), (po.ORA_F32, 100), (po.ORA_F32, 1028),
                                       (po.ORA_F32, 2000), (po.ORA_F16, 2056), (po.ORA_F16, 4000)])
def test_lloyd_step_padded_tails_and_second_sum_block(ctx, oracle, dtype, dim):
    """dims 1, 3, 100: the padded tail of the last 16-byte vector; fp32 dim > 1024 and fp16 dim > 2048: more than 256
    vectors per row, so center_sums_kernel runs a second block along the row"""
    samples, centers, labels = km.forced_step(5, 57, dim, seed=dim)
    closest, sums, counts = _step(ctx, oracle, po.OPS_L2, dtype, samples, centers)
    np.testing.assert_array_equal(closest, labels)
    _finish_vs_oracle(ctx, oracle, po.OPS_L2, dtype, samples, closest, sums, counts)


def test_lloyd_finish_clamps_infinite_sums(ctx, oracle):
    """two rows of +-3e38 in one cluster: the fp32 sum is +-inf, clamped to +-FLT_MAX before the division
    (src/ivfkmeans.c:212-216) -> +-FLT_MAX / 2"""
    rows = np.array([[3e38, -3e38], [3e38, -3e38], [1, 1]], dtype=np.float32)
    centers = np.array([[3e38, -3e38], [0, 0]], dtype=np.float32)
    closest = np.full(3, -1, dtype=np.int32)
    sums, counts, _ = api.lloyd_partial(ctx, api.PGV_OPS_L2, api.PGV_F32, 2, rows, centers, closest)
    assert closest.tolist() == [0, 0, 1] and counts.tolist() == [2, 1]
    assert np.isposinf(sums[0, 0]) and np.isneginf(sums[0, 1])
    got = _finish_vs_oracle(ctx, oracle, po.OPS_L2, po.ORA_F32, rows, closest, sums, counts)
    np.testing.assert_array_equal(got[0], np.array([km.FLT_MAX, -km.FLT_MAX]) / np.float32(2))


def _ulp_close(got, want64, dtype, what):
    """within 1 ulp of the center's type of the float64 value correctly rounded: the kernel's double norm moves the
    quotient by far less than half an fp32 ulp, so only a flipped final rounding can differ"""
    t = po.NP_OF[dtype]
    want = want64.astype(t)
    ulp = np.spacing(np.abs(want).astype(t)).astype(np.float64)
    bad = np.abs(got.astype(np.float64) - want.astype(np.float64)) > ulp
    assert not bad.any(), (what, np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def _normalised64(raw):
    raw = raw.astype(np.float64)
    norm = np.sqrt((raw * raw).sum(axis=1, keepdims=True))
    return np.where(norm > 0, raw / np.where(norm > 0, norm, 1.0), raw)


@pytest.mark.parametrize("ops", [po.OPS_IP, po.OPS_COSINE])
@pytest.mark.parametrize("dtype", BOTH)
def test_lloyd_step_spherical_finish(ctx, oracle, ops, dtype):
    """the clustered lattice under the spherical distance: exact assignment; centers = the L2 finish normalised, within
    1 ulp; a cluster whose rows sum to zero stays zero; a refilled row ends at unit norm"""
    k, per, seed, _ = km.LATTICE_RUN
    samples = km.clustered_lattice(k, per, seed)
    dim = samples.shape[1]
    firsts = [int(np.flatnonzero(np.abs(samples[:, 6 * c:6 * c + 6]).sum(axis=1) > 0)[0]) for c in range(k)]
    centers = np.concatenate([samples[firsts], -samples[firsts[:1]]])          # the last center attracts nobody
    closest, sums, counts = _step(ctx, oracle, ops, dtype, samples, centers)
    assert counts[k] == 0 and (counts[:k] == per).all()
    sums = sums.copy()
    sums[3] = 0.0                                                             # +v and -v rows: the sum cancels
    draws = (np.arange(dim) + 1.0) / (dim + 2.0)
    rng = km.ScriptedRng(0, draws)
    got = api.lloyd_finish(ctx, POPS[ops], DT[dtype], dim, sums, counts, rng.rng)
    assert (rng.left, rng.overrun) == (0, 0)
    raw = (sums / np.maximum(counts, 1).astype(np.float32)[:, None]).astype(np.float32)
    raw[k] = draws.astype(np.float32)
    raw = raw.astype(po.NP_OF[dtype])                                          # UpdateCenter, then the norm function
    _ulp_close(got, _normalised64(raw), dtype, "spherical centers")
    assert (got[3] == 0).all()
    norms = np.linalg.norm(got.astype(np.float64), axis=1)
    np.testing.assert_allclose(np.delete(norms, 3), 1.0, rtol=2e-3 if dtype == po.ORA_F16 else 1e-6)
    # and the oracle's own normalisation is inside the same band
    want, _ = oracle.kmeans_compute_new_centers(ops, dtype, _as(samples, dtype), closest, k + 1, oracle.prng(5))
    keep = [c for c in range(k) if c != 3]
    _ulp_close(want[keep], _normalised64(raw[keep]), dtype, "oracle centers")


# ------------------------------------------------------------------------------------------ whole runs
def _run_twice(ctx, oracle, ops, dtype, samples, k, stream):
    samples = _as(samples, dtype)
    runs = []
    for _ in range(2):
        rng, keep = km.oracle_rng(oracle, stream)
        runs.append(api.kmeans(ctx, POPS[ops], DT[dtype], samples.shape[1], samples, k, rng))
    (c1, cl1, it1), (c2, cl2, it2) = runs
    assert c1.tobytes() == c2.tobytes() and cl1.tobytes() == cl2.tobytes() and it1 == it2
    return c1, cl1, it1


@pytest.mark.parametrize("k,dtype", [(12, po.ORA_F32), (80, po.ORA_F32), (1100, po.ORA_F32), (80, po.ORA_F16),
                                     ("iterating", po.ORA_F32), ("iterating", po.ORA_F16)])
def test_whole_run_is_the_models_on_separated_sets(ctx, oracle, k, dtype):
    """pgv_kmeans = k-means++ and plain Lloyd on one stream: centers, closest and the iteration count of the model,
    on sets where no assignment is a close call (gap >= 1e-3, test_kmeans_model_cpu.py).  k = 12: the per-query
    argmin; k = 80: the MFMA argmin; k = 1100: 1100 picks and the offsets carry; "iterating": k = 12 on clusters close
    enough that members change center for 5 iterations.  Twice, byte-identical."""
    samples, stream = km.whole_run_samples(k)
    k = km.ITERATING_RUN[0] if k == "iterating" else k
    want_c, want_cl, want_it, gaps = km.lloyd_model(oracle, po.OPS_L2, dtype, _as(samples, dtype), k, stream)
    assert min(gaps) >= km.GAP_FLOOR
    centers, closest, iters = _run_twice(ctx, oracle, po.OPS_L2, dtype, samples, k, stream)
    np.testing.assert_array_equal(closest, want_cl)
    np.testing.assert_array_equal(centers, want_c)
    assert iters == want_it


def test_whole_run_refills_on_the_stream_kmeanspp_drew_from(ctx, oracle):
    """k = 40 over 12 distinct rows: 28 centers duplicate others, lose every tie to the lower index and are refilled --
    dim draws each, in center order, after k-means++'s 39 draws on the same stream.  Every sample is at distance
    exactly 0 from its center, so no rounding decides anything"""
    samples = np.ascontiguousarray(np.tile(km.exact_rows(12, 8, seed=511), (25, 1)))
    want_c, want_cl, want_it, _ = km.lloyd_model(oracle, po.OPS_L2, po.ORA_F32, samples, 40, 23)
    centers, closest, iters = _run_twice(ctx, oracle, po.OPS_L2, po.ORA_F32, samples, 40, 23)
    assert np.unique(closest).size == 12
    np.testing.assert_array_equal(closest, want_cl)
    np.testing.assert_array_equal(centers, want_c)
    assert iters == want_it


def test_whole_run_spherical_lattice(ctx, oracle):
    k, per, seed, stream = km.LATTICE_RUN
    samples = km.clustered_lattice(k, per, seed)
    _, want_cl, want_it, gaps = km.lloyd_model(oracle, po.OPS_IP, po.ORA_F32, samples, k, stream)
    assert min(gaps) >= km.GAP_FLOOR
    centers, closest, iters = _run_twice(ctx, oracle, po.OPS_IP, po.ORA_F32, samples, k, stream)
    np.testing.assert_array_equal(closest, want_cl)
    assert iters == want_it
    raw, _ = oracle.kmeans_compute_new_centers(po.OPS_L2, po.ORA_F32, samples, want_cl, k, oracle.prng(1))
    _ulp_close(centers, _normalised64(raw), po.ORA_F32, "lattice centers")


def test_group_of_one_is_the_single_run_on_the_long_chain(ctx):
    """pgv_kmeans_sharded with one rank packs, all-reduces and unpacks its sums, counts and totals through RCCL: on
    the order-sensitive chain it must still give pgv_kmeans's bytes"""
    rows = km.long_chain()
    comm = api.Comm(ctx, backend="rccl")
    try:
        c1, cl1, it1 = api.kmeans(ctx, api.PGV_OPS_L2, api.PGV_F32, 3, rows, 3, api.make_rng(seed=4))
        c2, cl2, it2 = comm.kmeans(api.PGV_OPS_L2, api.PGV_F32, 3, rows, 3, api.make_rng(seed=4))
    finally:
        comm.close()
    assert c1.tobytes() == c2.tobytes() and cl1.tobytes() == cl2.tobytes() and it1 == it2


# ------------------------------------------------------------------------------------------ verdicts
def _still_answers(ctx, oracle):
    rows, centers = km.exact_rows(50, 8, seed=71), km.exact_rows(7, 8, seed=72)
    got, _ = api.assign(ctx, api.PGV_L2SQ, api.PGV_F32, 8, centers, rows)
    want, _ = oracle.assign(po.OPS_L2, po.ORA_F32, centers, rows)
    np.testing.assert_array_equal(got, want)


def _verdict(ctx, oracle, ops, dtype, samples, k, message):
    """CheckCenters (src/ivfkmeans.c:490-547): the reference's error text, where -- and only where -- the oracle's
    run fails; the context goes on working afterwards"""
    samples = _as(samples, dtype)
    ora_it = oracle.kmeans(ops, dtype, samples, k, oracle.prng(3))[2]
    rng, keep = km.oracle_rng(oracle, 3)
    if message is None:
        assert ora_it >= 1
        centers, closest, iters = api.kmeans(ctx, POPS[ops], DT[dtype], samples.shape[1], samples, k, rng)
        _still_answers(ctx, oracle)
        return centers, closest, iters
    assert ora_it == -1
    with pytest.raises(PgvError) as err:
        api.kmeans(ctx, POPS[ops], DT[dtype], samples.shape[1], samples, k, rng)
    assert err.value.code == PGV_ERR_DATA and err.value.message.startswith(message), err.value.message
    _still_answers(ctx, oracle)


def test_verdict_nan(ctx, oracle):
    samples = km.exact_rows(40, 4, seed=81)
    samples[17, 2] = np.nan
    _verdict(ctx, oracle, po.OPS_L2, po.ORA_F32, samples, 3, "NaN detected")


def test_verdict_infinite(ctx, oracle):
    """an fp16 row with an infinite element: its cluster's sum is inf, clamped to FLT_MAX, and FLT_MAX / count rounds
    to an infinite half"""
    samples = km.exact_rows(40, 4, seed=82)
    samples[11, 1] = np.inf
    _verdict(ctx, oracle, po.OPS_L2, po.ORA_F16, samples, 3, "Infinite value detected")


@pytest.mark.parametrize("dtype", BOTH)
def test_verdict_zero_norm_is_cosines_alone(ctx, oracle, dtype):
    """+v / -v pairs in the one cluster of k = 1: the center sums to zero and stays zero through the normalisation.
    CheckNorms runs for the opclass with a norm function, cosine; under inner product the same input builds"""
    v = np.array([[0.5, 0.5, -0.5, 0.5], [0.5, -0.5, 0.5, 0.5]], dtype=np.float32)
    samples = np.concatenate([v, -v, v, -v])
    _verdict(ctx, oracle, po.OPS_COSINE, dtype, samples, 1, "Zero norm detected")
    centers, closest, iters = _verdict(ctx, oracle, po.OPS_IP, dtype, samples, 1, None)
    assert (centers == 0).all() and (closest == 0).all() and iters == 2
    centers, _, _ = _verdict(ctx, oracle, po.OPS_L2, dtype, samples, 1, None)
    assert (centers == 0).all()
