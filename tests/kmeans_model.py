"""A host restatement of the IVFFlat build's k-means (pgvector_amd/csrc/kernels_kmeans.hip and its drivers), in numpy,
and the data the edge tests are built from.

init_centers restates the reference's k-means++ (src/ivfkmeans.c:23-91) step by step: fp32 weights that start at
FLT_MAX, the squared distance taken in double, the total summed in sample order in double, and the sequential walk
`choice -= weight[j]; if (choice <= 0) break` over samples 0 .. n - 2 with sample n - 1 as the fall-through.
draw_for turns that around: it finds the draw for which the walk lands exactly on a wanted sample, so a test can aim
at the last sample of a block, the first of the next, or a sample behind a run of zero weights.  lloyd_model is plain
Lloyd with the product's stopping rule, every step taken by the oracle (src/ivfkmeans.c:151-236,
src/ivfutils.c:301-361).  Nothing here imports the package except ScriptedRng and oracle_rng, which need its callback types.

The data builders make inputs on which fp32 arithmetic is exact (integers, sums below 2^24) -- there any association
gives the same bits, so a difference is a wrong index, a lost member or a dropped carry, never rounding -- and one
input on which it is not: a long chain whose fp32 sum depends on the order of its terms."""
import ctypes as C
import math

import numpy as np

from oracle import pyoracle as po

FLT_MAX = np.float32(3.4028234663852886e38)
BLOCK = 256                  # kernels_kmeans.hip kKmThreads: samples per weight block, blocks per walk batch
EXACT = float(1 << 24)       # integers up to here are exact in fp32


# ------------------------------------------------------------------------------------------ k-means++
def _raw(samples, center, spherical):
    """the fp32 kernel value of every sample against one center, accumulated over the dimensions in order: L2 squared,
    or the inner product (src/vector.c:560-575, :640-655; halfvec rows are widened to float first)"""
    s = np.asarray(samples).astype(np.float32)
    c = np.asarray(center).astype(np.float32)
    acc = np.zeros(s.shape[0], dtype=np.float32)
    for d in range(s.shape[1]):
        if spherical:
            acc += s[:, d] * c[d]
        else:
            diff = s[:, d] - c[d]
            acc += diff * diff
    return acc


def _distance(raw, spherical):
    """the k-means distance in double: sqrt((double) l2sq), or acos(clamp(ip)) / pi (src/vector.c:588, :705-722).
    acos through math.acos on the distinct values: numpy's own arccos need not be libm's"""
    raw = raw.astype(np.float64)
    if not spherical:
        return np.sqrt(raw)
    ip = np.clip(raw, -1.0, 1.0)
    uniq, inv = np.unique(ip, return_inverse=True)
    return np.array([math.acos(v) / math.pi for v in uniq], dtype=np.float64)[inv]


def running_sums(weights):
    """the double running sum of the fp32 weights in sample order; [-1] is the reference's `sum`"""
    return np.add.accumulate(np.asarray(weights, dtype=np.float32).astype(np.float64))


def walk(weights, choice):
    """the reference's walk: the first j in 0 .. n - 2 with choice - w[0] - ... - w[j] <= 0 (subtracted one at a time,
    in double), else n - 1"""
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    n = w.size
    if n == 1:
        return 0
    left = np.subtract.accumulate(np.concatenate([[choice], w[:n - 1]]))[1:]
    hit = np.flatnonzero(left <= 0)
    return int(hit[0]) if hit.size else n - 1


def init_centers(samples, k, first, draws, spherical=False):
    """-> (picked [k], weights after each round [k - 1 x n] fp32, the draws used).  `first` is RandomInt() % n, draws
    the k - 1 RandomDouble() values; a draw may be a function of the round's weights (see draw_for), resolved when its
    round comes.  A function that returns None fails the call: the caller asked for a target that cannot be hit."""
    samples = np.asarray(samples)
    n = samples.shape[0]
    weight = np.full(n, FLT_MAX, dtype=np.float32)
    picked = [int(first)]
    history, used = [], []
    for i in range(k - 1):
        distance = _distance(_raw(samples, samples[picked[i]], spherical), spherical)
        distance = distance * distance
        closer = distance < weight.astype(np.float64)
        weight = np.where(closer, distance.astype(np.float32), weight)
        history.append(weight.copy())
        draw = draws[i]
        if callable(draw):
            draw = draw(weight)
            assert draw is not None, "round %d: no draw reaches the target" % i
        used.append(float(draw))
        picked.append(walk(weight, running_sums(weight)[-1] * float(draw)))
    return np.array(picked, dtype=np.int64), np.array(history, dtype=np.float32).reshape(k - 1, n), used


def draw_for(weights, target):
    """a double u in [0, 1) for which fl(total * u) is exactly the running sum up to and including sample `target`, so
    the walk reaches 0 -- not below -- at `target`; None if no neighbour of the quotient gives that product or the walk
    would not end there (a zero-weight target behind an equal running sum).  target n - 1 is the fall-through: the
    largest u below 1, provided its product still exceeds the running sum up to n - 2."""
    run = running_sums(weights)
    total, n = float(run[-1]), run.size
    if target == n - 1:
        u = math.nextafter(1.0, 0.0)
        return u if (n == 1 or total * u > run[n - 2]) else None
    want = float(run[target])
    if not (total > 0) or not (want > 0):
        return None
    q = want / total
    for u in (q, math.nextafter(q, 0.0), math.nextafter(q, 1.0), math.nextafter(math.nextafter(q, 0.0), 0.0),
              math.nextafter(math.nextafter(q, 1.0), 1.0)):
        if 0.0 <= u < 1.0 and total * u == want and walk(weights, total * u) == target:
            return u
    return None


def aim(target):
    """a draw for init_centers that lands the walk exactly on `target`"""
    return lambda weights: draw_for(weights, target)


# ------------------------------------------------------------------------------------------ Lloyd
def relative_gap(samples, centers, spherical=False, chunk=4096):
    """the smallest (second best - best) / second best k-means distance over the samples, in float64"""
    s = np.asarray(samples).astype(np.float64)
    c = np.asarray(centers).astype(np.float64)
    if c.shape[0] < 2:
        return 1.0
    worst = np.inf
    for lo in range(0, s.shape[0], chunk):
        x = s[lo:lo + chunk]
        if spherical:
            d = np.arccos(np.clip(x @ c.T, -1.0, 1.0)) / np.pi
        else:
            d = np.sqrt(np.maximum((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T), 0.0))
        two = np.partition(d, 1, axis=1)[:, :2]
        gap = (two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)
        worst = min(worst, float(gap.min()))
    return worst


def lloyd_model(ora, ops, dtype, samples, k, seed, max_iterations=500):
    """k-means++ and plain Lloyd on one ora_prng stream -> (centers, closest, iterations, gaps): per iteration the
    oracle's exact assignment, then its ComputeNewCenters; it stops when an iteration other than the first changes
    nothing, that iteration's finish step still run (src/ivfkmeans.c:482-483).  gaps[i] is relative_gap under the
    centers iteration i assigned with."""
    samples = ora.arr(samples, dtype)
    spherical = ops in (po.OPS_IP, po.OPS_COSINE)
    rng = ora.prng(seed)
    centers = ora.kmeans_init_centers(ops, dtype, samples, k, rng)
    closest = np.full(samples.shape[0], -1, dtype=np.int32)
    gaps, iterations = [], 0
    for it in range(max_iterations):
        iterations = it + 1
        gaps.append(relative_gap(samples, centers, spherical))
        new, _ = ora.lloyd_assign(ops, dtype, samples, centers)
        changes = int((new != closest).sum())
        closest = new
        centers, _ = ora.kmeans_compute_new_centers(ops, dtype, samples, closest, k, rng)
        if changes == 0 and it != 0:
            break
    return centers, closest, iterations, gaps


# ------------------------------------------------------------------------------------------ a scripted pgv_rng
class ScriptedRng:
    """a pgv_rng that replays a list: one u32, then the doubles.  Keep the object alive for the whole call -- it owns
    the callback thunks the library calls through.  Running off the list is recorded, not raised (an exception cannot
    cross the C frame): check `overrun` and `left` afterwards."""

    def __init__(self, u32, doubles):
        from pgvector_amd import _lib, api
        self.doubles = [float(x) for x in doubles]
        self.at = 0
        self.u32_calls = 0
        self.overrun = 0

        def next_double(_state):
            if self.at >= len(self.doubles):
                self.overrun += 1
                return 0.5
            self.at += 1
            return self.doubles[self.at - 1]

        def next_u32(_state):
            self.u32_calls += 1
            return int(u32) & 0xffffffff
        self._cbs = (_lib.NEXT_DOUBLE(next_double), _lib.NEXT_U32(next_u32))
        self.rng = api.make_rng(next_double=self._cbs[0], next_u32=self._cbs[1])

    @property
    def left(self):
        return len(self.doubles) - self.at


def oracle_rng(ora, seed):
    """a pgv_rng that draws from the oracle's pg_prng stream -> (rng, the state to keep alive)"""
    from pgvector_amd import api
    st = ora.prng(seed)
    return api.make_rng(next_double=ora.lib.ora_prng_double_cb, next_u32=ora.lib.ora_prng_u32_cb,
                        state=C.cast(C.pointer(st), C.c_void_p)), st


# ------------------------------------------------------------------------------------------ data
def exact_rows(n, dim, seed, high=64, distinct=True):
    """(a) integer rows in [0, high): squared distances stay below 2^24, and so does any sum of up to
    2^24 / (high - 1) rows -- fp32 arithmetic on them is exact in every association.  distinct: no two rows equal, so
    a center names the sample it was copied from."""
    assert dim * (high - 1) ** 2 < EXACT
    rng = np.random.default_rng(seed)
    x = rng.integers(0, high, (n, dim)).astype(np.float32)
    if distinct:
        for _ in range(8):
            _, idx = np.unique(x, axis=0, return_index=True)
            if x.shape[0] == idx.size:
                break
            dup = np.setdiff1d(np.arange(n), idx)
            x[dup] = rng.integers(0, high, (dup.size, dim)).astype(np.float32)
        assert np.unique(x, axis=0).shape[0] == n
    return x


def with_duplicate_run(x, start, length):
    """rows start .. start + length - 1 all become row `start`: once it is a center their weights are 0"""
    x = x.copy()
    x[start:start + length] = x[start]
    return x


def forced_step(k, n, dim, empty=(), seed=0, spacing=32, jitter=4):
    """one Lloyd step whose assignment is forced -> (samples, centers, labels).  Center c sits at spacing x (c % 64,
    c // 64) in the first two dimensions (the first only when dim == 1) and at 0 elsewhere; sample j belongs to the
    j-th cluster of a shuffled round over the non-empty ones and sits at its center plus integers in [0, jitter) in
    every dimension.  The other dimensions add the same to every center's distance, so the labels hold whatever dim
    is, and every value is an integer small enough for exact fp32 sums and squared distances."""
    rng = np.random.default_rng(seed)
    centers = np.zeros((k, dim), dtype=np.float32)
    if dim == 1:
        centers[:, 0] = spacing * np.arange(k)
    else:
        centers[:, 0] = spacing * (np.arange(k) % 64)
        centers[:, 1] = spacing * (np.arange(k) // 64)
    alive = np.array([c for c in range(k) if c not in set(empty)], dtype=np.int64)
    assert alive.size > 0
    labels = alive[rng.permutation(n) % alive.size] if n >= alive.size else alive[:n]
    labels = labels[rng.permutation(n)]
    samples = centers[labels] + rng.integers(0, jitter, (n, dim)).astype(np.float32)
    assert float(np.abs(samples).max()) ** 2 * min(dim, 2) + dim * jitter ** 2 < EXACT
    assert float(samples.max()) * n < EXACT
    return samples, centers, labels.astype(np.int32)


def separated_clusters(k, per, dim, seed, spread=1, pitch=512):
    """(b) `per` integer points within `spread` of each of k integer cluster centres `pitch` apart on a grid over all
    dimensions, shuffled.  Every squared distance between two samples stays below 2^24 and every coordinate below
    2048, so the k-means++ weights are exact in fp32 and the rows are exact in fp16 as well; the centres a run
    computes are means and are not integers, which is what the gap condition of the whole-run tests is for."""
    rng = np.random.default_rng(seed)
    side = 2
    while side ** dim < k:
        side += 1
    assert dim * ((side - 1) * pitch + 2 * spread) ** 2 < EXACT and (side - 1) * pitch + 2 * spread < 2048
    cells = rng.permutation(side ** dim)[:k]
    centres = np.stack(np.unravel_index(cells, (side,) * dim), -1).astype(np.int64) * pitch
    x = np.repeat(centres, per, axis=0) + rng.integers(-spread, spread + 1, (k * per, dim))
    x = x[rng.permutation(x.shape[0])] + spread
    return np.ascontiguousarray(x.astype(np.float32))


def pairwise_sum(rows):
    """fp32 column sums the way numpy takes them along a contiguous axis: in pairs, not in row order"""
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float32).T).sum(axis=1, dtype=np.float32)


def sequential_sum(rows):
    """fp32 column sums in row order, one addition at a time: the chain SumCenters runs"""
    return np.add.accumulate(np.asarray(rows).astype(np.float32), axis=0, dtype=np.float32)[-1]


def long_chain(n=60037, dim=3, seed=0):
    """(c) non-integer fp32 rows in [0.25, 1.25) for one cluster: over >= 50 000 terms the sequential fp32 sum differs
    in bits from the pairwise sum numpy takes, and from the sum taken last to first -- asserted here"""
    assert n >= 50000
    x = (np.random.default_rng(seed).random((n, dim), dtype=np.float32) + np.float32(0.25)).astype(np.float32)
    seq = sequential_sum(x)
    assert (seq != pairwise_sum(x)).all(), "chain is not order-sensitive against the pairwise sum"
    assert (seq != sequential_sum(x[::-1])).all(), "chain is not order-sensitive against the reversed sum"
    return x


def unit_lattice(n, dim, seed):
    """unit vectors with four entries of +-0.5: every inner product is a multiple of 0.25, exact in fp32"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, dim), dtype=np.float32)
    for i in range(n):
        x[i, rng.choice(dim, 4, replace=False)] = rng.choice([-0.5, 0.5], 4)
    return x


# ------------------------------------------------------------------------------------------ shared scenarios
KMPP_SCRIPT_N = 131073       # 513 blocks: the block walk needs three batches of 256, the last block holds one sample
KMPP_RUN = (1000, 400)       # rows 1000 .. 1399 are one row: 400 zero weights once it is a center, over two block edges


def kmpp_script(n=KMPP_SCRIPT_N, dim=8, seed=1001):
    """the scripted k-means++ run of the edge tests -> (samples, first, draws, targets): after a first center in the
    middle, the walk is aimed exactly at the last sample of block 0, the first sample of block 256 (the first block of
    the second batch), the head of the duplicate run, the sample just before the run (a walk that does not stop at 0
    crosses all 400 zero weights), the first sample after it, sample 0 by a draw of 0.0, and the fall-through n - 1"""
    x = with_duplicate_run(exact_rows(n, dim, seed), *KMPP_RUN)
    head, length = KMPP_RUN
    targets = [BLOCK - 1, BLOCK * BLOCK, head, head - 1, head + length, 0, n - 1]
    draws = [aim(t) for t in targets]
    draws[5] = 0.0
    return x, 70000, draws, targets


# (k, points per cluster, data seed, stream seed): seeds for which every iteration's gap is >= GAP_FLOOR, asserted in
# test_kmeans_model_cpu.py.  k = 12 takes the per-query argmin, k = 80 the MFMA argmin, k = 1100 the offsets carry.
GAP_FLOOR = 1e-3
WHOLE_RUNS = {12: (12, 30, 2101, 31), 80: (80, 30, 2102, 32), 1100: (1100, 30, 2103, 33)}


# a set that is NOT settled by its first step: clusters of radius 8 only 32 apart, so k-means++ doubles up in some and
# Lloyd moves members between centers for several iterations (5 here) while no assignment is a close call
ITERATING_RUN = (12, 30, 4030, 100, 8, 32)   # k, per, data seed, stream seed, spread, pitch


def whole_run_samples(k):
    """-> (samples, stream seed); k = "iterating" names ITERATING_RUN"""
    if k == "iterating":
        kk, per, seed, stream, spread, pitch = ITERATING_RUN
        return separated_clusters(kk, per, 8, seed, spread=spread, pitch=pitch), stream
    kk, per, seed, stream = WHOLE_RUNS[k]
    return separated_clusters(kk, per, 8, seed), stream


def clustered_lattice(k, per, seed):
    """unit_lattice's kind of rows (four entries of +-0.5, every inner product a multiple of 0.25) in k clusters: cluster
    c owns dimensions 6c .. 6c + 5 and a sign for each, a member uses four of the six.  Members of one cluster share
    at least two dimensions (inner product >= 0.5), members of different clusters none (0) -> dim = 6 k"""
    rng = np.random.default_rng(seed)
    x = np.zeros((k * per, 6 * k), dtype=np.float32)
    signs = rng.choice([-0.5, 0.5], (k, 6)).astype(np.float32)
    for i in range(k * per):
        c = i % k
        use = rng.choice(6, 4, replace=False)
        x[i, 6 * c + use] = signs[c, use]
    return x[rng.permutation(k * per)]


# the spherical whole run: (k, members per cluster, data seed, stream seed) of a clustered_lattice, chosen like WHOLE_RUNS
LATTICE_RUN = (10, 40, 3002, 42)

# boundary targets on unit_lattice(1200, 16, 351) from first = 600: last sample of block 0, first of block 1, last of
# block 3, the fall-through; test_kmeans_model_cpu.py checks that draw_for reaches each
LATTICE_TARGETS = [255, 256, 1023, 1199]
