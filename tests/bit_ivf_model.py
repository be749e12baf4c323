"""numpy model of IVFFlat over bit strings (`USING ivfflat (col bit_hamming_ops)`), written from the reference's text on
top of tests/bit_model.py: what tests/test_gpu_bit_ivf.py compares the device against, itself pinned by
tests/test_bit_ivf_model_cpu.py.

Scan side (src/ivfscan.c)
  rank_lists    GetScanLists (:47-118): ascending by (distance, list id) -- the set at the boundary is the reference's
                (its strict `<` at :92 admits no later list at an equal distance), the order among equal distances is
                the library's rule
  scan_stream   GetScanItems (:123-187): the probed lists in probe order, rows in row order; a NULL query scores 0
  scan_head     the head of the sorted stream: ascending by (distance, insertion position), +inf / -1 padded
Build side (src/ivfkmeans.c, src/ivfutils.c, src/ivfbuild.c)
  assign        AddTupleToSort's argmin (src/ivfbuild.c:183-192): the first strictly-smallest center
  init_centers  InitCenters (:23-91) with hamming_distance
  update_centers  ComputeNewCenters + BitSumCenter + BitUpdateCenter
  kmeans_sticky   the loop the library runs; kmeans_elkan is the literal transcription of :246-485 that pins it, and
                  kmeans_fresh the deliberately WRONG loop (lowest-index argmin every iteration) that shows the test
                  shapes tell the two apart
Every generator is an object with next_double() / next_u32(); ModelRng is one, and hands the same stream to the library
as C callbacks (pgv_rng)."""
import random

import numpy as np

import bit_model as bm

FLT_MAX = np.float32(3.4028234663852886e+38)
# (n, nbits, k): the shapes on which the sticky loop is pinned to the Elkan transcription and the device to the sticky loop
KMEANS_SHAPES = [(300, 16, 8), (300, 13, 8), (500, 52, 20), (200, 8, 16), (64, 3, 5), (400, 130, 7), (257, 40, 33)]


def kmeans_case(n, nbits, k):
    """-> (samples, the seed of the case's generator)"""
    return rand_bits(n, nbits, 1000 * n + nbits), 7 * k + nbits


def rand_bits(n, nbits, seed):
    """n packed bit strings of nbits (first bit in the top bit of byte 0, pad bits zero, as PostgreSQL keeps them)"""
    rng = np.random.default_rng(seed)
    return np.packbits(rng.integers(0, 2, (n, nbits), dtype=np.uint8), axis=1)


def hamming_matrix(a, b, chunk=1 << 22):
    """[len(a) x len(b)] int64 Hamming distances of packed rows (bit_model.hamming's table, a block of rows at a time)"""
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.int64)
    step = max(1, chunk // max(1, b.shape[0] * max(1, b.shape[1])))
    for lo in range(0, a.shape[0], step):
        out[lo:lo + step] = bm.POPCOUNT[a[lo:lo + step, None, :] ^ b[None, :, :]].sum(axis=2)
    return out


class ModelRng:
    """a deterministic stream with the two draws the reference makes (RandomDouble, RandomInt) and a count of each"""

    def __init__(self, seed):
        self._r = random.Random(seed)
        self.doubles = 0
        self.u32s = 0
        self._keep = None

    def next_double(self):
        self.doubles += 1
        return self._r.random()

    def next_u32(self):
        self.u32s += 1
        return self._r.getrandbits(32)

    def pgv(self):
        """the same stream as a pgv_rng of C callbacks (keep this object alive for the whole call)"""
        from pgvector_amd import _lib, api
        self._keep = (_lib.NEXT_DOUBLE(lambda _s: self.next_double()), _lib.NEXT_U32(lambda _s: self.next_u32()))
        return api.make_rng(next_double=self._keep[0], next_u32=self._keep[1])


# ------------------------------------------------------------------------------------------------ scan side
def rank_lists(centers, queries, maxprobes):
    """-> (lists [nq x maxprobes] int32, dist [nq x maxprobes] float32)"""
    queries = np.asarray(queries, dtype=np.uint8)
    lists = np.empty((queries.shape[0], maxprobes), dtype=np.int32)
    dist = np.empty((queries.shape[0], maxprobes), dtype=np.float32)
    for q in range(queries.shape[0]):
        d = bm.hamming(queries[q], centers)
        order = np.argsort(d, kind="stable")[:maxprobes]  # stable: equal distances keep list-id order
        lists[q], dist[q] = order, d[order]
    return lists, dist


def scan_stream(offsets, rows, query, lists):
    """-> (dist [m] float32, slot [m] int64) in tuplesort input order"""
    slots = [np.arange(offsets[l], offsets[l + 1], dtype=np.int64) for l in lists]
    slot = np.concatenate(slots) if slots else np.zeros(0, dtype=np.int64)
    if query is None:  # ZeroDistance (src/ivfscan.c:192-196)
        return np.zeros(slot.size, dtype=np.float32), slot
    return bm.hamming(query, np.asarray(rows, dtype=np.uint8)[slot]).astype(np.float32), slot


def scan_head(offsets, rows, query, lists, k):
    """-> (dist [k] float32, slot [k] int64): ascending by (distance, insertion position), +inf / -1 padded"""
    d, s = scan_stream(offsets, rows, query, lists)
    order = np.argsort(d, kind="stable")[:k]
    dist = np.full(k, np.inf, dtype=np.float32)
    slot = np.full(k, -1, dtype=np.int64)
    dist[:order.size], slot[:order.size] = d[order], s[order]
    return dist, slot


def scan_batch(offsets, rows, queries, probe_lists, k):
    heads = [scan_head(offsets, rows, q, pl, k) for q, pl in zip(queries, probe_lists)]
    return np.array([h[0] for h in heads], dtype=np.float32).reshape(-1, k), \
        np.array([h[1] for h in heads], dtype=np.int64).reshape(-1, k)


def search(centers, offsets, rows, queries, probes, k):
    """-> (dist [nq x k], slot [nq x k], lists [nq x probes])"""
    lists, _ = rank_lists(centers, queries, probes)
    dist, slot = scan_batch(offsets, rows, queries, lists, k)
    return dist, slot, lists


# ------------------------------------------------------------------------------------------------ build side
def assign(centers, rows, chunk=8192):
    """-> (list [n] int32, dist [n] float32): np.argmin takes the first of equal minima, the reference's strict `<`"""
    rows = np.asarray(rows, dtype=np.uint8)
    out = np.empty(rows.shape[0], dtype=np.int32)
    dist = np.empty(rows.shape[0], dtype=np.float32)
    for lo in range(0, rows.shape[0], chunk):
        d = hamming_matrix(centers, rows[lo:lo + chunk]).T
        out[lo:lo + chunk] = d.argmin(axis=1)
        dist[lo:lo + chunk] = d.min(axis=1)
    return out, dist


def walk(weight, choice):
    """`choice -= weight[j]; if (choice <= 0) break;` over j < n - 1, one subtraction at a time in double
    (src/ivfkmeans.c:79-84)"""
    n = weight.size
    if n == 1:
        return 0
    left = np.subtract.accumulate(np.concatenate([[choice], weight[:n - 1].astype(np.float64)]))[1:]
    hit = np.flatnonzero(left <= 0)
    return int(hit[0]) if hit.size else n - 1


def init_centers(samples, k, rng):
    """InitCenters (src/ivfkmeans.c:23-91) -> the picked sample of every center [k]"""
    samples = np.asarray(samples, dtype=np.uint8)
    n = samples.shape[0]
    picked = [rng.next_u32() % n]
    weight = np.full(n, FLT_MAX, dtype=np.float32)
    for i in range(k - 1):
        d = bm.hamming(samples[picked[i]], samples).astype(np.float64)
        d = d * d
        weight = np.where(d < weight.astype(np.float64), d.astype(np.float32), weight)
        total = float(np.add.accumulate(weight.astype(np.float64))[-1])  # `sum += weight[j]` in sample order, in double
        picked.append(walk(weight, total * rng.next_double()))
    return np.array(picked, dtype=np.int64)


def update_centers(samples, closest, k, nbits, rng):
    """ComputeNewCenters (src/ivfkmeans.c:179-236) with BitSumCenter / BitUpdateCenter (src/ivfutils.c:325-370)
    -> (centers [k x bytes] uint8, counts [k] int32)"""
    samples = np.asarray(samples, dtype=np.uint8).reshape(-1, (nbits + 7) // 8)
    bits = np.unpackbits(samples, axis=1)[:, :nbits].astype(np.float32)
    agg = np.zeros((k, nbits), dtype=np.float32)
    np.add.at(agg, np.asarray(closest, dtype=np.int64), bits)  # x[i] += 0.0 / 1.0: exact below 2^24
    counts = np.bincount(np.asarray(closest, dtype=np.int64), minlength=k).astype(np.int32)
    for c in range(k):
        if counts[c] > 0:
            agg[c] /= np.float32(counts[c])
        else:
            for i in range(nbits):
                agg[c, i] = np.float32(rng.next_double())
    return np.packbits(agg > np.float32(0.5), axis=1), counts


def lloyd_step(samples, centers, closest, nbits, rng):
    """one iteration of the loop the library runs -> (new centers, counts, changes, the new assignment)"""
    closest = np.asarray(closest, dtype=np.int32)
    k = np.asarray(centers).shape[0]
    if np.asarray(samples).shape[0] == 0:
        new = closest.copy()
    else:
        d = hamming_matrix(samples, centers)
        best = d.argmin(axis=1).astype(np.int32)
        have = closest >= 0
        stay = have & ~(d.min(axis=1) < d[np.arange(d.shape[0]), np.where(have, closest, 0)])
        new = np.where(stay, closest, best).astype(np.int32)
    changes = int((new != closest).sum())
    centers, counts = update_centers(samples, new, k, nbits, rng)
    return centers, counts, changes, new


def _random_centers(k, nbits, rng):
    """RandomCenters (src/ivfkmeans.c:110-133)"""
    return update_centers(np.zeros((0, (nbits + 7) // 8), dtype=np.uint8), np.zeros(0, dtype=np.int32), k, nbits, rng)[0]


def kmeans_sticky(samples, nbits, k, rng, max_iterations=500):
    """-> (centers, closest, iterations): iteration 0 assigns every sample to the first strictly-nearest center, every
    later one keeps a sample where it is unless a center is strictly closer; it stops when an iteration other than the
    first moves nothing"""
    samples = np.asarray(samples, dtype=np.uint8)
    n = samples.shape[0]
    if n == 0:
        return _random_centers(k, nbits, rng), np.zeros(0, dtype=np.int32), 0
    centers = samples[init_centers(samples, k, rng)]
    closest = np.full(n, -1, dtype=np.int32)
    iterations = 0
    for it in range(max_iterations):
        iterations = it + 1
        centers, _, changes, closest = lloyd_step(samples, centers, closest, nbits, rng)
        if changes == 0 and it != 0:
            break
    return centers, closest, iterations


def kmeans_fresh(samples, nbits, k, rng, max_iterations=500):
    """the WRONG loop (what the float pgv_kmeans does): the lowest-index argmin is re-taken every iteration"""
    samples = np.asarray(samples, dtype=np.uint8)
    centers = samples[init_centers(samples, k, rng)]
    closest = np.full(samples.shape[0], -1, dtype=np.int32)
    iterations = 0
    for it in range(max_iterations):
        iterations = it + 1
        new, _ = assign(centers, samples)
        changes = int((new != closest).sum())
        closest = new
        centers, _ = update_centers(samples, closest, k, nbits, rng)
        if changes == 0 and it != 0:
            break
    return centers, closest, iterations


def kmeans_elkan(samples, nbits, k, rng):
    """ElkanKmeans, src/ivfkmeans.c:246-485, statement by statement; the bounds are fp32 like the reference's.  The
    distance function is hamming_distance as a double"""
    samples = np.asarray(samples, dtype=np.uint8)
    n = samples.shape[0]
    as_int = lambda rows: [int.from_bytes(bytes(r), "big") for r in np.asarray(rows, dtype=np.uint8)]
    s_int = as_int(samples)
    dist = lambda a, b: float(bin(a ^ b).count("1"))
    f32 = np.float32

    # InitCenters (:23-91): the picks, and lowerBound[j][i] = distance to center i
    picked = init_centers(samples, k, rng)
    centers = samples[picked].copy()
    c_int = as_int(centers)
    lower = hamming_matrix(samples, centers).astype(np.float32)
    upper = np.zeros(n, dtype=np.float32)
    closest = np.zeros(n, dtype=np.int64)
    # :323-344
    for j in range(n):
        min_distance, closest_center = FLT_MAX, 0
        for c in range(k):
            distance = lower[j, c]
            if distance < min_distance:
                min_distance, closest_center = distance, c
        upper[j], closest[j] = min_distance, closest_center

    halfcdist = np.zeros((k, k), dtype=np.float32)
    s = np.zeros(k, dtype=np.float32)
    iterations = 0
    for iteration in range(500):
        iterations = iteration + 1
        changes = 0
        # Step 1 (:356-367)
        for j in range(k):
            for c in range(j + 1, k):
                halfcdist[j, c] = halfcdist[c, j] = f32(0.5 * dist(c_int[j], c_int[c]))
        # s(c) (:370-387)
        for j in range(k):
            min_distance = FLT_MAX
            for c in range(k):
                if j != c and halfcdist[j, c] < min_distance:
                    min_distance = halfcdist[j, c]
            s[j] = min_distance
        rjreset = iteration != 0
        for j in range(n):
            # Step 2 (:396)
            if upper[j] <= s[closest[j]]:
                continue
            rj = rjreset
            for c in range(k):
                # Step 3 (:407-414)
                if c == closest[j]:
                    continue
                if upper[j] <= lower[j, c]:
                    continue
                if upper[j] <= halfcdist[closest[j], c]:
                    continue
                # Step 3a (:419-430)
                if rj:
                    dxcx = f32(dist(s_int[j], c_int[closest[j]]))
                    lower[j, closest[j]] = dxcx
                    upper[j] = dxcx
                    rj = False
                else:
                    dxcx = upper[j]
                # Step 3b (:433-449)
                if dxcx > lower[j, c] or dxcx > halfcdist[closest[j], c]:
                    dxc = f32(dist(s_int[j], c_int[c]))
                    lower[j, c] = dxc
                    if dxc < dxcx:
                        closest[j] = c
                        upper[j] = dxc
                        changes += 1
        # Step 4 (:454)
        new_centers, _ = update_centers(samples, closest, k, nbits, rng)
        n_int = as_int(new_centers)
        # Step 5 (:457-471)
        newcdist = np.array([dist(c_int[j], n_int[j]) for j in range(k)], dtype=np.float32)
        lower = np.maximum(lower - newcdist[None, :], f32(0))
        # Step 6 (:475-476)
        upper = upper + newcdist[closest]
        # Step 7 (:479-480)
        centers, c_int = new_centers, n_int
        if changes == 0 and iteration != 0:
            break
    return centers, closest.astype(np.int32), iterations


def build(rows, nbits, lists, rng, samples=None):
    """the index api.build_bit_ivf makes -> (centers, list_offsets [lists + 1], order: the row of every slot)"""
    rows = np.asarray(rows, dtype=np.uint8)
    centers, _, _ = kmeans_sticky(rows if samples is None else samples, nbits, lists, rng)
    assigned, _ = assign(centers, rows)
    order = np.argsort(assigned, kind="stable")
    offsets = np.zeros(lists + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(assigned, minlength=lists))
    return centers, offsets, order
