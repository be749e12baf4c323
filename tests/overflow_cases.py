"""Where overflowed distances (+inf, -inf, NaN) sort in a top-k: the host model and the inputs of
tests/test_overflow_cases_cpu.py and tests/test_gpu_overflow_order.py.  Plain numpy.

THE DATA RULE.  Everything is fp32 with small-integer coordinates in [-3, 3]; a few planted rows, centers or queries
carry +-HUGE = 3e19 in coordinate 0 (and in coordinate 1 where a NaN is wanted).  A product or a squared difference of
two small integers is a small integer; HUGE * HUGE and (HUGE - small)^2 are +-inf at once; HUGE * 0 is 0; HUGE - HUGE is 0.
No term is a finite number of HUGE's size, so a partial sum is either an exact small integer or already non-finite, and
every distance is an exact small integer, +-inf or NaN IN ANY ORDER OF SUMMATION: numpy's fp32 value is the reference's
bit for bit, and the matrix cores'.  That is why
  * under the inner product every ORDINARY vector has 0 in coordinates 0 and 1 (an ordinary query never sees a planted row
    overflow there: a product overflows only when both factors are huge -- overflow needs a huge query);
  * L2 overflows for an ordinary query against a planted row and for a huge query against every ordinary row;
  * L1 cannot overflow with 3e19 at all (|3e19 - x| is 3e19): its planted value is HUGE_L1 = 3e38, rows carry +-3e38 and
    only a huge query against a row of the other sign gives +inf (|3e38 + 3e38|); an ordinary pair with one huge side is
    exactly 3e38, since the small terms vanish below its ulp in any order.
tests/test_overflow_cases_cpu.py asserts the rule for every case built here: three summation orders, identical bits.

THE ONE EXCEPTION: NaN.  A NaN needs +inf and -inf to meet, and whether they do depends on HOW the sum is formed, not
only on its order.  A fused multiply-add does not round its product: with the accumulator at +inf, fma(HUGE, -HUGE, +inf)
adds the exact finite -9e38 to +inf and stays +inf, where a separate multiply gives -inf and then NaN.  One sequential
chain of FMAs can never produce NaN from finite elements; two partial accumulators (SIMD lanes, matrix-core blocks) that
have each overflowed can.  The reference is built with -ffp-contract=fast for an FMA machine, so its own value for such
a pair is NaN, +inf or -inf by its compiler's vectorisation; the device's vector-ALU kernels (FMA chains) and its
matrix-core kernels differ in the same way.  Such pairs are AMBIGUOUS: `ambiguous` marks them (NEG_IP only: L2's and
L1's terms have one sign), the CPU test shows that the fused orders really differ on exactly these pairs and on no other,
and check_head takes the entry's own value for an ambiguous row -- provided it is NaN, +inf or -inf -- before it
compares.  Everything else about such a row is still checked: it is a real row, comes out once, sorts where its value
belongs and is never mistaken for padding.

THE MODEL.  expected_head orders by float8 (-inf < finite < +inf < NaN; src/ivfscan.c's tuplesort on float8, restated by
oracle/oracle_ivf.c's float8_cmp / scan_item_cmp) and breaks ties by lower position.  check_head is the one comparison
every device entry goes through.  -0 and +0 are one float8 value and the device's keys fold them: both sides are
compared after adding +0."""
import numpy as np

HUGE = np.float32(3e19)
HUGE_L1 = np.float32(3e38)
L2, NEG_IP, L1 = 0, 1, 2          # pgv_metric's values
METRIC_NAMES = {L2: "l2", NEG_IP: "negip", L1: "l1"}
PINF_BITS = np.uint32(0x7f800000)


# ------------------------------------------------------------------------------------------------------ distances
def _terms(metric, q, rows):
    """[nq x n x dim] fp32 terms, each computed as the reference computes it"""
    q, r = q[:, None, :], rows[None, :, :]
    with np.errstate(over="ignore", invalid="ignore"):
        if metric == L2:
            d = q - r
            return d * d
        if metric == L1:
            return np.abs(q - r)
        return q * r


def _sum(t, order):
    """fp32 sum over the last axis in the given order of additions"""
    with np.errstate(over="ignore", invalid="ignore"):
        if order == "pairwise":
            while t.shape[-1] > 1:
                if t.shape[-1] % 2:
                    t = np.concatenate([t, np.zeros(t.shape[:-1] + (1,), np.float32)], axis=-1)
                t = t[..., 0::2] + t[..., 1::2]
            return t[..., 0]
        idx = range(t.shape[-1]) if order == "forward" else range(t.shape[-1] - 1, -1, -1)
        acc = np.zeros(t.shape[:-1], np.float32)
        for j in idx:
            acc = acc + t[..., j]
        return acc


def _fused(metric, q, rows, order):
    """the same sums as one chain of fused multiply-adds: fp32(a * b + acc) with the product unrounded (float64 holds a
    product of two fp32 values exactly, and on this data the float64 sum is exact or beyond fp32's range)"""
    q, r = q[:, None, :].astype(np.float64), rows[None, :, :].astype(np.float64)
    dim = q.shape[-1]
    acc = np.zeros((q.shape[0], r.shape[1]), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in (range(dim) if order == "fused" else range(dim - 1, -1, -1)):
            if metric == L2:
                d = (q[..., j] - r[..., j]).astype(np.float32).astype(np.float64)
                acc = (d * d + acc.astype(np.float64)).astype(np.float32)
            elif metric == L1:
                acc = acc + np.abs(q[..., j] - r[..., j]).astype(np.float32)
            else:
                acc = (q[..., j] * r[..., j] + acc.astype(np.float64)).astype(np.float32)
    return acc


ORDERS = ("forward", "reversed", "pairwise", "fused", "fused_reversed")


def distances(metric, queries, rows, order="forward", chunk=16):
    """[nq x n] fp32 kernel values (L2 squared / negative inner product / L1), -0 folded into +0.  order: one of ORDERS"""
    queries, rows = np.ascontiguousarray(queries, np.float32), np.ascontiguousarray(rows, np.float32)
    out = np.empty((len(queries), len(rows)), np.float32)
    for q0 in range(0, len(queries), chunk):
        if order.startswith("fused"):
            s = _fused(metric, queries[q0:q0 + chunk], rows, order)
        else:
            s = _sum(_terms(metric, queries[q0:q0 + chunk], rows), order)
        out[q0:q0 + chunk] = (-s if metric == NEG_IP else s) + np.float32(0)
    assert out.dtype == np.float32
    return out


def bits(a):
    """uint32 images with every NaN as one pattern and -0 as +0"""
    a = np.ascontiguousarray(a, dtype=np.float32) + np.float32(0)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def ambiguous(dist):
    """the pairs whose value depends on how the sum is formed (the module docstring): where the unfused sum is NaN"""
    return np.isnan(np.asarray(dist))


def classes(dist):
    """the value classes a set of distances holds, for the tests' own 'is this case what it claims' assertions"""
    d = np.asarray(dist)
    return dict(ninf=int(np.isneginf(d).sum()), finite=int(np.isfinite(d).sum()), pinf=int(np.isposinf(d).sum()),
                nan=int(np.isnan(d).sum()))


# ---------------------------------------------------------------------------------------------------------- model
def float8_order(dist):
    """positions in float8 order (-inf < finite < +inf < NaN), ties by lower position"""
    d = np.asarray(dist, dtype=np.float32)
    nan = np.isnan(d)
    return np.lexsort((np.arange(len(d)), nan, np.where(nan, np.inf, d)))


def expected_head(dist, k):
    """-> (positions, distances) of the first min(k, len) entries of the float8-ordered stream"""
    order = float8_order(dist)[:k]
    return order, np.asarray(dist, dtype=np.float32)[order]


def settle_ambiguous(got_dist, got_ids, cand_ids, cand_dist, what=""):
    """cand_dist with every ambiguous row's NaN replaced by the value the entry reports for that row, which must be NaN,
    +inf or -inf; an ambiguous row the entry did not return keeps NaN (it is then held to sort last)"""
    amb = ambiguous(cand_dist)
    if not amb.any():
        return cand_dist
    out = cand_dist.copy()
    at = {int(c): i for i, c in enumerate(cand_ids) if amb[i]}
    for g, d in zip(np.asarray(got_ids).tolist(), np.asarray(got_dist, dtype=np.float32)):
        if g in at:
            assert np.isnan(d) or np.isinf(d), (what, "row %d: NaN, +inf or -inf by the order of its sum, not" % g, float(d))
            out[at[g]] = d
    return out


def check_head(got_dist, got_ids, cand_ids, cand_dist, k, ordered, what=""):
    """One query's output (got_dist [k], got_ids [k]; -1 / ~0 = none) against the model over its real rows: cand_ids [m]
    are the ids the entry reports for them, in the entry's position order, cand_dist [m] their model distances.
      1. the first min(k, m) distances are the model's bit for bit (NaN matches NaN)
      2. none of those is "none"
      3. everything past m is +inf / none
      4. ids are distinct
      5. every returned id is a real row whose own model distance is the one the output claims
    An ambiguous row (NaN in cand_dist, see the module docstring) first takes the value the entry gives it.
      6. ordered (the entry promises ties by lower index / position): ids element for element; else, inside a class of
         equal distances, as sets -- the class the head's end cuts need only supply members"""
    got_dist, got_ids = np.asarray(got_dist, dtype=np.float32), np.asarray(got_ids).astype(np.int64)
    cand_ids, cand_dist = np.asarray(cand_ids).astype(np.int64), np.asarray(cand_dist, dtype=np.float32)
    assert got_dist.shape == got_ids.shape == (k,), (what, got_dist.shape, got_ids.shape)
    cand_dist = settle_ambiguous(got_dist, got_ids, cand_ids, cand_dist, what)
    m = len(cand_ids)
    n = min(k, m)
    order, want_d = expected_head(cand_dist, n)
    gb, wb = bits(got_dist), bits(want_d)
    assert np.array_equal(gb[:n], wb), (what, "distances", got_dist[:n].tolist(), want_d.tolist())
    assert (got_ids[:n] != -1).all(), (what, "a 'none' among the first %d" % n, got_ids.tolist())
    assert (gb[n:] == PINF_BITS).all() and (got_ids[n:] == -1).all(), (what, "padding", got_dist[n:].tolist(),
                                                                       got_ids[n:].tolist())
    assert len(set(got_ids[:n].tolist())) == n, (what, "an id twice", got_ids.tolist())
    sorter = np.argsort(cand_ids, kind="stable")
    assert (np.diff(cand_ids[sorter]) > 0).all(), (what, "the case's own ids repeat")
    where = sorter[np.minimum(np.searchsorted(cand_ids, got_ids[:n], sorter=sorter), max(m - 1, 0))] if n else sorter[:0]
    assert np.array_equal(cand_ids[where], got_ids[:n]), (what, "an id that is no row of this query", got_ids[:n].tolist())
    assert np.array_equal(bits(cand_dist[where]), gb[:n]), (what, "a row under another row's distance", got_ids[:n].tolist())
    want_ids = cand_ids[order]
    if ordered:
        assert np.array_equal(got_ids[:n], want_ids), (what, "ids", got_ids[:n].tolist(), want_ids.tolist())
        return
    all_bits = bits(cand_dist)
    i = 0
    while i < n:
        j = i + 1
        while j < n and wb[j] == wb[i]:
            j += 1
        members = set(cand_ids[all_bits == wb[i]].tolist())
        got = set(got_ids[i:j].tolist())
        if j == n:
            assert got <= members, (what, "class at %d" % i, sorted(got), sorted(members))
        else:
            assert got == members, (what, "class at %d" % i, sorted(got), sorted(members))
        i = j


def pad_stream(dist, ids, k):
    """a reference stream of n <= k entries as a device output of k (+inf / -1 behind it)"""
    n = len(ids)
    d = np.full(k, np.inf, np.float32)
    i = np.full(k, -1, np.int64)
    d[:n], i[:n] = np.asarray(dist, dtype=np.float32), np.asarray(ids).astype(np.int64)
    return d, i


# ------------------------------------------------------------------------------------------------- IVFFlat (section 1)
N, DIM, NLISTS = 8192, 64, 64
# (nq, probes, k): tests/test_gpu_scan_path_edges.py's route table (share = nq * probes / 64)
SHAPES = [(4, 6, 10), (5, 6, 10), (5, 5, 10), (128, 1, 10), (128, 2, 10), (128, 2, 192), (128, 2, 193), (128, 6, 10),
          (128, 7, 10), (127, 2, 10)]
HUGE_LISTS = (10, 20, 30, 40)          # centers with HUGE in coordinate 0: near for a huge query only
SHORT_LISTS = tuple(range(50, 58))     # eight lists around one point, 9 rows in all
SHORT_SIZES = (4, 4, 0, 1, 0, 0, 0, 0)
PLANTED_LISTS = (50, 51, 3, 17, 25, 33, 44, 60)   # three overflow rows each (the first two are short lists)


def ivf_case(metric):
    """-> dict(metric, centers [64 x 64], offsets [65], rows [8192 x 64], tids, ordinary [128 x 64], huge [128 x 64])

    Explicit centers and list offsets: which lists a query probes follows from the centers alone, and a row need not be
    nearest to its list's center (a scan does not care).
      L2      rows and queries in [-3, 3].  Four lists (HUGE_LISTS) have HUGE in their center's coordinate 0 and hold
              two rows with x0 = HUGE each: +inf away from an ordinary query, the only finite rows for a huge one.  Eight
              SHORT_LISTS of 9 rows in all sit around one point; a query aimed there probes nothing else at up to 7 probes,
              so its head runs finite -> +inf -> padding inside k = 10.  PLANTED_LISTS hold three rows with x0 = HUGE each.
              `huge` queries have q0 = HUGE: every center but HUGE_LISTS' is +inf away (ties: the lower list id, lists
              0, 1, 2 -- which hold no planted row), every ordinary row is +inf away and at most 8 probed rows are finite.
      NEG_IP  every ordinary vector has 0 in coordinates 0 and 1.  PLANTED_LISTS hold (HUGE, 0, ..), (-HUGE, 0, ..) and
              (HUGE, HUGE, ..); `huge` alternates (HUGE, 0, ..), for which these are -inf, +inf, -inf, and
              (HUGE, -HUGE, ..), for which they are -inf, +inf, NaN.  For `ordinary` queries (zeros there) they are small
              integers.  HUGE_LISTS are ordinary lists here."""
    rng = np.random.default_rng(7100 + metric)
    ip = metric == NEG_IP
    centers = rng.integers(-2, 3, (NLISTS, DIM)).astype(np.float32)
    point = rng.integers(-2, 3, DIM).astype(np.float32)
    for j, l in enumerate(SHORT_LISTS):       # the short lists' centers: one point, coordinate 8 + j moved by one
        centers[l] = point
        centers[l, 8 + j] += 1.0 if point[8 + j] < 2 else -1.0
    if ip:
        centers[:, :2] = 0
    else:
        centers[list(HUGE_LISTS), 0] = HUGE
    sizes = rng.integers(60, 231, NLISTS)
    sizes[list(SHORT_LISTS)] = SHORT_SIZES
    free = [l for l in range(NLISTS) if l not in SHORT_LISTS]
    sizes[free] += (N - sizes.sum()) // len(free)
    sizes[free[-1]] += N - sizes.sum()
    assert sizes.sum() == N and sizes[free].min() > 20
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = rng.integers(-3, 4, (N, DIM)).astype(np.float32)
    if ip:
        rows[:, :2] = 0
    for l in PLANTED_LISTS:
        at = offsets[l] + rng.choice(sizes[l], 3, replace=False)
        if ip:
            rows[at[0], 0] = HUGE
            rows[at[1], 0] = -HUGE
            rows[at[2], :2] = HUGE
        else:
            rows[at, 0] = HUGE
    if not ip:
        for l in HUGE_LISTS:
            rows[offsets[l] + rng.choice(sizes[l], 2, replace=False), 0] = HUGE
    # queries: a center plus -1 .. 1 noise in a few coordinates; every fourth at the short lists, every fourth at a
    # planted list, the rest anywhere
    target = rng.integers(0, NLISTS, 128)
    target[0::4] = rng.choice(SHORT_LISTS, 32)
    target[1::4] = rng.choice(PLANTED_LISTS, 32)
    target[[0, 64, 127]] = (50, 51, 53)       # the queries compared with the oracle's search
    ordinary = centers[target].copy()
    ordinary[:, 0] = rng.integers(-2, 3, 128)     # (a HUGE_LISTS target: an ordinary query all the same)
    for i in range(128):
        c = rng.choice(np.arange(20, DIM), 3, replace=False)
        ordinary[i, c] = np.clip(ordinary[i, c] + rng.integers(-1, 2, 3), -3, 3)
    huge = ordinary.copy()
    huge[:, 0] = HUGE
    if ip:
        ordinary[:, :2] = 0
        huge[:, 1] = 0
        huge[1::2, 1] = -HUGE
    return dict(metric=metric, centers=np.ascontiguousarray(centers), offsets=offsets, rows=np.ascontiguousarray(rows),
                tids=(np.arange(N, dtype=np.uint64) << np.uint64(16)) | np.uint64(1),
                ordinary=np.ascontiguousarray(ordinary), huge=np.ascontiguousarray(huge))


def ivf_probes(case, queries, probes):
    """the model's GetScanLists: [nq x probes] list ids, float8 order over the centers' distances, ties to the lower id"""
    dc = distances(case["metric"], queries, case["centers"])
    return np.stack([expected_head(dc[i], probes)[0] for i in range(len(queries))]).astype(np.int32), dc


def ivf_candidates(case, lists, dist_row):
    """one query's real rows in the scan's position order (probe after probe) -> (slots, their model distances)"""
    off = case["offsets"]
    slots = np.concatenate([np.arange(off[l], off[l + 1]) for l in lists] + [np.empty(0, np.int64)]).astype(np.int64)
    return slots, dist_row[slots]


def ivf_mixes():
    """name -> (metric, which query set, PGV_SCAN_SHADOW): the four cases every shape runs on"""
    return {"a": (L2, "ordinary", "1"), "b": (L2, "ordinary", "0"), "c": (NEG_IP, "mixed", "0"), "d": (L2, "huge", "1")}


def ivf_queries(case, which):
    if which == "mixed":       # huge and ordinary interleaved in threes, the oracle's three queries huge, ordinary, huge
        q = case["ordinary"].copy()
        sel = (np.arange(128) // 3) % 2 == 0
        sel[[0, 64, 127]] = (True, False, True)
        q[sel] = case["huge"][sel]
        return q
    return case[which]


# the selection classes: one probed list of SEL_M rows of which SEL_FINITE are finite
SEL_M = (1000, 4000, 20000)
SEL_FINITE = 5
SEL_K = (3, 5, 6, 17, 40)
SEL_NQ = 40


def selection_case(m, huge_queries):
    """a two-list L2 index (4-d; list 1 is empty and 50 away) whose list 0 has m rows, SEL_FINITE of them finite:
    ordinary queries against rows that carry x0 = HUGE but for five, or huge queries against ordinary rows of which
    five carry x0 = HUGE"""
    rng = np.random.default_rng(7300 + m + int(huge_queries))
    rows = rng.integers(-3, 4, (m, 4)).astype(np.float32)
    five = rng.choice(m, SEL_FINITE, replace=False)
    queries = rng.integers(-2, 3, (SEL_NQ, 4)).astype(np.float32)
    if huge_queries:
        rows[five, 0] = HUGE
        queries[:, 0] = HUGE
    else:
        keep = rows[five, 0].copy()
        rows[:, 0] = HUGE
        rows[five, 0] = keep
    centers = np.array([[0, 0, 0, 0], [50, 50, 50, 50]], dtype=np.float32)
    return dict(metric=L2, centers=centers, offsets=np.array([0, m, m], dtype=np.int64), rows=np.ascontiguousarray(rows),
                tids=np.arange(m, dtype=np.uint64), queries=np.ascontiguousarray(queries))


# ------------------------------------------------------------------------------------------- center ranking (section 2)
RANK_NLISTS = 70
RANK_MAXPROBES = (1, 4, 5, 64, 70)
RANK_NQ = (1, 33, 128)


def rank_case(metric):
    """70 centers x 64-d and two pools of 128 queries (`huge_first` starts with a huge query, `ordinary_first` is the
    same pool reversed), huge queries at every 7th place.
      L2      four centers have c0 = HUGE (finite for a huge query only), two have c1 = HUGE (+inf for every query): six
              overflow against an ordinary query, all but four against a huge one (q0 = HUGE, q1 small).
      NEG_IP  33 centers with c0 = HUGE, 33 with c0 = -HUGE, four with 0; c1 = 0 throughout and ordinary queries have
              0 in both: an ordinary query sees small integers only (the rule above), a huge one -inf for 33, +inf for 33.
    No NaN center: the reference's heap is not defined on them."""
    assert metric in (L2, NEG_IP)
    rng = np.random.default_rng(7200 + metric)
    centers = rng.integers(-3, 4, (RANK_NLISTS, DIM)).astype(np.float32)
    queries = rng.integers(-3, 4, (128, DIM)).astype(np.float32)
    is_huge = np.arange(128) % 7 == 0
    if metric == L2:
        centers[[5, 21, 40, 66], 0] = HUGE
        centers[[13, 58], 1] = HUGE
        queries[is_huge, 0] = HUGE
    else:
        centers[:, :2] = 0
        perm = rng.permutation(RANK_NLISTS)
        centers[perm[:33], 0] = HUGE
        centers[perm[33:66], 0] = -HUGE
        queries[:, :2] = 0
        queries[is_huge, 0] = HUGE
    # any rows will do: ranking reads the centers alone
    rows = rng.integers(-3, 4, (RANK_NLISTS * 3, DIM)).astype(np.float32)
    if metric == NEG_IP:
        rows[:, :2] = 0
    offsets = (np.arange(RANK_NLISTS + 1) * 3).astype(np.int64)
    return dict(metric=metric, centers=np.ascontiguousarray(centers), offsets=offsets, rows=rows,
                tids=np.arange(len(rows), dtype=np.uint64), huge_first=np.ascontiguousarray(queries),
                ordinary_first=np.ascontiguousarray(queries[::-1]))


# ---------------------------------------------------------------------------------------------- exact top-k (section 3)
EXACT_NQ = (3, 64, 128)
EXACT_N = (63, 64, 200)
EXACT_DIM = 16


def huge_of(metric):
    return HUGE_L1 if metric == L1 else HUGE


def exact_case(metric, nq, n, huge_queries):
    """rows [n x 16] with every 7th row planted, queries [nq x 16] ordinary or (every other one) huge.
    L2: planted rows carry x0 = HUGE.  NEG_IP: (HUGE, 0), (-HUGE, 0), (HUGE, HUGE) in turn, huge queries (HUGE, 0) and
    (HUGE, -HUGE) in turn.  L1: x0 = +-HUGE_L1 in turn, huge queries q0 = HUGE_L1."""
    rng = np.random.default_rng(7400 + 100 * metric + n + nq)
    big = huge_of(metric)
    rows = rng.integers(-3, 4, (n, EXACT_DIM)).astype(np.float32)
    queries = rng.integers(-3, 4, (nq, EXACT_DIM)).astype(np.float32)
    planted = np.arange(3, n, 7)
    if metric == NEG_IP:
        rows[:, :2] = 0
        queries[:, :2] = 0
        rows[planted[0::3], 0] = big
        rows[planted[1::3], 0] = -big
        rows[planted[2::3], :2] = big
    elif metric == L1:
        rows[planted[0::2], 0] = big
        rows[planted[1::2], 0] = -big
    else:
        rows[planted, 0] = big
    if huge_queries:
        hq = np.arange(0, nq, 2)
        queries[hq, 0] = big
        if metric == NEG_IP:
            queries[hq[1::2], 1] = -big
    return np.ascontiguousarray(queries), np.ascontiguousarray(rows)


# --------------------------------------------------------------------------------------------------- rerank (section 4)
RERANK_KC, RERANK_NQ, RERANK_N, RERANK_DIM = 16, 4, 40, 8


def rerank_case(metric):
    """-> (queries [4 x 8], rows [40 x 8], cand [4 x 16]).  Rows 0 .. 9 are planted (L2 / L1: +inf for the queries here;
    NEG_IP: -inf, +inf, NaN in turn for query 1 and 3, -inf / +inf for 0 and 2), rows 10 .. 39 ordinary.
      query 0   -1 interleaved with finite, +inf (and -inf / NaN) candidates, a "none" in front of a +inf one
      query 1   starts with -1, -1; its real candidates end with non-finite ones
      query 2   only non-finite real candidates, between -1s
      query 3   sixteen real candidates, no -1"""
    rng = np.random.default_rng(7500 + metric)
    big = huge_of(metric)
    rows = rng.integers(-3, 4, (RERANK_N, RERANK_DIM)).astype(np.float32)
    queries = rng.integers(-3, 4, (RERANK_NQ, RERANK_DIM)).astype(np.float32)
    if metric == NEG_IP:
        rows[:, :2] = 0
        rows[0:10:3, 0] = big
        rows[1:10:3, 0] = -big
        rows[2:10:3, :2] = big
        queries[:, 0] = big
        queries[:, 1] = (0, -big, 0, -big)
    elif metric == L1:
        rows[:10, 0] = -big
        queries[:, 0] = big
    else:
        rows[:10, 0] = big
    cand = np.array([[12, -1, 0, 20, -1, 1, 2, -1, 31, 3, -1, -1, 15, 4, -1, 5],
                     [-1, -1, 25, 11, 6, -1, 30, 7, 8, -1, 19, 0, -1, 1, 2, -1],
                     [-1, 3, -1, 4, 5, -1, -1, 6, -1, -1, 7, 8, -1, -1, -1, -1],
                     [10, 0, 11, 1, 12, 2, 13, 3, 14, 4, 15, 5, 16, 6, 17, 7]], dtype=np.int64)
    return np.ascontiguousarray(queries), np.ascontiguousarray(rows), cand


# --------------------------------------------------------------------------------------------- sparse top-k (section 5)
SPARSE_DIM, SPARSE_N = 50000, 200


def sparse_case(metric, nq):
    """CSR queries and rows over 50 000 dimensions, at most 8 stored elements each, drawn from a pool of 40 indices so
    that vectors share some; index 0 and 1 are the planted coordinates (stored only where they are non-zero).
    -> (queries csr, rows csr, dense queries [nq x 42], dense rows [200 x 42]): the dense twins hold the pool's columns
    only -- an index neither side stores adds 0 to every sum"""
    rng = np.random.default_rng(7600 + 10 * metric + nq)
    big = huge_of(metric)
    pool = np.sort(rng.choice(np.arange(2, SPARSE_DIM), 40, replace=False))
    pool[-1] = SPARSE_DIM - 1
    cols = np.concatenate([[0, 1], pool])

    def dense(n):
        d = np.zeros((n, 42), np.float32)
        for r in range(n):
            c = rng.choice(40, rng.integers(0, 7), replace=False) + 2
            d[r, c] = rng.integers(-3, 4, len(c))      # (a stored 0.0 is legal, but here zeros are simply not stored)
        return d
    rows, queries = dense(SPARSE_N), dense(nq)
    planted = np.arange(2, SPARSE_N, 9)
    if metric == NEG_IP:
        rows[planted[0::3], 0] = big
        rows[planted[1::3], 0] = -big
        rows[planted[2::3], :2] = big
        queries[0::2, 0] = big
        queries[0::4, 1] = -big
    elif metric == L1:
        rows[planted[0::2], 0] = big
        rows[planted[1::2], 0] = -big
        queries[0::2, 0] = big
    else:
        rows[planted, 0] = big
        queries[0::3, 0] = big

    def csr(d):
        ptr, idx, val = [0], [], []
        for r in d:
            nz = np.nonzero(r)[0]
            idx.extend(cols[nz].tolist())
            val.extend(r[nz].tolist())
            ptr.append(len(idx))
        assert max(np.diff(ptr)) <= 8
        return np.array(ptr, np.int64), np.array(idx, np.int32), np.array(val, np.float32)
    return csr(queries), csr(rows), queries, rows


# ------------------------------------------------------------------------------------------------------ HNSW (section 6)
HNSW_FORMS = ("l2", "l1", "negip")
HNSW_METRIC = {"l2": L2, "l1": L1, "negip": NEG_IP}


def hnsw_overflow(form, elements, queries):
    """tests/hnsw_tie_cases.random_graph's elements and queries with overflow planted AFTER the graph was built: coordinate
    0 of every 20th element is HUGE (negip: +-HUGE in turn; l1: +-HUGE_L1 in turn) and every 6th query (8 of 48) has
    q0 = HUGE / HUGE_L1.  negip: coordinate 0 of every OTHER element and query becomes 0 (the rule above).  No NaN.
    -> (elements, queries, the planted elements' indexes)"""
    metric = HNSW_METRIC[form]
    big = huge_of(metric)
    e, q = elements.copy(), queries.copy()
    planted = np.arange(0, len(e), 20)
    if metric == NEG_IP:
        e[:, 0] = 0
        q[:, 0] = 0
    e[planted, 0] = big
    if metric != L2:
        e[planted[1::2], 0] = -big
    q[0::6, 0] = big
    return np.ascontiguousarray(e), np.ascontiguousarray(q), planted
