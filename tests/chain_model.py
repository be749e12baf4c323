"""A host model of the accumulator chains of the matrix-core L2 / inner-product kernels, and adversarial data built
with it.  numpy only; nothing here imports the package.

The deterministic rounding band of the MFMA L2 paths (ScanBound, pgvector_amd/csrc/pgv_internal.h) charges one unit
roundoff per product of an accumulator chain.  It is valid only while its chain length agrees with the kernels, so this
file restates, per kernel form, WHICH element of a row joins WHICH chain in WHAT order and how the chains are joined:

  scan32   mfma_scan_kernel, tasks of 17 .. 32 queries (kernels_mfma.hip:1129-1212; Mma4, :144-157), two or three stages
  scan16   its 16-wide path for tasks of <= 16 queries (:1213-1267; Mma16x4, :181-200)
  scan64   its 64-query form, tasks of 33 .. 64 queries (:1040-1127; Mma, :123-137)
  dense    mfma_dense_kernel (kernels_dense.hip:119-176; DenseMma, :38-51)
  argmin   mfma_argmin_kernel: ONE chain over the whole row (kernels_mfma.hip:275-), which STARTS at -|c|^2 / 2 so
           that -2 acc = |c|^2 - 2 a.c; assign_set() swamps it, argmin_reach() says how far that can go

A row is streamed in 128-byte slices of eight 16-byte vectors.  In the 32-wide shapes step c of a slice gives the lanes
of half h vector 2 c + h; in the 16-wide shapes step c gives lane group kg vector kg + 4 c.  An fp32 instruction
(32x32x2 / 16x16x4) takes ONE float of every lane's vector, k ascending with the lane half / group; the project's record
(tools/mfma_numerics.py) is that it is an fmaf chain in that order, bit for bit.  An fp16 instruction takes the whole
vector of every lane (32x32x16: 16 products, 16x16x32: 32 products) and is NOT an fmaf chain: for fp16 the maps give
chain membership only, and nothing here predicts fp16 bits.

The evaluator runs an fp32 chain map exactly: a product of two fp32 values is exact in float64, and the addition uses an
error-free two-sum with a correction where the float64 sum sits on an fp32 half-way point, so the result is fmaf's.

The swamping builders make a dot product err by almost its whole bound: every chain starts with a product of about 1
and every later product is just under (the accumulator stays, the value errs DOWN) or just over (it steps a whole ulp,
the value errs UP) half an ulp of the accumulator.  |q_i| = |x_i| up to 2^-10, so Cauchy-Schwarz is tight.

|x|^2 as row_norms_kernel computes it is MODELLED too (row_norms), bit for bit for fp32: the adversarial margins below
are stated on the values the kernels produce, and g_norm |x|^2 is not taken out of them.  No practical input reaches
the g_norm and g_ref terms on their own: the row norm is a sum of dim / 64 squares per lane (its error on these rows is
a few u |x|^2, against 14 .. 34 u charged), and g_ref scales with the DISTANCE, which is ~1e-5 of |x|^2 wherever the
band matters.  Both are a sixteenth of the g_dot term or less; the sets below leave them alone.  (Measured on an
MI355X: with g_norm = 0 and with g_ref = 0 every test of tests/test_gpu_scan_band.py still passes.)

What the model says is OUT OF REACH, so that no test is forced:
  * scan_bound_chain ignoring its chain length on a ragged dim.  At 1600-d the quarter forms charge 416 + 4 against
    the 400 + 4 of ld / 4: the two bands part at 1.92 eps above the k-th value, and the true neighbour of the best set
    sits 1.77 eps above it (every candidate must stay below the true neighbour), see test_chain_model_cpu.py.  What does
    catch a wrong chain length is the library's own figure (pgv_scan_chain_length) compared with the chain maps.
  * the assignment's band at half width (argmin_reach): its chain starts at -|c|^2 / 2, and whichever way the products
    go, either the accumulator passes through zero (rows near the center: at most a third of the term per direction)
    or the distance itself is large and its own term gamma_x d covers the rest."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
F32, F16 = "f32", "f16"
FORMS = ("scan32", "scan16", "scan64", "dense", "argmin")
DELTA = 2.0 ** -10   # how far the swamping products sit from half an ulp, relatively


# ------------------------------------------------------------------------------------------------- chain maps
def padded(dim, dtype):
    """pgv_internal.h padded_dim: whole 16-byte vectors"""
    per = 4 if dtype == F32 else 8
    return (dim + per - 1) // per * per


def slices(dim, dtype):
    """128-byte slices of a row, and the slices per quarter of the 64-query / dense forms"""
    per = 32 if dtype == F32 else 64
    n = (padded(dim, dtype) + per - 1) // per
    return n, (n + 3) // 4


def _slice_order_f32(sl):
    """elements of slice sl in the order ONE fp32 accumulator meets them (Mma<float> / DenseMma<float>): step c reads
    vectors 2 c (half 0) and 2 c + 1 (half 1); instruction e multiplies float e of both, k = half ascending"""
    return [32 * sl + 8 * c + 4 * h + e for c in range(4) for e in range(4) for h in range(2)]


def chain_map(form, dtype, dim):
    """(chains, join): chains is a list of lists of element indices < dim, in the order their products are added;
    join is 'pairs' ((c0 + c1) + (c2 + c3)) or 'seq' (((0 + c0) + c1) + c2 ...)"""
    assert form in FORMS
    ld = padded(dim, dtype)
    ns, quarter = slices(dim, dtype)
    if dtype == F32:
        if form in ("scan32", "scan16"):
            # scan32: vector 2 c + h, float e -> chain e; scan16: vector kg + 4 c, float e -> chain e, k = kg ascending:
            # either way chain e meets elements e, e + 4, e + 8, ... in ascending order
            chains = [list(range(e, ld, 4)) for e in range(4)]
            join = "pairs"
        else:
            per = ns if form == "argmin" else quarter
            chains = [sum((_slice_order_f32(sl) for sl in range(s0, min(ns, s0 + per))), []) for s0 in range(0, ns, per)]
            join = "seq"
    else:
        if form == "scan32":      # Mma4<__half>: step c -> chain c, halves [16 c, 16 c + 16) of the slice
            chains = [[64 * sl + 16 * c + j for sl in range(ns) for j in range(16)] for c in range(4)]
            join = "pairs"
        elif form == "scan16":    # Mma16x4<__half>: step c of slice sl -> chain c + 2 (sl & 1), halves [32 c, 32 c + 32)
            chains = [[] for _ in range(4)]
            for sl in range(ns):
                for c in range(2):
                    chains[c + 2 * (sl & 1)] += [64 * sl + 32 * c + j for j in range(32)]
            join = "pairs"
        else:
            per = ns if form == "argmin" else quarter
            chains = [list(range(64 * s0, 64 * min(ns, s0 + per))) for s0 in range(0, ns, per)]
            join = "seq"
    return [[i for i in ch if i < dim] for ch in chains], join


def longest_chain(form, dtype, dim):
    return max(len(ch) for ch in chain_map(form, dtype, dim)[0])


# ------------------------------------------------------------------------------------------------- the bound
def gamma_n(n, v=U):
    """pgv_internal.h gamma_n: computed in double, returned as float"""
    return float(np.float32(n * v / (1.0 - n * v)))


def scan_chain_length(dim, dtype, wide):
    """kernels_mfma.hip scan_chain_length: products per chain of mfma_scan_kernel, whichever form takes a task"""
    ld = padded(dim, dtype)
    ns, quarter = slices(dim, dtype)
    if dtype == F32:
        return max(ld // 4, 32 * quarter if wide else 0)
    return max(16 * ns, 32 * ((ns + 1) // 2), 64 * quarter if wide else 0)


def dense_chain_length(dim, dtype):
    """kernels_dense.hip dense_chain_length"""
    return slices(dim, dtype)[1] * (32 if dtype == F32 else 64)


def parent_chain_length(dim, dtype, wide):
    """what the bound assumed before scan_chain_length existed: ld / 4 (scan_bound), dense_chain_length when wide"""
    return dense_chain_length(dim, dtype) if wide else padded(dim, dtype) / 4.0


def charged_chain(path, dtype, dim):
    """the chain length the host charges on each path: 'scan' (list scan, 32-query kernel), 'scan_wide' (64-query
    kernel), 'rank' / 'topk32' (dense_scan: the 32-query kernel), 'topk128' (mfma_dense_kernel)"""
    if path == "topk128":
        return dense_chain_length(dim, dtype)
    return scan_chain_length(dim, dtype, path == "scan_wide")


def forms_of(path):
    """the kernel forms whose values a path's band must cover"""
    return {"scan": ("scan32", "scan16"), "rank": ("scan32", "scan16"), "topk32": ("scan32", "scan16"),
            "scan_wide": ("scan32", "scan16", "scan64"), "topk128": ("dense",)}[path]


def scan_bound(dim, dtype, chain=None):
    """pgv_internal.h scan_bound / scan_bound_chain, deterministic mode: (g_dot, g_norm, g_ref) as floats"""
    ld = padded(dim, dtype)
    if chain is None:
        chain = ld / 4.0
    return (gamma_n(chain + 4.0), gamma_n(ld / 64.0 + 10.0), float(np.float32(2.0) * np.float32(gamma_n(ld + 2.0))))


def band_eps(bound, qn, rn):
    """batch_recheck_kernel / batch_fix_kernel (kernels_query.hip:366-378) in fp32, g_sq = 0: eps of a query with
    |q|^2 = qn against an index whose largest |x|^2 is rn"""
    g_dot, g_norm, _ = (np.float32(b) for b in bound)
    qn, rn = np.float32(qn), np.float32(rn)
    cross = np.float32(2.0) * np.sqrt(qn * rn, dtype=np.float32)
    return np.float32(1.001) * (g_dot * cross + g_norm * rn)


def stat_eps(dim, dtype, qn, rn):
    """the same under the STATISTICAL bound (scan_bound, bound_mode 0): g_sq (|q| + |x|)^2, g_sq = 8 sqrt(ld + 4) u.
    With |q| = |x| that is 32 sqrt(ld) u |q||x| against the deterministic ~(ld / 2 + 8) u |q||x|: the statistical band
    is the WIDER one below ~4100 dimensions and loses a swamped neighbour only above"""
    g_sq = np.float32(8.0) * np.sqrt(np.float32(padded(dim, dtype)) + np.float32(4.0)) * np.float32(5.9604645e-8)
    qn, rn = np.float32(qn), np.float32(rn)
    return np.float32(1.001) * g_sq * (qn + rn + np.float32(2.0) * np.sqrt(qn * rn, dtype=np.float32))


def band_edge(bound, a_k, qn, rn, width=2.0):
    """the largest pre-filter value still inside the band around the k-th value a_k; width 2 is the kernels', 1 the
    half-width band the adversarial sets are built to defeat"""
    eps = band_eps(bound, qn, rn)
    edge = np.float32(a_k) + np.float32(width) * eps
    return edge + np.float32(bound[2]) * np.abs(edge + np.float32(qn))


# ------------------------------------------------------------------------------------------------- exact fp32 arithmetic
def fmaf(a, b, c):
    """fl32(a b + c) for float32 arrays, correctly rounded: the product is exact in float64; s = fl64(c + p) with its
    error e by two-sum; s rounds to fp32 as the exact sum does unless s lies on an fp32 half-way point and e != 0, where
    the sign of e decides"""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = c64 + p
    bb = s - c64
    e = (c64 - (s - bb)) + (p - bb)
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)
    other = r.astype(np.float64) + 2.0 * d            # the fp32 neighbour on s's far side, if s is a half-way point
    tie = (d != 0.0) & (other.astype(np.float32).astype(np.float64) == other) & (e != 0.0)
    if np.any(tie):
        lo, hi = np.minimum(r.astype(np.float64), other), np.maximum(r.astype(np.float64), other)
        r = np.where(tie, np.where(e > 0.0, hi, lo), r.astype(np.float64)).astype(np.float32)
    return r


def fmaf_exact(a, b, c):
    """the same in rational arithmetic, one value at a time (the evaluator's reference)"""
    t = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return round_f32(t)


def round_f32(t):
    """a Fraction to the nearest float32, ties to even (normal range)"""
    if t == 0:
        return np.float32(0.0)
    sign = -1 if t < 0 else 1
    t = abs(t)
    e = 0
    while t >= 2:
        t /= 2
        e += 1
    while t < 1:
        t *= 2
        e -= 1
    m = t * (1 << 23)
    f = m.numerator // m.denominator
    rem = m - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f & 1):
        f += 1
    return np.float32(sign * float(Fraction(f, 1 << 23) * Fraction(2) ** e))


def _padded_index(chains):
    n = max(len(ch) for ch in chains)
    idx = np.full((n, len(chains)), -1, dtype=np.int64)
    for c, ch in enumerate(chains):
        idx[:len(ch), c] = ch
    return idx


def chain_dot(form, rows, q):
    """q . x of every row as the fp32 kernel form accumulates it, bit for bit (float32 [n])"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32)
    chains, join = chain_map(form, F32, rows.shape[1])
    idx = _padded_index(chains)
    xz = np.concatenate([rows, np.zeros((rows.shape[0], 1), np.float32)], axis=1)   # index -1: the zero padding
    qz = np.concatenate([q, np.zeros(1, np.float32)])
    acc = np.zeros((rows.shape[0], idx.shape[1]), dtype=np.float32)
    for step in idx:
        acc = fmaf(xz[:, step], qz[step][None, :], acc)
    if join == "pairs":
        return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    total = np.zeros(rows.shape[0], dtype=np.float32)
    for c in range(acc.shape[1]):
        total = total + acc[:, c]
    return total


def chain_dot_exact(form, row, q):
    """one row, in rational arithmetic"""
    chains, join = chain_map(form, F32, len(row))
    accs = []
    for ch in chains:
        a = np.float32(0.0)
        for i in ch:
            a = fmaf_exact(row[i], q[i], a)
        accs.append(a)
    add = lambda x, y: round_f32(Fraction(float(x)) + Fraction(float(y)))  # noqa: E731
    if join == "pairs":
        return add(add(accs[0], accs[1]), add(accs[2], accs[3]))
    total = np.float32(0.0)
    for a in accs:
        total = add(total, a)
    return total


def row_norms(rows, dtype=F32):
    """|x|^2 as row_norms_kernel computes it (kernels_mfma.hip:1276-1296): lane l folds vectors l, l + 64, ... with one
    fmaf per element, then the 64 lanes are added by a butterfly (xor 32, 16, .. 1); lane 0's value"""
    np_t = np.float32 if dtype == F32 else np.float16
    rows = np.ascontiguousarray(rows, dtype=np_t).astype(np.float32)
    per = 4 if dtype == F32 else 8
    n, dim = rows.shape
    ld = padded(dim, dtype)
    nvec = ld // per
    trips = (nvec + 63) // 64
    x = np.zeros((n, trips * 64 * per), dtype=np.float32)
    x[:, :dim] = rows
    x = x.reshape(n, trips, 64, per)
    acc = np.zeros((n, 64), dtype=np.float32)
    for t in range(trips):
        for j in range(per):
            acc = fmaf(x[:, t, :, j], x[:, t, :, j], acc)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ m]
    return acc[:, 0]


def l2_values(form, rows, q):
    """fma(-2, q.x, |x|^2): the pre-filter value of every row, as the fp32 kernels produce it"""
    return fmaf(np.float32(-2.0), chain_dot(form, rows, q), row_norms(rows))


def true_values(rows, q):
    """|x|^2 - 2 q.x in float64"""
    x = np.asarray(rows).astype(np.float64)
    q64 = np.asarray(q).astype(np.float64)
    return np.sum(x * x, axis=1) - 2.0 * (x @ q64)


def exact_form_f32(rows, q):
    """sum((q - x)^2) in the reference's fp32 form (one accumulator, elements in order): what decides among candidates"""
    rows = np.asarray(rows, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32)
    acc = np.zeros(rows.shape[0], dtype=np.float32)
    for i in range(rows.shape[1]):
        d = q[i] - rows[:, i]
        acc = fmaf(d, d, acc)
    return acc


# ------------------------------------------------------------------------------------------------- swamping inputs
SMALL = 2.0 ** -12


def swamp(form, dtype, dim, direction, n=1):
    """(rows [n x dim], q): every chain's first product is 1, every later one 2^-24 (1 -+ DELTA): with direction -1 the
    accumulator never moves and the computed dot product is too SMALL by ~u per product; with +1 it steps a whole ulp
    every time and comes out too LARGE by as much.  All values are fp16-representable.  claimed_fraction() says how much
    of g_dot |q||x| that is."""
    chains, _ = chain_map(form, dtype, dim)
    q = np.full(dim, SMALL, dtype=np.float32)
    x = np.full(dim, SMALL * (1.0 + direction * DELTA), dtype=np.float32)
    for ch in chains:
        if ch:
            q[ch[0]] = 1.0
            x[ch[0]] = 1.0
    return np.tile(x, (n, 1)), q


def heads(form, dtype, dim):
    return [ch[0] for ch in chain_map(form, dtype, dim)[0] if ch]


def claimed_fraction(form, dtype, dim, chain):
    """the error of a swamped dot product over gamma_(chain + 4) |q||x|, from the construction alone: (len - 1) products
    of 2^-24 (1 - DELTA) lost or gained per chain (the upward ones gain 2^-23 - p each), |q||x| ~ sum |q_i x_i|"""
    chains, _ = chain_map(form, dtype, dim)
    lost = sum(len(ch) - 1 for ch in chains if ch) * U * (1.0 - DELTA)
    total = sum(1.0 + (len(ch) - 1) * U * (1.0 + DELTA) for ch in chains if ch)
    return lost / (gamma_n(chain + 4.0) * total * (1.0 + 2.0 ** -18))


def attained_fraction(value, rows, q, chain):
    """|computed - true| / (gamma_(chain + 4) |q||x|) per row, the true dot product in float64"""
    x = np.asarray(rows).astype(np.float64)
    q64 = np.asarray(q).astype(np.float64)
    true = x @ q64
    return np.abs(np.asarray(value).astype(np.float64) - true) / (
        gamma_n(chain + 4.0) * np.linalg.norm(q64) * np.linalg.norm(x, axis=1))


# ------------------------------------------------------------------------------------------------- adversarial L2 sets
def approx_candidates(k):
    """pgv_abi_common.h approx_candidates"""
    if k <= 8:
        return 32
    if 4 * k > 256:
        return k + 64
    kp = 64
    while kp < 4 * k:
        kp <<= 1
    return kp


class BandSet:
    """rows, one query and the groups: `true` (one row T, the real nearest, its value swamped UP), `decoy` (k rows,
    truly farther, swamped DOWN), `filler` (honest rows, farther still, between the half band and T by value)"""

    def __init__(self, form, dtype, dim, k, rows, query, groups, chain):
        self.form, self.dtype, self.dim, self.k, self.chain = form, dtype, dim, k, chain
        np_t = np.float32 if dtype == F32 else np.float16
        self.rows = np.ascontiguousarray(rows, dtype=np_t)
        self.query = np.ascontiguousarray(query, dtype=np_t)
        assert (self.rows.astype(np.float64) == np.asarray(rows, dtype=np.float64)).all()   # representable as built
        self.groups = {g: np.asarray(v, dtype=np.int64) for g, v in groups.items()}

    def want(self):
        """the true top k (row indices, nearest first) by float64 distance"""
        d = np.sum((self.rows.astype(np.float64) - self.query.astype(np.float64)) ** 2, axis=1)
        return np.lexsort((np.arange(d.size), d))[:self.k], d

    def margins(self, values=None, bound=None):
        """from the modelled (or given) pre-filter values: T's rank by value, and how far the candidates reach past the
        k-th value in units of eps -- `inside_full` <= 2 <= and `outside_half` > 1 is what makes the set adversarial"""
        v = l2_values(self.form, self.rows, self.query) if values is None else np.asarray(values, dtype=np.float32)
        bound = bound or scan_bound(self.dim, self.dtype, self.chain)
        qn = row_norms(self.query[None, :], self.dtype)[0]
        rn = row_norms(self.rows, self.dtype).max()
        eps = float(band_eps(bound, qn, rn))
        order = np.lexsort((np.arange(v.size), v))
        kp = approx_candidates(self.k)
        a_k = float(v[order[self.k - 1]])
        t = int(self.groups["true"][0])
        cand = v[order[:kp]]
        return {"eps": eps, "a_k": a_k, "rank_T": int(np.flatnonzero(order == t)[0]), "kprime": kp,
                "T_over_ak": (float(v[t]) - a_k) / eps,
                "last_candidate": (float(cand[-1]) - a_k) / eps,
                "flag_full": bool((cand <= band_edge(bound, a_k, qn, rn, 2.0)).all()),
                "flag_half": bool((cand <= band_edge(bound, a_k, qn, rn, 1.0)).all()),
                "T_in_full_band": bool(v[t] <= band_edge(bound, a_k, qn, rn, 2.0))}


def band_set(form, dtype, dim, k=10, chain=None, seed=0, extra_fillers=6):
    """The attack on one kernel form.  q = 1 on the chain heads, 2^-12 elsewhere.
      T       heads 1 + 8 g (g = 2^-14 for fp32, 2^-10 for fp16: the grid near 1), the rest 2^-12 (1 - DELTA): the dot
              product is swamped DOWN, the value a = |x|^2 - 2 q.x comes out too LARGE by ~2 (chain - 1) u per chain
      decoy j heads 1 + (16 + j) g on the first head, the rest 2^-12 (1 + DELTA): swamped UP, a too SMALL; truly
              farther than T by ~((16 + j)^2 - 64) g^2 -- distinct, and apart by far more than g_ref times the distance
      filler  heads 1 + m_i g, the rest 0: no product rounds, a is honest; truly farther still, (dim - heads) 2^-24 +
              sum m_i^2 g^2 from q, chosen (from the model for fp32, from float64 for fp16) so that a lies past the
              half-width band and short of T
    More than k' - k fillers, so T ranks beyond k' by value."""
    chain = chain if chain is not None else scan_chain_length(dim, dtype, form in ("scan64",))
    rng = np.random.default_rng(seed)
    hd = heads(form, dtype, dim)
    g = 2.0 ** -14 if dtype == F32 else 2.0 ** -10
    _, q = swamp(form, dtype, dim, -1)
    t_row = swamp(form, dtype, dim, -1)[0][0].astype(np.float64)
    t_row[hd[0]] = 1.0 + 8 * g if dtype == F32 else 1.0
    decoys = np.tile(swamp(form, dtype, dim, +1)[0][0].astype(np.float64), (k, 1))
    # fp16: the grid near 1 is 2^-10, so the decoys take (a, b) steps on two heads with distinct a^2 + b^2 (<= 17)
    steps16 = ((1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (4, 0), (4, 1))
    assert dtype == F32 or (k <= len(steps16) and len(hd) >= 2)
    for j in range(k):
        if dtype == F32:
            decoys[j, hd[0]] = 1.0 + (16 + j) * g
        else:
            decoys[j, hd[0]] = 1.0 + steps16[j][0] * g
            decoys[j, hd[1]] = 1.0 + steps16[j][1] * g
    kp = approx_candidates(k)
    need = kp - k + extra_fillers
    bound = scan_bound(dim, dtype, chain)
    base = np.concatenate([t_row[None, :], decoys])
    np_t = np.float32 if dtype == F32 else np.float16
    qn = row_norms(q[None, :].astype(np_t), dtype)[0]
    rn = row_norms(base.astype(np_t), dtype).max()
    eps = float(band_eps(bound, qn, rn))
    if dtype == F32:
        v = l2_values(form, base, q)
        a_k, a_t = float(v[1:].max()), float(v[0])
    else:   # no bit-exact model: aim at the window the fp32 geometry would have, in float64
        tv = true_values(base.astype(np_t), q.astype(np_t))
        a_k, a_t = float(tv[1:].max()), float(tv[1:].max()) + 1.6 * eps
    lo, hi = a_k + 1.08 * eps, min(a_t - 0.04 * eps, a_k + 1.9 * eps)
    assert hi > lo, (lo, hi, eps)
    # a filler's true value is -|q|^2 + |x - q|^2; |x - q|^2 = tail + g^2 sum m_i^2 with tail = (dim - heads) 2^-24
    tail = (dim - len(hd)) * SMALL ** 2
    q2 = float(np.sum(q.astype(np.float64) ** 2))
    fillers, seen = [], set()
    for _ in range(200000):
        if len(fillers) >= need:
            break
        target = (rng.uniform(lo, hi) + q2 - tail) / g ** 2
        if target <= 0:
            continue
        m = np.zeros(len(hd))
        left = target
        for i in range(len(hd)):     # split the squared length over the heads
            part = left if i == len(hd) - 1 else rng.uniform(0.2, 0.8) * left
            m[i] = np.floor(np.sqrt(part)) * rng.choice([-1.0, 1.0])
            left -= m[i] ** 2
        key = tuple(m)
        if key in seen or np.abs(m).max() * g >= 0.25:
            continue
        f = np.zeros(dim)
        f[hd] = 1.0 + m * g
        val = (float(l2_values(form, f[None, :], q)[0]) if dtype == F32
               else float(true_values(f[None, :].astype(np_t), q.astype(np_t))[0]))
        if lo <= val <= hi:
            seen.add(key)
            fillers.append(f)
    assert len(fillers) >= need, (len(fillers), need, lo, hi)
    rows = np.concatenate([base, np.array(fillers)])
    labels = np.array(["true"] + ["decoy"] * k + ["filler"] * len(fillers))
    perm = rng.permutation(rows.shape[0])
    rows, labels = rows[perm], labels[perm]
    groups = {name: np.flatnonzero(labels == name) for name in ("true", "decoy", "filler")}
    return BandSet(form, dtype, dim, k, rows, q, groups, chain)


# ------------------------------------------------------------------------------------------------- the assignment
def argmin_bound(dim, dtype):
    """pgv_internal.h argmin_bound, deterministic mode: (gamma, gamma_exact) in fp32 arithmetic"""
    ld = padded(dim, dtype)
    u = np.float32(5.9604645e-8)
    n1, n2 = np.float32(ld + 1) * u, np.float32(ld + 2) * u
    return float(n1 / (np.float32(1.0) - n1)), float(n2 / (np.float32(1.0) - n2))


def argmin_reach(t, rho, gamma_scale=0.5, exact_scale=1.0):
    """(inversion, band) in units of gamma |c|^2 for a row a with |a| = t |c| and a.c = rho |a||c|: the chain runs from
    -|c|^2 / 2 to -|c|^2 / 2 + a.c monotonically at best, each product can cost at most u times the accumulator's
    magnitude, so one value errs by at most 2 gamma max|acc| and two values can be inverted by twice that; the band
    between two centers is 2 (gamma (|c|^2 + 2 |a||c|) + gamma_x d) with d = |a - c|^2, gamma_x ~ gamma; the scales
    are the mutation's (gamma halved: 0.5, 1)"""
    end = -0.5 + rho * t
    inversion = 4.0 * max(0.5, abs(end))
    d = 1.0 + t * t - 2.0 * rho * t
    band = 2.0 * (gamma_scale * (1.0 + 2.0 * t) + exact_scale * d)
    return inversion, band


def assign_set(dim, dtype, n_centers=96, n_rows=256):
    """(rows, centers, T): every row is a = (2, 2^-11, 2^-11, ...).  Center T = (2, 2^-12 (1 - DELTA), ...) is the true
    nearest; its chain goes -2, +2, then products of 2^-23 (1 - DELTA), just under half an ulp of an accumulator in
    [2, 4): it never moves and T's value comes out too LARGE.  Three decoys (2 + j 2^-9, 2^-12 (1 + DELTA), ...) step a
    whole ulp every time and come out too SMALL; they are truly farther by ~(j 2^-9)^2.  That is a third of the term per
    direction (argmin_reach(1, 1)): inside the band, so the rows must be rechecked -- and they are then decided by the
    exact form.  The other centers are far away ((-2 + j 2^-8, 0, ...))."""
    np_t = np.float32 if dtype == F32 else np.float16
    a = np.full(dim, 2.0 ** -11)
    a[0] = 2.0
    centers = np.zeros((n_centers, dim))
    centers[:, 0] = -2.0 + (1 + np.arange(n_centers)) * 2.0 ** -8
    t = n_centers // 2
    centers[t] = SMALL * (1.0 - DELTA)
    centers[t, 0] = 2.0
    for j, at in enumerate((3, t + 7, n_centers - 2), start=1):
        centers[at] = SMALL * (1.0 + DELTA)
        centers[at, 0] = 2.0 + j * 2.0 ** -9
    rows = np.tile(a, (n_rows, 1))
    assert (centers.astype(np_t) == centers).all() and (rows.astype(np_t) == rows).all()
    return np.ascontiguousarray(rows, dtype=np_t), np.ascontiguousarray(centers, dtype=np_t), t
