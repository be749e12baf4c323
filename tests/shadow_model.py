"""A host model of the fp16 residual shadow (pgvector_amd/csrc/kernels_shadow.hip), in numpy and float64, and the
adversarial data built with it.

The model restates what the shadow kernels compute -- the index scale s, the fp16 shadow rows, E and P, and per query
s_q, the cast query and the terms of the rounding band (pgv_internal.h, next to ScanBound) -- without the fp32 rounding
of the band's own arithmetic.  It is for BUILDING data whose margins are known, not for checking the kernels: the GPU
tests compare the kernels with the oracle.  Nothing here imports the package.

The two adversarial sets put a true neighbour behind more than k' other rows in shadow order, by almost the whole
representation term of the band (2 |q| E for rows, 2 |q - q^| P for the query), while filler rows sit between the
true neighbours and the decoys: a band that is too narrow proves the wrong candidate set complete."""
import numpy as np

H = 2.0 ** -12     # half an fp16 step in [0.5, 1) at the scales below (the step there is 2 H)
TAU = 2.0 ** -24   # how far the off-grid elements sit from the half-way point


def scale_for(m):
    """kernels_shadow.hip scale_for: 2^-s takes the largest magnitude m into [2^13, 2^14) (0 / non-finite: 0)"""
    m = float(m)
    if not (m > 0.0) or not np.isfinite(m):
        return 0
    return int(np.frexp(m)[1]) - 14


def list_of_rows(list_offsets):
    off = np.asarray(list_offsets, dtype=np.int64)
    return np.repeat(np.arange(off.size - 1), np.diff(off))


def shadow_rows(rows, centers, list_offsets):
    """(s, the fp16 shadow rows, E, P): fp16(float32(x - c_l) 2^-s), round to nearest even like __float2half, and the
    largest |rho - 2^s shadow| and |2^s shadow| over the rows, in float64"""
    rows = np.asarray(rows, dtype=np.float32)
    centers = np.asarray(centers, dtype=np.float32)
    rho32 = rows - centers[list_of_rows(list_offsets)]
    s = scale_for(np.max(np.abs(rho32))) if rho32.size else 0
    sh = np.ldexp(rho32, -s).astype(np.float32).astype(np.float16)
    back = np.ldexp(sh.astype(np.float64), s)
    rho = rows.astype(np.float64) - centers[list_of_rows(list_offsets)].astype(np.float64)
    E = float(np.sqrt(np.max(np.sum((rho - back) ** 2, axis=1))))
    P = float(np.sqrt(np.max(np.sum(back ** 2, axis=1))))
    return s, sh, E, P


def cast_query(q):
    """(s_q, fp16 query): fp16(q 2^-s_q) with s_q from the query's own largest |q_i|"""
    q = np.asarray(q, dtype=np.float32)
    sq = scale_for(np.max(np.abs(q)))
    return sq, np.ldexp(q, -sq).astype(np.float32).astype(np.float16)


def query_terms(q, s, E, P, dot_chain=None):
    """the parts of shadow_query_kernel's qeps for one query, in float64 (the fp32 rounding-up is left out):
    rep_rows = 2 |q| E, rep_query = 2 |q - q^| P, dot = gamma_(chain + 4) 2 |q^| P, and `exponent` = 1 + s + s_q,
    outside [-125, 125] of which the kernel makes the whole term infinite"""
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    sq, qh = cast_query(q)
    back = np.ldexp(qh.astype(np.float64), sq)
    u = 2.0 ** -24
    n = (dot_chain if dot_chain is not None else chain_length(q64.size)) + 4.0
    g_dot = n * u / (1.0 - n * u)
    t = {"s_q": sq, "exponent": 1 + s + sq, "qn": float(np.linalg.norm(q64)), "dq": float(np.linalg.norm(q64 - back)),
         "qh": float(np.linalg.norm(back))}
    t["rep_rows"] = 2.0 * t["qn"] * E
    t["rep_query"] = 2.0 * t["dq"] * P
    t["dot"] = g_dot * 2.0 * t["qh"] * P
    t["eps"] = t["rep_rows"] + t["rep_query"] + t["dot"]
    return t


def chain_length(dim):
    """kernels_mfma.hip shadow_chain_length: products per accumulator chain of the fp16 scan's widest form (64 halves a
    slice, whole slices padded)"""
    n = (dim + 63) // 64
    return max(16 * n, 32 * ((n + 1) // 2), 64 * ((n + 3) // 4))


def exact_values(rows, q):
    """|x|^2 - 2 q.x in float64: the quantity the scan ranks by (the distance minus |q|^2)"""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    return np.sum(x * x, axis=1) - 2.0 * (x @ q64)


def shadow_values(rows, centers, list_offsets, q):
    """the pre-filter value of every row for query q as the shadow scan forms it, in float64:
    |x|^2 - 2 q.c_l - 2^(1 + s + s_q) (q^ . shadow)"""
    s, sh, _, _ = shadow_rows(rows, centers, list_offsets)
    sq, qh = cast_query(q)
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)
    c = np.asarray(centers, dtype=np.float32).astype(np.float64)[list_of_rows(list_offsets)]
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    acc = sh.astype(np.float64) @ qh.astype(np.float64)
    return np.sum(x * x, axis=1) - 2.0 * (c @ q64) - np.ldexp(acc, 1 + s + sq)


class AdversarialSet:
    """one list (center 0), a query and the row groups: `true` (the real top 10), `decoy` (look nearer in shadow
    order), `filler` (on the fp16 grid, between the two), `other` (the sentinel)"""

    def __init__(self, rows, query, groups):
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.query = np.ascontiguousarray(query, dtype=np.float32)
        self.groups = {k: np.asarray(v, dtype=np.int64) for k, v in groups.items()}
        self.centers = np.zeros((1, self.rows.shape[1]), dtype=np.float32)
        self.list_offsets = np.array([0, self.rows.shape[0]], dtype=np.int64)

    def model(self):
        s, sh, E, P = shadow_rows(self.rows, self.centers, self.list_offsets)
        return s, sh, E, P, query_terms(self.query, s, E, P)


def row_inversion_set(dim=256, m=8, n_true=10, n_decoy=20, n_filler=50, seed=0):
    """Rows off the fp16 grid, query exact (q = 1: |q - q^| = 0).  A sentinel row with one element at -1 fixes s = -13,
    where [0.5, 1) has the fp16 step 2 H.  True rows sit just below a half step (0.75 + H - TAU: rounded down, error +H
    along q); decoy rows just above one, moved by +-2 H m on alternate elements (rounded up, error -H; exactly farther by
    about 1024 H^2 m^2).  Fillers lie on the grid, 318..367 H above the true rows in exact value: behind the decoys
    and ahead of the true rows in shadow order, and past half the band."""
    assert dim % 2 == 0 and dim >= 240
    rng = np.random.default_rng(seed)
    q = np.ones(dim, dtype=np.float32)
    sentinel = np.full(dim, 0.75, dtype=np.float32)
    sentinel[0] = -1.0
    true = np.full((n_true, dim), 0.75 + H - TAU, dtype=np.float32)
    sign = np.where(np.arange(dim) % 2 == 0, 1.0, -1.0)
    decoy = np.empty((n_decoy, dim), dtype=np.float32)
    for i in range(n_decoy):
        decoy[i] = 0.75 + H + TAU + 2 * H * m * (sign if i % 2 == 0 else -sign)
    filler = np.full((n_filler, dim), 0.75, dtype=np.float32)
    for i in range(n_filler):
        lowered = rng.permutation(dim)[:190 + i]
        filler[i, lowered] = np.float32(0.75 - 2 * H)
    return _assemble(rng, sentinel, true, decoy, filler, q)


def query_inversion_set(dim=256, j=12, n_true=10, n_decoy=20, n_filler=50, seed=1):
    """Rows ON the fp16 grid (E = 0), the query just off its half steps: q_i = 0.75 + H - sigma_i TAU with sigma
    alternating, so q - q^ = sigma (H - TAU).  True rows 0.5 sigma + 2 H j on one element of each sign (exactly nearer by
    about 6 H j), decoys -0.5 sigma: the query's rounding pushes the true rows up by 256 (H - TAU) and the decoys down as
    much.  Fillers 0.5 tau (tau orthogonal to sigma: no push) moved down on pairs of elements to sit 230..248 H above
    the true rows."""
    assert dim % 4 == 0 and dim >= 64
    rng = np.random.default_rng(seed)
    sigma = np.where(np.arange(dim) % 2 == 0, 1.0, -1.0)
    tau = np.where(np.arange(dim) % 4 < 2, 1.0, -1.0)
    q = (0.75 + H - sigma * TAU).astype(np.float32)
    true = np.tile(0.5 * sigma, (n_true, 1))
    true[:, 0] += 2 * H * j
    true[:, 1] += 2 * H * j
    decoy = np.tile(-0.5 * sigma, (n_decoy, 1))
    filler = np.tile(0.5 * tau, (n_filler, 1))
    pairs = np.arange(0, dim, 4)
    for i in range(n_filler):
        units = 78 + i % 9  # total downward shift in steps of 2 H, spread over four pairs (elements 4p, 4p + 1)
        chosen = rng.choice(pairs, 4, replace=False)
        split = np.full(4, units // 4)
        split[:units % 4] += 1
        for p, k in zip(chosen, split):
            filler[i, p] -= 2 * H * k
            filler[i, p + 1] -= 2 * H * k
    return _assemble(rng, None, true.astype(np.float32), decoy.astype(np.float32), filler.astype(np.float32), q)


def _assemble(rng, sentinel, true, decoy, filler, q):
    """rows in a shuffled stream order (no group is favoured by its position)"""
    parts = [("true", true), ("decoy", decoy), ("filler", filler)]
    if sentinel is not None:
        parts.append(("other", sentinel[None, :]))
    rows = np.concatenate([p for _, p in parts]).astype(np.float32)
    labels = np.concatenate([[name] * len(p) for name, p in parts])
    perm = rng.permutation(rows.shape[0])
    rows, labels = rows[perm], labels[perm]
    groups = {name: np.flatnonzero(labels == name) for name, _ in parts}
    return AdversarialSet(rows, q, groups)


def approx_candidates(k):
    """pgv_abi_common.h: the candidates k' the batched L2 scan takes by pre-filter value"""
    if k <= 8:
        return 32
    if 4 * k > 256:
        return k + 64
    kp = 64
    while kp < 4 * k:
        kp <<= 1
    return kp
