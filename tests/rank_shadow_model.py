"""A host model of the center shadow: the fp16 copy of an fp32 L2 index's centers that the batch
ranking multiplies, its rounding band (pgv_internal.h, "The center shadow"), and the chain that hands the pair terms
t = -2 q.c_l from the ranking's exact recheck to the shadow scan (kernels_query.hip group_distance_dot).  numpy only;
float64 for the truth and the band, float32 operation by operation for what the kernels compute.  Nothing here imports
the package."""
import numpy as np

import shadow_model as sm

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)


def gamma(n):
    return n * U / (1.0 - n * U)


def row_geom_f32(dim):
    """kernels_scan.hip row_geom for fp32 rows: (ld, nvec, lg)"""
    ld = (dim + 3) // 4 * 4
    nvec = ld // 4
    best_lg, best_cost = 6, -1
    for lg in range(6, -1, -1):
        lpr = 1 << lg
        trips = (nvec + lpr - 1) // lpr
        cost = (trips * lpr - nvec) * 64 // lpr
        if trips > 64:
            continue
        if best_cost < 0 or cost < best_cost:
            best_cost, best_lg = cost, lg
    return ld, nvec, best_lg


def pair_chain_length(dim):
    """pgv_internal.h pair_chain_length: roundings on the way to t, the longer of the two routes"""
    ld, nvec, lg = row_geom_f32(dim)
    by_pair_kernel = (ld + 63) // 64 + 6
    per_lane = (nvec + (1 << lg) - 1) >> lg
    by_recheck = 4 * ((per_lane + 1) // 2) + 1 + lg
    return max(by_pair_kernel, by_recheck), by_pair_kernel, by_recheck


def cast_centers(centers):
    """(s_c, fp16 centers, E_c, P_c): fp16(c 2^-s_c), E_c = max |c - 2^s_c c~|, P_c = max |2^s_c c~| in float64"""
    c = np.asarray(centers, dtype=np.float32)
    s = sm.scale_for(np.max(np.abs(c))) if c.size else 0
    with np.errstate(over="ignore", under="ignore"):
        ch = np.ldexp(c, -s).astype(np.float32).astype(np.float16)
    back = np.ldexp(ch.astype(np.float64), s)
    E = float(np.sqrt(np.max(np.sum((c.astype(np.float64) - back) ** 2, axis=1))))
    P = float(np.sqrt(np.max(np.sum(back ** 2, axis=1))))
    return s, ch, E, P


def rank_band(q, s_c, E_c, P_c, cn_max, dim):
    """shadow_query_kernel's ceps for one query plus the recheck's g_norm term, in float64 (the width of a - s the
    ranking allows for), and the exponent 1 + s_c + s_q"""
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    sq, qh = sm.cast_query(q)
    back = np.ldexp(qh.astype(np.float64), sq)
    qn, dq, qhn = np.linalg.norm(q64), np.linalg.norm(q64 - back), np.linalg.norm(back)
    g_dot = gamma(sm.chain_length(dim) + 4.0)
    ld = (dim + 3) // 4 * 4
    g_norm = gamma(ld / 64.0 + 10.0)
    cn = cn_max * (1.0 + g_norm)
    eps = 2.0 * (qn * E_c + dq * P_c) + g_dot * 2.0 * qhn * P_c + 4.0 * U * (cn + 2.0 * qhn * P_c * (1.0 + g_dot))
    eps = eps * (1.0 + 2.0 ** -20) + 4.0 * FLT_MIN
    e = 1 + s_c + sq
    if e < -125 or e > 125 or not eps < 1e30:
        eps = np.inf
    return eps + g_norm * cn_max, e


def center_norms_f32(centers):
    """row_norms_kernel: per lane one fmaf chain over its 16-byte vectors (4 elements each), 6 shuffle additions"""
    c = np.asarray(centers, dtype=np.float32)
    ld = (c.shape[1] + 3) // 4 * 4
    x = np.zeros((c.shape[0], (ld + 255) // 256 * 256), dtype=np.float32)
    x[:, :c.shape[1]] = c
    x = x.reshape(c.shape[0], -1, 64, 4)  # [row, trip, lane, element]
    acc = np.zeros((c.shape[0], 64), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for t in range(x.shape[1]):
            for e in range(4):
                acc = _fma32(x[:, t, :, e], x[:, t, :, e], acc)
        for o in (32, 16, 8, 4, 2, 1):
            acc = (acc + acc[:, np.arange(64) ^ o]).astype(np.float32)
    return acc[:, 0]


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product and sum are exact in float64 unless the exponents lie ~29 apart (then the
    double rounding can differ from fmaf's by one fp32 ulp of the smaller term: far inside every bound checked here)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def ranking_values_f32(centers, queries):
    """what the fp16 ranking computes for every (query, center), fp32 step by step: four interleaved accumulator chains
    over the fp16 products (chain = element // 16 % 4 is one of the kernel's forms; any split into four is within the
    same bound), joined pairwise, then fmaf(-2^(1 + s_c + s_q), acc, |c|^2).  Returns (values [nq x nc], exponents)"""
    c = np.asarray(centers, dtype=np.float32)
    s_c, ch, _, _ = cast_centers(c)
    cn = center_norms_f32(c)
    out = np.empty((len(queries), c.shape[0]), dtype=np.float32)
    exps = []
    dim = c.shape[1]
    pad = (-dim) % 64
    chp = np.pad(ch.astype(np.float32), ((0, 0), (0, pad)))
    for i, q in enumerate(queries):
        sq, qh = sm.cast_query(q)
        qp = np.pad(qh.astype(np.float32), (0, pad))
        prod = chp * qp[None, :]  # exact in fp32: fp16 x fp16
        acc = np.zeros((c.shape[0], 4), dtype=np.float32)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            for j in range(prod.shape[1]):
                k = (j // 16) % 4
                acc[:, k] = (acc[:, k] + prod[:, j]).astype(np.float32)
            tot = ((acc[:, 0] + acc[:, 1]).astype(np.float32) + (acc[:, 2] + acc[:, 3]).astype(np.float32)).astype(np.float32)
            e = 1 + s_c + sq
            f = np.float32(np.ldexp(1.0, min(max(e, -125), 125)))
            out[i] = _fma32(-f * np.ones_like(tot), tot, cn)
        exps.append(e)
    return out, exps


def true_values(centers, queries):
    c = np.asarray(centers, dtype=np.float32).astype(np.float64)
    q = np.asarray(queries, dtype=np.float32).astype(np.float64)
    return (c * c).sum(1)[None, :] - 2.0 * q @ c.T


def recheck_dot_f32(q, c):
    """group_distance_dot's q.c for one row, fp32 step by step: 2^lg lanes, each two fmaf chains taking its vectors in
    turn, one addition, lg DPP additions (pairwise over the lanes)"""
    q = np.asarray(q, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    ld, nvec, lg = row_geom_f32(q.size)
    lpr = 1 << lg
    qp = np.zeros(ld, dtype=np.float32)
    cp = np.zeros(ld, dtype=np.float32)
    qp[:q.size], cp[:c.size] = q, c
    lanes = np.zeros(lpr, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for lane in range(lpr):
            d = [np.float32(0), np.float32(0)]
            for n, v in enumerate(range(lane, nvec, lpr)):
                for e in range(4):
                    d[n & 1] = _fma32(qp[4 * v + e], cp[4 * v + e], d[n & 1])
            lanes[lane] = np.float32(d[0] + d[1])
        w = lanes
        while w.size > 1:  # (the DPP network adds lanes pairwise, lg levels)
            w = (w[0::2] + w[1::2]).astype(np.float32)
    return np.float32(-2.0) * w[0]
