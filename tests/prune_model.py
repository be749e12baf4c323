"""Host model of probe pruning (pgvector_amd/csrc/pgv_internal.h, beside ScanBound): which probed lists of
one query the batched shadow scan may skip.  The same arithmetic as probe_margins / probe_near / probe_far / probe_dropped
and the host half of shadow_create's radii, in float64 -- square root, division, multiplication and addition are correctly
rounded on both sides, so for inputs with the same bits the model and the kernels decide alike.

    m     the smallest count such that probes 0 .. m-1 hold >= k rows together (none: nothing is dropped)
    tau   max over i < m of sqrt(d_i) + R_i
    probe j >= m is dropped iff sqrt(d_j) - R_j > tau          (with the margins below; equality keeps)
"""
import numpy as np

U = 2.0 ** -24


def margins(dim):
    """(g, a): relative and absolute rounding of an fp32 sum of ld squares of differences, ld = the padded row length"""
    ld = (dim + 3) // 4 * 4
    n = (ld + 4.0) * U
    return n / (1.0 - n), (ld + 4.0) * 2.0 ** -149


def radii(centers, off, rows):
    """R_l >= max |x - c_l| over list l's rows as the index keeps it: fp64, inflated by 1e-9, rounded UP into fp32; an
    empty list 0, anything non-finite +inf"""
    out = np.zeros(centers.shape[0], dtype=np.float32)
    for l in range(centers.shape[0]):
        x = rows[off[l]:off[l + 1]].astype(np.float64)
        if x.shape[0] == 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            r2 = float(np.max(np.sum((x - centers[l].astype(np.float64)) ** 2, axis=1)))
        R = np.sqrt(r2) * (1.0 + 1e-9) if r2 == r2 else np.inf
        if not np.isfinite(R):
            out[l] = np.inf
            continue
        f = np.float32(R)
        if float(f) < R:
            f = np.nextafter(f, np.float32(np.inf))
        out[l] = f
    return out


def center_distances(q, centers, lists):
    """the fp32 sum((q - c)^2) of the probed lists (the reference's form; any order of summation lies inside the margins).
    A list id < 0 (a fill entry) gets 0"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        c = centers[np.maximum(lists, 0)].astype(np.float32)
        d = np.sum((q.astype(np.float32)[None, :] - c) ** 2, axis=1, dtype=np.float32)
    return np.where(lists >= 0, d, np.float32(0)).astype(np.float32)


def dropped(d, R, lens, k, dim, lists=None):
    """d, R, lens: the probes' center distances (fp32), radii (fp32) and rows, in probe order -> bool per probe"""
    g, a = margins(dim)
    n = len(d)
    live = np.ones(n, dtype=bool) if lists is None else np.asarray(lists) >= 0
    d64, R64 = np.asarray(d, dtype=np.float64), np.asarray(R, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        near = np.where(live, np.sqrt((d64 + a) / (1.0 - g)) + R64, 0.0)
        far = np.sqrt(np.maximum(d64 - a, 0.0) / (1.0 + g)) - R64
    out = np.zeros(n, dtype=bool)
    rows, tau, finite, m = 0, 0.0, True, 0
    while m < n and rows < k:
        rows += int(lens[m]) if live[m] else 0
        finite = finite and bool(near[m] < np.inf)
        tau = near[m] if near[m] > tau else tau
        m += 1
    if rows < k or not finite:
        return out
    hi2 = tau * tau * (1.0 + g) + a
    if not hi2 < 3.0e38:
        return out
    for j in range(m, n):
        if not live[j] or not (far[j] > 0.0) or not (far[j] < np.inf):
            continue
        lo2 = far[j] * far[j] * (1.0 - g) - a
        out[j] = lo2 > hi2 * (1.0 + 2.0 ** -40)
    return out


def dropped_for(q, centers, off, R, lists, k):
    """the probes of `lists` (one query's, in probe order) that are dropped"""
    lists = np.asarray(lists)
    lens = np.where(lists >= 0, np.diff(off)[np.maximum(lists, 0)], 0)
    return dropped(center_distances(q, centers, lists), np.where(lists >= 0, R[np.maximum(lists, 0)], np.float32(0)),
                   lens, k, centers.shape[1], lists)


def rank_lists(q, centers, probes):
    """the `probes` nearest centers by the fp32 distance, ties to the lower id (GetScanLists)"""
    d = center_distances(q, centers, np.arange(centers.shape[0]))
    key = np.where(np.isnan(d), np.float32(np.inf), d)
    return np.argsort(key, kind="stable")[:probes].astype(np.int32)
