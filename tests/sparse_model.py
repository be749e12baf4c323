"""numpy model of the sparsevec entries (pgv_sparse_distance_batch, pgv_sparse_cosine_distance_batch, pgv_sparse_topk) in
float64: what tests/test_gpu_sparse.py compares the device against, itself pinned by tests/test_sparse_model_cpu.py to the
reference's recorded results (tests/golden/sparsevec_known_answers.json).

Vectors are CSR triples (ptr int64 [n + 1], idx int32, val float32).  A distance is the sum of the terms the reference adds
(src/sparsevec.c:826-1060), found by intersecting the two sorted index lists:
    L2 squared      (a - b)^2 on a shared index, a^2 and b^2 on an index only one side stores
    inner product   a * b on shared indices only (the kernel value is its negation)
    L1              |a - b|, |a|, |b|
    cosine          1 - clamp(ip / sqrt(na * nb)) from the three sums, each rounded to fp32 first (they are floats there)
The terms are formed and added in float64 ("exact": every term of fp32 data is exact or within 2^-53 in float64); the
kernel value is that sum rounded to fp32, which is the reference's result whenever its fp32 arithmetic is exact (integer
data) and its +-Infinity when the sum leaves fp32's range.  Beside each value come S = sum |term| and the term count m:
any order of m fp32 additions of terms carrying at most two roundings each is within (m + 2) 2^-24 S of exact."""
import numpy as np

L2SQ, NEG_IP, L1 = 0, 1, 2  # pgv_metric


def parse(text):
    """'{1:3,2:4}/2' (1-based indices, any order of the text's elements kept sorted) -> (dim, idx int32, val float32)"""
    body, dim = text.strip().rsplit("/", 1)
    items = [e.split(":") for e in body.strip()[1:-1].split(",") if e.strip()]
    pairs = sorted((int(i) - 1, np.float32(v)) for i, v in items)
    return int(dim), np.array([p[0] for p in pairs], dtype=np.int32), np.array([p[1] for p in pairs], dtype=np.float32)


def csr(vectors):
    """[(idx, val), ..] -> (ptr, idx, val)"""
    ptr = np.zeros(len(vectors) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(i) for i, _ in vectors])
    idx = np.concatenate([np.asarray(i, dtype=np.int32) for i, _ in vectors] + [np.zeros(0, dtype=np.int32)])
    val = np.concatenate([np.asarray(v, dtype=np.float32) for _, v in vectors] + [np.zeros(0, dtype=np.float32)])
    return ptr, idx, val


def vector(rows, r):
    ptr, idx, val = rows
    return idx[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]]


def _one_side(metric, x):
    return x * x if metric == L2SQ else np.abs(x)


def _both(metric, a, b):
    if metric == NEG_IP:
        return a * b
    return (a - b) ** 2 if metric == L2SQ else np.abs(a - b)


def _intersect(query, rows):
    """per stored row element: its row, whether the query stores its index, and where"""
    qi = np.asarray(query[0], dtype=np.int64)
    ptr, idx, _ = rows
    n = len(ptr) - 1
    row_of = np.repeat(np.arange(n), np.diff(ptr))
    pos = np.searchsorted(qi, idx)
    hit = np.zeros(len(idx), dtype=bool)
    if len(qi):
        inside = pos < len(qi)
        hit[inside] = qi[pos[inside]] == idx[inside]
    return n, row_of, pos, hit


def sums(metric, query, rows):
    """one query against every row -> (exact [n] float64: the sum of the reference's terms -- the inner product itself
    for NEG_IP --, S [n] = sum |term|, m [n] = how many terms)"""
    n, row_of, pos, hit = _intersect(query, rows)
    qv = np.asarray(query[1], dtype=np.float64)
    rv = np.asarray(rows[2], dtype=np.float64)
    matched_q = np.zeros(len(rv))
    matched_q[hit] = qv[pos[hit]]
    if metric == NEG_IP:
        terms = np.where(hit, rv * matched_q, 0.0)
        m = np.bincount(row_of[hit], minlength=n)
        tail = tail_abs = np.zeros(n)
    else:
        terms = np.where(hit, _both(metric, rv, matched_q), _one_side(metric, rv))
        # the query's elements no row element met, row by row
        unmatched = np.ones((n, len(qv)), dtype=bool)
        unmatched[row_of[hit], pos[hit]] = False
        tail = (unmatched * _one_side(metric, qv)[None, :]).sum(axis=1)
        tail_abs = tail
        m = np.diff(rows[0]) + unmatched.sum(axis=1)
    exact = np.bincount(row_of, weights=terms, minlength=n) + tail
    S = np.bincount(row_of, weights=np.abs(terms), minlength=n) + tail_abs
    return exact, S, m.astype(np.int64)


def to_fp32(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


def distances(metric, query, rows):
    """-> (kernel values [n] float32, exact [n] float64, S [n], m [n]); the NEG_IP values are negated"""
    exact, S, m = sums(metric, query, rows)
    if metric == NEG_IP:
        exact = -exact
    return to_fp32(exact), exact, S, m


def cosine(query, rows):
    """sparsevec_cosine_distance (src/sparsevec.c:972-1011) from the exact sums rounded to fp32 -> [n] float64; NaN where
    a norm is zero or the sums left fp32's range"""
    ip = to_fp32(sums(NEG_IP, query, rows)[0]).astype(np.float64)
    na = np.float64(to_fp32((np.asarray(query[1], dtype=np.float64) ** 2).sum()))
    nb = to_fp32(np.bincount(_intersect(query, rows)[1], weights=np.asarray(rows[2], dtype=np.float64) ** 2,
                             minlength=len(rows[0]) - 1)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sim = ip / np.sqrt(na * nb)
        sim = np.where(sim > 1, 1.0, np.where(sim < -1, -1.0, sim))
        return 1.0 - sim


def topk(metric, queries, rows, k):
    """-> (dist [nq x k] float32, idx [nq x k] int64, bound inputs exact / S / m as [nq x n]): ascending by (value, row),
    +inf / -1 beyond n"""
    nq, n = len(queries[0]) - 1, len(rows[0]) - 1
    dist = np.full((nq, k), np.inf, dtype=np.float32)
    idx = np.full((nq, k), -1, dtype=np.int64)
    exact, S, m = np.zeros((nq, n)), np.zeros((nq, n)), np.zeros((nq, n), dtype=np.int64)
    for q in range(nq):
        d, exact[q], S[q], m[q] = distances(metric, vector(queries, q), rows)
        order = np.argsort(d, kind="stable")[:k]  # stable: equal values keep row order
        dist[q, :len(order)] = d[order]
        idx[q, :len(order)] = order
    return dist, idx, exact, S, m


def bound(S, m, rtol):
    """|fp32 sum in any order - exact| <= (m + 2) 2^-24 S; the project's rtol x S where that is the larger"""
    return np.maximum((np.asarray(m) + 2) * 2.0 ** -24, rtol) * np.asarray(S)


# ---- the reference's regression transcript (tests/golden/sparsevec_known_answers.json) --------------------------------
# SQL function -> (pgv_metric, the float8 post-op the caller applies to the fp32 kernel value)
SQL_FUNCTIONS = {"l2_distance": (L2SQ, np.sqrt), "inner_product": (NEG_IP, np.negative),
                 "negative_inner_product": (NEG_IP, np.asarray), "l1_distance": (L1, np.asarray)}


def printed(x):
    """a float8 as psql prints it (extra_float_digits 1: the shortest text that reads back)"""
    x = float(x)
    if np.isnan(x):
        return "NaN"
    if np.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    s = repr(x + 0.0)  # -0.0 + 0.0 = 0.0
    return s[:-2] if s.endswith(".0") else s


def known_answer(case, kernel=None):
    """the printed result of a golden case from `kernel(metric or "cosine", dim, a, b)` -> the fp32 kernel value (float8
    for cosine) of query a against the single row b; the model's own values when kernel is None"""
    dim, ai, av = parse(case["a"])
    _, bi, bv = parse(case["b"])
    a, b = (ai, av), csr([(bi, bv)])
    if case["fn"] == "cosine_distance":
        return printed(kernel("cosine", dim, a, b) if kernel else cosine(a, b)[0])
    metric, post = SQL_FUNCTIONS[case["fn"]]
    value = kernel(metric, dim, a, b) if kernel else distances(metric, a, b)[0][0]
    with np.errstate(invalid="ignore"):
        return printed(post(np.float64(value)))
