"""The distance functions tests/bit_build_model.py takes, for a build over sparsevec elements (tests/test_sparse_build_model_cpu.py,
tests/test_gpu_sparse_hnsw_build.py): no GPU, no ctypes.

On a buildable sparse mirror the build-side value of the pair {a, b} of element slots is ONE number wherever it is computed:
score(row = the smaller slot, query = the larger slot), i.e. pgv_hnsw_score_pairs(a = min, b = max).  The
search ranks by it, the lists hold it, the selections compare it.  So a model of the build needs the values of all pairs
under that rule and nothing else: oriented_matrix() asks a scorer for them once -- pgv_hnsw_score_pairs on the device, or
sparse_model on the CPU -- and functions() hands them to bit_build_model.build as key, value and pair.  `same` looks at the
CSR bytes, as datumIsEqual does in FindDuplicateInMemory: the same number of stored elements, equal index bytes, equal
value bytes."""
import numpy as np

import sparse_model as sm


def oriented_pairs(a, b):
    """slot pairs as the rule scores them: (min, max)"""
    a, b = np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32)
    return np.minimum(a, b), np.maximum(a, b)


def oriented_matrix(score, n, chunk=1 << 20):
    """score(a, b) -> float32 values of (row a[i], query b[i]); D[x, y] = D[y, x] = score(min(x, y), max(x, y)) for all n
    elements, the diagonal included"""
    a, b = np.triu_indices(n)
    a, b = a.astype(np.int32), b.astype(np.int32)
    vals = np.concatenate([np.asarray(score(a[i:i + chunk], b[i:i + chunk]), dtype=np.float32) for i in range(0, len(a), chunk)])
    D = np.empty((n, n), dtype=np.float32)
    D[a, b] = vals
    D[b, a] = vals
    return D


def model_score(metric, csr):
    """sparse_model's values for (row a[i], query b[i]) of the rows themselves: exact on integer data, where the order of the
    additions does not matter"""
    def score(a, b):
        out = np.empty(len(a), dtype=np.float32)
        for q in np.unique(b):
            at = np.flatnonzero(b == q)
            out[at] = sm.distances(metric, sm.vector(csr, int(q)), csr)[0][a[at]]
        return out
    return score


def same_bytes(csr):
    ptr, idx, val = csr
    idx, val = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(val, dtype=np.float32)

    def same(a, b):
        ia, ib = idx[ptr[a]:ptr[a + 1]], idx[ptr[b]:ptr[b + 1]]
        return len(ia) == len(ib) and ia.tobytes() == ib.tobytes() and \
            val[ptr[a]:ptr[a + 1]].tobytes() == val[ptr[b]:ptr[b + 1]].tobytes()
    return same


def functions(D, csr):
    """key, value, pair, same for bit_build_model.build from the matrix of oriented_matrix().  Keys are compared as Python
    floats: -0.0 and +0.0 tie, as they do under the walk's float_to_key"""
    def key(q, e):
        return float(D[q, e])

    def value(q, ids):
        return D[q, np.asarray(ids, dtype=np.int64)].astype(np.float32)

    def pair(ids):
        ids = np.asarray(ids, dtype=np.int64)
        return D[np.ix_(ids, ids)].astype(np.float32)
    return key, value, pair, same_bytes(csr)
