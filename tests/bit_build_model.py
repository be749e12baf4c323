"""Host model of the in-memory HNSW build's serial loop (InsertTupleInMemory, src/hnswbuild.c:436-476: HnswFindElementNeighbors,
the duplicate check, HnswUpdateNeighborsInMemory), for tests/test_bit_build_model_cpu.py and tests/test_gpu_bit_hnsw_build.py:
no GPU, no ctypes.  It composes the models the device code is already held to --

  hnsw_walk_model.walk               HnswSearchLayer per layer, qlevel = the insert level, layers = every searched layer's W
  hnsw_link_model.host_select        SelectNeighbors for the new element's own lists
  hnsw_link_model.update_connection  HnswUpdateConnection for every list the new element links into

-- over TWO distance functions, because a build under bit_jaccard_ops has two:

  key(q, e)      what the search ranks by: the reference's float8, exactly (for Jaccard a fractions.Fraction)
  value(q, ids)  what a candidate carries from then on: (float) of the float8 (HnswCandidate.distance is a float; the casts
                 are at src/hnswutils.c:1052 and :1336) -- what selection and HnswUpdateConnection compare
  pair(ids)      value() between all of ids, a float32 matrix

For Hamming (and for squared L2 on integer grids) the two are the same numbers.  W keeps the search's order: a new element's
list is not sorted again (sortCandidates == false, :1351), so two candidates whose float8 differ and whose floats are equal
stay in the float8's order, and CheckElementCloser's `<=` (:1052) sees them as equal.

Ties of the key are walked in the order hnsw_walk_model documents (the device's); the reference leaves it open."""
from contextlib import contextmanager

import numpy as np

import hnsw_link_model as lm_model
from hnsw_walk_model import walk

HEAPTIDS = 10  # HNSW_HEAPTIDS (src/hnsw.h)


@contextmanager
def _pairs_from(pair):
    """hnsw_link_model.update_connection takes its pair distances from pair_matrix(rows, metric, ids): for the duration of
    a build they come from `pair` instead (the model's rows are whatever the callables close over)"""
    saved = lm_model.pair_matrix
    lm_model.pair_matrix = lambda rows, metric, idx, reuse=False: np.asarray(pair(list(idx)), dtype=np.float32)
    try:
        yield
    finally:
        lm_model.pair_matrix = saved


def find_neighbors(e, level, levels, nbr_start, nbr, m, entry, ef_construction, key, value, pair):
    """HnswFindElementNeighbors for element e -> {lc: dict(w: W's ids nearest first, keys, dist: their floats,
    ids / sel_dist / closer: the selection in r's order)} for lc = min(level, entry's level) .. 0"""
    w = walk(lambda x: key(e, x), levels, nbr_start, nbr, m, entry, ef_construction, qlevel=level)
    out = {}
    for lc, (ids, keys) in w.layers.items():
        ids = np.asarray(ids, dtype=np.int32)
        dist = np.asarray(value(e, ids.tolist()), dtype=np.float32)
        lmax = 2 * m if lc == 0 else m
        tri = None
        if len(ids) > lmax:
            D = np.asarray(pair(ids.tolist()), dtype=np.float32)
            tri = np.concatenate([D[u, :u] for u in range(1, len(ids))])
        si, sd, sc = lm_model.host_select(ids, dist, tri, lmax)
        out[lc] = dict(w=ids.tolist(), keys=list(keys), dist=dist, ids=si, sel_dist=sd, closer=sc)
    return out


def build(levels, m, ef_construction, key, value, pair, same):
    """the serial loop over elements 0 .. n - 1 with the given levels; same(a, b): the two rows are equal byte for byte.
    -> dict(entry, nbr_start, nbr, dup_of, nelements, mismatches: updates where the reference's cached form of
    SelectNeighbors and Algorithm 4 with every flag recomputed disagreed -- none, ever)"""
    levels = np.ascontiguousarray(levels, dtype=np.int32)
    n = len(levels)
    g = lm_model.Graph(np.zeros((1, 1), np.float32), lm_model.L2, m, levels)
    nbr_start = np.zeros(n + 1, np.int64)
    nbr_start[1:] = np.cumsum((levels.astype(np.int64) + 2) * m)
    nbr = np.full(int(nbr_start[-1]), -1, np.int32)
    dup_of = np.full(n, -1, np.int32)
    heaptids = np.ones(n, np.int32)
    entry, linked = -1, 0

    def store(x, lc):
        lmax = 2 * m if lc == 0 else m
        o = int(nbr_start[x]) + (int(levels[x]) - lc) * m
        lst = g.list_of(x, lc).elem
        nbr[o:o + lmax] = -1
        nbr[o:o + len(lst)] = lst

    with _pairs_from(pair):
        for e in range(n):
            if entry < 0:
                entry, linked = e, 1
                continue
            found = find_neighbors(e, int(levels[e]), levels, nbr_start, nbr, m, entry, ef_construction, key, value, pair)
            # FindDuplicateInMemory (src/hnswbuild.c:313-364): the layer-0 neighbors in list order, out at the first one
            # that is not the same row; the first identical one with room takes the heap TID
            for ne in found[0]["ids"]:
                if not same(e, ne):
                    break
                if heaptids[ne] < HEAPTIDS:
                    heaptids[ne] += 1
                    dup_of[e] = ne
                    break
            if dup_of[e] >= 0:
                continue
            linked += 1
            g.nbatch += 1
            for lc in sorted(found, reverse=True):   # HnswUpdateNeighborsInMemory (src/hnswbuild.c:376-431)
                f = found[lc]
                lst = g.list_of(e, lc)
                lst.elem, lst.dist = [int(x) for x in f["ids"]], [float(x) for x in f["sel_dist"]]
                lst.cf, lst.closer_set = list(f["closer"]), False
                store(e, lc)
                for owner, d in zip(f["ids"], f["sel_dist"]):
                    lm_model.update_connection(g, owner, lc, e, d)
                    store(owner, lc)
            if levels[e] > levels[entry]:
                entry = e
    return dict(entry=entry, nbr_start=nbr_start, nbr=nbr, dup_of=dup_of, nelements=linked,
                mismatches=sum(1 for ev in g.events if ev["mismatch"]))


# --------------------------------------------------------------------------------------------------------- distances
def l2_functions(rows):
    """squared L2 over rows that are small integers: exact in fp32, key and value are the same numbers"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    pair_matrix = lm_model.pair_matrix   # (the function itself: build() stands `pair` in for the module's name)

    def key(q, e):
        d = rows[e] - rows[q]
        return float(np.dot(d, d))

    def value(q, ids):
        return lm_model.distances_to(rows, lm_model.L2, q, ids).astype(np.float32)

    def pair(ids):
        return pair_matrix(rows, lm_model.L2, ids)

    def same(a, b):
        return bool(np.array_equal(rows[a], rows[b]))
    return key, value, pair, same


def hamming_functions(packed):
    """bit_hamming_ops over packed rows: counts, exact"""
    from bit_model import hamming
    packed = np.ascontiguousarray(packed, dtype=np.uint8)

    def key(q, e):
        return int(hamming(packed[q], packed[e:e + 1])[0])

    def value(q, ids):
        return hamming(packed[q], packed[np.asarray(ids, dtype=np.int64)]).astype(np.float32)

    def pair(ids):
        return np.stack([value(i, ids) for i in ids])

    def same(a, b):
        return bool(np.array_equal(packed[a], packed[b]))
    return key, value, pair, same


def jaccard_functions(packed):
    """bit_jaccard_ops over packed rows: the search ranks by the exact ratio, the lists hold jaccard_model.ref_float"""
    import jaccard_model as jm
    packed = np.ascontiguousarray(packed, dtype=np.uint8)

    def key(q, e):
        x, u = jm.counts(packed[q], packed[e:e + 1])
        return jm.fraction(x[0], u[0])

    def value(q, ids):
        return jm.ref_floats(packed[q], packed[np.asarray(ids, dtype=np.int64)])

    def pair(ids):
        return np.stack([value(i, ids) for i in ids])

    def same(a, b):
        return bool(np.array_equal(packed[a], packed[b]))
    return key, value, pair, same


def table_functions(xu):
    """hand-made Jaccard cases: xu[(a, b)] = (x, u) for a < b (missing pairs are disjoint: distance 1); no two rows equal"""
    import jaccard_model as jm

    def get(a, b):
        return (0, 1) if a == b else xu.get((min(a, b), max(a, b)), (1, 1))

    def key(q, e):
        return jm.fraction(*get(q, e))

    def value(q, ids):
        return np.array([jm.ref_float(*get(q, i)) for i in ids], dtype=np.float32)

    def pair(ids):
        return np.stack([value(i, ids) for i in ids])
    return key, value, pair, lambda a, b: a == b
