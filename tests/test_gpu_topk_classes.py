"""The batched selection runs as one kernel per class of segment length (kernels_select.hip: small <= 1024 values,
medium <= 4096, long: 4 / 12 / 16 resident float4 per thread, and 16 resident + up to 16 transient ones for segments
up to 32 768; past that, the general path), the class picked on the host from a bound on the segment length.  The result is defined exactly -- the k smallest by
(value, position), ties to the lower position -- so every case here is compared for equality.

All inputs are small integers: every inner product is an integer far below 2^24, exact in fp32 in any summation
order, and numpy alone is the reference.

  * fixed-length segments: pgv_rank_lists of an inner-product index with one row per list; 33 queries (more than
    24, fewer than 128) take dense_scan + launch_topk_segments over [33 x nlists].  nlists sits on, below and above
    every boundary between two forms; where it is no multiple of 4 the 33 segments start at every alignment.
  * variable segments: search_batch (probes 4, 40 queries) of indexes whose list lengths put segments on the
    boundaries, past 20 480, past 32 768 and down to 1-3 rows in one batch, and whose bound (the rows of the 4 longest lists)
    selects each class -- once far above every real segment.
"""
import numpy as np
import pytest

from pgvector_amd import api

DIM = 8
NQ_FIXED = 33
NLISTS = [1021, 1024, 1025, 4093, 4096, 4097, 12287, 12288, 12289, 16383, 16384, 16385, 20479, 20480, 20481,
          32767, 32768]  # (an index holds 32 768 lists at most; 32 767 lists start at every alignment: with the ragged front
#                            counted in, some of their segments are past the long class's last form)
MAXPROBES = [1, 10, 64, 129]


def _fixed_data(nlists, kind):
    """(centers, queries) as integer-valued float32"""
    rng = np.random.default_rng(1000 + nlists)
    if kind == "wide":      # few ties
        centers = rng.integers(-100, 101, size=(nlists, DIM))
    elif kind == "narrow":  # 17 distinct values at most: runs of equal keys longer than 256 and than 1024
        centers = rng.integers(-1, 2, size=(nlists, DIM))
    else:                   # every center the same: the ordered tie pass
        centers = np.tile(rng.integers(-100, 101, size=(1, DIM)), (nlists, 1))
    lo, hi = (-1, 2) if kind == "narrow" else (-100, 101)
    queries = rng.integers(lo, hi, size=(NQ_FIXED, DIM))
    return centers.astype(np.float32), queries.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("nlists", NLISTS)
def test_fixed_segments_every_boundary(ctx, nlists):
    offsets = np.arange(nlists + 1, dtype=np.int64)  # one row per list
    for kind in ("wide", "narrow", "equal"):
        centers, queries = _fixed_data(nlists, kind)
        vals = -(queries.astype(np.int64) @ centers.astype(np.int64).T)  # exact
        order = np.argsort(vals, axis=1, kind="stable")                  # ties to the lower list id
        ix = api.IvfIndex(ctx, api.PGV_NEG_IP, api.PGV_F32, DIM, centers, offsets, centers)
        try:
            for maxprobes in MAXPROBES:
                lists, dist = ix.rank_lists(queries, maxprobes)
                want = order[:, :maxprobes]
                assert np.array_equal(lists, want.astype(np.int32)), (nlists, kind, maxprobes)
                want_d = np.take_along_axis(vals, want, axis=1).astype(np.float32)
                assert np.array_equal(dist, want_d), (nlists, kind, maxprobes)
        finally:
            ix.close()


# ---------------------------------------------------------------------------------------------- variable segments
# 64 lists with centers (l, -l^2, 0, ...): a query (4 t + 1, 2, ...) scores list l as 2 (l - t - 1/4)^2 + const, so it
# probes t, t + 1, t - 1, t + 2 in that order -- the four lists of "window" w when t = 4 w + 1.
VAR_LISTS = 64
VAR_PROBES = 4
VAR_NQ = 40
VAR_T = [4 * w + 1 for w in range(16)] + [4 * w + 3 for w in range(15)] + [4 * w + 2 for w in range(9)]

VAR_LENS = {
    # the boundaries of the long class, segments past 20 480 and past 32 768, several of 1-3 rows; bound 32 769
    "edges": [4096, 4096, 4096, 4095,  4096, 4096, 4096, 4096,  4097, 4096, 4096, 4096,  5125, 5125, 5125, 5125,
              1, 0, 0, 0,  0, 1, 1, 0,  1, 1, 0, 1,  5120, 5120, 5120, 5120,
              3072, 3072, 3072, 3073,  1024, 1024, 1024, 1025,  256, 256, 256, 257,  3, 0, 0, 0,
              8192, 8192, 8192, 8193,  4000, 4000, 4000, 2336,  8192, 8192, 8192, 8190,  2048, 2047, 1, 0],
    # one long list per window: the bound (~20 000) is four times any real segment
    "loose": [x for w in range(16) for x in (5000 + w, 1, 2, 0)],
    # the four longest lists hold <= 4093 rows: the medium class, segments either side of 1024
    "medium": [x for w in range(16) for x in ((1000 + w, 3, 0, 1) if w % 2 == 0 else (400, 400, 400, 400 + w))],
    # ... <= 1021 rows: the small class
    "small": [x for w in range(16) for x in ((255, 255, 255, 254 - w) if w % 2 == 0 else (w, 0, 2, 1))],
}


def _variable_case(name):
    """the index's arrays, the queries, and per query the probed lists in probe order (numpy's own ranking)"""
    lens = np.asarray(VAR_LENS[name], dtype=np.int64)
    assert lens.shape[0] == VAR_LISTS and len(VAR_T) == VAR_NQ
    rng = np.random.default_rng(7)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offsets[-1])
    rows = rng.integers(-50, 51, size=(n, DIM)).astype(np.float32)
    tids = (np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(11))
    centers = np.zeros((VAR_LISTS, DIM), dtype=np.float32)
    centers[:, 0] = np.arange(VAR_LISTS)
    centers[:, 1] = -np.arange(VAR_LISTS) ** 2
    queries = rng.integers(-20, 21, size=(VAR_NQ, DIM)).astype(np.float32)
    queries[:, 0] = 4 * np.asarray(VAR_T) + 1
    queries[:, 1] = 2
    cvals = -(queries.astype(np.int64) @ centers.astype(np.int64).T)
    probe = np.argsort(cvals, axis=1, kind="stable")[:, :VAR_PROBES]
    seg_len = lens[probe].sum(axis=1)
    bound = int(np.sort(lens)[::-1][:VAR_PROBES].sum())
    return dict(lens=lens, offsets=offsets, rows=rows, tids=tids, centers=centers, queries=queries, probe=probe,
                seg_len=seg_len, bound=bound)


def test_variable_cases_have_the_intended_lengths():
    """CPU: the chosen centers rank the windows as intended, and the segment lengths and bounds are the ones the
    GPU test is about"""
    for name in VAR_LENS:
        c = _variable_case(name)
        for q, t in enumerate(VAR_T):
            assert c["probe"][q].tolist() == [t, t + 1, t - 1, t + 2], (name, q)
    e = _variable_case("edges")
    got = set(e["seg_len"].tolist())
    assert {16383, 16384, 16385, 20480, 20500, 32766, 12289, 4097, 1025, 14336, 4096}.issubset(got), sorted(got)
    assert max(got) == 32769 and e["bound"] == 32769
    assert {1, 2, 3}.issubset(got)
    loose = _variable_case("loose")
    assert loose["bound"] > 16384 + 3 and loose["seg_len"].max() < 5020  # the long class for segments a quarter of it
    med = _variable_case("medium")
    assert 1024 < med["bound"] + 3 <= 4096 and med["seg_len"].min() <= 1021 and med["seg_len"].max() > 1024
    small = _variable_case("small")
    assert small["bound"] + 3 <= 1024 and small["seg_len"].max() == 1019


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VAR_LENS))
def test_variable_segments(ctx, name):
    c = _variable_case(name)
    rows64, q64 = c["rows"].astype(np.int64), c["queries"].astype(np.int64)
    ix = api.IvfIndex(ctx, api.PGV_NEG_IP, api.PGV_F32, DIM, c["centers"], c["offsets"], c["rows"], c["tids"])
    try:
        heads = []  # per query: (distances, tids) of its whole segment, sorted by (distance, position)
        for q in range(VAR_NQ):
            slots = np.concatenate([np.arange(c["offsets"][l], c["offsets"][l + 1]) for l in c["probe"][q]])
            d = -(rows64[slots] @ q64[q])
            o = np.argsort(d, kind="stable")
            heads.append((d[o].astype(np.float32), c["tids"][slots[o]]))
        for k in (1, 10, 64):
            dist, _, tid = ix.search_batch(c["queries"], VAR_PROBES, k, want_tid=True)
            for q in range(VAR_NQ):
                wd, wt = heads[q]
                m = min(k, wd.shape[0])
                assert np.array_equal(dist[q, :m], wd[:m]), (name, k, q, int(c["seg_len"][q]))
                assert np.array_equal(tid[q, :m], wt[:m]), (name, k, q, int(c["seg_len"][q]))
                assert np.isposinf(dist[q, m:]).all() and (tid[q, m:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), (name, k, q)
    finally:
        ix.close()
