"""IVFFlat over bit strings on the device -- pgv_index_upload_bits and the scan entries on such an index
(hamming_list_kernel, the Hamming center ranking), pgv_bit_assign, pgv_bit_lloyd_step, pgv_bit_kmeans and the Python
builders on top -- against the numpy model of tests/bit_ivf_model.py, which tests/test_bit_ivf_model_cpu.py pins to the
oracle, to the literal transcription of the reference's ElkanKmeans and to the reference's recorded answer.  Everything
here is integer arithmetic: every comparison is exact equality of both distances and ids."""
import ctypes as C

import numpy as np
import pytest

import bit_ivf_model as im
import bit_model as bm
from helpers import assert_topk_equiv, gen
from oracle import pyoracle as po
from pgvector_amd import _lib, api
from bit_ivf_model import KMEANS_SHAPES, kmeans_case

pytestmark = pytest.mark.gpu

TASK_ROWS = 256     # rows of one task of hamming_list_kernel (kBitThreads, kernels_bit.hip)
SLICE_BITS = 1024   # kBitSliceBits: the bits of a row a lane holds in registers at a time


def tids_of(n):
    return (np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(7))


def make_index(ctx, nbits, lens, seed, rows=None, centers=None):
    """-> (BitIvfIndex, centers, offsets, rows): lists of the given lengths over random bit strings"""
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offsets[-1])
    rows = im.rand_bits(n, nbits, seed) if rows is None else rows
    centers = im.rand_bits(len(lens), nbits, seed + 1) if centers is None else centers
    return api.BitIvfIndex(ctx, nbits, centers, offsets, rows, tids=tids_of(n)), centers, offsets, rows


def check_search(ix, centers, offsets, rows, queries, probes, k, what, model=None):
    dist, slot, tid = ix.search_batch(queries, probes, k, want_tid=True)
    wd, ws, _ = model if model is not None else im.search(centers, offsets, rows, queries, probes, k)
    assert dist.dtype == np.float32 and slot.dtype == np.int64 and dist.shape == slot.shape == (queries.shape[0], k)
    assert np.array_equal(slot, ws), (what, "slots", np.argwhere(slot != ws)[:5].tolist())
    assert np.array_equal(dist, wd), (what, "distances", np.argwhere(dist != wd)[:5].tolist())
    want_tid = np.where(ws >= 0, tids_of(rows.shape[0] + 1)[np.maximum(ws, 0)], np.uint64(0xffffffffffffffff))
    assert np.array_equal(tid, want_tid), (what, "tids")


# ------------------------------------------------------------------------------------------------ the batched search
@pytest.mark.parametrize("nbits", [1, 7, 8, 9, 127, 128, 129, 136, SLICE_BITS - 1, SLICE_BITS, SLICE_BITS + 1, 1536, 4104, 64000])
def test_search_every_row_length(ctx, nbits):
    """whole bytes / ragged last byte, the 16-byte vector edge, an odd vector count (136), one below / at / one above the
    register slice, the headline 1536, five slices (4104) and the longest row an index may hold; 600 rows in 7 ragged
    lists, one of them empty"""
    ix, centers, offsets, rows = make_index(ctx, nbits, [130, 0, 257, 1, 90, 60, 62], 100 + nbits % 97)
    queries = im.rand_bits(5, nbits, 7)
    check_search(ix, centers, offsets, rows, queries, 3, 10, "nbits %d" % nbits)
    assert _lib.lib.pgv_index_nbits(ix.h) == nbits and ix.rows == 600 and _lib.lib.pgv_index_lists(ix.h) == 7
    ix.close()


@pytest.mark.parametrize("nbits", [0, 64001])
def test_upload_rejects_bit_lengths_outside_1_to_64000(ctx, nbits):
    nbytes = max(1, (nbits + 7) // 8)
    with pytest.raises(api.PgvError) as e:
        api.BitIvfIndex(ctx, nbits, np.zeros((1, nbytes), dtype=np.uint8), np.array([0, 1]), np.zeros((1, nbytes), dtype=np.uint8))
    assert e.value.code == _lib.PGV_ERR_DIMS


def test_search_task_edges(ctx):
    """lists of 0, 1, one below / exactly / one above a task's 256 rows and two tasks and one row; every list probed"""
    lens = [0, 1, TASK_ROWS - 1, TASK_ROWS, TASK_ROWS + 1, 2 * TASK_ROWS + 1]
    ix, centers, offsets, rows = make_index(ctx, 200, lens, 31)
    queries = im.rand_bits(3, 200, 32)
    check_search(ix, centers, offsets, rows, queries, len(lens), 50, "task edges")
    check_search(ix, centers, offsets, rows, queries, len(lens), int(offsets[-1]) + 5, "task edges, every row")
    ix.close()


@pytest.fixture(scope="module")
def group_case(ctx):
    ix, centers, offsets, rows = make_index(ctx, 96, [300, 40], 41)
    queries = im.rand_bits(65, 96, 42)
    yield ix, centers, offsets, rows, queries, im.search(centers, offsets, rows, queries, 2, 10)
    ix.close()


@pytest.mark.parametrize("nq", [1, 7, 8, 9, 16, 17, 31, 32, 33, 65])
def test_search_group_edges(group_case, nq):
    """two lists, both probed: exactly nq pairs on each list -- a group short of / exactly / one past 8, 16 and 32 pairs
    (the clamped tail pairs), and three groups (65).  The share nq x 2 / 2 = nq also walks the three instantiations:
    QT 8 below 8, QT 16 from 8 to 15, QT 32 from 16 on"""
    ix, centers, offsets, rows, queries, (wd, ws, wl) = group_case
    check_search(ix, centers, offsets, rows, np.ascontiguousarray(queries[:nq]), 2, 10, "nq %d" % nq,
                 model=(wd[:nq], ws[:nq], wl[:nq]))


@pytest.mark.parametrize("probes", [1, 5, 40])
def test_search_share_regimes(ctx, probes):
    """64 queries x 40 lists: 1.6, 8 and 64 queries per list on average.  The library has no hook that reports the
    instantiation; by hamming_list_group_size (kernels_bit.hip: the smallest QT the share stays below) probes 1 runs
    hamming_list_kernel<8>, probes 5 <16> and probes 40 <32>, where every list is split into two groups"""
    rng = np.random.default_rng(51)
    lens = rng.integers(0, 120, 40).tolist()
    ix, centers, offsets, rows = make_index(ctx, 300, lens, 52)
    queries = im.rand_bits(64, 300, 53)
    check_search(ix, centers, offsets, rows, queries, probes, 12, "probes %d" % probes)
    ix.close()


def test_search_ties_all_rows_identical(ctx):
    """every distance equal: the answer is the probe order (lower list id first among equal centers), then the position"""
    lens = [5, 300, 0, 7]
    rows = np.tile(im.rand_bits(1, 70, 61), (sum(lens), 1))
    centers = np.tile(im.rand_bits(1, 70, 62), (4, 1))
    ix, centers, offsets, rows = make_index(ctx, 70, lens, 0, rows=rows, centers=centers)
    queries = im.rand_bits(3, 70, 63)
    dist, slot, _ = ix.search_batch(queries, 4, 20)
    assert slot.tolist() == [list(range(20))] * 3  # lists 0, 1, 2, 3 in id order, rows in row order
    check_search(ix, centers, offsets, rows, queries, 4, 20, "identical rows")
    check_search(ix, centers, offsets, rows, queries, 2, 310, "identical rows, two lists")
    ix.close()


def test_search_long_tie_runs(ctx):
    """20 000 x 64-bit rows in 16 lists, probes 4, k 300: the heads hold runs of 100 and more equal distances, which only
    the insertion position orders"""
    nbits, lists = 64, 16
    rows0 = im.rand_bits(20000, nbits, 71)
    centers = im.rand_bits(lists, nbits, 72)
    assigned, _ = im.assign(centers, rows0)
    order = np.argsort(assigned, kind="stable")
    lens = np.bincount(assigned, minlength=lists).tolist()
    ix, centers, offsets, rows = make_index(ctx, nbits, lens, 0, rows=rows0[order], centers=centers)
    queries = im.rand_bits(4, nbits, 73)
    model = im.search(centers, offsets, rows, queries, 4, 300)
    for q in range(4):
        _, runs = np.unique(model[0][q], return_counts=True)
        assert runs.max() >= 100, runs
    check_search(ix, centers, offsets, rows, queries, 4, 300, "tie runs", model=model)
    ix.close()


def test_search_padding(ctx):
    """fewer than k tuples in the probed lists: +inf / -1 behind them; a query whose probed lists are all empty: nothing
    but padding"""
    nbits = 33
    centers = np.packbits(np.array([[0] * nbits, [1] * nbits, [1] * 16 + [0] * 17], dtype=np.uint8), axis=1)
    lens = [0, 4, 0]
    ix, centers, offsets, rows = make_index(ctx, nbits, lens, 81, centers=centers)
    queries = np.ascontiguousarray(centers[[1, 0, 2]])
    dist, slot, tid = ix.search_batch(queries, 1, 6, want_tid=True)
    assert (slot[0, :4] >= 0).all() and slot[0, 4:].tolist() == [-1, -1] and np.isinf(dist[0, 4:]).all()
    assert (slot[1:] == -1).all() and np.isinf(dist[1:]).all() and (tid[1:] == np.uint64(0xffffffffffffffff)).all()
    check_search(ix, centers, offsets, rows, queries, 1, 6, "padding")
    check_search(ix, centers, offsets, rows, queries, 2, 6, "padding, two probes")
    ix.close()


# ------------------------------------------------------------------------------------------------ the pieces
@pytest.mark.parametrize("nlists", [1, 31, 32, 33, 300])
def test_rank_lists(ctx, nlists):
    """GetScanLists with maxprobes = 1, 5 and nlists; one center, one below / at / one above 32 and more than one
    256-row tile of centers; duplicate centers resolve to the lower id"""
    nbits = 90
    centers = im.rand_bits(nlists, nbits, 90 + nlists)
    if nlists >= 31:
        centers[7] = centers[3]
        centers[nlists - 1] = centers[3]
    ix, centers, offsets, rows = make_index(ctx, nbits, [2] * nlists, 91, centers=centers)
    queries = np.concatenate([im.rand_bits(4, nbits, 92), centers[3:4]])
    for maxprobes in sorted({1, min(5, nlists), nlists}):
        lists, dist = ix.rank_lists(queries, maxprobes)
        wl, wd = im.rank_lists(centers, queries, maxprobes)
        assert lists.dtype == np.int32 and np.array_equal(lists, wl) and np.array_equal(dist, wd), maxprobes
    if nlists >= 31:
        assert lists[4, :3].tolist() == [3, 7, nlists - 1]
    ix.close()


def test_scan_lists(ctx):
    """the stream in probe order with its slots; a NULL query scores every tuple 0 (ZeroDistance); an output too small
    for the lists is an argument error that reports the count"""
    lens = [3, 0, TASK_ROWS + 5, 40]
    ix, centers, offsets, rows = make_index(ctx, 1030, lens, 111)
    query = im.rand_bits(1, 1030, 112)[0]
    for lists in ([2, 0, 3], [3], [1], [0, 1, 2, 3], [2, 2]):
        dist, slot = ix.scan_lists(query, lists)
        wd, ws = im.scan_stream(offsets, rows, query, lists)
        assert np.array_equal(slot, ws) and np.array_equal(dist, wd), lists
    dist, slot = ix.scan_lists(None, [3, 0])
    assert not dist.any() and slot.tolist() == list(range(offsets[3], offsets[4])) + [0, 1, 2]
    count = C.c_int64()
    lists = np.array([2], dtype=np.int32)
    small = np.empty(10, dtype=np.float32), np.empty(10, dtype=np.int64)
    rc = _lib.lib.pgv_scan_lists(ix.h, api.ptr(query), api.ptr(lists), 1, api.ptr(small[0]), api.ptr(small[1]), 10, C.byref(count))
    assert rc == _lib.PGV_ERR_ARG and count.value == TASK_ROWS + 5
    with pytest.raises(api.PgvError) as e:
        ix.scan_lists(query, [4])
    assert e.value.code == _lib.PGV_ERR_ARG
    ix.close()


def test_scan_batch_honours_the_callers_lists(ctx):
    lens = [30, 300, 0, 17, 64]
    ix, centers, offsets, rows = make_index(ctx, 257, lens, 121)
    queries = im.rand_bits(9, 257, 122)
    probe_lists = np.array([[4, 1, 0], [3, 2, 1], [0, 4, 3]] * 3, dtype=np.int32)  # not ascending, not by distance
    dist, slot, tid = ix.scan_batch(queries, probe_lists, 40, want_tid=True)
    wd, ws = im.scan_batch(offsets, rows, queries, probe_lists, 40)
    assert np.array_equal(slot, ws) and np.array_equal(dist, wd)
    assert np.array_equal(tid[ws >= 0], tids_of(rows.shape[0])[ws[ws >= 0]])
    bad = probe_lists.copy()
    bad[5, 1] = 5
    with pytest.raises(api.PgvError) as e:
        ix.scan_batch(queries, bad, 40)
    assert e.value.code == _lib.PGV_ERR_ARG
    ix.close()


def test_tids_and_shared_views(ctx):
    """out_tid and pgv_index_tids; a pgv_index_share view on a second context answers identically, and goes on doing so
    after the owner is freed"""
    ix, centers, offsets, rows = make_index(ctx, 130, [100, 200, 50], 131)
    queries = im.rand_bits(6, 130, 132)
    dist, slot, tid = ix.search_batch(queries, 2, 15, want_tid=True)
    assert np.array_equal(ix.tids(slot.ravel()), tid.ravel()) and np.array_equal(tid, tids_of(350)[slot])
    ctx2 = api.Context(0)
    view = ix.share(ctx2)
    assert _lib.lib.pgv_index_nbits(view.h) == 130
    d2, s2, t2 = view.search_batch(queries, 2, 15, want_tid=True)
    assert np.array_equal(d2, dist) and np.array_equal(s2, slot) and np.array_equal(t2, tid)
    ix.close()
    d3, s3, t3 = view.search_batch(queries, 2, 15, want_tid=True)
    assert np.array_equal(d3, dist) and np.array_equal(s3, slot) and np.array_equal(t3, tid)
    lists, _ = view.rank_lists(queries, 3)
    assert np.array_equal(lists, im.rank_lists(centers, queries, 3)[0])
    view.close()
    ctx2.close()


@pytest.mark.parametrize("nbits", [128, 1024, 200])
def test_device_pointers(ctx, nbits):
    """queries and outputs in device memory next to host ones (nbits 1024: a query row that is whole slices is read in
    place)"""
    import torch
    ix, centers, offsets, rows = make_index(ctx, nbits, [70, 300, 20], 141)
    queries = im.rand_bits(10, nbits, 142)
    dist, slot, tid = ix.search_batch(queries, 2, 12, want_tid=True)
    dq = torch.from_numpy(queries).cuda()
    d_dist, d_slot, d_tid = ix.search_batch(dq, 2, 12, want_tid=True)
    assert d_dist.is_cuda and d_slot.is_cuda
    assert np.array_equal(d_dist.cpu().numpy(), dist) and np.array_equal(d_slot.cpu().numpy(), slot)
    assert np.array_equal(d_tid.cpu().numpy().view(np.uint64), tid)
    d_lists, d_cd = ix.rank_lists(dq, 3)
    lists, cd = ix.rank_lists(queries, 3)
    assert np.array_equal(d_lists.cpu().numpy(), lists) and np.array_equal(d_cd.cpu().numpy(), cd)
    b_dist, b_slot, _ = ix.scan_batch(dq, d_lists, 12)
    h_dist, h_slot, _ = ix.scan_batch(queries, lists, 12)
    assert np.array_equal(b_dist.cpu().numpy(), h_dist) and np.array_equal(b_slot.cpu().numpy(), h_slot)
    ix.close()


def test_entries_that_refuse_a_bit_index(ctx):
    ix, centers, offsets, rows = make_index(ctx, 64, [10, 10], 151)
    query = im.rand_bits(1, 64, 152)
    lib = _lib.lib
    handle = C.create_string_buffer(256)
    sink = api._SINK(lambda *a: 0)
    out = np.zeros(64, dtype=np.float32)
    q = C.c_void_p()
    tid = np.zeros(1, dtype=np.uint64)
    calls = {
        "pgv_index_set_overlap": lambda: lib.pgv_index_set_overlap(ix.h, 2),
        "pgv_index_export": lambda: lib.pgv_index_export(ix.h, handle),
        "pgv_index_drain": lambda: lib.pgv_index_drain(ix.h, 0, sink, None),
        "pgv_index_shadow_cast": lambda: lib.pgv_index_shadow_cast(ix.h, api.ptr(query), 1, api.ptr(out), None, None, None, None),
        "pgv_query_begin": lambda: lib.pgv_query_begin(ix.h, C.byref(q)),
        "pgv_search_batch_sharded": lambda: lib.pgv_search_batch_sharded(None, ix.h, api.ptr(query), 1, 1, 1, api.ptr(out),
                                                                       api.ptr(tid)),
    }
    for name, call in calls.items():
        assert call() == _lib.PGV_ERR_ARG, name
        assert "bit index" in lib.pgv_last_error().decode(), name
    assert not q.value
    check_search(ix, centers, offsets, rows, query, 2, 5, "after the refusals")
    ix.close()
    data = gen(40, 8, seed=153)
    fx = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, 8, data[:2], np.array([0, 20, 40]), data)
    assert lib.pgv_index_nbits(fx.h) == 0 and lib.pgv_index_nbits(None) == -1
    fx.close()


# ------------------------------------------------------------------------------------------------ both Hamming kernels
@pytest.mark.parametrize("n", [1, TASK_ROWS - 1, TASK_ROWS, TASK_ROWS + 1, 2 * TASK_ROWS + 1])
@pytest.mark.parametrize("nbits", [1, SLICE_BITS - 1, SLICE_BITS, SLICE_BITS + 1, 1536])
def test_tile_and_list_kernels_count_alike(ctx, nbits, n):
    """hamming_tile_kernel and hamming_list_kernel walk a tile of rows the same way (kernels_bit.hip): over ONE set
    of packed rows and queries, the distances of pgv_bit_topk's matrix (read back through k = n: the matrix itself
    is not exposed) equal, as integers, those pgv_scan_lists streams from a bit index that holds the rows in two
    lists, split at a row count that is no multiple of 256 -- and both equal tests/bit_model.py. One bit, one below
    / at / one above the register slice and a slice and a half; one row, one below / at / one above the 256-row tile
    and two tiles and a row; 1, 9 and 33 queries: a lone query, a query group with a clamped tail and two 32-query
    tiles. pgv_scan_lists scores one query a call (groups of 8, one pair live); the same index's pgv_scan_batch with
    both lists probed by every query adds the groups of 8, 16 and 32 with live tails (hamming_list_group_size at
    shares 1, 9 and 33)"""
    rows = im.rand_bits(n, nbits, 300 + n)
    queries = im.rand_bits(33, nbits, 400 + nbits % 89)
    want = np.stack([bm.hamming(q, rows) for q in queries])
    split = 300 if n > 300 else (n + 1) // 2
    assert split % TASK_ROWS != 0
    ix = api.BitIvfIndex(ctx, nbits, im.rand_bits(2, nbits, 301), np.array([0, split, n]), rows)

    def as_matrix(dist, pos):
        """sorted or streamed (distance, row) pairs of each query -> int64 [nq x n], every row exactly once"""
        assert np.array_equal(np.sort(pos, axis=1), np.tile(np.arange(n), (pos.shape[0], 1)))
        assert np.array_equal(dist, np.rint(dist))
        mat = np.empty(pos.shape, dtype=np.int64)
        np.put_along_axis(mat, pos, dist.astype(np.int64), axis=1)
        return mat

    for nq in (1, 9, 33):
        qs = np.ascontiguousarray(queries[:nq])
        tiles = as_matrix(*api.bit_topk(ctx, nbits, qs, rows, n))
        streams = [ix.scan_lists(q, [0, 1]) for q in qs]
        lists = as_matrix(np.stack([d for d, _ in streams]), np.stack([s for _, s in streams]))
        dist, slot, _ = ix.scan_batch(qs, np.tile(np.array([0, 1], dtype=np.int32), (nq, 1)), n)
        groups = as_matrix(dist, slot)
        assert np.array_equal(tiles, lists), (nq, np.argwhere(tiles != lists)[:5].tolist())
        assert np.array_equal(tiles, groups), (nq, np.argwhere(tiles != groups)[:5].tolist())
        assert np.array_equal(tiles, want[:nq]), (nq, np.argwhere(tiles != want[:nq])[:5].tolist())
    ix.close()


# ------------------------------------------------------------------------------------------------ pgv_bit_assign
@pytest.mark.parametrize("k,n,nbits", [(1, 1, 1), (2, 255, 9), (33, 256, 128), (1000, 257, 1025), (33, 3000, 9), (1000, 3000, 128),
                                       (2, 3000, 1), (1, 257, 1025)])
def test_bit_assign(ctx, k, n, nbits):
    """one center, two, 33 and four 256-row tiles of them; 1 row, around 256 and 3 000 rows (the rows are the tile
    kernel's queries: groups of 32); a bit, a ragged byte, a whole vector and one bit past a slice.  Duplicate centers
    resolve to the lower id"""
    centers, rows = im.rand_bits(k, nbits, 160 + k), im.rand_bits(n, nbits, 161 + n)
    if k >= 33:
        centers[20] = centers[4]
        rows[n // 2] = centers[4]
    got, dist = api.bit_assign(ctx, nbits, centers, rows)
    want, wdist = im.assign(centers, rows)
    assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(dist, wdist)
    if k >= 33:
        assert got[n // 2] == 4 and dist[n // 2] == 0
    assert np.array_equal(api.bit_assign(ctx, nbits, centers, rows, want_dist=False)[0], want)


# ------------------------------------------------------------------------------------------------ pgv_bit_lloyd_step
def bits_of(strings):
    return np.packbits(np.array([[int(c) for c in s] for s in strings], dtype=np.uint8), axis=1)


def check_step(ctx, nbits, samples, centers, closest, seed=9):
    m_rng, d_rng = im.ModelRng(seed), im.ModelRng(seed)
    wc, wcounts, wchanges, wnew = im.lloyd_step(samples, centers, closest, nbits, m_rng)
    io = np.array(closest, dtype=np.int32)
    gc, gcounts, gchanges = api.bit_lloyd_step(ctx, nbits, samples, centers, io, rng=d_rng.pgv())
    assert np.array_equal(io, wnew), (io.tolist(), wnew.tolist())
    assert np.array_equal(gc, wc) and np.array_equal(gcounts, wcounts) and gchanges == wchanges
    assert (d_rng.doubles, d_rng.u32s) == (m_rng.doubles, m_rng.u32s)
    assert d_rng.next_double() == m_rng.next_double()  # the generator stands where the model's does
    return gc, gcounts, gchanges, io


def test_lloyd_step_fresh(ctx):
    samples, centers = im.rand_bits(700, 45, 171), im.rand_bits(9, 45, 172)
    _, counts, changes, new = check_step(ctx, 45, samples, centers, np.full(700, -1))
    assert changes == 700 and counts.sum() == 700 and np.array_equal(new, im.assign(centers, samples)[0])


def test_lloyd_step_exact_ties_move_nothing(ctx):
    """every sample is exactly as far from the other center as from its own (4 bits each): it stays where it is, where a
    fresh argmin would put all of them on center 0"""
    centers = bits_of(["11110000", "00001111"])
    samples = bits_of(["11001100", "00110011", "11000011"] * 4)
    closest = [1, 0, 1] * 4
    assert (im.hamming_matrix(samples, centers) == 4).all()
    _, counts, changes, new = check_step(ctx, 8, samples, centers, closest)
    assert new.tolist() == closest and changes == 0 and counts.tolist() == [4, 8]


def test_lloyd_step_strictly_closer_center_takes_the_sample(ctx):
    """11001100 is 4, 4 and 2 bits from the centers, 11110011 is 2, 6 and 4: whatever they were assigned to, the first
    go to center 2 and the second to center 0"""
    centers = bits_of(["11110000", "00001111", "11000000"])
    samples = bits_of(["11001100"] * 6 + ["11110011"] * 3)
    _, _, changes, new = check_step(ctx, 8, samples, centers, [1, 1, 0, 1, 0, 1, 2, 2, 1])
    assert new.tolist() == [2] * 6 + [0] * 3 and changes == 9


def test_lloyd_step_moves_to_the_lowest_index_among_the_closest(ctx):
    centers = bits_of(["111111", "000111", "000111", "000011"])
    samples = bits_of(["000111", "000111", "100111"])
    _, _, changes, new = check_step(ctx, 6, samples, centers, [0, 3, 3])
    assert new.tolist() == [1, 1, 1] and changes == 3
    _, _, changes, new = check_step(ctx, 6, samples, centers, [2, 2, 2])
    assert new.tolist() == [2, 2, 2] and changes == 0


def test_lloyd_step_half_set_bits_round_down_and_a_cluster_of_one(ctx):
    """an even cluster with exactly half its members' bits set gives 0 (x = 0.5 is not > 0.5); a cluster of one becomes
    its member"""
    centers = bits_of(["0000000000", "1111111111"])
    samples = bits_of(["1100000000", "0011000000", "1010000000", "0101000000", "1111101111"])
    new_centers, counts, _, new = check_step(ctx, 10, samples, centers, [-1] * 5)
    assert new.tolist() == [0, 0, 0, 0, 1] and counts.tolist() == [4, 1]
    assert np.array_equal(new_centers, bits_of(["0000000000", "1111101111"]))
    samples = bits_of(["1100000000", "1100000000", "1110000000", "0001000000"])
    new_centers, _, _, _ = check_step(ctx, 10, samples, centers[:1], [0] * 4)
    assert np.array_equal(new_centers, bits_of(["1100000000"]))  # 3/4, 3/4, 1/4, 1/4


def test_lloyd_step_empty_clusters_draw_center_major_and_bit_minor(ctx):
    nbits = 19
    centers = np.concatenate([im.rand_bits(2, nbits, 181), bits_of(["1" * nbits, "0" * nbits]), im.rand_bits(1, nbits, 182)])
    samples = np.concatenate([np.tile(centers[0], (5, 1)), np.tile(centers[4], (3, 1))])
    m_rng = im.ModelRng(77)
    new_centers, counts, _, _ = check_step(ctx, nbits, samples, centers, [-1] * 8, seed=77)
    assert counts.tolist() == [5, 0, 0, 0, 3]
    draws = [m_rng.next_double() for _ in range(3 * nbits)]  # clusters 1, 2, 3 in that order, nbits draws each
    want = np.packbits(np.array(draws, dtype=np.float32).reshape(3, nbits) > np.float32(0.5), axis=1)
    assert np.array_equal(new_centers[1:4], want)


def test_lloyd_step_rejects_an_assignment_outside_the_centers(ctx):
    samples, centers = im.rand_bits(4, 8, 191), im.rand_bits(2, 8, 192)
    with pytest.raises(api.PgvError) as e:
        api.bit_lloyd_step(ctx, 8, samples, centers, np.array([0, 1, 2, -1], dtype=np.int32))
    assert e.value.code == _lib.PGV_ERR_ARG


# ------------------------------------------------------------------------------------------------ pgv_bit_kmeans
@pytest.mark.parametrize("n,nbits,k", KMEANS_SHAPES)
def test_bit_kmeans_is_the_sticky_loop(ctx, n, nbits, k):
    """the shapes on which tests/test_bit_ivf_model_cpu.py shows the sticky loop to be ElkanKmeans and the fresh-argmin
    loop not to be"""
    samples, seed = kmeans_case(n, nbits, k)
    m_rng, d_rng = im.ModelRng(seed), im.ModelRng(seed)
    wc, wa, wi = im.kmeans_sticky(samples, nbits, k, m_rng)
    gc, ga, gi = api.bit_kmeans(ctx, nbits, samples, k, rng=d_rng.pgv())
    assert gi == wi and np.array_equal(ga, wa) and np.array_equal(gc, wc)
    assert (d_rng.doubles, d_rng.u32s) == (m_rng.doubles, m_rng.u32s)


def test_bit_kmeans_without_samples_draws_every_center(ctx):
    m_rng, d_rng = im.ModelRng(5), im.ModelRng(5)
    wc, _, wi = im.kmeans_sticky(np.zeros((0, 3), dtype=np.uint8), 21, 6, m_rng)
    gc, ga, gi = api.bit_kmeans(ctx, 21, np.zeros((0, 3), dtype=np.uint8), 6, rng=d_rng.pgv())
    assert gi == wi == 0 and ga is None and np.array_equal(gc, wc) and d_rng.doubles == m_rng.doubles == 6 * 21


def test_bit_kmeans_more_lists_than_distinct_samples(ctx):
    """036_ivfflat_bit_centers.pl: lists beyond the distinct values must not fail"""
    samples = np.tile(bits_of(["000", "101", "111"]), (5, 1))
    m_rng, d_rng = im.ModelRng(6), im.ModelRng(6)
    wc, wa, wi = im.kmeans_sticky(samples, 3, 9, m_rng)
    gc, ga, gi = api.bit_kmeans(ctx, 3, samples, 9, rng=d_rng.pgv())
    assert gi == wi and np.array_equal(ga, wa) and np.array_equal(gc, wc) and d_rng.doubles == m_rng.doubles


def test_bit_kmeans_rejects_2_to_the_24_samples_without_touching_them(ctx):
    centers = np.zeros((2, 1), dtype=np.uint8)
    for n in (1 << 24, (1 << 24) + 5):
        rc = _lib.lib.pgv_bit_kmeans(ctx.h, 8, None, n, 2, 0, None, api.ptr(centers), None, None)
        assert rc == _lib.PGV_ERR_ARG and "2^24" in _lib.lib.pgv_last_error().decode()
    for nbits in (0, 64001):
        assert _lib.lib.pgv_bit_kmeans(ctx.h, nbits, None, 0, 2, 0, None, api.ptr(centers), None, None) == _lib.PGV_ERR_DIMS


# ------------------------------------------------------------------------------------------------ end to end
def test_build_and_recall_at_the_references_own_shape(ctx):
    """test/t/035_ivfflat_bit_build_recall.pl: 100 000 x 52 random bits, lists 100 (k-means over 10 000 samples), 20
    queries, LIMIT 20.  build_bit_ivf equals the model's build, every search equals the model's, and recall against the
    tie-tolerant expected set (:85-90: every row no farther than the 20th) is at least the reference's floors"""
    nbits, lists, limit = 52, 100, 20
    rows = im.rand_bits(100000, nbits, 201)
    samples = np.ascontiguousarray(rows[np.random.default_rng(202).choice(100000, 10000, replace=False)])
    queries = im.rand_bits(20, nbits, 203)
    m_rng, d_rng = im.ModelRng(204), im.ModelRng(204)
    wcenters, woffsets, worder = im.build(rows, nbits, lists, m_rng, samples=samples)
    ix, centers, offsets = api.build_bit_ivf(ctx, nbits, rows, lists, rng=d_rng.pgv(), samples=samples)
    assert np.array_equal(centers, wcenters) and np.array_equal(offsets, woffsets)
    assert np.array_equal(ix.tids(np.arange(100000)), worder.astype(np.uint64))
    exact = im.hamming_matrix(queries, rows)
    listed = rows[worder]
    for probes, floor in ((1, 0.08), (10, 0.50), (100, 1.00)):
        dist, slot, tid = ix.search_batch(queries, probes, limit, want_tid=True)
        wd, ws, _ = im.search(centers, offsets, listed, queries, probes, limit)
        assert np.array_equal(dist, wd) and np.array_equal(slot, ws), probes
        correct = 0
        for q in range(20):
            expected = set(np.flatnonzero(exact[q] <= np.sort(exact[q])[limit - 1]).tolist())
            correct += sum(int(t) in expected for t in tid[q][slot[q] >= 0])
        print("probes %d: recall %.3f" % (probes, correct / (20 * limit)))
        assert correct / (20 * limit) >= floor, probes
    ix.close()


@pytest.mark.parametrize("dtype", [po.ORA_F32, po.ORA_F16])
def test_binary_search_ivf(ctx, oracle, dtype):
    """2 000 x 64-d rows: quantise -> the model's search of the bit index for kc candidates -> the model's rerank"""
    half = dtype == po.ORA_F16
    dt = api.PGV_F16 if half else api.PGV_F32
    rows = gen(2000, 64, seed=211, dist="clustered", dtype=dtype) - np.asarray(0.5, dtype=np.float16 if half else np.float32)
    queries = gen(8, 64, seed=212, dist="clustered", dtype=dtype) - np.asarray(0.5, dtype=np.float16 if half else np.float32)
    bits = bm.binary_quantize(rows)
    ix, centers, offsets = api.build_bit_ivf(ctx, 64, bits, 12, rng=im.ModelRng(213).pgv())
    order = ix.tids(np.arange(2000)).astype(np.int64)
    dist, idx, hamming, cand = api.binary_search_ivf(ctx, api.PGV_L2SQ, dt, 64, queries, rows, ix, 4, 60, 10, want_candidates=True)
    wh, ws, _ = im.search(centers, offsets, bits[order], bm.binary_quantize(queries), 4, 60)
    wc = np.where(ws >= 0, order[np.maximum(ws, 0)], -1)
    assert np.array_equal(hamming, wh) and np.array_equal(cand, wc)
    wd, wi = bm.rerank(oracle, api.PGV_L2SQ, half, queries, rows, wc, 10)
    for q in range(8):
        assert_topk_equiv(idx[q].tolist(), dist[q], wi[q].tolist(), wd[q], what="binary_search_ivf q%d" % q)
    ix.close()
