"""The numpy model of tests/bit_ivf_model.py against its sources: the oracle's ora_bit_hamming (the compiled restatement
of src/bitutils.c), tests/bit_model.py's exhaustive top-k, the literal transcription of the reference's ElkanKmeans
(src/ivfkmeans.c:246-485), the fp32 arithmetic of BitUpdateCenter and the reference's recorded answer for
`USING ivfflat (val bit_hamming_ops)` -- and the presence of the entries the model stands for."""
import ctypes

import numpy as np
import pytest

import bit_ivf_model as im
import bit_model as bm
from helpers import golden
from pgvector_amd import _lib, api

KNOWN = golden("ivfflat_bit_known_answers.json")
KMEANS_SHAPES, kmeans_case = im.KMEANS_SHAPES, im.kmeans_case


@pytest.mark.parametrize("nbits", [1, 9, 128, 136, 1536])
def test_model_hamming_matches_the_oracle(oracle, nbits):
    rows, centers = im.rand_bits(200, nbits, nbits), im.rand_bits(9, nbits, nbits + 1)
    query = im.rand_bits(1, nbits, nbits + 2)[0]
    want = oracle.bit_rows("ora_bit_hamming", query, rows)
    offsets = np.array([0, 50, 50, 200], dtype=np.int64)
    dist, slot = im.scan_stream(offsets, rows, query, [2, 0, 1])
    assert slot.tolist() == list(range(50, 200)) + list(range(50))
    assert np.array_equal(dist.astype(np.float64), want[slot])
    lists, cdist = im.rank_lists(centers, query[None, :], 9)
    cwant = oracle.bit_rows("ora_bit_hamming", query, centers)
    assert lists[0].tolist() == sorted(range(9), key=lambda l: (cwant[l], l))
    assert np.array_equal(cdist[0].astype(np.float64), cwant[lists[0]])
    assigned, adist = im.assign(centers, rows)
    for j in range(0, 200, 17):
        d = oracle.bit_rows("ora_bit_hamming", rows[j], centers)
        assert assigned[j] == int(np.argmin(d)) and adist[j] == d.min()


def test_model_search_over_every_list_is_the_exhaustive_topk():
    nbits, nlists = 40, 7
    rows, centers, queries = im.rand_bits(600, nbits, 1), im.rand_bits(nlists, nbits, 2), im.rand_bits(6, nbits, 3)
    assigned, _ = im.assign(centers, rows)
    order = np.argsort(assigned, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(assigned, minlength=nlists))]).astype(np.int64)
    dist, slot, _ = im.search(centers, offsets, rows[order], queries, nlists, 25)
    want, _ = bm.hamming_topk(queries, rows, 25)
    assert np.array_equal(dist, want)
    assert np.array_equal(bm.hamming_topk(queries, rows[order], 600)[0][:, :25], dist)
    for q in range(6):
        assert np.array_equal(bm.hamming(queries[q], rows[order][slot[q]]).astype(np.float32), dist[q])


def test_model_head_pads_and_breaks_ties_by_insertion_position():
    rows = np.zeros((6, 1), dtype=np.uint8)
    rows[1, 0] = 0x80
    offsets = np.array([0, 2, 2, 6], dtype=np.int64)
    dist, slot = im.scan_head(offsets, rows, np.zeros(1, dtype=np.uint8), [2, 1, 0], 8)
    assert slot.tolist() == [2, 3, 4, 5, 0, 1, -1, -1]
    assert dist.tolist() == [0, 0, 0, 0, 0, 1, np.inf, np.inf]
    dist, slot = im.scan_head(offsets, rows, np.zeros(1, dtype=np.uint8), [1], 3)
    assert slot.tolist() == [-1, -1, -1] and np.isinf(dist).all()


def test_sticky_loop_is_the_elkan_transcription_and_the_fresh_argmin_loop_is_not():
    """centers, assignments and iteration counts of the loop the library runs equal the literal ElkanKmeans on every
    shape; the loop that re-takes the lowest-index argmin differs on at least one (so seeds that stop telling the two
    apart are noticed)"""
    differs = 0
    for n, nbits, k in KMEANS_SHAPES:
        samples, seed = kmeans_case(n, nbits, k)
        r1, r2, r3 = im.ModelRng(seed), im.ModelRng(seed), im.ModelRng(seed)
        c1, a1, i1 = im.kmeans_sticky(samples, nbits, k, r1)
        c2, a2, i2 = im.kmeans_elkan(samples, nbits, k, r2)
        assert np.array_equal(c1, c2) and np.array_equal(a1, a2) and i1 == i2, (n, nbits, k)
        assert (r1.doubles, r1.u32s) == (r2.doubles, r2.u32s), (n, nbits, k)
        c3, a3, i3 = im.kmeans_fresh(samples, nbits, k, r3)
        differs += not (np.array_equal(c1, c3) and np.array_equal(a1, a3) and i1 == i3)
    assert differs >= 1


def test_center_bit_in_fp32_is_the_integer_majority():
    """(float) sum / (float) count > 0.5 (src/ivfkmeans.c:220, src/ivfutils.c:338) equals 2 sum > count for every
    count <= 4096: what lets the device keep integer counts"""
    for count in range(1, 4097):
        s = np.arange(0, count + 1)
        x = s.astype(np.float32) / np.float32(count)
        assert np.array_equal(x > np.float32(0.5), 2 * s > count), count


def test_model_update_centers_packs_majorities_and_draws_for_empty_clusters():
    samples = np.packbits(np.array([[1, 1, 0, 0, 1], [1, 0, 0, 0, 1], [0, 1, 0, 1, 1], [0, 0, 0, 1, 0]], dtype=np.uint8), axis=1)
    rng = im.ModelRng(3)
    centers, counts = im.update_centers(samples, [0, 0, 0, 0], 3, 5, rng)
    assert counts.tolist() == [4, 0, 0]
    assert np.unpackbits(centers[0])[:5].tolist() == [0, 0, 0, 0, 1]  # exactly half set -> 0; pad bits zero
    assert not np.unpackbits(centers, axis=1)[:, 5:].any()
    assert rng.doubles == 10  # two empty clusters x 5 bits, center-major
    replay = im.ModelRng(3)
    want = [[np.float32(replay.next_double()) > 0.5 for _ in range(5)] for _ in range(2)]
    assert np.unpackbits(centers[1:], axis=1)[:, :5].astype(bool).tolist() == want


def test_reference_known_answer():
    """test/sql/ivfflat_bit.sql: rows 000, 100, 111 and (inserted later) 110 in one list; ORDER BY val <~> B'111'"""
    pack = lambda strings: np.packbits(np.array([[int(c) for c in s] for s in strings], dtype=np.uint8), axis=1)
    rows, query = pack(KNOWN["rows"]), pack([KNOWN["query"]])
    offsets = np.array([0, len(KNOWN["rows"])], dtype=np.int64)
    centers = pack(["100"])
    dist, slot, lists = im.search(centers, offsets, rows, query, 1, 10)
    n = len(KNOWN["ordered"])
    assert [KNOWN["rows"][s] for s in slot[0][:n]] == KNOWN["ordered"]
    assert slot[0][n:].tolist() == [-1] * (10 - n) and np.isinf(dist[0][n:]).all()
    zeros, zslot = im.scan_stream(offsets, rows, None, [0])
    assert zslot.size == KNOWN["null_query_count"] and not zeros.any()


def test_library_and_api_have_the_bit_ivf_entries():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pgv_index_upload_bits", "pgv_index_nbits", "pgv_bit_assign", "pgv_bit_kmeans", "pgv_bit_lloyd_step"):
        assert hasattr(lib, name), "libpgv_hip.so does not export %s" % name
        assert name in _lib.SYMBOLS
    for name in ("BitIvfIndex", "bit_assign", "bit_kmeans", "bit_lloyd_step", "build_bit_ivf", "binary_search_ivf"):
        assert callable(getattr(api, name, None)), "pgvector_amd.api has no %s" % name
    for name in ("rank_lists", "scan_lists", "search_batch", "scan_batch", "share", "tids", "close"):
        assert callable(getattr(api.BitIvfIndex, name, None)), "BitIvfIndex has no %s" % name
    assert isinstance(api.BitIvfIndex.rows, property)
