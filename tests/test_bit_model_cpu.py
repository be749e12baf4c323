"""The numpy model of tests/bit_model.py against its two sources -- the oracle's ora_bit_hamming (the compiled
restatement of src/bitutils.c, itself pinned to the reference by tests/test_oracle_golden.py) and the reference's
recorded binary_quantize results -- and the presence of the entries the model stands for."""
import ctypes

import numpy as np
import pytest

import bit_model as bm
from helpers import golden
from pgvector_amd import _lib, api

QUANT_CASES = golden("binary_quantize_known_answers.json")["cases"]


@pytest.mark.parametrize("nbits", [1, 9, 128, 136, 1536])
def test_model_hamming_matches_the_oracle(oracle, nbits):
    rng = np.random.default_rng(nbits)
    nbytes = (nbits + 7) // 8
    rows = rng.integers(0, 256, (200, nbytes), dtype=np.uint8)
    query = rng.integers(0, 256, nbytes, dtype=np.uint8)
    want = oracle.bit_rows("ora_bit_hamming", query, rows)
    assert np.array_equal(bm.hamming(query, rows).astype(np.float64), want)
    dist, idx = bm.hamming_topk(query[None, :], rows, 17)
    order = sorted(range(200), key=lambda i: (want[i], i))[:17]
    assert idx[0].tolist() == order
    assert np.array_equal(dist[0].astype(np.float64), want[order])


def test_model_topk_pads_and_breaks_ties_by_index():
    rows = np.zeros((6, 2), dtype=np.uint8)
    rows[4, 0] = 0x80
    dist, idx = bm.hamming_topk(np.zeros((1, 2), dtype=np.uint8), rows, 10)
    assert idx[0].tolist() == [0, 1, 2, 3, 5, 4, -1, -1, -1, -1]
    assert dist[0].tolist() == [0, 0, 0, 0, 0, 1] + [np.inf] * 4


@pytest.mark.parametrize("case", QUANT_CASES, ids=["%s-%d" % (c["type"], len(c["input"])) for c in QUANT_CASES])
def test_model_binary_quantize_matches_the_reference_known_answers(case):
    x = np.array([case["input"]], dtype=np.float32 if case["type"] == "vector" else np.float16)
    got = np.unpackbits(bm.binary_quantize(x), axis=1)[0]
    n = len(case["bits"])
    assert "".join(str(b) for b in got[:n]) == case["bits"]
    assert not got[n:].any()  # the pad bits of the last byte


def test_model_binary_quantize_special_values():
    for dt in (np.float32, np.float16):
        tiny, sub = np.finfo(dt).tiny, np.finfo(dt).smallest_subnormal
        x = np.array([[0.0, -0.0, np.nan, np.inf, -np.inf, sub, tiny, -sub, -tiny]], dtype=dt)
        assert np.unpackbits(bm.binary_quantize(x), axis=1)[0][:9].tolist() == [0, 0, 0, 1, 0, 1, 1, 0, 0]


def test_model_rerank_orders_by_the_oracle_kernel(oracle):
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 1024, (50, 8)).astype(np.float32)
    queries = rng.integers(0, 1024, (2, 8)).astype(np.float32)
    cand = np.array([[7, -1, 3, 3, 40], [-1, -1, -1, -1, -1]], dtype=np.int64)
    dist, idx = bm.rerank(oracle, 0, False, queries, rows, cand, 4)
    d = lambda r: float(((rows[r].astype(np.float64) - queries[0]) ** 2).sum())
    want = sorted([(d(7), 0, 7), (d(3), 2, 3), (d(3), 3, 3), (d(40), 4, 40)])
    assert idx[0].tolist() == [w[2] for w in want]
    assert dist[0].tolist() == [w[0] for w in want]
    assert idx[1].tolist() == [-1] * 4 and np.isinf(dist[1]).all()


def test_library_and_api_have_the_binary_quantization_entries():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pgv_bit_topk", "pgv_binary_quantize", "pgv_rerank"):
        assert hasattr(lib, name), "libpgv_hip.so does not export %s" % name
        assert name in _lib.SYMBOLS
    for name in ("bit_topk", "binary_quantize", "rerank", "binary_search"):
        assert callable(getattr(api, name, None)), "pgvector_amd.api has no %s" % name
