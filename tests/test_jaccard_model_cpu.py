"""The Jaccard model of tests/jaccard_model.py against the compiled oracle and the reference's known answers, the claim
the device's key rests on -- floor(x * S / u) orders and ties exactly as the exact ratios and as the reference's doubles
do -- and the preconditions of tests/test_gpu_jaccard_hnsw.py: an fp32 key merges the planted pairs, and a walk over
merged keys gives another answer on the planted graphs, so those tests cannot pass by accident."""
import json
import os
import re
from fractions import Fraction

import numpy as np

import bit_hnsw_model as bhm
import hnsw_walk_model as wm
import jaccard_model as jm
from pgvector_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_double_is_the_oracles(oracle):
    for nbits, seed in ((1, 1), (7, 2), (64, 3), (129, 4), (1536, 5), (64000, 6)):
        rows, query = bhm.rand_bits(40, nbits, seed), bhm.rand_bits(1, nbits, 100 + seed)[0]
        rows[3] = 0             # no common bit: 1
        rows[4] = query         # identical: 0
        rows[5] = ~query        # disjoint (the pad bits too: whole bytes are counted)
        x, u = jm.counts(query, rows)
        want = oracle.bit_rows("ora_bit_jaccard", query, rows)
        got = np.array([jm.ref_double(a, b) for a, b in zip(x, u)])
        assert got.tolist() == want.tolist(), nbits
        assert got[3] == 1.0 and got[5] == 1.0 and (got[4] == 0.0 or not query.any())
    zero = np.zeros((1, 8), dtype=np.uint8)
    assert oracle.bit_rows("ora_bit_jaccard", zero[0], zero).tolist() == [1.0] == [jm.ref_double(0, 0)]
    assert jm.fraction(0, 0) == 1 and jm.key(0, 0) == jm.SCALE == jm.key(5, 5)


def test_model_double_is_the_references_known_answers():
    with open(os.path.join(ROOT, "tests", "golden", "bit_known_answers.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["func"] == "jaccard_distance" and "value" in c]
    assert len(cases) >= 5
    for c in cases:
        a = np.packbits(np.array([int(ch) for ch in c["a"]], dtype=np.uint8))
        b = np.packbits(np.array([int(ch) for ch in c["b"]], dtype=np.uint8))
        x, u = jm.counts(a, b[None, :])
        assert jm.ref_double(x[0], u[0]) == c["value"], c


def check_order(pairs, what):
    ties = 0
    for a, b in pairs:
        fa, fb = jm.fraction(*a), jm.fraction(*b)
        want = jm.sign(fa, fb)
        assert jm.sign(jm.key(*a), jm.key(*b)) == want, (what, "key", a, b)
        assert jm.sign(jm.ref_double(*a), jm.ref_double(*b)) == want, (what, "double", a, b)
        assert jm.key(*a) <= jm.SCALE < 0xFFFFFFFF
        ties += want == 0
    return ties


def test_key_orders_farey_neighbours_like_the_fractions():
    pairs = jm.farey_pairs()
    assert len(pairs) > 1000
    for (a, b), (c, d) in pairs[::97]:
        assert b * c - a * d == 1 and Fraction(c, d) - Fraction(a, b) == Fraction(1, b * d)
    assert check_order(pairs, "farey") == 0
    # the same pairs under an fp32 key, and under a scale below 64 000^2: merged
    merged32 = sum(jm.fp32_key(*a) == jm.fp32_key(*b) for a, b in pairs)
    merged31 = sum(a[0] * 2 ** 31 // a[1] == b[0] * 2 ** 31 // b[1] for a, b in pairs)
    assert merged32 > len(pairs) // 4 and merged31 > len(pairs) // 4, (merged32, merged31, len(pairs))


def test_key_orders_random_and_scaled_pairs_like_the_fractions():
    pairs = jm.random_pairs(100000, 5)
    ties = check_order(pairs, "random")
    assert 0 < ties < len(pairs) // 10  # (small denominators: some equal ratios, found as ties)
    scaled = jm.scaled_pairs(20000, 6)
    assert check_order(scaled, "scaled") == len(scaled)
    for a, b in scaled[:2000]:
        assert jm.ref_double(*a) == jm.ref_double(*b) and jm.key(*a) == jm.key(*b)


def test_planted_rows_have_the_planted_counts():
    q = jm.planted_query()
    for x, u in ((63000, 64000), (1000, 33000), (0, 32000), (16000, 48000), (32001, 64000)):
        gx, gu = jm.counts(q[0], jm.planted_row(x, u)[None, :])
        assert (int(gx[0]), int(gu[0])) == (x, u)


def test_planted_graphs_tell_merged_keys_from_exact_ones():
    """on every planted graph the model's walk over the exact ratios differs from its walk over fp32-merged keys in the
    elements or in so->tuples: the GPU test's expected answer cannot be reached by a walk that merges p and q"""
    cases = jm.planted_cases()
    assert sorted(cases) == ["cut_1", "cut_2", "stop_pq", "stop_qp"]
    for name, c in cases.items():
        exact = [jm.fraction(*xu) for xu in c["xu"]]
        merged = [jm.fp32_key(*xu) for xu in c["xu"]]
        assert len(set(exact)) == len(exact) and len(set(merged)) == len(merged) - 1, name
        a = wm.walk(exact.__getitem__, c["levels"], c["nbr_start"], c["nbr"], c["m"], c["entry"], c["ef"])
        b = wm.walk(merged.__getitem__, c["levels"], c["nbr_start"], c["nbr"], c["m"], c["entry"], c["ef"])
        k = wm.walk([jm.key(*xu) for xu in c["xu"]].__getitem__, c["levels"], c["nbr_start"], c["nbr"], c["m"], c["entry"], c["ef"])
        assert (a.ids, a.scored) != (b.ids, b.scored), name
        assert (a.ids, a.scored) == (k.ids, k.scored), name


def test_tie_free_generator_is_tie_free():
    queries, rows = jm.tie_free(3, 60, 1600, 5)
    for q in queries:
        fr = jm.fractions_of(q, rows)
        assert len(set(fr)) == len(fr) and all(f != 1 for f in fr)


def test_symbol_is_declared_and_exported():
    assert "pgv_hnsw_upload_jaccard" in _lib.SYMBOLS
    text = open(os.path.join(ROOT, "include", "pgv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bpgv_hnsw_upload_jaccard\s*\(", code)
    assert hasattr(_lib.lib, "pgv_hnsw_upload_jaccard")
