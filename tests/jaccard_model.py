"""Exact model of jaccard_distance over packed bit strings and of the device's 32-bit Jaccard key, for
tests/test_jaccard_model_cpu.py and tests/test_gpu_jaccard_hnsw.py: no GPU, no ctypes.

A pair of bit strings is reduced to two counts, x = popcount(a ^ b) and u = popcount(a | b), 0 <= x <= u <= 64 000.  The
reference (BitJaccardDistanceDefault, src/bitutils.c:99-131) counts ab = |a & b| = u - x, aa and bb (aa + bb - ab = u) and
returns 1 when ab is 0, else 1 - (double) ab / (double) u.  The exact distance is the rational x / u (1 when u is 0)."""
import math
from fractions import Fraction

import numpy as np

from bit_model import POPCOUNT

MAX_BITS = 64000
SCALE = 0xFFFFFF00  # kJaccardScale (pgvector_amd/csrc/pgv_device.h): 64 000^2 < SCALE < 2^32 - 1


def counts(query, rows):
    """packed query [bytes] against packed rows [n x bytes] -> (x [n], u [n]) int64"""
    query, rows = np.asarray(query, dtype=np.uint8), np.asarray(rows, dtype=np.uint8)
    return POPCOUNT[rows ^ query[None, :]].sum(1), POPCOUNT[rows | query[None, :]].sum(1)


def fraction(x, u):
    """the exact Jaccard distance"""
    x, u = int(x), int(u)
    return Fraction(x, u) if u > 0 else Fraction(1)


def ref_double(x, u):
    """the reference's float8 (a Python float is a C double, and / is IEEE division)"""
    ab, u = int(u) - int(x), int(u)
    return 1.0 if ab == 0 else 1.0 - float(ab) / float(u)


def ref_float(x, u):
    """what the device hands back: (float) of the reference's float8"""
    return np.float32(ref_double(x, u))


def key(x, u):
    """the device's key (jaccard_key): floor(x * SCALE / u); SCALE when the strings share no bit (u = 0 included)"""
    x, u = int(x), int(u)
    return SCALE if x >= u else x * SCALE // u


def fp32_key(x, u):
    """the key the walk would use if it ranked by the fp32 image of the reference's value: what this opclass cannot do"""
    return float(np.float32(ref_double(x, u)))


def fractions_of(query, rows):
    x, u = counts(query, rows)
    return [fraction(a, b) for a, b in zip(x, u)]


def ref_floats(query, rows):
    x, u = counts(query, rows)
    return np.array([ref_float(a, b) for a, b in zip(x, u)], dtype=np.float32)


# ------------------------------------------------------------------------------------------------------- generators
def farey_pairs(lo=63600, hi=MAX_BITS, offsets=(3, 7, 53, 211, 389), least=Fraction(0)):
    """neighbours in a Farey sequence, ((a, b), (c, d)) with b c - a d = 1: a / b < c / d are 1 / (b d) apart, the
    closest two different ratios of these denominators can be.  Denominators b in lo .. hi, d = b - offset (>= lo);
    both ratios >= least."""
    out = []
    for b in range(lo, hi + 1):
        for off in offsets:
            d = b - off
            if d < lo or math.gcd(b, d) != 1:
                continue
            c = pow(b, -1, d)
            a = (b * c - 1) // d
            if b * c - a * d == 1 and 0 <= a < b and 0 < c < d and Fraction(a, b) >= least:
                out.append(((a, b), (c, d)))
    return out


def random_pairs(count, seed):
    """pairs of (x, u) drawn over the whole range, small and large denominators alike"""
    rng = np.random.default_rng(seed)
    u = np.where(rng.random((count, 2)) < 0.5, rng.integers(1, 200, (count, 2)), rng.integers(1, MAX_BITS + 1, (count, 2)))
    x = (rng.random((count, 2)) * (u + 1)).astype(np.int64)
    return [((int(x[i, 0]), int(u[i, 0])), (int(x[i, 1]), int(u[i, 1]))) for i in range(count)]


def scaled_pairs(count, seed):
    """(x, u) against (g x, g u): equal ratios, which must be equal keys and equal doubles"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        u = int(rng.integers(1, 3200))
        x = int(rng.integers(0, u + 1))
        g = int(rng.integers(2, MAX_BITS // u + 1)) if MAX_BITS // u >= 2 else 1
        out.append(((x, u), (g * x, g * u)))
    return out


def sign(a, b):
    return (a > b) - (a < b)


def tie_free(nq, n, nbits, seed):
    """(queries, rows) packed, such that for every query the n exact distances are all different and none is 1: rows of
    every density are drawn 64 at a time and kept only if their ratio is new for every query"""
    rng = np.random.default_rng(seed)
    nbytes = (nbits + 7) // 8

    def draw(c):
        p = rng.uniform(.05, .95, (c, 1))
        bits = rng.random((c, 8 * nbytes)) < p
        bits[:, nbits:] = 0
        return np.packbits(bits, axis=1)

    queries = draw(nq)
    seen = [set() for _ in range(nq)]
    rows = []
    while len(rows) < n:
        batch = draw(64)
        fr = [fractions_of(q, batch) for q in queries]
        for j in range(64):
            if len(rows) < n and all(fr[q][j] not in seen[q] and fr[q][j] != 1 for q in range(nq)):
                for q in range(nq):
                    seen[q].add(fr[q][j])
                rows.append(batch[j])
    return queries, np.stack(rows)


# ----------------------------------------------------------------------------------------------------- planted pairs
PLANT_BITS, PLANT_ONES = MAX_BITS, 32000


def planted_query():
    """64 000 bits, the first 32 000 set"""
    bits = np.zeros(PLANT_BITS, dtype=np.uint8)
    bits[:PLANT_ONES] = 1
    return np.packbits(bits)[None, :]


def planted_row(x, u):
    """a row at exactly (x, u) from planted_query(): ab = u - x bits inside the query's ones, u - 32 000 outside them"""
    ab, outside = u - x, u - PLANT_ONES
    assert 0 <= ab <= PLANT_ONES and 0 <= outside <= PLANT_BITS - PLANT_ONES, (x, u)
    bits = np.zeros(PLANT_BITS, dtype=np.uint8)
    bits[:ab] = 1
    bits[PLANT_ONES:PLANT_ONES + outside] = 1
    return np.packbits(bits)


def planted_cases():
    """name -> dict(m, ef, xu: (x, u) per element, levels, nbr_start, nbr, entry = 0).  p < q are Farey neighbours that
    round to one fp32 value; the graphs are the tie traps of tests/hnsw_tie_cases.py with p and q where those have two
    equal distances, so a walk that merged p and q would take the tied branch and a walk that tells them apart must not.
      stop_pq / stop_qp: e0 -> x, y; x -> z; y -> t, ef 2.  One of x / y is pushed out of W by the other's neighbour at a
        distance STRICTLY beyond W's new furthest: it is no candidate any more (the strict stop test), its neighbour is
        never scored.  Merged keys would expand it: 5 scored instead of 4, and another W.
      cut_1 / cut_2: e0 lists q BEFORE p.  The cut by ef keeps p and drops q; merged keys keep batch order and keep q."""
    from hnsw_walk_model import tuples
    # (ratios >= 1 / 2 with u <= 64 000 have u - x <= 32 000 common bits: planted_row can make them)
    p, q = next(pr for pr in farey_pairs(least=Fraction(1, 2)) if fp32_key(*pr[0]) == fp32_key(*pr[1]))
    far, near3, near1, mid = (63000, 64000), (1000, 33000), (0, 32000), (16000, 48000)
    cases = {}

    def case(name, m, ef, xu, lists):
        levels, nbr_start, nbr = tuples(m, [0] * len(xu), lists)
        cases[name] = dict(m=m, ef=ef, xu=xu, levels=levels, nbr_start=nbr_start, nbr=nbr, entry=0)

    e0, x, y, z, t = range(5)
    case("stop_pq", 2, 2, [far, p, q, near3, near1], {(e0, 0): [x, y], (x, 0): [z], (y, 0): [t]})
    case("stop_qp", 2, 2, [far, q, p, near3, near1], {(e0, 0): [x, y], (x, 0): [z], (y, 0): [t]})
    case("cut_1", 2, 1, [far, q, p], {(0, 0): [1, 2]})
    case("cut_2", 2, 2, [far, mid, q, p, near1], {(0, 0): [1, 2, 3], (2, 0): [4]})
    return cases
