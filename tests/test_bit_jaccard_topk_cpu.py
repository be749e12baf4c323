"""pgv_bit_jaccard_topk without a GPU: the name is in the header, the library and the binding, and the order image
(jaccard_image, pgvector_amd/csrc/pgv_device.h), restated in exact integers, orders ratios of bit counts as their
fractions do and stays inside the finite normal floats."""
import os
import re

import numpy as np

import jaccard_model as jm
import pgvector_amd
from pgvector_amd import _lib, api

SCALE, BASE, GAP_AT, GAP = 4200000000, 0x00800000, 0x7f800000, 0x01000000  # kJaccardImage*
KEY_FLT_MAX = 0xff7fffff  # float_to_key(FLT_MAX)


def image_key(x, u):
    key = BASE + (SCALE if x >= u else x * SCALE // u)
    return key + GAP if key >= GAP_AT else key


def image_float(x, u):
    """key_to_float of the image's key"""
    key = image_key(x, u)
    return float(np.array([key & 0x7fffffff if key & 0x80000000 else ~key & 0xffffffff], dtype=np.uint32).view(np.float32)[0])


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(pgvector_amd.__file__), "..", "include", "pgv_hip.h")).read()
    assert re.search(r"\bpgv_bit_jaccard_topk\(pgv_ctx \* ctx, int nbits,", header)
    assert "pgv_bit_jaccard_topk" in _lib.SYMBOLS and hasattr(pgvector_amd.lib, "pgv_bit_jaccard_topk")
    assert callable(api.bit_jaccard_topk)


def test_image_orders_ratios_as_their_fractions():
    assert SCALE > jm.MAX_BITS ** 2
    pairs = jm.farey_pairs() + jm.random_pairs(20000, 3) + jm.scaled_pairs(2000, 4)
    for a, b in pairs:
        want = jm.sign(jm.fraction(*a), jm.fraction(*b))
        assert jm.sign(image_key(*a), image_key(*b)) == want, (a, b)
        assert jm.sign(image_float(*a), image_float(*b)) == want, (a, b)


def test_image_stays_inside_the_finite_normal_floats():
    assert image_key(0, 1) == BASE and image_key(0, 0) == image_key(5, 5) == BASE + SCALE + GAP <= KEY_FLT_MAX
    tiny = float(np.finfo(np.float32).tiny)
    for x, u in [(0, 1), (1, 64000), (31999, 64000), (1, 2), (32001, 64000), (63999, 64000), (1, 1), (0, 0)]:
        f = image_float(x, u)
        assert np.isfinite(f) and abs(f) >= tiny, (x, u, f)
    # the two keys around the gap: the last negative normal, the first positive one
    below = max(x for x in range(1, 64000) if image_key(x, 64000) < GAP_AT)
    assert image_float(below, 64000) < 0 < image_float(below + 1, 64000)
