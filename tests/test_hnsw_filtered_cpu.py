"""pgv_hnsw_scan_filtered without a GPU: the symbol in the header, the library and the binding; the bitmap the Python
face packs a filter into; and the preconditions of tests/test_gpu_hnsw_filtered.py -- on the same seeds, with model_scan
over exact host distances, every case named after a branch of hnswgettuple's loop really takes it, so that no GPU test
passes by never reaching its branch."""
import os
import re
import subprocess

import numpy as np
import pytest

import hnsw_filtered_cases as fc
import hnsw_scan_cases as sc
from hnsw_scan_model import model_scan
from pgvector_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "pgv_hip.h")) as f:
        header = f.read()
    decl = re.search(r"\bint\s+pgv_hnsw_scan_filtered\(([^;]*)\);", header)
    assert decl, "include/pgv_hip.h does not declare pgv_hnsw_scan_filtered"
    assert len(decl.group(1).split(",")) == 13
    assert "pgv_hnsw_scan_filtered" in _lib.SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT pgv_hnsw_scan_filtered$", out, re.M), "libpgv_hip.so does not export pgv_hnsw_scan_filtered"
    assert len(_lib.lib.pgv_hnsw_scan_filtered.argtypes) == 13
    assert re.search(r"#define\s+PGV_ABI_VERSION\s+1\b", header)


@pytest.mark.parametrize("n", (1, 31, 32, 33, 600))
def test_pack_keep_puts_element_e_at_bit_e_mod_32_of_word_e_div_32(n):
    rng = np.random.default_rng(n)
    for shape in ((n,), (5, n)):
        keep = rng.random(shape) < 0.5
        keep[..., n - 1] = True  # the last element's bit is the highest one used
        words = api.pack_keep(keep)
        assert words.dtype == np.uint32 and words.shape == shape[:-1] + ((n + 31) // 32,) and words.flags["C_CONTIGUOUS"]
        e = np.arange(n)
        assert np.array_equal((words[..., e >> 5] >> (e & 31).astype(np.uint32)) & 1, keep)
        if n % 32:  # nothing behind the last element
            assert not (words[..., -1] >> np.uint32(n % 32)).any()
    assert np.array_equal(api.pack_keep(np.ones(n, dtype=np.uint8)), api.pack_keep(np.ones(n, dtype=bool)))
    assert not api.pack_keep(np.zeros(n, dtype=bool)).any()


def test_pack_keep_packs_a_tensor_where_it_lives():
    torch = pytest.importorskip("torch")
    keep = np.random.default_rng(1).random((3, 77)) < 0.5
    got = api.pack_keep(torch.from_numpy(keep))
    assert got.dtype == torch.int32 and got.is_contiguous()
    assert np.array_equal(got.numpy().view(np.uint32), api.pack_keep(keep))


@pytest.fixture(scope="module")
def exact_models():
    rows, queries, graph = fc.float_case()
    m, entry, levels, start, nbr = graph
    d = sc.l2_table(queries, rows)
    for q in range(fc.NQ):
        assert len(np.unique(d[q])) == fc.N  # no ties: the device's fp32 order can differ from this one only by rounding

    def models(ef):
        return [lambda q=q: model_scan(d[q].tolist().__getitem__, levels, start, nbr, m, entry, ef) for q in range(fc.NQ)]
    return models


@pytest.mark.parametrize("name", list(fc.EDGES))
def test_edge_case_takes_its_branch(exact_models, name):
    want = fc.EDGES[name][4]
    seen = fc.edge_tags(name, exact_models)
    assert want <= seen, (name, sorted(want - seen))


def test_limits_switch_where_they_are_meant_to(exact_models):
    """max_scan_tuples 20000 is never reached, 1 is reached by the first batch, and 150 by the first batch of some queries
    and by a later one of others (ef 5; the first batch of ef 16 scores about 300 elements); with nothing kept every query
    runs to exhaustion, through the pool's drain or without it"""
    keep = fc.keep_mask(0.0, fc.N)
    for ef in fc.EFS:
        for limit in fc.LIMITS:
            walks = set()
            for make in exact_models(ef)[::4]:
                ids, _, tuples, batches, left, rp = fc.run_loop(fc.recorded(make, limit), fc.K, keep, False)
                kinds = [s[0] for s in rp.taken() if s[1]]
                assert ids == [] and left == 0 and batches == len(kinds)
                assert kinds == sorted(kinds, reverse=True)  # walks, then drains, never a walk again
                assert ("drain" in kinds) == (limit < 20000) and (limit < 20000 or tuples == fc.N)
                walks.add(kinds.count("walk"))
            if limit == 1:
                assert walks == {1}
            if limit == 150 and ef == 5:
                assert 1 in walks and max(walks) > 1
