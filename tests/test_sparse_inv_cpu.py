"""the inverted sparsevec rows' entries exist at every layer: header, library, ctypes table, Python class"""
import ctypes
import os
import re

from pgvector_amd import _lib, api

NAMES = ("pgv_sparse_rows_upload", "pgv_sparse_rows_free", "pgv_sparse_rows_topk")


def test_entries_are_declared_exported_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pgv_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert callable(api.SparseRows) and callable(api.SparseRows.topk) and callable(api.SparseRows.free)
    assert _lib.SPARSE_INV_ROWS in (2048, 4096) and 1 <= _lib.SPARSE_INV_QUERIES <= 16
