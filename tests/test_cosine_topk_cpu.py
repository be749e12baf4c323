"""pgv_cosine_topk without a GPU: the header declares it, the library exports it, the binding carries it, and a call on a
machine without a device is PGV_ERR_DEVICE (there is no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

import pgvector_amd
from pgvector_amd import _lib, api


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(pgvector_amd.__file__), "..", "include", "pgv_hip.h")).read()
    assert re.search(r"\bpgv_cosine_topk\(pgv_ctx \* ctx, pgv_dtype dtype, int dim,", header)
    assert "pgv_cosine_topk" in _lib.SYMBOLS and hasattr(pgvector_amd.lib, "pgv_cosine_topk")
    assert callable(api.cosine_topk)


def test_tensors_of_another_element_type_are_refused():
    import torch
    q16, x32 = torch.zeros((1, 4), dtype=torch.float16), torch.zeros((2, 4), dtype=torch.float32)
    for q, x in ((q16, x32), (x32[:1], q16), (x32[:1].double(), x32)):
        with pytest.raises(TypeError):
            api.cosine_topk(None, q, x, 1)


@pytest.mark.skipif(pgvector_amd.lib.pgv_device_count() > 0, reason="a GPU is present")
def test_no_device_is_an_error():
    """No context can be made without a device (test_abi_cpu.py), so the entry gets a zeroed buffer for one.  That rests
    on pgv_cosine_topk reading nothing of its context but the leading `device` member before hipSetDevice refuses: an
    entry that read more first would crash here instead of failing"""
    fake_ctx = ctypes.create_string_buffer(1 << 14)
    q, out_d, out_i = np.ones((1, 4), np.float32), np.zeros((1, 1), np.float64), np.zeros((1, 1), np.int64)
    rc = pgvector_amd.lib.pgv_cosine_topk(ctypes.cast(fake_ctx, ctypes.c_void_p), api.PGV_F32, 4, api.ptr(q), 1, api.ptr(q), 1,
                                          1, api.ptr(out_d), api.ptr(out_i))
    assert rc == _lib.PGV_ERR_DEVICE
