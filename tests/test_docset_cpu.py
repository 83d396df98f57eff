"""CPU-only checks of the doc-set entry points (tq_docset_batch, tq_docset_batch_device, tqh_docset_prepared):
exported, bound, and null arguments are errors with a message, not crashes.  No device compute here."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def test_docset_symbols_are_exported_and_bound(B):
    L = B.lib()
    for name in ("tq_docset_batch", "tq_docset_batch_device", "tqh_docset_prepared"):
        assert name in B.EXPORTS, name
        assert hasattr(L, name), "missing export " + name
        assert getattr(L, name).argtypes, name + " has no argtypes"
    assert B.KERNEL_DOCSET == 0x2000
    assert B.kernel_names(B.KERNEL_DOCSET) == ["docset"]
    for method in ("docset", "raw_docset", "raw_docset_device"):
        assert callable(getattr(B.DeviceIndex, method))


def test_docset_null_arguments_are_errors_not_crashes(B):
    L = B.lib()
    starts = np.zeros(2, np.uint64)
    docs = np.zeros(4, np.uint32)
    u64p = C.POINTER(C.c_uint64)
    assert L.tq_docset_batch(None, None, 1, B._u32(docs), 4, starts.ctypes.data_as(u64p)) != 0
    assert b"tq_docset_batch" in L.tq_last_error()
    assert L.tq_docset_batch(None, None, 0, None, 0, None) != 0
    assert L.tq_docset_batch_device(None, None, 1, None, 0, None, None) != 0
    assert b"tq_docset_batch_device" in L.tq_last_error()
    assert L.tqh_docset_prepared(None, None, None, 0, None) != 0
    assert L.tqh_last_error()
