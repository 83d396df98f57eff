"""CPU-only checks of the scored doc-set entry points (tq_docset_scored_batch, tq_docset_scored_batch_device,
tqh_docset_scored_prepared): exported, bound, and null arguments are errors with a message, not crashes.  No device
compute here."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def test_scored_docset_symbols_are_exported_and_bound(B):
    L = B.lib()
    for name in ("tq_docset_scored_batch", "tq_docset_scored_batch_device", "tqh_docset_scored_prepared"):
        assert name in B.EXPORTS, name
        assert hasattr(L, name), "missing export " + name
        assert getattr(L, name).argtypes, name + " has no argtypes"
    assert B.KERNEL_DOCSET_SCORE == 0x4000
    assert B.kernel_names(B.KERNEL_DOCSET_SCORE) == ["docset_score"]
    assert B.kernel_names(B.KERNEL_DOCSET | B.KERNEL_DOCSET_SCORE) == ["docset", "docset_score"]
    for method in ("docset_scored", "raw_docset_scored", "raw_docset_scored_device"):
        assert callable(getattr(B.DeviceIndex, method))


def test_scored_docset_null_arguments_are_errors_not_crashes(B):
    L = B.lib()
    starts = np.zeros(2, np.uint64)
    docs = np.zeros(4, np.uint32)
    scores = np.zeros(4, np.float32)
    u64p = C.POINTER(C.c_uint64)
    assert L.tq_docset_scored_batch(None, None, 1, B._u32(docs), B._f32(scores), 4, starts.ctypes.data_as(u64p)) != 0
    assert b"tq_docset_scored_batch" in L.tq_last_error()
    assert b"tq_docset_scored_batch_device" not in L.tq_last_error()
    assert L.tq_docset_scored_batch(None, None, 0, None, None, 0, None) != 0
    assert L.tq_docset_scored_batch_device(None, None, 1, None, None, 0, None, None) != 0
    assert b"tq_docset_scored_batch_device" in L.tq_last_error()
    assert L.tqh_docset_scored_prepared(None, None, None, None, 0, None) != 0
    assert L.tqh_last_error()
