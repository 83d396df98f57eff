"""tq_query.slop / tqh_query.slop (include/tantivy_amd.h "Sloppy phrases") on the CPU, the way tests/test_abi_cpu.py
reaches the library without a device: the field fills what was padding behind min_should_match, so the struct's size
and every other offset are what they were, and a zeroed query still means what it meant."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def _without_slop(struct):
    """The same struct laid out by ctypes from the field list without `slop`."""
    fields = [f for f in struct._fields_ if f[0] != "slop"]
    assert len(fields) == len(struct._fields_) - 1, "the struct has no slop field"
    return type(struct.__name__ + "Before", (C.Structure,), {"_fields_": fields})


@pytest.mark.parametrize("name", ["TqQuery", "TqhQuery"])
def test_slop_fills_padding(B, name):
    now = getattr(B, name)
    before = _without_slop(now)
    assert C.sizeof(now) == C.sizeof(before)
    assert now.slop.offset == now.min_should_match.offset + 4 and now.slop.size == 4
    for fname, _ in before._fields_:
        assert getattr(now, fname).offset == getattr(before, fname).offset, fname


def test_header_states_the_contract(B):
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "tantivy_amd.h")).read()
    assert "#define TQ_MAX_SLOP 255u" in src and "#define TQ_KERNEL_PHRASE_SLOP 0x40000u" in src
    assert "#define TQ_SLOP_CARRY_CAP %du" % B.SLOP_CARRY_CAP in src and B.SLOP_CARRY_CAP >= 32
    assert B.KERNEL_PHRASE_SLOP == 0x40000 and B.MAX_SLOP == 255
    assert hasattr(B.lib(), "tq_last_batch_slop_overflows")


def test_zeroed_query_still_answers(B):
    """tq_all_query_form needs no segment: a zeroed struct (slop 0) with one match-all clause is the query it was."""
    q = B.TqQuery()
    assert q.slop == 0 and bytes(q) == bytes(C.sizeof(B.TqQuery))
    rc, kind, base, min_should, keep_mask = B.all_query_form([B.TERM_ALL, 7], mode=B.MODE_BOOL, occurs=[1, 1])
    assert rc == 0 and keep_mask == 0b10 and min_should == 0  # `+* +a` is PLAIN: the All clause vanishes
    out = B.TqAllForm()
    terms = (C.c_uint32 * 1)(B.TERM_ALL)
    q.n_terms, q.terms, q.mode, q.k = 1, C.cast(terms, C.POINTER(C.c_uint32)), B.MODE_OR, 1
    assert B.lib().tq_all_query_form(C.byref(q), C.byref(out)) == 0
    assert out.base == 1.0 and out.keep_mask == 0
