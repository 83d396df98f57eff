"""CPU-only checks of the term-set entry points (include/tantivy_amd.h "term sets", tantivy_amd/csrc/tq_termset.cpp):
the three functions are declared, exported and bound; null arguments are errors, not crashes; tq_all_query_form counts an
arbitrary non-special handle — what a set's handle is — as a present list; and the literal model the GPU tests take their
expectations from (tests/all_model.py) gives a Should set clause the doc set of the union of its members.  No device
compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import all_model as AM

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
OK, ERR_INVALID = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("tq_term_set_prepare", "tq_term_set_info", "tq_term_set_release")


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def test_header_declares_the_three_functions():
    with open(os.path.join(ROOT, "include", "tantivy_amd.h")) as f:
        text = f.read()
    assert "---- term sets ----" in text
    flat = re.sub(r"\s+", " ", text)
    assert "int tq_term_set_prepare(tq_segment *seg, const tq_term_handle *members, uint32_t n, tq_term_handle *out);" in flat
    assert "int tq_term_set_info(tq_segment *seg, tq_term_handle set, uint32_t *n_docs, uint64_t *bytes);" in flat
    assert "int tq_term_set_release(tq_segment *seg, tq_term_handle set);" in flat


def test_symbols_are_exported_and_bound(B):
    L = B.lib()
    for name in FUNCTIONS:
        assert name in B.EXPORTS, name
        assert hasattr(L, name) and getattr(L, name).argtypes, name
    assert issubclass(B.RawHandle, int) and B.RawHandle(7) == 7
    for name in ("term_set_prepare", "term_set_info", "term_set_release"):
        assert callable(getattr(B.DeviceIndex, name)), name


def test_null_arguments_are_errors_not_crashes(B):
    L = B.lib()
    out = C.c_uint32(123)
    n_docs, nbytes = C.c_uint32(), C.c_uint64()
    members = (C.c_uint32 * 2)(0, 1)
    assert L.tq_term_set_prepare(None, members, 2, C.byref(out)) == ERR_INVALID
    assert b"tq_term_set_prepare" in L.tq_last_error()
    assert L.tq_term_set_prepare(None, None, 0, C.byref(out)) == ERR_INVALID
    assert out.value == 123
    assert L.tq_term_set_info(None, 0, C.byref(n_docs), C.byref(nbytes)) == ERR_INVALID
    assert b"tq_term_set_info" in L.tq_last_error()
    assert L.tq_term_set_release(None, 0) == ERR_INVALID
    assert b"tq_term_set_release" in L.tq_last_error()


def test_all_query_form_counts_any_other_handle_as_a_present_list(B):
    """What the routes of a set beside TQ_TERM_ALL rely on: the normal form needs no segment, so a handle that is neither
    TQ_TERM_ALL nor TQ_TERM_ABSENT — a term's or a set's — is a list that survives."""
    for h in (0, 5, 4097, 0x7FFFFFFF, 0xFFFFFFFD):
        rc, kind, base, min_should, mask = B.all_query_form([B.TERM_ALL, h], [1.0, 2.5], B.MODE_BOOL, [M, N], None, 0)
        assert (rc, kind, min_should, mask) == (OK, B.ALL_BASED, 0, 0b10), h  # `+* -set`: every doc minus the list
        assert base == 1.0
        rc, kind, base, min_should, mask = B.all_query_form([B.TERM_ALL, h], [1.0, 2.5], B.MODE_BOOL, [S, S], None, 0)
        assert (rc, kind, mask) == (OK, B.ALL_BASED, 0b10), h             # `* set`: every doc, the list adds its score
        rc, kind, base, min_should, mask = B.all_query_form([B.TERM_ALL, h], [1.0, 2.5], B.MODE_BOOL, [M, M], None, 0)
        assert (rc, kind, mask) == (OK, B.ALL_PLAIN, 0b10), h             # `+* +set` is `+set`
        rc, kind, base, min_should, mask = B.all_query_form([B.TERM_ALL, B.TERM_ABSENT], [1.0, 2.5], B.MODE_BOOL, [M, M], None, 0)
        assert (rc, kind) == (OK, B.ALL_EMPTY)


def test_model_gives_a_should_set_the_doc_set_of_the_union_of_its_members():
    """tests/all_model.py takes a set as one list (present = OR of the members, score = full(weight)).  Over random dense
    arrays: as a Should clause beside random Must / MustNot terms its doc set is that of the ("union", members) clause,
    and where the set is the only scoring clause every doc scores the weight."""
    rng = np.random.default_rng(20261019)
    n = 97
    for case in range(400):
        n_terms = int(rng.integers(2, 9))
        lists = {}
        for t in range(n_terms):
            p = rng.random(n) < rng.choice([0.02, 0.1, 0.4, 0.8])
            lists[t] = (p, (rng.random(n) * 3 + 0.01).astype(np.float32))
        members = [int(t) for t in rng.choice(n_terms, size=int(rng.integers(1, n_terms)), replace=False)]
        others = [t for t in range(n_terms) if t not in members]
        weight = np.float32(rng.choice([0.0, 1.0, 2.5]))
        present = np.zeros(n, bool)
        for t in members:
            present |= lists[t][0]
        with_set = dict(lists)
        with_set["set"] = (present, np.full(n, weight, np.float32))
        extra = [(int(rng.choice([M, N, S])), ("term", t)) for t in others[: int(rng.integers(0, 3))]]
        minimum = int(rng.integers(0, 2))
        docs_set, scores_set = AM.expect([(S, ("term", "set"))] + extra, minimum, with_set, n)
        docs_union, _ = AM.expect([(S, ("union", members))] + extra, minimum, lists, n)
        assert np.array_equal(docs_set, docs_union), (case, members, extra, minimum)
        alone_docs, alone_scores = AM.expect([(S, ("term", "set"))], 0, with_set, n)
        assert np.array_equal(alone_docs, np.nonzero(present)[0]) and np.all(alone_scores == weight), case
        # the model's intersections sort by present.sum(): the set's cost is its doc count
        assert AM.sub_scorer(n, ("term", "set"), with_set).cost == int(present.sum())
