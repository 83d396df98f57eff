"""CPU-only checks of tq_all_query_form (tantivy_amd/csrc/tq_all.cpp): the normal form of a flat query with AllQuery
clauses (TQ_TERM_ALL) against a literal model of BooleanWeight::complex_scorer (tests/all_model.py, written from
src/query/boolean_query/boolean_weight.rs:114-171, 236-431, 440-456).  No device compute here."""
import ctypes as C

import numpy as np
import pytest

from tests import all_model as AM

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, 1, 4
N_DOCS = 48  # dense arrays of the model
N_TERMS = 6
N_CASES = 24_000


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def test_symbol_is_exported_and_bound(B):
    L = B.lib()
    assert "tq_all_query_form" in B.EXPORTS
    assert hasattr(L, "tq_all_query_form") and L.tq_all_query_form.argtypes
    assert B.TERM_ALL == 0xFFFFFFFE and B.KERNEL_ALL == 0x8000 and B.kernel_names(B.KERNEL_ALL) == ["all"]
    assert (B.ALL_EMPTY, B.ALL_PLAIN, B.ALL_BASED) == (AM.ALL_EMPTY, AM.ALL_PLAIN, AM.ALL_BASED)


def test_null_arguments_are_errors_not_crashes(B):
    L = B.lib()
    f = B.TqAllForm()
    q = B.TqQuery()
    assert L.tq_all_query_form(None, C.byref(f)) == ERR_INVALID
    assert b"tq_all_query_form" in L.tq_last_error()
    assert L.tq_all_query_form(C.byref(q), None) == ERR_INVALID
    assert L.tq_all_query_form(C.byref(q), C.byref(f)) == ERR_INVALID  # no terms
    assert B.all_query_form([B.TERM_ALL] * 17, occurs=[M] * 17)[0] == ERR_INVALID
    assert B.all_query_form([B.TERM_ALL], occurs=None)[0] == ERR_INVALID  # TQ_MODE_BOOL without occurs
    assert B.all_query_form([B.TERM_ALL], occurs=[3])[0] == ERR_INVALID


def _lists(rng):
    """Dense (present, score) arrays of N_TERMS terms: densities from sparse to nearly full, positive f32 scores."""
    out = {}
    for t in range(N_TERMS):
        p = rng.random(N_DOCS) < (0.15, 0.3, 0.5, 0.7, 0.9, 0.05)[t]
        out[t] = (p, (rng.random(N_DOCS) * 3 + 0.01).astype(np.float32))
    return out


def _random_case(rng):
    """1-6 clauses of All / absent / term with a minimum of 0-4.  The two exclusions of the check — more than two Must
    terms, a one-clause query that carries a minimum — are enforced HERE: nothing is dropped afterwards."""
    n = int(rng.integers(1, 7))
    clauses, n_must_terms = [], 0
    terms = rng.permutation(N_TERMS)
    for i in range(n):
        occur = int(rng.choice([S, S, M, N]))
        r = rng.random()
        if r < 0.3:
            what = ("all", 1.0)
        elif r < 0.42:
            what = ("absent",)
        else:
            what = ("term", int(terms[i]))
            if occur == M:
                n_must_terms += 1
                if n_must_terms > 2:
                    occur = S
        clauses.append((occur, what))
    minimum = int(rng.integers(0, 5)) if n > 1 else 0
    return clauses, minimum


def _call(B, clauses, minimum, boosts=None):
    handles = [B.TERM_ALL if w[0] == "all" else B.TERM_ABSENT if w[0] == "absent" else 7 + w[1] for _, w in clauses]
    weights = [w[1] if w[0] == "all" else 1.5 for _, w in clauses] if boosts is None else boosts
    return B.all_query_form(handles, weights, B.MODE_BOOL, [o for o, _ in clauses], None, minimum)


def test_form_agrees_with_the_literal_model(B):
    """>= 20 000 random clause lists: the (kind, base, min_should, keep_mask) the literal model implies is the
    function's, and what that form computes (tests/all_model.eval_form: the rules of DESIGN.md "AllQuery") is what the
    literal model computes over dense arrays, docs and f32 scores bit for bit."""
    rng = np.random.default_rng(20261018)
    lists = _lists(rng)
    kinds = {AM.ALL_EMPTY: 0, AM.ALL_PLAIN: 0, AM.ALL_BASED: 0}
    for case in range(N_CASES):
        clauses, minimum = _random_case(rng)
        sc, trace = AM.complex_scorer(clauses, minimum, lists, N_DOCS)
        want = AM.implied_form(clauses, trace)
        rc, kind, base, min_should, keep_mask = _call(B, clauses, minimum)
        assert rc == OK, (case, clauses, minimum, B.lib().tq_last_error())
        assert (kind, base, min_should, keep_mask) == want, (case, clauses, minimum)
        present, score = AM.eval_form(want, clauses, lists, N_DOCS)
        assert np.array_equal(present, sc.present), (case, clauses, minimum)
        assert np.array_equal(score[present].view(np.uint32), sc.score[present].view(np.uint32)), (case, clauses, minimum)
        kinds[kind] += 1
    assert min(kinds.values()) > 1000, kinds  # every kind is well covered


def test_odd_but_literal_consequences(B):
    a, b, c = ("term", 0), ("term", 1), ("term", 2)
    star = ("all", 1.0)
    form = lambda cl, m=0: _call(B, cl, m)[1:]  # noqa: E731
    assert form([(M, star), (M, a)]) == (AM.ALL_PLAIN, 0.0, 0, 0b10)                 # `+* +a` scores bm25(a)
    assert form([(M, star), (S, a)]) == (AM.ALL_BASED, 1.0, 0, 0b10)                 # `+* a`: 1 + bm25(a) on every doc
    assert form([(M, star), (S, a), (S, b)], 2) == (AM.ALL_PLAIN, 0.0, 2, 0b110)     # a + b, no + 1
    assert form([(M, star), (S, a), (S, b), (S, c)], 2) == (AM.ALL_BASED, 1.0, 2, 0b1110)
    assert form([(S, star), (S, star), (S, a)], 2) == (AM.ALL_BASED, 1.0, 0, 0b100)  # every doc, s + 1
    assert form([(N, star)]) == (AM.ALL_EMPTY, 0.0, 0, 0)
    assert form([(M, a), (N, star)]) == (AM.ALL_EMPTY, 0.0, 0, 0)
    assert form([(S, star), (S, ("absent",))]) == (AM.ALL_BASED, 1.0, 0, 0)          # `* none` matches every doc
    assert form([(S, star), (S, a)], 2) == (AM.ALL_PLAIN, 0.0, 1, 0b10)              # a removed Should-All adds nothing
    assert form([(M, star), (N, a)]) == (AM.ALL_BASED, 1.0, 0, 0b10)
    # TQ_MODE_AND = all Must, TQ_MODE_OR = all Should with minimum 0
    assert B.all_query_form([B.TERM_ALL, 9], [1.0, 2.0], B.MODE_AND)[1:] == (AM.ALL_PLAIN, 0.0, 0, 0b10)
    assert B.all_query_form([B.TERM_ALL, 9], [1.0, 2.0], B.MODE_OR)[1:] == (AM.ALL_BASED, 1.0, 0, 0b10)
    assert B.all_query_form([B.TERM_ALL], None, B.MODE_AND)[1:] == (AM.ALL_BASED, 1.0, 0, 0)  # weights NULL: boost 1.0


def test_boosted_all(B):
    """A boosted All is no bare AllScorer: the reference does not remove it.  Doc sets never depend on the boost (the
    form is the unboosted query's); scores are taken only for the sole non-MustNot clause that holds anything."""
    a = ("term", 0)
    assert _call(B, [(S, ("all", 2.5))], 0) == (OK, AM.ALL_BASED, 2.5, 0, 0)
    assert _call(B, [(M, ("all", -1.0)), (N, a)], 0) == (OK, AM.ALL_BASED, -1.0, 0, 0b10)
    assert _call(B, [(S, ("all", 2.5)), (N, a), (S, ("absent",))], 0) == (OK, AM.ALL_BASED, 2.5, 0, 0b10)
    assert _call(B, [(N, ("all", 2.5)), (S, a)], 0) == (OK, AM.ALL_EMPTY, 0.0, 0, 0)
    for boosted, plain in (([(M, ("all", 2.0)), (S, a)], [(M, ("all", 1.0)), (S, a)]),
                           ([(S, ("all", 2.0)), (S, ("all", 1.0))], [(S, ("all", 1.0)), (S, ("all", 1.0))]),
                           ([(M, ("all", 0.5)), (M, a)], [(M, ("all", 1.0)), (M, a)])):
        rc, kind, base, min_should, keep_mask = _call(B, boosted, 0)
        assert rc == ERR_UNSUPPORTED and np.isnan(base), boosted
        assert b"boosted" in B.lib().tq_last_error()
        unboosted = _call(B, plain, 0)
        assert (kind, min_should, keep_mask) == (unboosted[1], unboosted[3], unboosted[4]), boosted
    assert _call(B, [(S, ("all", float("inf")))], 0)[0] == ERR_INVALID
    assert _call(B, [(S, ("all", float("nan"))), (S, a)], 0)[0] == ERR_INVALID
    # the boost changes no doc set: a boosted All stays an always-present scorer in the literal model
    rng = np.random.default_rng(7)
    lists = _lists(rng)
    for case in range(3000):
        clauses, minimum = _random_case(rng)
        boosted = [(o, ("all", 2.0) if w[0] == "all" and rng.random() < 0.6 else w) for o, w in clauses]
        sc, _ = AM.complex_scorer(boosted, minimum, lists, N_DOCS)
        _, kind, _, min_should, keep_mask = _call(B, boosted, minimum)
        present, _ = AM.eval_form((kind, 1.0, min_should, keep_mask), clauses, lists, N_DOCS)
        assert np.array_equal(present, sc.present), (case, boosted, minimum)


def test_refusals(B):
    ALL = B.TERM_ALL
    rc = B.all_query_form([ALL, 9], [1.0, 1.0], B.MODE_PHRASE)[0]
    assert rc == ERR_INVALID and b"phrase" in B.lib().tq_last_error()
    rc = B.all_query_form([ALL, 9, 10], [1.0] * 3, B.MODE_BOOL, [S, S, S], [0, 0, 1])[0]  # shares a clause_of value
    assert rc == ERR_UNSUPPORTED and b"clause_of" in B.lib().tq_last_error()
    rc = B.all_query_form([9, ALL, 10], [1.0] * 3, B.MODE_BOOL, [S, S, S], [0, 1, 1])[0]
    assert rc == ERR_UNSUPPORTED
    # a clause_of union beside an All clause of its own is fine: the union is one Should clause
    assert B.all_query_form([ALL, 9, 10, 11], [1.0] * 4, B.MODE_BOOL, [M, S, S, S], [0, 1, 1, 2], 2)[1:] == \
        (AM.ALL_PLAIN, 0.0, 2, 0b1110)
    assert B.all_query_form([ALL, 9, B.TERM_ABSENT, 11], [1.0] * 4, B.MODE_BOOL, [M, S, S, S], [0, 1, 1, 2], 1)[1:] == \
        (AM.ALL_BASED, 1.0, 1, 0b1010)
    # inside a nested query (tq_query.nested_occurs): refused
    q = B.TqQuery()
    hs = (C.c_uint32 * 3)(9, ALL, 10)
    oc = (C.c_uint8 * 3)(M, M, M)
    co = (C.c_uint8 * 3)(0, 1, 1)
    no = (C.c_uint8 * 3)(255, 1, 1)
    q.n_terms, q.mode, q.k = 3, B.MODE_BOOL, 1
    q.terms, q.occurs = C.cast(hs, C.POINTER(C.c_uint32)), C.cast(oc, C.POINTER(C.c_uint8))
    q.clause_of, q.nested_occurs = C.cast(co, C.POINTER(C.c_uint8)), C.cast(no, C.POINTER(C.c_uint8))
    f = B.TqAllForm()
    assert B.lib().tq_all_query_form(C.byref(q), C.byref(f)) == ERR_UNSUPPORTED
    assert b"nested" in B.lib().tq_last_error()
