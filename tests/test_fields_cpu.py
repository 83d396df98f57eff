"""CPU-only checks of multi-field segments (include/tantivy_amd.h "multi-field segments"): the model and fixtures of
tests/fields_model.py — their self-checks and the DISCRIMINATION of every scored GPU case: the same model under field 0's
fieldnorms and cache for every term (what a kernel that ignores the field tag computes) gives another top-k doc sequence
or scores off by more than 1e-3 relative — and whatever of the entry points' argument validation runs without a device
(as tests/test_abi_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import all_model as AM
from tests import fields_model as FM
from tests import phrase_model as PM

ERR_INVALID = 1


@pytest.fixture(scope="module")
def L():
    import tantivy_amd

    return tantivy_amd.binding.lib()


# ---- the fixtures are what the issue asks for
def test_fixture_x_shape():
    fx = FM.fixture_x()
    assert fx.max_doc == 6000 and len(fx.fields) == 3 and fx.bases == [0, 16, 16 + PM.NT, 16 + PM.NT + 2]
    dfs = [t.doc_freq for t in fx.fields[0].terms]
    assert dfs == FM.X_DFS0 and {1, 128, 129}.issubset(dfs)
    assert any(df < 128 for df in dfs) and any(df * 128 >= fx.max_doc for df in dfs) and any(1 < df < fx.max_doc // 128 for df in dfs)
    ids0 = fx.fn_ids(0)
    assert ids0.min() >= 1 and ids0.max() <= 39 and np.unique(ids0).size > 30
    assert sorted(set(fx.fn_values[1])) == [20, 40] and fx.fields[2].fieldnorm is None and np.all(fx.fn_ids(2) == 1)
    assert all(f.record_option == O.WITH_FREQS_AND_POSITIONS for f in fx.fields)
    # the saturated tf bytes of field 1 lie behind field 0's sub-file: a non-zero idx base, a non-zero pos base
    assert fx.fields[0].idx_len > 8 and fx.fields[0].pos_len > 0
    tfs = np.concatenate([O.decode_postings(fx.fields[1], t)[1] for t in (0, 1)])
    assert {254, 255, 256, 300}.issubset(set(int(x) for x in tfs))


def test_fixture_y_shape():
    fx = FM.fixture_y()
    assert fx.max_doc == 70_000 and len(fx.fields) == 2 and fx.max_doc > 65_536 and fx.max_doc % 32 != 0
    assert [t.doc_freq for t in fx.fields[1].terms] == FM.Y_DFS1
    for t in range(3):
        docs = set(int(d) for d in O.decode_postings(fx.fields[1], t)[0])
        assert set(FM.Y_EDGE_DOCS).issubset(docs)
    assert np.unique(fx.fn_ids(1)).size > 30 and set(fx.fn_values[0]) == {40}


def test_global_ids_round_trip():
    for make in FM.FIXTURES.values():
        fx = make()
        seen = [fx.field_of(g) for g in range(fx.n_terms)]
        assert [fx.gid(f, t) for f, t in seen] == list(range(fx.n_terms))
        with pytest.raises(KeyError):
            fx.field_of(fx.n_terms)


def test_list_scores_are_the_oracles_own():
    """A list of field f scored by the glue = the oracle's own unpruned scorer over field f's segment."""
    fx = FM.fixture_x()
    L_ = FM.FieldLists(fx)
    for g in (fx.gid(0, 6), fx.gid(1, 0), fx.gid(1, 3), fx.gid(2, 1)):
        f, t = fx.field_of(g)
        L_.need(g)
        seg = fx.fields[f]
        w = O.bm25_for_one_term(seg.terms[t].doc_freq, fx.max_doc, fx.avg(f))
        d, s = O.match_all(seg, [t], O.MODE_OR, weights=[w])
        present, score = L_.lists[g]
        assert np.array_equal(np.nonzero(present)[0], np.asarray(d)) and np.array_equal(score[d].view(np.uint32), np.asarray(s, np.float32).view(np.uint32))
    assert L_.cache.shape == (3, 256) and not np.array_equal(L_.cache[0], L_.cache[1])


def test_phrase_glue_is_the_phrase_models():
    fx = FM.fixture_x()
    t2 = PM.corpus("T2")
    L_ = FM.FieldLists(fx)
    for name, terms, offs in PM.QUERIES:
        if name not in FM.PHRASE_QUERIES or PM.ABSENT in terms:
            continue
        present, score = L_.phrase([fx.gid(1, t) for t in terms], offs)
        docs, sc, _ = t2.expect([q[0] for q in PM.QUERIES].index(name))
        assert np.array_equal(np.nonzero(present)[0], docs) and np.allclose(score[docs], sc, rtol=1e-6)


# ---- discrimination: a kernel that ignores the field tag cannot pass the scored GPU cases
def _model_clauses(clauses, L_):
    out = []
    for occur, what in clauses:
        for t in (what[1] if what[0] == "union" else [what[1]]):
            L_.need(t)
        out.append((occur, what))
    return out


@pytest.mark.parametrize("name", ["X", "Y"])
def test_flat_cases_discriminate(name):
    fx = FM.FIXTURES[name]()
    right, wrong = FM.FieldLists(fx), FM.FieldLists(fx, as_primary=True)
    for clauses, msm in FM.flat_cases(fx):
        a = AM.expect(_model_clauses(clauses, right), msm, right.lists, fx.max_doc)
        b = AM.expect(_model_clauses(clauses, wrong), msm, wrong.lists, fx.max_doc)
        assert a[0].size > 0, clauses
        assert np.array_equal(a[0], b[0]), clauses  # (the doc set does not depend on norms)
        assert FM.differs(a, b), clauses


@pytest.mark.parametrize("name", ["X", "Y"])
def test_tree_cases_discriminate(name):
    fx = FM.FIXTURES[name]()
    right, wrong = FM.FieldLists(fx), FM.FieldLists(fx, as_primary=True)
    for spec, msm in FM.tree_cases(fx):
        a, b = FM.tree_expect(right, spec, msm), FM.tree_expect(wrong, spec, msm)
        assert a[0].size > 0 and np.array_equal(a[0], b[0]), spec
        assert FM.differs(a, b), spec


def test_standalone_phrases_discriminate():
    fx = FM.fixture_x()
    right, wrong = FM.FieldLists(fx), FM.FieldLists(fx, as_primary=True)
    some = 0
    for name, terms, offs in PM.QUERIES:
        if name not in FM.PHRASE_QUERIES or PM.ABSENT in terms:
            continue
        gids = [fx.gid(1, t) for t in terms]
        pa, sa = right.phrase(gids, offs)
        pb, sb = wrong.phrase(gids, offs)
        assert np.array_equal(pa, pb)
        docs = np.nonzero(pa)[0].astype(np.uint32)
        if docs.size:  # ("nomatch" has no doc: nothing to discriminate)
            some += 1
            assert FM.differs((docs, sa[docs]), (docs, sb[docs])), name
    assert some >= 4


def test_term_set_cases_discriminate():
    """Case 4: the set itself is a constant, the term of the third field beside it is what a field-blind kernel gets wrong."""
    fx = FM.fixture_x()
    right, wrong = FM.FieldLists(fx), FM.FieldLists(fx, as_primary=True)
    for L_ in (right, wrong):
        FM.add_set(L_, ("set", 1.0), FM.set_members(fx), 1.0)
        FM.add_set(L_, ("set", 2.5), FM.set_members(fx), 2.5)
    assert np.array_equal(right.lists[("set", 1.0)][1], wrong.lists[("set", 1.0)][1])
    for clauses, msm in FM.set_cases(fx, ("set", 1.0), ("set", 2.5)):
        a = AM.expect(_model_clauses(clauses, right), msm, right.lists, fx.max_doc)
        b = AM.expect(_model_clauses(clauses, wrong), msm, wrong.lists, fx.max_doc)
        assert a[0].size > 0 and np.array_equal(a[0], b[0]), clauses
        assert FM.differs(a, b), clauses


def test_tree_expect_equals_the_oracle_on_one_field():
    """The nested-query glue against the oracle's own tree evaluation where the oracle can answer: every term of one field."""
    fx = FM.fixture_x()
    L_ = FM.FieldLists(fx)
    g = lambda t: fx.gid(1, t)  # noqa: E731
    for spec_l, spec_g in (([(O.MUST, 4), (O.MUST, [(O.MUST, 5), (O.MUST, 6)], 0)], [(FM.M, g(4)), (FM.M, [(FM.M, g(5)), (FM.M, g(6))], 0)]),
                           ([(O.SHOULD, [(O.MUST, 5), (O.MUST, 6)], 0), (O.SHOULD, 4)], [(FM.S, [(FM.M, g(5)), (FM.M, g(6))], 0), (FM.S, g(4))])):
        d, s = O.tree_match_all(fx.fields[1], spec_l, 0)
        wd, ws = FM.tree_expect(L_, spec_g, 0)
        assert np.array_equal(np.asarray(d, np.uint32), wd) and np.allclose(np.asarray(s, np.float32), ws, rtol=1e-5)


# ---- argument validation that needs no device
def test_exports_and_null_arguments(L):
    for name in ("tq_segment_upload_fields", "tq_term_prepare_field", "tq_term_prepare_batch_fields", "tq_term_field",
                 "tq_segment_get_fields_stats", "tqh_searcher_add_segment_fields", "tqh_searcher_add_remote_stats_fields"):
        assert hasattr(L, name), name
    seg = C.c_void_p()
    assert L.tq_segment_upload_fields(None, 0, 10, 1, None, 0, C.byref(seg)) == ERR_INVALID
    assert b"null" in L.tq_last_error()
    h, f = C.c_uint32(), C.c_uint32()
    assert L.tq_term_prepare_field(None, 0, 0, 0, 0, 0, 1, C.byref(h)) == ERR_INVALID
    assert L.tq_term_prepare_batch_fields(None, None, None, 0, None) == ERR_INVALID
    assert L.tq_term_field(None, 0, C.byref(f)) == ERR_INVALID
    assert L.tq_segment_get_fields_stats(None, None) == ERR_INVALID


def test_struct_layouts():
    import tantivy_amd.binding as B

    assert C.sizeof(B.TqFieldFiles) == 48 and C.sizeof(B.TqFieldsStats) == 16 and B.MAX_FIELDS == 8
    # the structs existing raw-ABI callers build keep their layout
    assert C.sizeof(B.TqTermInfo) == 32 and C.sizeof(B.TqQuery) == 104
