"""The plateau model (tests/plateau_model.py) on the CPU: the premises every batch of tests/test_gpu_plateau_ties.py
rests on — conditions, not measurements — and the model itself against the oracle's executors."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import plateau_model as P
from tests.helpers import rel_close


def _corpus(b):
    return P.CORPORA[b.corpus]()


@pytest.mark.parametrize("name", P.BATCH_NAMES)
def test_premises(name):
    """Class gap >= 1e-3 on every query; at least three quarters of the (query, k) pairs cut a class in two; a
    shared-launch batch has, for every k, a query whose k-th class holds more than 4 x (k + 64) docs inside one
    8 192-posting run of its leading list (a staging list is cut in the middle of a task)."""
    b, ans = P.batch(name), P.answers(name)
    c = _corpus(b)
    assert len(b.queries) >= 1
    for q, a in zip(b.queries, ans):
        assert a.min_gap >= P.MIN_GAP, (q, a.min_gap)
    pairs = [(qi, k) for qi in range(len(b.queries)) for k in b.ks]
    tie = [P.straddles(ans[qi], k, b.copies) for qi, k in pairs]
    assert 4 * sum(tie) >= 3 * len(pairs), (name, sum(tie), len(pairs))
    for k in b.ks:  # every k has tie cases
        assert any(P.straddles(a, k, b.copies) for a in ans), (name, k)
    if b.shared:
        for k in b.ks:
            best = max(P.kth_class_in_one_run(c, q, a, k) for q, a in zip(b.queries, ans))
            assert best > 4 * (k + 64), (name, k, best)
    if b.deleted:  # the deletes took the lowest docs of a class some (query, k) cuts: no row holds one, and rows moved
        moved = 0
        for q in b.queries:
            before, after = P.answer(c, q), P.answer(c, q, b.deleted)
            for k in b.ks:
                r0, r1 = P.row(before, k), P.row(after, k)
                assert not set(d for _, d, _ in r1) & set(b.deleted)
                moved += r0 != r1
        assert moved >= len(b.queries)


def test_batch_shapes():
    """What the GPU cases count on: the shared intersections are a few hundred queries with twins and a leader
    shared by more than 32 DISTINCT queries; the union batches span 2 to 8 terms; every boolean and tree shape
    survived the gap filter."""
    b = P.batch("shared_ands")
    c = _corpus(b)
    assert len(b.queries) >= 200 and len(set(b.queries)) < len(b.queries)
    by_leader = {}
    for q in set(b.queries):
        by_leader.setdefault(P.leading_list(c, q), set()).add(q)
    assert max(len(v) for v in by_leader.values()) > 32, {k: len(v) for k, v in by_leader.items()}
    assert {len(q.spec[0]) for q in b.queries} == {2, 3, 4}
    sizes = {len(q.spec[0]) for n in ("shared_unions_periodic", "shared_unions_equal_df") for q in P.batch(n).queries}
    assert sizes >= {2, 3, 4, 5, 6, 7, 8}, sizes
    assert {(q.spec[1], q.spec[2], q.spec[3]) for q in P.batch("shared_bools").queries} == \
        {(tuple(o), None if cf is None else tuple(cf), m) for o, cf, m in P.BOOL_SHAPES}
    assert len(P.batch("trees").queries) == 3 * len(P.TREE_SHAPES)
    used = {t for q in P.batch("shared_unions_periodic").queries for t in q.spec[0]}
    assert {5, 6} <= used  # the list without a bitmap and the list without a column
    # the 40 fillers are longer than both rare lists: the 40 doc-matrix columns never reach those
    per = P.periodic()
    by_df = sorted(range(len(per.lists)), key=lambda t: -per.df(t))
    assert by_df[-2:] == [6, 5] and len(by_df) >= 42 and per.df(5) == 129


def _oracle_all(c, q):
    seg = c.seg
    if q.kind in ("and", "or"):
        terms, boosts = q.spec
        mode = O.MODE_AND if q.kind == "and" else O.MODE_OR
        w = O.default_weights(seg, list(terms), mode, boosts=None if boosts is None else list(boosts))
        return O.match_all(seg, list(terms), mode, weights=w)
    if q.kind == "bool":
        terms, occ, cof, msm = q.spec
        return O.bool_match_all(seg, list(terms), list(occ), None if cof is None else list(cof), msm)
    if q.kind == "tree":
        return O.tree_match_all(seg, q.spec[0], q.spec[1])
    return O.match_all(seg, list(q.spec), O.MODE_PHRASE)


@pytest.mark.parametrize("name", [n for n in P.BATCH_NAMES if not n.startswith("two_segment")])
def test_model_against_the_oracle(name):
    """Match sets equal, scores within 1e-5, and for the flat 2-term queries (the oracle's order is canonical there)
    the expected row equal to the oracle's exhaustive top-k, docs and order."""
    b = P.batch(name)
    c = _corpus(b)
    seen = set()
    for q in b.queries:
        if repr(q) in seen:  # (twins)
            continue
        seen.add(repr(q))
        a = P.answer(c, q)  # (the oracle knows no deletes)
        d, s = _oracle_all(c, q)
        assert np.array_equal(a.docs, d.astype(np.int64)), q
        assert all(rel_close(x, float(y), 1e-5) for x, y in zip(a.scores.tolist(), s.tolist())), q
        if q.kind in ("and", "or") and len(q.spec[0]) == 2 and q.spec[1] is None:
            for k in b.ks:
                want = O.search(c.seg, list(q.spec[0]), O.MODE_AND if q.kind == "and" else O.MODE_OR, k, pruned=False)
                assert [doc for _, doc, _ in P.row(a, k)] == [doc for _, doc in want], (q, k)


def test_model_under_two_segments_statistics():
    """The two-segment batches: the model's scores under the doubled statistics against the oracle's weights."""
    for name in ("two_segment_ands", "two_segment_unions"):
        b = P.batch(name)
        c = _corpus(b)
        seg = c.seg
        for q in b.queries[::3]:
            terms, boosts = q.spec
            mode = O.MODE_AND if q.kind == "and" else O.MODE_OR
            w = O.default_weights(seg, list(terms), mode, total_num_docs=2 * seg.max_doc, total_num_tokens=2 * seg.total_num_tokens,
                                  dfs=[2 * c.df(t) for t in terms], boosts=None if boosts is None else list(boosts))
            d, s = O.match_all(seg, list(terms), mode, weights=w)
            a = P.answer(c, q, (), 2)
            assert np.array_equal(a.docs, d.astype(np.int64)), q
            assert all(rel_close(x, float(y), 1e-5) for x, y in zip(a.scores.tolist(), s.tolist())), q
            r = P.row(a, 10, copies=2)  # inside a class: every doc of segment 0 before any of segment 1
            assert r == sorted(r, key=lambda x: (-x[2], x[0], x[1])), q
        # rows that segment 0 fills alone (its share of the class holds k docs) and rows that need both segments
        rows = [P.row(a, 10, copies=2) for a in P.answers(name)]
        assert any({o for o, _, _ in r} == {0} for r in rows) and any({o for o, _, _ in r} == {0, 1} for r in rows), name
