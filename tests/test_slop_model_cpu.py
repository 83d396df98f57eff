"""tests/slop_model.py pinned to the reference's own vectors (tests/golden/phrase_slop_reference.json: the inputs and
expected outputs of phrase_scorer.rs's test_slop / test_merge_slop / test_carry_slop_intersection and of the index-level
slop tests of phrase_query/mod.rs), and the two properties the device contract is built on: the scored and the unscored
verdict differ, and the verdict depends on the lists' cost order."""
import json
import os

import pytest

from tests import phrase_model as PM
from tests import slop_model as SM

with open(os.path.join(os.path.dirname(__file__), "golden", "phrase_slop_reference.json")) as f:
    GOLD = json.load(f)


def _index(texts):
    """The reference's create_index over its default tokenizer (split on whitespace, lower-cased): term -> {doc: [pos]},
    fieldnorms = token counts (exact below 40 tokens)."""
    vocab, tp, norms = {}, [], []
    for d, text in enumerate(texts):
        toks = text.lower().split()
        norms.append(len(toks))
        for p, tok in enumerate(toks):
            t = vocab.setdefault(tok, len(vocab))
            if t == len(tp):
                tp.append({})
            tp[t].setdefault(d, []).append(p)
    return vocab, tp, norms


@pytest.mark.parametrize("case", GOLD["pair_merge"], ids=lambda c: "%s|%s~%d" % (c["left"], c["right"], c["slop"]))
def test_pair_walk_vectors(case):
    assert SM.pair_merge(case["left"], case["right"], case["slop"]) == case["kept"]
    assert SM.pair_count(case["left"], case["right"], case["slop"]) == len(case["kept"])
    assert SM.pair_exists(case["left"], case["right"], case["slop"]) == bool(case["kept"])


@pytest.mark.parametrize("case", GOLD["carry"], ids=lambda c: "%s~%d" % (c["lists"], c["slop"]))
def test_carry_vectors(case):
    count, out = SM.fold_reference_style(case["lists"], case["slop"])
    assert [list(x) for x in out] == case["out"]
    assert count == case["count"]


@pytest.mark.parametrize("case", GOLD["index"], ids=lambda c: c["name"])
def test_index_level_cases(case):
    vocab, tp, norms = _index(case["texts"])
    terms = [vocab.get(w, PM.ABSENT) for w in case["phrase"]]
    exp = SM.SlopExpect(tp, terms, list(range(len(terms))), case["slop"], norms)
    if case["hits"] is not None:
        assert exp.docs.size == case["hits"], exp.docs
    # assert_nearly_equals!(left, right) of the reference: |left - right| <= 0.0005 (src/lib.rs, its default epsilon)
    eps = GOLD["score_epsilon"]
    assert eps == 0.0005
    for at, want in case.get("scores", {}).items():
        assert abs(float(exp.scores[int(at)]) - want) <= eps, (at, exp.scores, want)


def test_scored_and_unscored_verdicts_differ():
    # doc "a x b x c", phrase "a b c", slop 1: the counting walk carries the slop spent on a..b and has none left for
    # b..c; the existence walk of the last list forgets it
    _, tp, _ = _index(["a x b x c"])
    v = SM.verdicts(tp, [0, 2, 3], [0, 1, 2], 1)[0]
    assert v.count == 0 and v.exists is True


def test_verdict_depends_on_cost_order():
    # doc 0 = "x b x a c", phrase "a b c", slop 3.  The two indexes differ in the doc freqs of a and c alone (filler docs
    # that hold one term): walked a, b, c the doc does not match; walked c, b, a it does.
    doc = {0: [3], 1: [1], 2: [4]}

    def index(dfs):
        tp = []
        for t in range(3):
            lists = {100 * (t + 1) + i: [0] for i in range(dfs[t] - 1)}
            lists[0] = doc[t]
            tp.append(lists)
        return tp

    a = SM.verdicts(index((1, 2, 3)), [0, 1, 2], [0, 1, 2], 3)[0]
    b = SM.verdicts(index((3, 2, 1)), [0, 1, 2], [0, 1, 2], 3)[0]
    assert SM.cost_order(index((1, 2, 3)), [0, 1, 2]) == [0, 1, 2] and SM.cost_order(index((3, 2, 1)), [0, 1, 2]) == [2, 1, 0]
    assert a.count == 0 and b.count == 1, (a.count, b.count)


def test_stable_tie_and_adjusted_positions():
    tp = [{0: [5], 1: [1]}, {0: [7], 2: [1]}, {0: [9]}]
    assert SM.cost_order(tp, [0, 1, 2]) == [2, 0, 1]  # rarest first, the tie of terms 0 and 1 in phrase order
    assert SM.cost_order(tp, [1, 0, 2]) == [2, 0, 1]  # (indices into the phrase: term 1 stands first there)
    assert SM.adjusted_lists(tp, [0, 1, 2], [0, 1, 3], 0) == [[9], [8], [9]]


def test_two_terms_carry_nothing():
    v = SM.doc_verdict([[1, 2, 3, 4, 5, 6, 7, 8] * 1, [2, 9]], 3)
    assert v.longest == 0 and v.count == 2
