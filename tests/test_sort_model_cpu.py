"""CPU checks of sort by fast field (TopDocs::order_by_fast_field; tests/sort_model.py, tantivy_amd.binding): the closed form
that tests/test_gpu_sort.py holds the device to IS what the reference's TopNComputer yields when it is fed in ascending doc
order; merge_sorted_top_k is the closed form over the concatenated segments; and the C ABI of the feature is declared,
bound and exported.  No device compute here."""
import os
import re

import numpy as np
import pytest

from tests import sort_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 7, 64)


def _random_input(rng, n_docs, n_distinct, null_fraction, hi_bits=False):
    """match docs (a random half of n_docs), values of 2-4 distinct kinds, a presence pattern."""
    pool = [0, (1 << 64) - 1, 1 << 30, (1 << 30) - 1, 12345][:n_distinct] if hi_bits else list(range(5, 5 + n_distinct))
    present = rng.random(n_docs) >= null_fraction
    values = [int(pool[i]) for i in rng.integers(0, len(pool), size=int(present.sum()))]
    match = np.nonzero(rng.random(n_docs) < 0.5)[0]
    return match, values, present


@pytest.mark.parametrize("comparator", sorted(SM.COMPARATORS))
@pytest.mark.parametrize("k", KS)
def test_top_n_computer_yields_the_closed_form(comparator, k):
    order, nulls = SM.COMPARATORS[comparator]
    rng = np.random.default_rng(1000 * k + len(comparator))
    seen_long_tie = False
    for trial in range(40):
        n_docs = int(rng.integers(1, 6 * k + 40))
        null_fraction = [0.0, 0.3, 0.9, 1.0][trial % 4]
        match, values, present = _random_input(rng, n_docs, 2 + trial % 3, null_fraction, hi_bits=trial % 5 == 0)
        want = SM.expected_sorted(match, values, present, k, order, nulls)
        got = SM.top_n_reference(match, values, present, k, comparator)
        assert got == want, (comparator, k, trial)
        assert len(want) == min(k, match.size)
        # more than 2k docs share the k-th key: the threshold is strict, so the FIRST of them by doc id stay
        if len(want) == k:
            kth = want[-1][1]
            rows = np.cumsum(present) - 1
            same = sum(1 for d in match if (int(values[rows[d]]) if present[d] else None) == kth)
            seen_long_tie = seen_long_tie or same > 2 * k
    assert seen_long_tie, "no input had more than 2k docs on the k-th key"


def test_full_column_and_every_doc_on_one_key():
    """present=None (row = doc); every value equal: the row is the first k matches, whatever the comparator."""
    match = np.arange(3, 500, 3)
    values = [7] * 500
    for comparator, (order, nulls) in SM.COMPARATORS.items():
        for k in KS:
            want = SM.expected_sorted(match, values, None, k, order, nulls)
            assert [d for d, _ in want] == match[:k].tolist()
            assert SM.top_n_reference(match, values, None, k, comparator) == want


def test_the_four_comparators_are_two_choices():
    docs = [0, 1, 2, 3]
    values, present = [10, 20], [True, False, True, False]  # doc 0: 10, doc 2: 20, docs 1 and 3: no value
    order_of = lambda o, n: [d for d, _ in SM.expected_sorted(docs, values, present, 4, o, n)]  # noqa: E731
    assert order_of(SM.DESC, SM.NULLS_LAST) == [2, 0, 1, 3]    # Natural = Order::Desc
    assert order_of(SM.ASC, SM.NULLS_LAST) == [0, 2, 1, 3]     # ReverseNoneLower = Order::Asc
    assert order_of(SM.ASC, SM.NULLS_FIRST) == [1, 3, 0, 2]    # Reverse
    assert order_of(SM.DESC, SM.NULLS_FIRST) == [1, 3, 2, 0]   # NaturalNoneHigher
    for name, (o, n) in SM.COMPARATORS.items():
        assert [d for d, _ in SM.top_n_reference(docs, values, present, 4, name)] == order_of(o, n), name


# ---- the binding and the C ABI (these fail without the feature)
@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def test_merge_sorted_top_k_is_the_closed_form_over_the_segments(B):
    rng = np.random.default_rng(5)
    for trial in range(30):
        order, nulls = [(o, n) for o in (0, 1) for n in (0, 1)][trial % 4]
        n_seg, k, offset = int(rng.integers(1, 5)), int(rng.integers(1, 12)), int(rng.integers(0, 4))
        rows, flat = [], []
        for seg_ord in range(n_seg):
            n_docs = int(rng.integers(0, 40))
            match, values, present = _random_input(rng, n_docs, 3, [0.0, 0.5, 1.0][trial % 3], hi_bits=trial % 2 == 0)
            top = SM.expected_sorted(match, values, present, k + offset, order, nulls)  # what a segment returns
            stride = k + offset + 2
            docs = np.full(stride, 0x7FFFFFFF, np.uint32)
            vals = np.zeros(stride, np.uint64)
            has = np.zeros(stride, np.uint8)
            for i, (d, v) in enumerate(top):
                docs[i], vals[i], has[i] = d, (0 if v is None else v), (v is not None)
            rows.append((docs, vals, has, len(top)))
            rank_rows = np.cumsum(present) - 1
            flat += [(SM.rank_key(int(values[rank_rows[d]]) if present[d] else None, order, nulls), seg_ord, int(d),
                      int(values[rank_rows[d]]) if present[d] else None) for d in match]
        flat.sort(key=lambda e: e[:3])
        want = [(v, s, d) for _, s, d, v in flat[offset: offset + k]]
        assert B.merge_sorted_top_k(rows, k, order, nulls, offset) == want, trial


def _header():
    return open(os.path.join(ROOT, "include", "tantivy_amd.h")).read()


def test_header_declares_the_feature_and_the_binding_agrees(B):
    src = _header()
    enums = dict(re.findall(r"\b(TQ_SORT_DESC|TQ_SORT_ASC|TQ_NULLS_LAST|TQ_NULLS_FIRST)\s*=\s*(\d+)", src))
    assert enums == {"TQ_SORT_DESC": "0", "TQ_SORT_ASC": "1", "TQ_NULLS_LAST": "0", "TQ_NULLS_FIRST": "1"}
    assert re.search(r"enum\s+tq_sort_order\s*\{", src) and re.search(r"enum\s+tq_sort_nulls\s*\{", src)
    assert (B.SORT_DESC, B.SORT_ASC, B.NULLS_LAST, B.NULLS_FIRST) == (0, 1, 0, 1)
    assert (SM.DESC, SM.ASC, SM.NULLS_LAST, SM.NULLS_FIRST) == (B.SORT_DESC, B.SORT_ASC, B.NULLS_LAST, B.NULLS_FIRST)
    masks = {name: int(v, 16) for name, v in re.findall(r"#define\s+(TQ_KERNEL_[A-Z_]+)\s+(0x[0-9a-fA-F]+)u", src)}
    assert B.KERNEL_SORT == masks["TQ_KERNEL_SORT"]
    others = [v for n, v in masks.items() if n != "TQ_KERNEL_SORT"]
    assert bin(masks["TQ_KERNEL_SORT"]).count("1") == 1 and masks["TQ_KERNEL_SORT"] not in others
    assert B.kernel_names(B.KERNEL_SORT) == ["sort"]
    assert int(re.search(r"#define\s+TQ_MAX_K\s+(\d+)u", src).group(1)) == B.MAX_K
    assert '"sort_slices"' in src
    assert "algorithmic_bytes" in src[src.index("sort by fast field"): src.index("enum tq_sort_order")]


def test_library_exports_both_entry_points(B):
    L = B.lib()
    declared = set(re.findall(r"\b(tq_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for name in ("tq_search_sorted_batch", "tq_search_sorted_batch_device"):
        assert name in declared and name in B.EXPORTS and hasattr(L, name), name
    # null arguments are errors, not crashes; the message names the function
    assert L.tq_search_sorted_batch(None, None, 1, 0, 0, 0, 1, None, None, None, None) != 0
    assert b"tq_search_sorted_batch" in L.tq_last_error()
    assert L.tq_search_sorted_batch_device(None, None, 1, 0, 0, 0, 1, None, None, None, None, None) != 0
    assert b"tq_search_sorted_batch_device" in L.tq_last_error()
