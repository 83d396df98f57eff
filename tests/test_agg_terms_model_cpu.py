"""CPU checks of the terms aggregation (tq_agg_terms_batch*; tests/terms_model.py, tantivy_amd.binding): the closed form
that tests/test_gpu_agg_terms.py holds the device to agrees with the transliteration of the reference's segment collector on
everything the reference specifies; the tie rule; the host helpers against the reference's own expectations; the plan's
arithmetic at its edges; and the C ABI is declared, bound and exported.  No device compute here, and no tolerance: every
comparison is ==."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import terms_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def _columns():
    """name -> (u64 per doc, has per doc, match docs, info)"""
    rng = np.random.default_rng(20261101)
    md = 900
    out = {}

    def add(name, vals, has, match):
        u64 = np.zeros(md, np.uint64)
        u64[has] = vals
        out[name] = (u64, has, match, TM.column_info(vals))

    every = np.ones(md, bool)
    some = rng.random(md) < 0.5
    most = np.nonzero(rng.random(md) < 0.7)[0]
    add("random skewed", (rng.zipf(1.5, size=md) % 40).astype(np.uint64) * np.uint64(3) + np.uint64(17), every, most)
    add("all counts equal", np.arange(md, dtype=np.uint64) % np.uint64(30), every, np.arange(md))
    add("every key once", np.uint64(1 << 60) + np.arange(md, dtype=np.uint64)[::-1] * np.uint64(1000), every, most)
    add("optional", rng.integers(0, 25, size=int(some.sum())).astype(np.uint64), some, most)
    add("optional without a value", np.zeros(0, np.uint64), np.zeros(md, bool), most)
    add("empty match", rng.integers(0, 25, size=md).astype(np.uint64), every, np.zeros(0, np.int64))
    add("one key", np.full(md, 7, np.uint64), every, most)
    return out


COLUMNS = _columns()


@pytest.mark.parametrize("order", TM.ORDERS)
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_the_two_models_agree_on_what_the_reference_specifies(name, order):
    u64, has, match, info = COLUMNS[name]
    distinct = TM.closed_form(u64, has, match, info, order, 1)[0]["distinct"]
    assert (distinct == 0) == (name in ("optional without a value", "empty match"))
    rng = np.random.default_rng(3)
    for size in sorted({1, max(1, distinct - 1), max(1, distinct), distinct + 1}):
        rec, keys, counts = TM.closed_form(u64, has, match, info, order, size)
        ref = TM.reference_segment(u64, has, match, order, size, rng)
        where = (name, order, size)
        assert sorted(counts) == sorted(c for _, c in ref["entries"]), where
        assert rec["sum_other_doc_count"] == ref["sum_other_doc_count"], where
        assert rec["doc_count_error_upper_bound"] == ref["doc_count_error_upper_bound"], where
        assert rec["distinct"] == ref["distinct"] == distinct and rec["n_returned"] == len(keys) == len(counts) == min(size, distinct), where
        assert rec["count"] == sum(counts) + rec["sum_other_doc_count"] == int(has[match].sum()) and rec["matches"] == match.size
        assert (rec["sum_other_doc_count"] == 0) == (distinct <= size) and rec["out_of_range"] == 0
        if order in (TM.KEY_ASC, TM.KEY_DESC):  # nothing ties: the kept entries are determined
            assert sorted(zip(keys, counts)) == sorted(ref["entries"]), where
        per_key = dict(zip(keys, counts))
        assert all(int((u64[match][has[match]] == np.uint64(k)).sum()) == c for k, c in per_key.items())
    if name == "all counts equal":
        assert len(set(TM.closed_form(u64, has, match, info, order, 30)[2])) == 1


def test_the_tie_rule_is_ascending_key():
    # values 5 5 9 9 2 2 7: counts {2: 2, 5: 2, 7: 1, 9: 2}
    u64 = np.array([5, 5, 9, 9, 2, 2, 7], np.uint64)
    has = np.ones(7, bool)
    info = TM.column_info(u64)
    assert info == {"min_value": 2, "max_value": 9, "gcd": 1, "num_rows": 7}

    def rows(order, size):
        rec, keys, counts = TM.closed_form(u64, has, np.arange(7), info, order, size)
        return list(zip(keys, counts)), rec["sum_other_doc_count"], rec["doc_count_error_upper_bound"]

    assert rows(TM.COUNT_DESC, 2) == ([(2, 2), (5, 2)], 3, 2)  # of three keys holding two docs the two smallest survive
    assert rows(TM.COUNT_DESC, 3) == ([(2, 2), (5, 2), (9, 2)], 1, 1)
    assert rows(TM.COUNT_ASC, 2) == ([(7, 1), (2, 2)], 4, 2)
    assert rows(TM.COUNT_ASC, 4) == ([(7, 1), (2, 2), (5, 2), (9, 2)], 0, 0)
    assert rows(TM.KEY_ASC, 3) == ([(2, 2), (5, 2), (7, 1)], 2, 2)
    assert rows(TM.KEY_DESC, 1) == ([(9, 2)], 5, 1)
    # the transliteration agrees on the counts, the sum and the bound whatever survives there
    ref = TM.reference_segment(u64, has, np.arange(7), TM.COUNT_DESC, 2)
    assert sorted(c for _, c in ref["entries"]) == [2, 2] and (ref["sum_other_doc_count"], ref["doc_count_error_upper_bound"]) == (3, 2)


def test_merge_and_finalize_against_the_references_expectations(B):
    # intermediate_agg_result.rs, test_prune_intermediate_results_*: a 10, b 5, c 20, d 1, e 15 (keys 0..4 here)
    u64 = np.repeat(np.arange(5, dtype=np.uint64), [10, 5, 20, 1, 15])
    has = np.ones(u64.size, bool)
    info = TM.column_info(u64)
    whole = B.merge_terms([{"entries": {0: 10, 1: 5, 2: 20, 3: 1, 4: 15}, "sum_other_doc_count": 0, "doc_count_error_upper_bound": 0}])
    # the final cut at size 2 keeps c and e, adds 10 + 5 + 1 to sum_other and nothing to the error bound
    final = B.terms_finalize(whole, size=2)
    assert final == {"buckets": [(2, 20), (4, 15)], "sum_other_doc_count": 16, "doc_count_error_upper_bound": 0}
    # the segment cut at segment_size 4 drops d: sum_other 1, error bound 1
    rec, keys, counts = TM.closed_form(u64, has, np.arange(u64.size), info, TM.COUNT_DESC, 4)
    assert list(zip(keys, counts)) == [(2, 20), (4, 15), (0, 10), (1, 5)]
    assert (rec["sum_other_doc_count"], rec["doc_count_error_upper_bound"]) == (1, 1)
    row = np.zeros(1, B.AGG_TERMS_DTYPE)
    for k, v in rec.items():
        row[0][k] = v
    row = row[0]
    # merge_fruits: counts add per key, sum_other and the bounds add; a segment contributes its first n_returned entries
    other = (np.array([4, 9, 77], np.uint64), np.array([3, 2, 99], np.uint32), {"n_returned": 2, "sum_other_doc_count": 5, "doc_count_error_upper_bound": 2})
    merged = B.merge_terms([(np.array(keys, np.uint64), np.array(counts, np.uint32), row), other])
    assert merged == {"entries": {2: 20, 4: 18, 0: 10, 1: 5, 9: 2}, "sum_other_doc_count": 6, "doc_count_error_upper_bound": 3}
    assert B.merge_terms([merged, B.merge_terms([])]) == merged
    assert B.terms_finalize(merged, size=2) == {"buckets": [(2, 20), (4, 18)], "sum_other_doc_count": 6 + 17, "doc_count_error_upper_bound": 3}
    assert B.terms_finalize(merged, size=10, min_doc_count=6, order=B.TERMS_KEY_DESC)["buckets"] == [(4, 18), (2, 20), (0, 10)]
    assert B.terms_finalize(merged, size=3, order=B.TERMS_COUNT_ASC) == \
        {"buckets": [(9, 2), (1, 5), (0, 10)], "sum_other_doc_count": 6 + 38, "doc_count_error_upper_bound": 3}
    assert [k for k, _ in B.terms_finalize(merged, size=10, order=B.TERMS_KEY_ASC)["buckets"]] == [0, 1, 2, 4, 9]
    tie = {"entries": {8: 3, 1: 3, 5: 3}, "sum_other_doc_count": 0, "doc_count_error_upper_bound": 0}
    assert B.terms_finalize(tie, size=2)["buckets"] == [(1, 3), (5, 3)]


def _info(lo, hi, gcd, rows=10):
    return {"min_value": lo, "max_value": hi, "gcd": gcd, "num_rows": rows}


def test_the_plan(B):
    cases = [_info(17, 17 + 1000 * 41, 1000), _info(5, 5, 1), _info(0, 0, 1, 0), _info(1 << 63, (1 << 63) + 65535, 1),
             _info(0, 65535 * 8, 8), _info(M64 - 1000, M64, 1), _info(M64 - 65535 * 3, M64, 3)]
    for info in cases:
        want = TM.terms_plan(info)
        assert B.agg_terms_plan(info) == want, info
    assert B.agg_terms_plan(cases[0])["n_keys"] == 42      # gcd > 1
    assert B.agg_terms_plan(cases[1])["n_keys"] == 1       # min = max
    assert B.agg_terms_plan(cases[2])["n_keys"] == 0       # an empty column
    assert B.agg_terms_plan(cases[3])["n_keys"] == 65536   # the most keys served
    assert B.agg_terms_plan(cases[5]) == {"n_keys": 1001, "min_value": M64 - 1000, "gcd": 1}  # max = u64::MAX
    for info, count in ((_info(0, 65536, 1), "65537"), (_info(9, 9 + 65536 * 1000, 1000), "65537"), (_info(0, M64, 1), "18446744073709551616")):
        with pytest.raises(TM.Refused) as mi:
            TM.terms_plan(info)
        with pytest.raises(B.TantivyAmdError) as ei:
            B.agg_terms_plan(info)
        assert mi.value.kind == "unsupported" and ei.value.code == 4, info
        assert "n_keys" in str(ei.value) and count in str(ei.value) and "tq_agg_terms_plan" in str(ei.value), ei.value
    assert B.agg_terms_max_size() == B.AGG_TERMS_MAX_SIZE == TM.MAX_SIZE == 1024
    B.agg_terms_plan(cases[0], segment_size=1024)
    for bad in ({"segment_size": 0}, {"segment_size": 1025}, {"order": 4}):
        with pytest.raises(TM.Refused):
            TM.terms_plan(cases[0], **bad)
        with pytest.raises(B.TantivyAmdError) as ei:
            B.agg_terms_plan(cases[0], **bad)
        assert ei.value.code == 1 and list(bad)[0] in str(ei.value), ei.value
    # an empty column is planned before its key range is looked at; the request is still checked
    with pytest.raises(B.TantivyAmdError):
        B.agg_terms_plan(cases[2], segment_size=0)


def _header():
    return open(os.path.join(ROOT, "include", "tantivy_amd.h")).read()


def test_header_declares_the_feature_and_the_binding_agrees(B):
    from tantivy_amd import build

    src = _header()
    masks = {name: int(v, 16) for name, v in re.findall(r"#define\s+(TQ_KERNEL_[A-Z_]+)\s+(0x[0-9a-fA-F]+)u", src)}
    assert B.KERNEL_AGG_TERMS == masks["TQ_KERNEL_AGG_TERMS"] == 0x400000
    assert masks["TQ_KERNEL_AGG_TERMS"] not in [v for n, v in masks.items() if n != "TQ_KERNEL_AGG_TERMS"]
    assert B.kernel_names(B.KERNEL_AGG_TERMS) == ["agg_terms"] and B.kernel_names(B.KERNEL_AGG_SUB) == ["agg_sub"]
    assert sorted(B.KERNEL_NAMES) == sorted(masks.values())
    # the record: 40 bytes, the same fields in the same order and widths
    assert B.AGG_TERMS_DTYPE.itemsize == 40 and re.search(r"\}\s*tq_agg_terms_t\s*;\s*/\* 40 bytes \*/", src)
    fields = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct tq_agg_terms_t \{(.*?)\}", src, re.S).group(1), flags=re.S)
    declared = [(n.strip(), t) for t, names in re.findall(r"\b(uint64_t|uint32_t)\s+([a-z_, ]+);", fields) for n in names.split(",")]
    width = {"uint64_t": np.uint64, "uint32_t": np.uint32}
    assert [(n, np.dtype(width[t])) for n, t in declared] == [(n, B.AGG_TERMS_DTYPE[n]) for n in B.AGG_TERMS_DTYPE.names]
    assert list(B.AGG_TERMS_DTYPE.names) == list(TM.FIELDS)
    assert C.sizeof(B.TqAggTermsRequest) == 12 and C.sizeof(B.TqAggTermsPlan) == 24
    orders = dict(re.findall(r"(TQ_TERMS_[A-Z_]+) = (\d)", src))
    assert {k: int(v) for k, v in orders.items()} == {"TQ_TERMS_COUNT_DESC": B.TERMS_COUNT_DESC, "TQ_TERMS_COUNT_ASC": B.TERMS_COUNT_ASC,
                                                      "TQ_TERMS_KEY_ASC": B.TERMS_KEY_ASC, "TQ_TERMS_KEY_DESC": B.TERMS_KEY_DESC}
    assert (B.TERMS_COUNT_DESC, B.TERMS_COUNT_ASC, B.TERMS_KEY_ASC, B.TERMS_KEY_DESC) == TM.ORDERS
    assert re.search(r"#define TQ_AGG_TERMS_MAX_SIZE 1024u", src)
    # the kernels are registered with their translation unit, and the unit is built
    for k in ("agg_terms_count_kernel", "agg_terms_select_kernel", "agg_terms_init_kernel"):
        assert build.KERNEL_FILES[k] == "tq_agg_terms.hip", k
    names = [os.path.basename(p) for p in build.SOURCES]
    assert "tq_agg_terms.hip" in names and "tq_agg_terms.cpp" in names
    assert all(os.path.exists(p) for p in build.SOURCES)


def test_library_exports_the_entry_points(B):
    L = B.lib()
    declared = set(re.findall(r"\b(tq_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for name in ("tq_agg_terms_plan", "tq_agg_terms_batch", "tq_agg_terms_batch_device", "tq_agg_terms_lds_capacities",
                 "tq_agg_terms_max_size"):
        assert name in declared and name in B.EXPORTS and hasattr(L, name), name
    # null arguments are errors, not crashes; the message names the function
    assert L.tq_agg_terms_batch(None, None, 1, None, None, None, None, 0) != 0 and b"tq_agg_terms_batch:" in L.tq_last_error()
    assert L.tq_agg_terms_batch_device(None, None, 1, None, None, None, None, 0, None) != 0
    assert b"tq_agg_terms_batch_device:" in L.tq_last_error()
    assert L.tq_agg_terms_plan(None, None, None) != 0 and b"tq_agg_terms_plan:" in L.tq_last_error()
    small, large = B.agg_terms_lds_capacities()
    assert 16 < small < large and 4 * large + 16640 <= 65536  # (the table beside the slabs in the static 64 KB)
