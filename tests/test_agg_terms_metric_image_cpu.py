"""CPU checks of the order value of a terms entry under a metric order: tq_agg_terms_metric_image through ctypes — the
__host__ __device__ code of tantivy_amd/csrc/tq_agg_metric_image.hpp that agg_terms_sub_select_kernel runs — against Python
ints and fractions (tests/terms_sub_model.image: the AVG quotient is Python's int / int, correctly rounded, half to even);
and the C ABI of tq_agg_terms_sub_batch* is declared, bound and exported, with the refusals of its host-only parts.  No
device, no tolerance: every comparison is ==."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import agg_model as GM
from tests import terms_sub_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def _rec(count, total, lo=0, hi=0):
    """a record with the u64-space sum `total`"""
    assert 0 <= total < 1 << 96
    return {"count": count, "min_value": lo, "max_value": hi, "sum_lo": total & M64, "sum_hi": total >> 64}


def _rec_typed(count, typed, vt):
    """a record whose exact TYPED sum is `typed`"""
    return _rec(count, typed + (count << 63 if vt == GM.I64 else 0))


def _check(B, rec, vt, where=None):
    for metric in SM.METRICS:
        if vt == GM.F64 and metric in (SM.SUM, SM.AVG):
            continue
        assert B.agg_terms_metric_image(rec, vt, metric) == SM.image(rec, vt, metric), (where, rec, vt, metric)


def test_counts_and_sums_at_the_edges(B):
    for count in (1, 3, (1 << 31) - 1):
        for total in ((1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 64) - 1, 1 << 64, (1 << 64) + 1, (1 << 94) - 12345, (1 << 94) + 7, 1, 0):
            if total >= count << 64:  # (a sum of `count` u64 values)
                continue
            _check(B, _rec(count, total, 5, 9), GM.U64, "u64")
        for typed in (-(1 << 53) - 1, -(1 << 53), -(1 << 53) + 1, -1, 0, 1, (1 << 53) - 1, (1 << 53) + 1, -(1 << 64) - 1, (1 << 64) + 1,
                      (1 << 93) + 99, -(1 << 93) - 99):
            if abs(typed) > count << 63:  # (a sum of `count` i64 values)
                continue
            _check(B, _rec_typed(count, typed, GM.I64), GM.I64, "i64")


def test_avg_halfway_cases_round_to_even(B):
    """Quotients exactly between two f64, and one unit of the numerator either side: sum = (2 m + 1) * 2^e * count / 2 with
    m of 53 bits is the midpoint of m * 2^e and (m + 1) * 2^e."""
    seen = set()
    for count in (1, 3, 6, (1 << 31) - 1):
        for m in ((1 << 52), (1 << 52) + 1, (1 << 53) - 1, (1 << 53) - 2, (1 << 52) + 12345):
            for e in (1, 2, 11):  # the f64 spacing is 2^e: the midpoint (2 m + 1) * 2^(e - 1) is an integer
                mid = (2 * m + 1) << (e - 1)
                total = mid * count
                if total >= min(1 << 95, count << 64):
                    continue
                for delta, want in ((0, "even"), (-1, "down"), (1, "up")):
                    rec = _rec(count, total + delta)
                    got = B.agg_terms_metric_image(rec, GM.U64, SM.AVG)
                    lo, hi = SM.f64_image(float(m << e)), SM.f64_image(float((m + 1) << e))
                    assert float(m << e) == m << e and hi > lo
                    expect = {"even": lo if m % 2 == 0 else hi, "down": lo, "up": hi}[want]
                    assert got == expect == SM.image(rec, GM.U64, SM.AVG), (count, m, e, delta)
                    seen.add(want)
                    # the same magnitudes, negative, through I64 (where `count` i64 values can sum to it)
                    if total + delta > count << 63:
                        continue
                    seen.add("negative")
                    rec = _rec_typed(count, -(total + delta), GM.I64)
                    assert B.agg_terms_metric_image(rec, GM.I64, SM.AVG) == SM.image(rec, GM.I64, SM.AVG) == SM.f64_image(
                        -float((m << e) if expect == lo else ((m + 1) << e))), (count, m, e, delta)
    assert seen == {"even", "down", "up", "negative"}
    # a fraction below 1 and a quotient that needs every bit: 1 / 3, 2 / 3, (2^53 + 1) / 3
    for total, count in ((1, 3), (2, 3), ((1 << 53) + 1, 3), (1, (1 << 31) - 1), ((1 << 94) + 1, (1 << 31) - 1)):
        rec = _rec(count, total)
        assert B.agg_terms_metric_image(rec, GM.U64, SM.AVG) == SM.f64_image(total / count)


def test_an_empty_record_is_typed_zero(B):
    empty = SM.empty_record()
    for vt in (GM.U64, GM.I64, GM.F64):
        zero = GM.to_u64(0.0 if vt == GM.F64 else 0, vt)
        assert B.agg_terms_metric_image(empty, vt, SM.VALUE_COUNT) == 0
        assert B.agg_terms_metric_image(empty, vt, SM.MIN) == B.agg_terms_metric_image(empty, vt, SM.MAX) == zero
        if vt != GM.F64:
            assert B.agg_terms_metric_image(empty, vt, SM.AVG) == SM.f64_image(0.0) == 1 << 63
            assert B.agg_terms_metric_image(empty, vt, SM.SUM) == ((1 << 95) if vt == GM.I64 else 0)
        _check(B, empty, vt, "empty")
    # inside an I64 range: below a positive value's image, above a negative one's
    pos, neg = _rec_typed(2, 5, GM.I64), _rec_typed(2, -5, GM.I64)
    for metric in (SM.SUM, SM.AVG):
        assert B.agg_terms_metric_image(neg, GM.I64, metric) < B.agg_terms_metric_image(empty, GM.I64, metric) < B.agg_terms_metric_image(pos, GM.I64, metric)


def test_f64_min_max(B):
    vals = [0.0, -0.0, float("inf"), float("-inf"), -1.5, 1.5, -1e300, 1e-300, 5e-324, -5e-324]
    images = {}
    for x in vals:
        u = GM.to_u64(x, GM.F64)
        rec = _rec(1, 0, u, u)
        for metric in (SM.MIN, SM.MAX):
            assert B.agg_terms_metric_image(rec, GM.F64, metric) == u == SM.image(rec, GM.F64, metric)
        images[repr(x)] = u
    order = sorted(vals, key=lambda x: images[repr(x)])
    assert order[0] == float("-inf") and order[-1] == float("inf")
    assert all(a <= b for a, b in zip(order, order[1:]))  # (monotone; -0.0 sorts below +0.0 as an image, equal as an f64)
    assert images["-0.0"] < images["0.0"]


def test_random_records_and_monotonicity(B):
    rng = np.random.default_rng(20261202)
    recs = {GM.U64: [], GM.I64: []}
    for _ in range(3000):
        vt = GM.U64 if rng.random() < 0.5 else GM.I64
        count = int(rng.integers(1, 1 << 31)) if rng.random() < 0.5 else int(rng.integers(1, 50))
        bits = int(rng.integers(1, 65))
        vals_hi = (1 << bits) - 1
        total = int(rng.integers(0, 1 << 62)) * count >> int(rng.integers(0, 62)) if bits > 40 else int(rng.integers(0, vals_hi + 1)) * count
        total = min(total, count * M64)
        lo, hi = sorted(int(x) for x in rng.integers(0, 1 << 63, size=2))
        rec = _rec(count, total, lo, hi)
        _check(B, rec, vt, "random")
        recs[vt].append(rec)
    # close pairs: the same count, sums a few units apart — quotients that f64 may or may not separate
    for _ in range(500):
        count = int(rng.integers(1, 1000))
        total = int(rng.integers(1 << 52, 1 << 60))
        for d in (1, 2, count, count + 1):
            recs[GM.U64] += [_rec(count, total), _rec(count, total + d)]
    checked = 0
    for vt, rs in recs.items():
        idx = rng.integers(0, len(rs), size=(4000, 2))
        for metric in SM.METRICS:
            for i, j in idx.tolist():
                a, b = rs[i], rs[j]
                ra, rb = SM.metric_rational(a, vt, metric), SM.metric_rational(b, vt, metric)
                if metric == SM.AVG:
                    differ = float(ra) != float(rb)  # (Fraction -> float is correctly rounded)
                else:
                    differ = True  # (the image is the exact integer)
                if ra < rb and differ:
                    assert B.agg_terms_metric_image(a, vt, metric) < B.agg_terms_metric_image(b, vt, metric), (a, b, vt, metric)
                    checked += 1
                elif ra == rb:
                    assert B.agg_terms_metric_image(a, vt, metric) == B.agg_terms_metric_image(b, vt, metric), (a, b, vt, metric)
    assert checked > 10000  # (40 000 pairs, about half of them a < b: at least half of those were held to the order)
    assert float(Fraction((1 << 53) + 1, 3)) == ((1 << 53) + 1) / 3


def _header():
    return open(os.path.join(ROOT, "include", "tantivy_amd.h")).read()


def test_header_declares_the_feature_and_the_binding_agrees(B):
    from tantivy_amd import build

    src = _header()
    masks = {name: int(v, 16) for name, v in re.findall(r"#define\s+(TQ_KERNEL_[A-Z_]+)\s+(0x[0-9a-fA-F]+)u", src)}
    assert B.KERNEL_AGG_TERMS_SUB == masks["TQ_KERNEL_AGG_TERMS_SUB"] == 0x800000
    assert masks["TQ_KERNEL_AGG_TERMS_SUB"] not in [v for n, v in masks.items() if n != "TQ_KERNEL_AGG_TERMS_SUB"]
    assert B.kernel_names(B.KERNEL_AGG_TERMS_SUB) == ["agg_terms_sub"]
    assert C.sizeof(B.TqAggTermsSubRequest) == 20 and re.search(r"\}\s*tq_agg_terms_sub_request\s*;\s*/\* 20 bytes \*/", src)
    assert B.TqAggTermsSubRequest.metric_value_type.offset == 16 and B.TqAggTermsSubRequest.order_metric.offset == 17
    assert B.TqAggTermsSubRequest.reserved.offset == 18
    assert B.AGG_BUCKET_STATS_DTYPE.itemsize == 40 and tuple(B.AGG_BUCKET_STATS_DTYPE.names) == SM.RECORD_FIELDS
    metrics = {k: int(v) for k, v in re.findall(r"(TQ_METRIC_[A-Z_]+) = (\d)", src)}
    assert metrics == {"TQ_METRIC_VALUE_COUNT": B.METRIC_VALUE_COUNT, "TQ_METRIC_MIN": B.METRIC_MIN, "TQ_METRIC_MAX": B.METRIC_MAX,
                       "TQ_METRIC_SUM": B.METRIC_SUM, "TQ_METRIC_AVG": B.METRIC_AVG}
    assert (B.METRIC_VALUE_COUNT, B.METRIC_MIN, B.METRIC_MAX, B.METRIC_SUM, B.METRIC_AVG) == SM.METRICS
    orders = {k: int(v) for k, v in re.findall(r"#define (TQ_TERMS_METRIC_[A-Z]+) (\d)u", src)}
    assert orders == {"TQ_TERMS_METRIC_DESC": B.TERMS_METRIC_DESC, "TQ_TERMS_METRIC_ASC": B.TERMS_METRIC_ASC}
    assert (B.TERMS_COUNT_DESC, B.TERMS_COUNT_ASC, B.TERMS_KEY_ASC, B.TERMS_KEY_DESC, B.TERMS_METRIC_DESC, B.TERMS_METRIC_ASC) == SM.ORDERS
    for k in ("agg_terms_sub_count_kernel", "agg_terms_sub_select_kernel", "agg_terms_sub_init_kernel"):
        assert build.KERNEL_FILES[k] == "tq_agg_terms_sub.hip", k
    names = [os.path.basename(p) for p in build.SOURCES]
    assert "tq_agg_terms_sub.hip" in names and "tq_agg_terms_sub.cpp" in names
    assert "tq_agg_metric_image.hpp" in [os.path.basename(p) for p in build.HEADERS]
    assert all(os.path.exists(p) for p in build.SOURCES + build.HEADERS)


def test_library_exports_the_entry_points_and_refuses_on_the_host(B):
    L = B.lib()
    declared = set(re.findall(r"\b(tq_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for name in ("tq_agg_terms_sub_batch", "tq_agg_terms_sub_batch_device", "tq_agg_terms_sub_lds_capacities", "tq_agg_terms_metric_image"):
        assert name in declared and name in B.EXPORTS and hasattr(L, name), name
    # null arguments are errors, not crashes; the message names the function
    assert L.tq_agg_terms_sub_batch(None, None, 1, None, None, None, None, None, 0) != 0
    assert b"tq_agg_terms_sub_batch:" in L.tq_last_error()
    assert L.tq_agg_terms_sub_batch_device(None, None, 1, None, None, None, None, None, 0, None) != 0
    assert b"tq_agg_terms_sub_batch_device:" in L.tq_last_error()
    out = (C.c_uint64 * 2)()
    assert L.tq_agg_terms_metric_image(None, 0, 0, out) == 1 and b"tq_agg_terms_metric_image:" in L.tq_last_error()
    small, large = B.agg_terms_sub_lds_capacities()
    assert 16 < small < large and 40 * large + 16384 + 160 <= 65536  # (the table beside the slabs in the static 64 KB)
    # the plan of the terms part still refuses the metric orders
    info = {"min_value": 0, "max_value": 9, "gcd": 1, "num_rows": 10}
    for order in (B.TERMS_METRIC_DESC, B.TERMS_METRIC_ASC):
        with pytest.raises(B.TantivyAmdError) as ei:
            B.agg_terms_plan(info, order=order)
        assert ei.value.code == 1 and "tq_agg_terms_plan" in str(ei.value)
    rec = SM.empty_record()
    for vt, metric, code in ((3, 0, 1), (0, 5, 1), (GM.F64, SM.SUM, 4), (GM.F64, SM.AVG, 4)):
        with pytest.raises(B.TantivyAmdError) as ei:
            B.agg_terms_metric_image(rec, vt, metric)
        assert ei.value.code == code and "tq_agg_terms_metric_image" in str(ei.value), (vt, metric, ei.value)
    for bad in (dict(rec, count=1 << 32), dict(rec, sum_hi=1 << 32)):
        with pytest.raises(B.TantivyAmdError) as ei:
            B.agg_terms_metric_image(bad, GM.U64, SM.AVG)
        assert ei.value.code == 1


def test_merge_and_finalize_on_the_host(B):
    """merge_terms_sub adds counts and records per key; terms_sub_finalize orders by the merged metric, an entry without a
    metric value as f64::MIN at this stage — last under DESC, first under ASC — where the segment stage used 0."""
    I = GM.I64

    def r(vals):
        return SM.record_of([GM.to_u64(v, I) for v in vals], I)

    seg1 = ([10, 20, 30], [3, 2, 1], [r([5, 7]), r([-4]), SM.empty_record()], {"n_returned": 3, "sum_other_doc_count": 4, "doc_count_error_upper_bound": 1})
    seg2 = ([20, 40, 99], [1, 5, 9], [r([-6, 1]), r([100]), r([1])], {"n_returned": 2, "sum_other_doc_count": 0, "doc_count_error_upper_bound": 2})
    merged = B.merge_terms_sub([seg1, seg2])
    assert merged["sum_other_doc_count"] == 4 and merged["doc_count_error_upper_bound"] == 3
    assert {k: c for k, (c, _) in merged["entries"].items()} == {10: 3, 20: 3, 30: 1, 40: 5}  # (99 is past n_returned)
    assert merged["entries"][20][1] == dict(r([-4, -6, 1]), sum=sum(GM.to_u64(v, I) for v in (-4, -6, 1)))
    assert B.merge_terms_sub([merged]) == merged and B.merge_terms_sub([B.merge_terms_sub([seg1]), seg2]) == merged
    fin = B.terms_sub_finalize(merged, I, size=3, order=B.TERMS_METRIC_DESC, order_metric=B.METRIC_AVG)
    assert [(k, c) for k, c, _ in fin["buckets"]] == [(40, 5), (10, 3), (20, 3)] and fin["sum_other_doc_count"] == 4 + 1
    assert fin["buckets"][2][2]["avg"] == -3.0 and fin["buckets"][1][2] == {"count": 2, "sum": 12, "min": 5, "max": 7, "avg": 6.0}
    asc = B.terms_sub_finalize(merged, I, size=10, order=B.TERMS_METRIC_ASC, order_metric=B.METRIC_AVG)
    assert [k for k, _, _ in asc["buckets"]] == [30, 20, 10, 40]  # (no value: f64::MIN, below -3.0; at the segment stage it is 0)
    assert asc["buckets"][0][2]["avg"] is None
    desc = B.terms_sub_finalize(merged, I, size=10, order=B.TERMS_METRIC_DESC, order_metric=B.METRIC_MIN)
    assert [k for k, _, _ in desc["buckets"]] == [40, 10, 20, 30]
    by_count = B.terms_sub_finalize(merged, I, size=10, order=B.TERMS_METRIC_DESC, order_metric=B.METRIC_VALUE_COUNT)
    assert [k for k, _, _ in by_count["buckets"]] == [20, 10, 40, 30]
    old = B.terms_sub_finalize(merged, I, size=2, order=B.TERMS_COUNT_DESC)
    assert [(k, c) for k, c, _ in old["buckets"]] == B.terms_finalize({"entries": {k: c for k, (c, _) in merged["entries"].items()},
                                                                        "sum_other_doc_count": 4, "doc_count_error_upper_bound": 3},
                                                                       size=2)["buckets"]
