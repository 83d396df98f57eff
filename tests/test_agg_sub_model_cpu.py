"""CPU checks of the sub-aggregations (tq_agg_sub_batch*; tests/agg_sub_model.py, tantivy_amd.binding): the closed form
that tests/test_gpu_agg_sub.py holds the device to IS the reference's nested path — per bucket an IntermediateStats fed in
doc order — wherever every partial sum is below 2^53; the bucketing rules and the invariants between the record, the row
and the bucket records; the host helpers; and the C ABI is declared, bound and exported.  No device compute here, and no
tolerance: every comparison is ==."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import agg_model as GM
from tests import agg_sub_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def _as_row(B, rec):
    row = np.zeros(1, B.AGG_BUCKET_STATS_DTYPE)
    for k, v in rec.items():
        row[0][k] = v
    return row[0]


def _case(rng, vt_b, md=600):
    """An Optional bucket column A of small U64 values, an Optional metric column B of typed values below 2^40 in
    magnitude, a match set of ~70 % of the docs, and a plan of 7-wide buckets with hard bounds that cut both ends."""
    has_a, has_b = rng.random(md) < 0.8, rng.random(md) < 0.6
    col_a = GM.Column(rng.integers(0, 200, size=int(has_a.sum())).astype(np.uint64), has_a, md)
    lo = 0 if vt_b == GM.U64 else -(1 << 40)
    typed = [int(x) for x in rng.integers(lo, 1 << 40, size=int(has_b.sum()))]
    if vt_b == GM.I64:
        typed[0] = -abs(typed[0]) - 1  # (some value is negative)
    col_b = GM.Column(np.array([GM.to_u64(x, vt_b) for x in typed], np.uint64), has_b, md)
    plan = GM.histogram_plan(col_a.info, GM.U64, 7.0, 0.5, (20.0, 150.0))
    match = np.nonzero(rng.random(md) < 0.7)[0]
    return col_a, col_b, plan, match


@pytest.mark.parametrize("vt_b", [GM.U64, GM.I64])
def test_closed_form_is_the_nested_path_below_2_53(B, vt_b):
    rng = np.random.default_rng(40 + vt_b)
    for trial in range(10):
        col_a, col_b, plan, match = _case(rng, vt_b)
        rec, counts, records = SM.expected_sub(match, col_a, GM.U64, plan, col_b, vt_b)
        ref_counts, ref_stats, largest = SM.reference_sub(match, col_a, GM.U64, plan, col_b, vt_b)
        assert largest < 2.0 ** 53  # 600 docs x 2^40 < 2^50: every partial sum of every bucket is exact in f64
        assert ref_counts == counts and sum(counts) == rec["in_bounds"] and len(records) == plan["n_buckets"] > 10
        for i, (r, st) in enumerate(zip(records, ref_stats)):
            got, ref = GM.finalize(r, vt_b), st.finalize()
            assert B.agg_stats_finalize(_as_row(B, r), vt_b) == got
            assert got["count"] == ref["count"] <= counts[i]
            if ref["count"] == 0:
                assert (r["min_value"], r["max_value"], r["sum_lo"], r["sum_hi"]) == (GM.MASK, 0, 0, 0) and got["min"] is None
                continue
            assert float(got["sum"]) == ref["sum"] and float(got["min"]) == ref["min"] and float(got["max"]) == ref["max"]
            assert got["avg"] == ref["avg"]


def test_bucketing_rules():
    md = 12
    has_a = np.array([1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1], bool)
    a_vals = np.array([5, 15, 16, 25, 26, 99, 10, 19, 20, 29], np.uint64)  # docs 0 1 2 4 5 6 7 8 10 11
    has_b = np.array([1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1], bool)
    b_vals = np.arange(100, 100 + int(has_b.sum()), dtype=np.uint64)
    col_a, col_b = GM.Column(a_vals, has_a, md), GM.Column(b_vals, has_b, md)
    plan = GM.histogram_plan(col_a.info, GM.U64, 10.0, 0.0, (10.0, 29.0))
    assert (plan["base_pos"], plan["n_buckets"]) == (1, 2)
    rec, counts, records = SM.expected_sub(np.arange(md), col_a, GM.U64, plan, col_b, GM.U64)
    # docs 3 and 9 have no A value, docs 0 (5) and 6 (99) are outside the hard bounds: they reach no bucket
    assert rec["matches"] == 12 and rec["count"] == 10 and rec["in_bounds"] == 8 and counts == [4, 4]
    # bucket [10, 20): docs 1 2 7 8, of which 2 7 8 have a B value; bucket [20, 30): docs 4 5 10 11, of which 4 5 11
    b_of = lambda d: int(col_b.u64[d])  # noqa: E731
    assert records[0] == {"count": 3, "min_value": b_of(2), "max_value": b_of(8), "sum_lo": b_of(2) + b_of(7) + b_of(8), "sum_hi": 0}
    assert records[1] == {"count": 3, "min_value": b_of(4), "max_value": b_of(11), "sum_lo": b_of(4) + b_of(5) + b_of(11), "sum_hi": 0}
    ref_counts, ref_stats, _ = SM.reference_sub(np.arange(md), col_a, GM.U64, plan, col_b, GM.U64)
    assert ref_counts == counts and [s.count for s in ref_stats] == [3, 3]
    # a match set that skips a bucket leaves its record empty
    _, counts, records = SM.expected_sub([4, 5], col_a, GM.U64, plan, col_b, GM.U64)
    assert counts == [0, 2] and records[0] == SM.empty_record() and records[1]["count"] == 2


@pytest.mark.parametrize("full_b", [True, False])
def test_invariants_between_record_row_and_bucket_records(full_b):
    rng = np.random.default_rng(7)
    md = 3000
    has_a = rng.random(md) < 0.9
    col_a = GM.Column(rng.integers(0, 5000, size=int(has_a.sum())).astype(np.uint64), has_a, md)
    has_b = np.ones(md, bool) if full_b else rng.random(md) < 0.5
    b_vals = rng.integers(0, 1 << 63, size=int(has_b.sum())).astype(np.uint64) * np.uint64(2) + np.uint64(1)  # (64 bits wide)
    col_b = GM.Column(b_vals, None if full_b else has_b, md)
    plan = GM.histogram_plan(col_a.info, GM.U64, 100.0, 0.0, (500.0, 4000.0))
    match = np.nonzero(rng.random(md) < 0.8)[0]
    rec, counts, records = SM.expected_sub(match, col_a, GM.U64, plan, col_b, GM.U64)
    assert 0 < rec["in_bounds"] < rec["count"] < rec["matches"]
    valued = sum(r["count"] for r in records)
    assert valued <= rec["in_bounds"] and (valued == rec["in_bounds"]) == full_b
    assert all(r["count"] <= c for r, c in zip(records, counts))
    docs, _ = SM.bucket_of_docs(match, col_a, GM.U64, plan)
    total = sum(int(col_b.u64[d]) for d in docs if col_b.has[d])
    assert sum(r["sum_lo"] + (r["sum_hi"] << 64) for r in records) == total and total >> 64 > 0
    assert min(r["min_value"] for r in records) == min(int(col_b.u64[d]) for d in docs if col_b.has[d])


def test_merge_bucket_stats_over_three_segments(B):
    rng = np.random.default_rng(13)
    parts, want = [], {}
    for lo, hi in ((100, 300), (0, 120), (1000, 1100)):
        n = 200
        col_a = GM.Column(rng.integers(lo, hi, size=n).astype(np.uint64), None, n)
        b_vals = rng.integers(0, 1 << 62, size=n).astype(np.uint64) * np.uint64(4)  # (three segments' sums pass 2^64)
        col_b = GM.Column(b_vals, None, n)
        plan = GM.histogram_plan(col_a.info, GM.U64, 7.0, 0.5)
        match = np.nonzero(rng.random(n) < 0.8)[0]
        _, counts, records = SM.expected_sub(match, col_a, GM.U64, plan, col_b, GM.U64)
        rows = np.zeros(plan["n_buckets"], B.AGG_BUCKET_STATS_DTYPE)
        for i, r in enumerate(records):
            for k in SM.RECORD_FIELDS:
                rows[i][k] = r[k]
        parts.append((plan, rows))
        for d in match:
            want.setdefault(GM.bucket_pos(float(col_a.u64[d]), 7.0, 0.5), []).append(int(col_b.u64[d]))
    assert len({p["base_pos"] for p, _ in parts}) == 3
    keys, merged = B.merge_bucket_stats(parts)
    lo_pos, hi_pos = min(want), max(want)
    assert keys == [float(pos) * 7.0 + 0.5 for pos in range(lo_pos, hi_pos + 1)] and len(merged) == len(keys)
    assert keys == B.merge_histograms([(p, np.zeros(p["n_buckets"], np.uint32)) for p, _ in parts])[0]
    for pos, m in zip(range(lo_pos, hi_pos + 1), merged):
        vals = want.get(pos, [])
        assert m["count"] == len(vals) and m["sum"] == sum(vals) == m["sum_lo"] + (m["sum_hi"] << 64)
        assert (m["min_value"], m["max_value"]) == ((min(vals), max(vals)) if vals else (GM.MASK, 0))
        assert B.agg_stats_finalize(m, GM.U64) == GM.finalize(m, GM.U64)
    assert any(m["sum_hi"] > 0 for m in merged) and any(m["count"] == 0 for m in merged)
    assert B.merge_bucket_stats([]) == ([], [])
    # a bucket record finalizes like a top-level one: I64 subtracts count * 2^63
    rec = {"count": 2, "min_value": GM.to_u64(-7, GM.I64), "max_value": GM.to_u64(3, GM.I64),
           "sum_lo": (GM.to_u64(-7, GM.I64) + GM.to_u64(3, GM.I64)) & GM.MASK, "sum_hi": (GM.to_u64(-7, GM.I64) + GM.to_u64(3, GM.I64)) >> 64}
    assert B.agg_stats_finalize(_as_row(B, rec), GM.I64) == {"count": 2, "sum": -4, "min": -7, "max": 3, "avg": -2.0}
    assert B.agg_stats_finalize(_as_row(B, SM.empty_record()), GM.U64) == {"count": 0, "sum": 0, "min": None, "max": None, "avg": None}


def _header():
    return open(os.path.join(ROOT, "include", "tantivy_amd.h")).read()


def test_header_declares_the_feature_and_the_binding_agrees(B):
    src = _header()
    masks = {name: int(v, 16) for name, v in re.findall(r"#define\s+(TQ_KERNEL_[A-Z_]+)\s+(0x[0-9a-fA-F]+)u", src)}
    assert B.KERNEL_AGG_SUB == masks["TQ_KERNEL_AGG_SUB"] == 0x200000
    assert masks["TQ_KERNEL_AGG_SUB"] not in [v for n, v in masks.items() if n != "TQ_KERNEL_AGG_SUB"]
    assert B.kernel_names(B.KERNEL_AGG_SUB) == ["agg_sub"] and B.kernel_names(B.KERNEL_AGG) == ["agg"]
    for name in ("tq_agg_metric_request", "tq_agg_bucket_stats_t"):
        assert re.search(r"\}\s*%s\s*;" % name, src), name
    assert C.sizeof(B.TqAggMetricRequest) == 8 and B.AGG_BUCKET_STATS_DTYPE.itemsize == 40
    fields = re.search(r"typedef struct tq_agg_bucket_stats_t \{(.*?)\}", src, re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S)) == list(B.AGG_BUCKET_STATS_DTYPE.names)
    assert all(B.AGG_BUCKET_STATS_DTYPE[n] == np.uint64 for n in B.AGG_BUCKET_STATS_DTYPE.names)
    fields = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct tq_agg_metric_request \{(.*?)\}", src, re.S).group(1), flags=re.S)
    declared = re.findall(r"\b(uint32_t|uint8_t)\s+([a-z_]+)(?:\[(\d+)\])?\s*;", fields)
    ctype = {"uint32_t": C.c_uint32, "uint8_t": C.c_uint8}
    assert [(n, ctype[t] * int(k) if k else ctype[t]) for t, n, k in declared] == \
        [(n, t) for n, t in B.TqAggMetricRequest._fields_] and len(declared) == 3
    # the new section stands below the declaration of tq_agg_batch_device
    assert src.index("int tq_agg_batch_device(") < src.index("sub-aggregations: stats of a second column") < src.index("int tq_agg_sub_batch(")


def test_library_exports_the_entry_points(B):
    L = B.lib()
    declared = set(re.findall(r"\b(tq_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for name in ("tq_agg_sub_batch", "tq_agg_sub_batch_device", "tq_agg_sub_lds_capacities"):
        assert name in declared and name in B.EXPORTS and hasattr(L, name), name
    # null arguments are errors, not crashes; the message names the function
    assert L.tq_agg_sub_batch(None, None, 1, None, None, None, None, None, 0) != 0 and b"tq_agg_sub_batch:" in L.tq_last_error()
    assert L.tq_agg_sub_batch_device(None, None, 1, None, None, None, None, None, 0, None) != 0
    assert b"tq_agg_sub_batch_device:" in L.tq_last_error()
    small, large = B.agg_sub_lds_capacities()
    assert 1 <= small <= large and 40 * large + 16384 <= 65536  # (the table beside the slabs in the static 64 KB)
