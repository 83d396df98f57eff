"""CPU checks of the aggregations over a fast field (tq_agg_batch*; tests/agg_model.py, tantivy_amd.binding): the exact
integer stats that tests/test_gpu_agg.py holds the device to ARE the reference's Kahan f64 stats wherever every partial sum
is below 2^53; tq_agg_histogram_plan — host arithmetic, no device — is the model's normalize_histogram_req +
compute_dense_range bit for bit; the merge and finalize helpers; and the C ABI of the feature is declared, bound and
exported.  No device compute here, and no tolerance: every comparison is ==."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import agg_model as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_MAX = GM.F64_MAX


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def _as_row(B, rec):
    row = np.zeros(1, B.AGG_STATS_DTYPE)
    for k, v in rec.items():
        row[0][k] = v
    return row[0]


# ---- the model and the binding's finalize: exact sums = Kahan sums below 2^53
@pytest.mark.parametrize("value_type", [GM.U64, GM.I64])
def test_exact_sums_are_the_kahan_sums_below_2_53(B, value_type):
    rng = np.random.default_rng(3 + value_type)
    for trial in range(20):
        n = int(rng.integers(1, 400))
        if value_type == GM.U64:
            typed = [int(x) for x in rng.integers(0, 1 << 40, size=n)]
        else:
            typed = [int(x) for x in rng.integers(-(1 << 40), 1 << 40, size=n)]
            typed[0] = -abs(typed[0]) - 1  # (some value is negative)
        # every partial sum stays below 2^53 in magnitude: n * 2^40 < 2^49
        u = [GM.to_u64(x, value_type) for x in typed]
        assert [GM.typed_from_u64(v, value_type) for v in u] == typed
        md = n + 5
        present = np.zeros(md, bool)
        present[rng.choice(md, size=n, replace=False)] = True
        col = GM.Column(np.array(u, np.uint64), present, md)
        match = np.nonzero(rng.random(md) < 0.7)[0]
        rec, _ = GM.expected(match, col, value_type)
        got = GM.finalize(rec, value_type)
        assert B.agg_stats_finalize(_as_row(B, rec), value_type) == got
        in_order = [int(col.u64[d]) for d in match if col.has[d]]
        ref = GM.reference_stats(in_order, value_type)
        assert got["count"] == ref["count"] == len(in_order)
        if not in_order:
            assert got["min"] is None and ref["min"] is None and got["avg"] is None and ref["avg"] is None
            continue
        assert float(got["sum"]) == ref["sum"] and abs(got["sum"]) < 1 << 53
        assert float(got["min"]) == ref["min"] and float(got["max"]) == ref["max"]
        assert got["avg"] == ref["avg"]  # (exact int / int and f64 / f64 round the same quotient)


def test_sum_past_2_64_and_the_i64_offset(B):
    top = (1 << 64) - 1
    col = GM.Column(np.array([top, top - 1, top - 2, 5], np.uint64), None, 4)
    rec, _ = GM.expected([0, 1, 2, 3], col, GM.U64)
    assert rec["sum_hi"] == 2 and rec["sum_lo"] + (rec["sum_hi"] << 64) == 3 * top - 3 + 5
    assert B.agg_stats_finalize(_as_row(B, rec), B.VALUE_U64)["sum"] == 3 * top + 2
    assert B.merge_agg_stats([_as_row(B, rec)] * 2)["sum"] == 6 * top + 4
    typed = [-5, 7, -(1 << 62), 3]
    col = GM.Column(np.array([GM.to_u64(x, GM.I64) for x in typed], np.uint64), None, 4)
    rec, _ = GM.expected([0, 1, 2, 3], col, GM.I64)
    fin = GM.finalize(rec, GM.I64)
    assert fin["sum"] == sum(typed) and fin["min"] == -(1 << 62) and fin["max"] == 7 and fin["count"] == 4
    assert B.agg_stats_finalize(_as_row(B, rec), B.VALUE_I64) == fin


def test_conversions_keep_order_and_round_trip(B):
    for vt, xs in ((GM.I64, [-(1 << 63), -1, 0, 1, (1 << 63) - 1]),
                   (GM.F64, [-math.inf, -1.5, -0.0, 0.0, 2.5, math.inf]), (GM.U64, [0, 1, (1 << 64) - 1])):
        u = [GM.to_u64(x, vt) for x in xs]
        assert u == sorted(u) and len(set(u)) == len(u)
        assert [GM.f64_from_u64(v, vt) for v in u] == [float(x) for x in xs]
        assert GM.f64_array(np.array(u, np.uint64), vt).tolist() == [float(x) for x in xs]
        assert [B.agg_value_from_u64(v, vt) for v in u] == [GM.typed_from_u64(v, vt) for v in u] == list(xs)
    assert math.copysign(1.0, GM.f64_from_u64(GM.to_u64(-0.0, GM.F64), GM.F64)) == -1.0
    assert math.isnan(GM.f64_from_u64(GM.to_u64(math.nan, GM.F64), GM.F64))
    assert (GM.sat_i64(1e300), GM.sat_i64(-1e300), GM.sat_i64(math.nan), GM.sat_i64(-2.5)) == (GM.I64_MAX, GM.I64_MIN, 0, -2)
    assert GM.bucket_pos(-0.5, 1.0, 0.0) == -1 and GM.bucket_pos(-7.0, 2.0, 0.0) == -4  # floor towards -inf


ERR_INVALID, ERR_UNSUPPORTED = 1, 4


def _info(vt, lo, hi, rows=1000):
    return {"min_value": GM.to_u64(lo, vt), "max_value": GM.to_u64(hi, vt), "gcd": 1, "resident_bytes": 0, "num_rows": rows,
            "num_bits": 0, "codec": 0, "cardinality": 0}


def _same_plan(B, info, vt, interval, offset=0.0, hard_bounds=None):
    want = GM.histogram_plan(info, vt, interval, offset, hard_bounds)
    got = B.agg_histogram_plan(info, vt, interval, offset, hard_bounds)
    assert got == want, (got, want)
    # bit for bit, not merely ==
    for k in ("bounds_min", "bounds_max", "interval", "offset"):
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), k
    return got


def test_histogram_plan_is_the_model(B):
    # a fractional offset
    p = _same_plan(B, _info(GM.U64, 3, 1000), GM.U64, 10.0, 0.25)
    assert (p["base_pos"], p["n_buckets"]) == (0, 100)
    p = _same_plan(B, _info(GM.U64, 0, 1000), GM.U64, 10.0, 0.25)
    assert p["base_pos"] == -1  # floor((0 - 0.25) / 10)
    # negative I64 values: floor towards -inf
    p = _same_plan(B, _info(GM.I64, -25, 14), GM.I64, 10.0)
    assert (p["base_pos"], p["n_buckets"]) == (-3, 5)
    # date-like nanoseconds near 1.7e18, an hour's interval: the value itself rounds to a multiple of 256
    lo, hi = 1_700_000_000_123_456_789, 1_700_086_400_987_654_321
    assert float(lo) != lo
    p = _same_plan(B, _info(GM.I64, lo, hi), GM.I64, 3.6e12)
    assert p["n_buckets"] == int(math.floor(float(hi) / 3.6e12)) - int(math.floor(float(lo) / 3.6e12)) + 1 == 25
    # F64 columns whose min / max are -inf / +inf: the sentinel bounds clip them to +-DBL_MAX
    p = _same_plan(B, _info(GM.F64, -math.inf, math.inf), GM.F64, 1e305)
    assert p["base_pos"] == int(math.floor(-F64_MAX / 1e305)) and p["n_buckets"] == 2 * 1798 and p["bounds_min"] == -F64_MAX
    p = _same_plan(B, _info(GM.F64, -math.inf, math.inf), GM.F64, 0.5, 0.1, (-3.0, 4.0))
    assert (p["bounds_min"], p["bounds_max"]) == (-3.0, 4.0) and p["base_pos"] == -7 and p["n_buckets"] == 7 + 8
    with pytest.raises(B.TantivyAmdError) as ei:  # (without bounds and with a sane interval: far too many buckets)
        B.agg_histogram_plan(_info(GM.F64, -math.inf, math.inf), GM.F64, 1.0)
    assert ei.value.code == ERR_UNSUPPORTED
    # NaNs at the ends of an F64 column's order: f64::max / min take the bounds
    nan_lo, nan_hi = GM.to_u64(-math.nan, GM.F64), GM.to_u64(math.nan, GM.F64)
    info = dict(_info(GM.F64, 0.0, 0.0), min_value=min(nan_lo, nan_hi), max_value=max(nan_lo, nan_hi))
    _same_plan(B, info, GM.F64, 1.0, 0.0, (-5.0, 5.0))
    # hard bounds that cut, that contain the column (the sentinel), that miss it
    p = _same_plan(B, _info(GM.U64, 0, 8191), GM.U64, 128.0, 0.0, (1000.0, 5000.0))
    assert (p["bounds_min"], p["bounds_max"], p["base_pos"], p["n_buckets"]) == (1000.0, 5000.0, 7, 33)
    p = _same_plan(B, _info(GM.U64, 0, 8191), GM.U64, 128.0, 0.0, (0.0, 8191.0))
    assert (p["bounds_min"], p["bounds_max"], p["n_buckets"]) == (-F64_MAX, F64_MAX, 64)
    p = _same_plan(B, _info(GM.U64, 0, 8191), GM.U64, 128.0, 0.0, (9000.0, 9999.0))
    assert p["n_buckets"] == 0 and p["bounds_min"] == 9000.0
    p = _same_plan(B, _info(GM.U64, 0, 8191, rows=0), GM.U64, 128.0)
    assert p["n_buckets"] == 0
    # the bucket cap
    p = _same_plan(B, _info(GM.U64, 0, 65535), GM.U64, 1.0)
    assert p["n_buckets"] == 65536 == B.AGG_MAX_BUCKETS == GM.MAX_BUCKETS
    with pytest.raises(GM.Refused) as mi:
        GM.histogram_plan(_info(GM.U64, 0, 65536), GM.U64, 1.0)
    assert mi.value.kind == "unsupported"
    with pytest.raises(B.TantivyAmdError) as ei:
        B.agg_histogram_plan(_info(GM.U64, 0, 65536), GM.U64, 1.0)
    assert ei.value.code == ERR_UNSUPPORTED and "65537" in str(ei.value) and "tq_agg_histogram_plan" in str(ei.value)
    with pytest.raises(B.TantivyAmdError) as ei:  # positions that saturate
        B.agg_histogram_plan(_info(GM.U64, 0, (1 << 64) - 1), GM.U64, 1e-300)
    assert ei.value.code == ERR_UNSUPPORTED
    with pytest.raises(GM.Refused):
        GM.histogram_plan(_info(GM.U64, 0, (1 << 64) - 1), GM.U64, 1e-300)


@pytest.mark.parametrize("kwargs", [
    dict(interval=0.0), dict(interval=-1.0), dict(interval=math.inf), dict(interval=math.nan),
    dict(interval=1.0, offset=math.inf), dict(interval=1.0, offset=math.nan),
    dict(interval=1.0, hard_bounds=(5.0, 4.0)), dict(interval=1.0, hard_bounds=(-math.inf, 4.0)),
    dict(interval=1.0, hard_bounds=(0.0, math.nan)), dict(interval=1.0, value_type=3),
])
def test_histogram_plan_refuses_what_the_model_refuses(B, kwargs):
    kwargs = dict(kwargs)
    vt = kwargs.pop("value_type", GM.U64)
    info = _info(GM.U64, 0, 100)
    with pytest.raises(GM.Refused) as mi:
        GM.histogram_plan(info, vt, **kwargs)
    assert mi.value.kind == "invalid"
    with pytest.raises(B.TantivyAmdError) as ei:
        B.agg_histogram_plan(info, vt, **kwargs)
    assert ei.value.code == ERR_INVALID and "tq_agg_histogram_plan" in str(ei.value)


def test_merge_and_finalize_helpers_over_three_segments(B):
    rng = np.random.default_rng(12)
    for vt in (GM.U64, GM.I64, GM.F64):
        interval, offset = 7.0, 0.5
        recs, parts, all_f = [], [], []
        for seg_ord, (lo, hi) in enumerate(((100, 300), (-50, 120), (1000, 1100))):
            if vt == GM.U64:
                lo = max(lo, 0)
            n = 200
            typed = [float(x) + 0.25 for x in rng.integers(lo, hi, size=n)] if vt == GM.F64 else [int(x) for x in rng.integers(lo, hi, size=n)]
            u = np.array([GM.to_u64(x, vt) for x in typed], np.uint64)
            if seg_ord == 0 and vt == GM.U64:
                u[:3] = (1 << 64) - 1 - np.arange(3, dtype=np.uint64)  # (the merged sum passes 2^64)
            col = GM.Column(u, None, n)
            hard = (0.0, 1050.0)
            plan = GM.histogram_plan(col.info, vt, interval, offset, hard)
            assert B.agg_histogram_plan(dict(col.info, gcd=1), vt, interval, offset, hard) == plan
            match = np.nonzero(rng.random(n) < 0.8)[0]
            rec, counts = GM.expected(match, col, vt, plan)
            assert B.agg_stats_finalize(_as_row(B, rec), vt) == GM.finalize(rec, vt)
            recs.append(rec)
            parts.append((plan, np.array(counts, np.uint32)))
            all_f += [f for f in GM.f64_array(col.u64[match], vt).tolist() if 0.0 <= f <= 1050.0]
        assert len({p["base_pos"] for p, _ in parts}) == 3
        merged = B.merge_agg_stats([_as_row(B, r) for r in recs])
        total = sum(r["sum_lo"] + (r["sum_hi"] << 64) for r in recs)
        assert merged["sum"] == total and (merged["sum_hi"] > 0) == (vt != GM.F64)  # (F64: no sum)
        assert merged["count"] == sum(r["count"] for r in recs) and merged["matches"] == sum(r["matches"] for r in recs)
        assert merged["min_value"] == min(r["min_value"] for r in recs) and merged["max_value"] == max(r["max_value"] for r in recs)
        assert B.agg_stats_finalize(merged, vt) == GM.finalize(merged, vt)
        keys, counts = B.merge_histograms(parts)
        want = {}
        for f in all_f:
            pos = GM.bucket_pos(f, interval, offset)
            want[pos] = want.get(pos, 0) + 1
        lo_pos, hi_pos = min(want), max(want)
        assert keys[0] <= float(lo_pos) * interval + offset and len(keys) == len(counts)
        got = {k: c for k, c in zip(keys, counts) if c}
        assert got == {float(pos) * interval + offset: c for pos, c in want.items()}
        assert sum(counts) == len(all_f) == merged["in_bounds"]
    assert B.merge_histograms([]) == ([], [])
    assert B.agg_stats_finalize(_as_row(B, GM.expected([], GM.Column(np.array([1], np.uint64), None, 1), GM.U64)[0]), GM.U64) == \
        {"count": 0, "sum": 0, "min": None, "max": None, "avg": None}


def _header():
    return open(os.path.join(ROOT, "include", "tantivy_amd.h")).read()


def test_header_declares_the_feature_and_the_binding_agrees(B):
    src = _header()
    enums = dict(re.findall(r"\b(TQ_VALUE_U64|TQ_VALUE_I64|TQ_VALUE_F64)\s*=\s*(\d+)", src))
    assert enums == {"TQ_VALUE_U64": "0", "TQ_VALUE_I64": "1", "TQ_VALUE_F64": "2"}
    assert (B.VALUE_U64, B.VALUE_I64, B.VALUE_F64) == (GM.U64, GM.I64, GM.F64) == (0, 1, 2)
    masks = {name: int(v, 16) for name, v in re.findall(r"#define\s+(TQ_KERNEL_[A-Z_]+)\s+(0x[0-9a-fA-F]+)u", src)}
    assert B.KERNEL_AGG == masks["TQ_KERNEL_AGG"] == 0x100000
    assert masks["TQ_KERNEL_AGG"] not in [v for n, v in masks.items() if n != "TQ_KERNEL_AGG"]
    assert B.kernel_names(B.KERNEL_AGG) == ["agg"]
    assert int(re.search(r"#define\s+TQ_AGG_MAX_BUCKETS\s+(\d+)u", src).group(1)) == B.AGG_MAX_BUCKETS
    assert '"agg_slices"' in src and '"agg_lds_buckets"' in src
    for name in ("tq_agg_request", "tq_agg_hist_plan_t", "tq_agg_stats_t"):
        assert re.search(r"\}\s*%s\s*;" % name, src), name
    assert B.AGG_STATS_DTYPE.itemsize == 64 and C.sizeof(B.TqAggRequest) == 40 and C.sizeof(B.TqAggHistPlan) == 32
    fields = re.search(r"typedef struct tq_agg_stats_t \{(.*?)\}", src, re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", fields) == list(B.AGG_STATS_DTYPE.names)
    doc = src[src.index("aggregations over a fast field"): src.index("enum tq_value_type")]
    assert "algorithmic_bytes" in doc and "WRITTEN AS 0" in doc and "NaN" in doc


def test_library_exports_the_three_entry_points(B):
    L = B.lib()
    declared = set(re.findall(r"\b(tq_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for name in ("tq_agg_histogram_plan", "tq_agg_batch", "tq_agg_batch_device"):
        assert name in declared and name in B.EXPORTS and hasattr(L, name), name
    # null arguments are errors, not crashes; the message names the function
    assert L.tq_agg_histogram_plan(None, None, None) != 0 and b"tq_agg_histogram_plan" in L.tq_last_error()
    assert L.tq_agg_batch(None, None, 1, None, None, None, 0) != 0 and b"tq_agg_batch" in L.tq_last_error()
    assert L.tq_agg_batch_device(None, None, 1, None, None, None, 0, None) != 0 and b"tq_agg_batch_device" in L.tq_last_error()
