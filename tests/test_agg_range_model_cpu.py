"""CPU checks of the range aggregation (tq_agg_range_batch*; tests/range_agg_model.py, tantivy_amd.binding): the recorded
results of the reference's own unit tests (tests/golden/agg_range_reference.json) through the model AND through the
library's host-only plan and search — the search being the very code the kernel runs (tq_agg_range_search.hpp); the
saturating conversions; model plan == library plan over random range sets; the closed form tests/test_gpu_agg_range.py
holds the device to IS the reference's collect wherever the starts are strictly increasing, and its integer sums are the
reference's Kahan sums below 2^53; the decisions where the reference leaves the result open (an empty range counts nothing, a
range that starts above its end is refused); every refusal; key strings; the host helpers; and the C ABI is declared, bound
and exported.  No device compute here, and no tolerance: every comparison is ==."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

from tests import agg_model as GM
from tests import range_agg_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = RM.TOP
ERR_INVALID, ERR_UNSUPPORTED = 1, 4
VT = {"U64": GM.U64, "I64": GM.I64, "F64": GM.F64}


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "agg_range_reference.json")) as f:
        return json.load(f)["cases"]


def _u64(x):
    if isinstance(x, str):
        return {"MIN": 0, "MAX": TOP, "MAX-1": TOP - 1}[x]
    return GM.to_u64(x["f64"], GM.F64) if "f64" in x else int(x["u64"])


def _lib_plan(B, vt, ranges):
    return B.agg_range_plan(vt, ranges)


# ---- the reference's own unit tests
@pytest.mark.parametrize("case", _golden(), ids=lambda c: c["name"])
def test_recorded_results_of_the_reference(B, case):
    vt = VT[case["value_type"]]
    ranges = [tuple(r) for r in case["ranges"]]
    model = RM.plan(vt, ranges)
    assert _lib_plan(B, vt, ranges) == model
    if "n_buckets" in case:
        assert len(model) == case["n_buckets"]
    for i, (s, e) in enumerate(case.get("buckets_prefix", [])):
        assert (model[i]["start"], model[i]["end"]) == (_u64(s), _u64(e)), i
    for i, ins in enumerate(case.get("inserted_prefix", [])):
        assert (model[i]["source"] is None) == ins
    starts = RM.starts_of(model)
    for v, pos in case.get("search", []):
        v = _u64(v)
        assert RM.reference_bucket_pos(starts, v) == RM.bucket_of(starts, v) == B.agg_range_bucket_of(starts, v) == pos, v
    keys = [RM.key_of(b, vt) for b in model]
    assert keys == [B.range_key(b, vt) for b in model]
    if "keys" in case:
        assert keys == case["keys"]
    if "first_key" in case:
        assert (keys[0], keys[-1]) == (case["first_key"], case["last_key"])


# ---- conversions
def test_saturating_conversions(B):
    inf = math.inf
    want = {
        GM.U64: [(-1.0, 0), (-0.0, 0), (0.5, 0), (2.0 ** 63, 1 << 63), (2.0 ** 64, TOP), (inf, TOP), (-inf, 0), (1e30, TOP), (7.9, 7)],
        GM.I64: [(-1.0, (1 << 63) - 1), (-0.0, 1 << 63), (0.5, 1 << 63), (2.0 ** 63, TOP), (2.0 ** 64, TOP), (inf, TOP), (-inf, 0),
                 (-2.0 ** 63, 0), (-1e30, 0), (-7.9, (1 << 63) - 7)],
        # (the image: positive floats get the sign bit set, negative ones are inverted; -0.0 sits right below 0.0)
        GM.F64: [(-1.0, 0x400FFFFFFFFFFFFF), (-0.0, (1 << 63) - 1), (0.0, 1 << 63), (0.5, 0xBFE0000000000000),
                 (2.0 ** 63, 0xC3E0000000000000), (2.0 ** 64, 0xC3F0000000000000), (inf, 0xFFF0000000000000), (-inf, 0x000FFFFFFFFFFFFF)],
    }
    for vt, table in want.items():
        for val, u in table:
            assert RM.convert_bound(val, vt) == u, (vt, val)
            # through the library: as the start of a range with an open end (the plan's last bucket is that range)
            plan = _lib_plan(B, vt, [(val, None)])
            assert plan[-1] == {"start": u, "end": TOP, "source": 0} and (u == 0) == (len(plan) == 1), (vt, val, plan)
            # ... and as the end of a range with an open start
            plan = _lib_plan(B, vt, [(None, val)])
            assert plan[0] == {"start": 0, "end": u, "source": 0} and (u == TOP) == (len(plan) == 1), (vt, val, plan)
    # the F64 image keeps the order, infinities at the ends of the finite values
    xs = [-inf, -1e300, -1.0, -0.0, 0.0, 5e-324, 1.0, 1e300, inf]
    img = [RM.convert_bound(x, GM.F64) for x in xs]
    assert img == sorted(img) and len(set(img)) == len(img)


# ---- model plan == library plan
def _random_ranges(rng, vt, n):
    """n non-overlapping ranges cut from sorted random bounds, some adjacent, some with holes, shuffled; maybe open ends"""
    if vt == GM.F64:
        pts = np.sort(rng.normal(0.0, 1e3, size=2 * n))
    elif vt == GM.I64:
        pts = np.sort(rng.integers(-10 ** 6, 10 ** 6, size=2 * n)).astype(np.float64) + rng.choice([0.0, 0.25], size=2 * n)
    else:
        pts = np.sort(rng.integers(0, 10 ** 6, size=2 * n)).astype(np.float64) + rng.choice([0.0, 0.5], size=2 * n)
    out = []
    for i in range(n):
        lo, hi = float(pts[2 * i]), float(pts[2 * i + 1])
        if i + 1 < n and rng.random() < 0.4:
            hi = float(pts[2 * i + 2])  # adjacent to the next one
        out.append((lo, hi))
    if rng.random() < 0.3:
        out[0] = (None, out[0][1])
    if rng.random() < 0.3:
        out[-1] = (out[-1][0], None)
    order = rng.permutation(n)
    return [out[i] for i in order]


@pytest.mark.parametrize("vt", [GM.U64, GM.I64, GM.F64])
def test_model_plan_is_the_library_plan(B, vt):
    rng = np.random.default_rng(70 + vt)
    seen_hole = seen_adjacent = 0
    for trial in range(60):
        ranges = _random_ranges(rng, vt, int(rng.integers(1, 12)))
        model = RM.plan(vt, ranges)
        assert _lib_plan(B, vt, ranges) == model, ranges
        assert model[0]["start"] == 0 and model[-1]["end"] == TOP
        assert all(a["end"] == b["start"] for a, b in zip(model, model[1:]))
        assert sorted(b["source"] for b in model if b["source"] is not None) == list(range(len(ranges)))
        seen_hole += sum(b["source"] is None for b in model[1:-1])
        seen_adjacent += sum(a["source"] is not None and b["source"] is not None for a, b in zip(model, model[1:]))
    assert seen_hole and seen_adjacent
    # dicts with "from" / "to" are the same request
    assert _lib_plan(B, vt, [{"from": 1.0, "to": 5.0}, {"from": 9.0}]) == RM.plan(vt, [(1.0, 5.0), (9.0, None)])


# ---- the search at every boundary
def _plan_of(n_buckets):
    """n_buckets buckets on a U64 column from k user ranges 7 wide, 10 apart: k ranges, k - 1 holes and the outer bucket
    behind make 2k buckets when the first range starts at 0, one more (the outer bucket in front) when it starts at 10"""
    if n_buckets == 1:
        return [(None, None)]
    if n_buckets % 2:
        k = (n_buckets - 1) // 2
        return [(10.0 * (i + 1), 10.0 * (i + 1) + 7.0) for i in range(k)]
    k = n_buckets // 2
    return [(10.0 * i, 10.0 * i + 7.0) for i in range(k)]


@pytest.mark.parametrize("n_buckets", [1, 2, 3, 63, 64, 65, 1023, 1024])
def test_bucket_of_at_every_boundary(B, n_buckets):
    ranges = _plan_of(n_buckets)
    model = RM.plan(GM.U64, ranges)
    assert len(model) == n_buckets and _lib_plan(B, GM.U64, ranges) == model
    starts = RM.starts_of(model)
    assert starts == sorted(set(starts))  # strictly increasing
    sa = np.array(starts, np.uint64)
    probes = {0, TOP}
    for s in starts:
        probes |= {max(s - 1, 0), s, min(s + 1, TOP)}
    for v in sorted(probes):
        want = int(np.searchsorted(sa, np.uint64(v), "right")) - 1
        assert RM.bucket_of(starts, v) == RM.reference_bucket_pos(starts, v) == B.agg_range_bucket_of(starts, v) == want, v
        assert model[want]["start"] <= v and (v < model[want]["end"] or v == TOP)
    assert B.agg_range_bucket_of(starts, TOP) == n_buckets - 1


# ---- closed form == transliteration; integer sums == Kahan sums
def _case(rng, vt_b, md=600):
    has_a, has_b = rng.random(md) < 0.8, rng.random(md) < 0.6
    col_a = GM.Column(rng.integers(0, 200, size=int(has_a.sum())).astype(np.uint64), has_a, md)
    lo = 0 if vt_b == GM.U64 else -(1 << 40)
    typed = [int(x) for x in rng.integers(lo, 1 << 40, size=int(has_b.sum()))]
    col_b = GM.Column(np.array([GM.to_u64(x, vt_b) for x in typed], np.uint64), has_b, md)
    match = np.nonzero(rng.random(md) < 0.7)[0]
    return col_a, col_b, match


def _as_row(B, rec):
    row = np.zeros(1, B.AGG_BUCKET_STATS_DTYPE)
    for k, v in rec.items():
        row[0][k] = v
    return row[0]


@pytest.mark.parametrize("vt_b", [GM.U64, GM.I64])
def test_closed_form_is_the_reference_collect_below_2_53(B, vt_b):
    rng = np.random.default_rng(90 + vt_b)
    for trial in range(10):
        col_a, col_b, match = _case(rng, vt_b)
        buckets = RM.plan(GM.U64, [(20.0, 50.0), (50.0, 90.5), (120.0, 150.0), (3.0, 7.0)])
        starts = RM.starts_of(buckets)
        assert starts == sorted(set(starts)) and len(buckets) == 8
        rec, counts, records = RM.expected_range(match, col_a, buckets, col_b, vt_b)
        ref_counts, ref_stats, largest = RM.reference_range(match, col_a, buckets, col_b, vt_b)
        assert largest < 2.0 ** 53  # 600 docs x 2^40 < 2^50: every partial sum of every bucket is exact in f64
        assert ref_counts == counts and sum(counts) == rec["count"] == rec["in_bounds"] and all(counts)
        assert RM.expected_range(match, col_a, buckets)[:2] == (rec, counts)  # (counts alone: the same record and row)
        for i, (r, st) in enumerate(zip(records, ref_stats)):
            got, ref = GM.finalize(r, vt_b), st.finalize()
            assert B.agg_stats_finalize(_as_row(B, r), vt_b) == got
            assert got["count"] == ref["count"] <= counts[i]
            if ref["count"] == 0:
                assert r == RM.empty_record() and got["min"] is None
                continue
            assert float(got["sum"]) == ref["sum"] and float(got["min"]) == ref["min"] and float(got["max"]) == ref["max"]
            assert got["avg"] == ref["avg"]


def test_an_empty_range_counts_nothing(B):
    """0.1 .. 0.9 on an integer column converts to [0, 0): it shares its start with the bucket behind it.  The last bucket
    whose start <= value is never the empty one; what the reference's binary search returns there depends on which of the
    equal starts it meets."""
    ranges = [(0.1, 0.9), (0.9, 10.0), (10.0, 10.5), (10.5, 20.0)]
    buckets = RM.plan(GM.U64, ranges)
    assert _lib_plan(B, GM.U64, ranges) == buckets
    assert [(b["start"], b["end"], b["source"]) for b in buckets] == [(0, 0, 0), (0, 10, 1), (10, 10, 2), (10, 20, 3), (20, TOP, None)]
    starts = RM.starts_of(buckets)
    for v, want in ((0, 1), (9, 1), (10, 3), (19, 3), (20, 4), (TOP, 4)):
        assert RM.bucket_of(starts, v) == B.agg_range_bucket_of(starts, v) == want
    assert RM.reference_bucket_pos(starts, 10) in (2, 3)  # (the reference: either of the equal starts)
    md = 64
    col = GM.Column(np.arange(md, dtype=np.uint64) % 25, None, md)
    rec, counts, _ = RM.expected_range(np.arange(md), col, buckets)
    assert counts[0] == counts[2] == 0 and sum(counts) == md and counts[1] > 0 and counts[3] > 0


# ---- refusals
def _refused(B, vt, ranges, code, *words):
    with pytest.raises(B.TantivyAmdError) as ei:
        B.agg_range_plan(vt, ranges)
    assert ei.value.code == code and "tq_agg_range_plan" in str(ei.value) and all(w in str(ei.value) for w in words), ei.value
    if vt <= GM.F64:
        with pytest.raises(RM.Refused) as mi:
            RM.plan(vt, ranges)
        assert mi.value.kind == ("invalid" if code == ERR_INVALID else "unsupported")


def test_refusals(B):
    L = B.lib()
    _refused(B, GM.U64, [], ERR_INVALID, "n_ranges")
    _refused(B, 3, [(1.0, 2.0)], ERR_INVALID, "value_type 3")
    _refused(B, GM.F64, [(1.0, math.nan)], ERR_INVALID, "range 0", "NaN")
    _refused(B, GM.U64, [(0.0, 1.0), (math.nan, None)], ERR_INVALID, "range 1", "NaN")
    _refused(B, GM.U64, [(0.0, 10.0), (30.0, 40.0), (5.0, 20.0)], ERR_INVALID, "overlapping ranges 0 and 2")
    _refused(B, GM.I64, [(-5.0, None), (None, -4.0)], ERR_INVALID, "overlapping ranges 1 and 0")
    # an empty range behind the range that shares its start: the stable sort leaves it there, and the pair overlaps
    _refused(B, GM.U64, [(10.9, 50.0), (10.2, 10.9)], ERR_INVALID, "overlapping ranges 0 and 1")
    assert len(B.agg_range_plan(GM.U64, [(10.2, 10.9), (10.9, 50.0)])) == 4
    _refused(B, GM.U64, [(0.0, 1.0), (10.0, 5.0)], ERR_INVALID, "range 1", "above its end")
    _refused(B, GM.F64, [(1.0, -1.0)], ERR_INVALID, "range 0", "above its end")
    # 512 ranges with a hole behind each, the first from 0: 512 + 511 + 1 = 1 024 buckets pass, one more range does not
    many = [(10.0 * i, 10.0 * i + 7.0) for i in range(513)]
    assert len(B.agg_range_plan(GM.U64, many[:512])) == 1024 == B.AGG_RANGE_MAX_BUCKETS == RM.MAX_BUCKETS
    _refused(B, GM.U64, [(10.0 * (i + 1), 10.0 * (i + 1) + 7.0) for i in range(512)], ERR_UNSUPPORTED, "1025")
    _refused(B, GM.U64, many, ERR_UNSUPPORTED, "1026")
    # non-zero reserved bytes, null arguments: straight at the C ABI
    req, keep = B._agg_range_request(0, GM.U64, [(1.0, 2.0)])
    out, n = (B.TqAggRangeBucket * 8)(), C.c_uint32(77)
    assert L.tq_agg_range_plan(C.byref(req), out, 8, C.byref(n)) == 0 and n.value == 3
    keep[0].reserved[5] = 1
    assert L.tq_agg_range_plan(C.byref(req), out, 8, C.byref(n)) == ERR_INVALID and b"tq_agg_range_plan" in L.tq_last_error()
    assert b"reserved" in L.tq_last_error() and n.value == 0
    keep[0].reserved[5] = 0
    req.reserved2 = 1
    assert L.tq_agg_range_plan(C.byref(req), out, 8, C.byref(n)) == ERR_INVALID and b"reserved" in L.tq_last_error()
    req.reserved2 = 0
    assert L.tq_agg_range_plan(C.byref(req), out, 2, C.byref(n)) == ERR_INVALID and b"cap 2" in L.tq_last_error() and n.value == 3
    assert L.tq_agg_range_plan(None, out, 8, C.byref(n)) == ERR_INVALID and b"tq_agg_range_plan: null argument" in L.tq_last_error()
    assert L.tq_agg_range_plan(C.byref(req), out, 8, None) == ERR_INVALID
    req.ranges = None
    assert L.tq_agg_range_plan(C.byref(req), out, 8, C.byref(n)) == ERR_INVALID and b"null argument" in L.tq_last_error()


# ---- keys
def test_key_strings(B):
    for x, text in ((0.0, "0"), (-0.0, "-0"), (0.1, "0.1"), (10.0, "10"), (-10.0, "-10"), (1e21, "1000000000000000000000"),
                    (1e16, "10000000000000000"), (1.5e-7, "0.00000015"), (123456.789, "123456.789"), (2.0 ** 63, "9223372036854776000"),
                    (math.inf, "inf"), (-math.inf, "-inf"), (5e-324, "0." + "0" * 323 + "5")):
        assert RM.f64_display(x) == B.f64_display(x) == text, x
        if math.isfinite(x):
            assert float(text) == x  # (round-trips)
    for vt, ranges, keys in (
            (GM.U64, [(10.0, 100.0)], ["*-10", "10-100", "100-*"]),
            (GM.U64, [(None, 1e21)], ["*-*"]),  # (saturated: the end is UINT64_MAX)
            (GM.I64, [(-10.0, -1.0)], ["*--10", "-10--1", "-1-*"]),
            (GM.I64, [(-0.0, 3.5)], ["*-0", "0-3", "3-*"]),
            (GM.F64, [(-0.0, 1e21)], ["*--0", "-0-1000000000000000000000", "1000000000000000000000-*"]),
            (GM.F64, [(0.0, 0.1), (0.1, 0.2)], ["*-0", "0-0.1", "0.1-0.2", "0.2-*"])):
        plan = RM.plan(vt, ranges)
        assert [RM.key_of(b, vt) for b in plan] == [B.range_key(b, vt) for b in B.agg_range_plan(vt, ranges)] == keys


# ---- the host helpers
def test_merge_ranges_and_finalize(B):
    rng = np.random.default_rng(3)
    ranges = [(100.0, 200.0), (0.0, 50.0)]
    buckets = RM.plan(GM.U64, ranges)
    assert len(buckets) == 4
    md = 300
    parts, all_docs = [], []
    cols = []
    for seg in range(3):
        has_b = rng.random(md) < 0.5
        col_a = GM.Column(rng.integers(0, 260, size=md).astype(np.uint64), None, md)
        col_b = GM.Column(np.array([GM.to_u64(int(x), GM.I64) for x in rng.integers(-1000, 1000, size=int(has_b.sum()))], np.uint64), has_b, md)
        match = np.nonzero(rng.random(md) < 0.6)[0]
        _, counts, records = RM.expected_range(match, col_a, buckets, col_b, GM.I64)
        parts.append((B.agg_range_plan(GM.U64, ranges), counts, [_as_row(B, r) for r in records]))
        cols.append((col_a, col_b, match))
    plan, counts, recs = B.merge_ranges(parts)
    assert plan == buckets and counts == [sum(p[1][i] for p in parts) for i in range(4)]
    for i in range(4):
        typed = []
        for col_a, col_b, match in cols:
            docs = match[(np.searchsorted(np.array(RM.starts_of(buckets), np.uint64), col_a.u64[match], "right") - 1) == i]
            typed += [GM.typed_from_u64(v, GM.I64) for v in col_b.u64[docs][col_b.has[docs]].tolist()]
        fin = B.agg_stats_finalize(recs[i], GM.I64)
        assert fin == {"count": len(typed), "sum": sum(typed), "min": min(typed), "max": max(typed), "avg": sum(typed) / len(typed)}
    # counts alone
    plan2, counts2, none = B.merge_ranges([(p, c, None) for p, c, _ in parts])
    assert (plan2, counts2, none) == (plan, counts, None)
    with pytest.raises(AssertionError):
        B.merge_ranges([parts[0], (B.agg_range_plan(GM.U64, [(0.0, 50.0)]), [0, 0], None)])
    out = B.range_finalize(plan, counts, recs, GM.U64, GM.I64, keys=["hot", None])
    assert [e["key"] for e in out] == ["*-50", "50-100", "hot", "200-*"]  # (from 0 on a U64 column IS the open start)
    assert [(e["from"], e["to"]) for e in out] == [(None, 50.0), (50.0, 100.0), (100.0, 200.0), (200.0, None)]
    assert [e["doc_count"] for e in out] == counts and out[2]["stats"] == B.agg_stats_finalize(recs[2], GM.I64)
    plain = B.range_finalize(plan, counts, None, GM.U64)
    assert all("stats" not in e for e in plain) and [e["key"] for e in plain] == ["*-50", "50-100", "100-200", "200-*"]
    f = B.range_finalize(B.agg_range_plan(GM.F64, [(-1.5, 2.5)]), [1, 2, 3], None, GM.F64)
    assert [(e["key"], e["from"], e["to"]) for e in f] == [("*--1.5", None, -1.5), ("-1.5-2.5", -1.5, 2.5), ("2.5-*", 2.5, None)]


# ---- header, binding, build, exports
def _header():
    return open(os.path.join(ROOT, "include", "tantivy_amd.h")).read()


def test_header_declares_the_feature_and_the_binding_agrees(B):
    from tantivy_amd import build

    src = _header()
    masks = {name: int(v, 16) for name, v in re.findall(r"#define\s+(TQ_KERNEL_[A-Z_]+)\s+(0x[0-9a-fA-F]+)u", src)}
    assert B.KERNEL_AGG_RANGE == masks["TQ_KERNEL_AGG_RANGE"] == 0x1000000
    assert masks["TQ_KERNEL_AGG_RANGE"] not in [v for n, v in masks.items() if n != "TQ_KERNEL_AGG_RANGE"]
    assert B.kernel_names(B.KERNEL_AGG_RANGE) == ["agg_range"] and B.KERNEL_NAMES[0x1000000] == "agg_range"
    assert re.search(r"#define\s+TQ_AGG_RANGE_MAX_BUCKETS\s+1024u", src) and B.AGG_RANGE_MAX_BUCKETS == 1024
    for name, ctype in (("tq_agg_range_t", B.TqAggRange), ("tq_agg_range_request", B.TqAggRangeRequest),
                        ("tq_agg_range_bucket_t", B.TqAggRangeBucket)):
        m = re.search(r"\}\s*%s\s*;\s*/\*\s*(\d+) bytes\s*\*/" % name, src)
        assert m and C.sizeof(ctype) == int(m.group(1)) == 24, name
    fields = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct tq_agg_range_bucket_t \{(.*?)\}", src, re.S).group(1), flags=re.S)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", fields) == [n for n, _ in B.TqAggRangeBucket._fields_]
    assert src.index("int tq_agg_terms_metric_image(") < src.index("range aggregation: doc counts") < src.index("int tq_agg_range_plan(")
    assert build.KERNEL_FILES["agg_range_kernel"] == "tq_agg_range.hip" and "tq_agg_range.hip" in build.WALK_FILES
    assert "tq_agg_range_search.hpp" in build.WALK_HEADERS
    names = [os.path.basename(p) for p in build.SOURCES]
    assert "tq_agg_range.hip" in names and "tq_agg_range.cpp" in names
    assert "tq_agg_range_search.hpp" in [os.path.basename(p) for p in build.HEADERS]
    assert all(os.path.exists(p) for p in build.SOURCES + build.HEADERS)
    assert build.kernel_hash(["agg_range_kernel<true, false, true, 128u>"]) != build.kernel_hash(["agg_kernel<true, 2048u>"])


def test_library_exports_the_entry_points(B):
    L = B.lib()
    declared = set(re.findall(r"\b(tq_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for name in ("tq_agg_range_plan", "tq_agg_range_bucket_of", "tq_agg_range_batch", "tq_agg_range_batch_device",
                 "tq_agg_range_lds_capacities"):
        assert name in declared and name in B.EXPORTS and hasattr(L, name), name
    # null arguments are errors, not crashes, and need no device; the message names the function
    assert L.tq_agg_range_batch(None, None, 1, None, None, None, None, None, 0) == ERR_INVALID
    assert b"tq_agg_range_batch: null argument" in L.tq_last_error()
    assert L.tq_agg_range_batch_device(None, None, 1, None, None, None, None, None, 0, None) == ERR_INVALID
    assert b"tq_agg_range_batch_device: null argument" in L.tq_last_error()
    assert B.agg_range_bucket_of([], 5) == 0 and L.tq_agg_range_bucket_of(None, 3, 5) == 0
    small, large = B.agg_range_lds_capacities()
    # the record table beside 1 024 starts and the slabs in the static 64 KB (the wavefronts' parts alias the slabs)
    assert 1 <= small <= large <= 1024 and 40 * large + 8 * 1024 + 16384 <= 65536
