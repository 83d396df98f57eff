"""CPU checks of the terms x histogram aggregation (tq_agg_terms_hist_batch*; tests/terms_hist_model.py,
tantivy_amd.binding): the closed form that tests/test_gpu_agg_terms_hist.py holds the device to agrees with the literal
per-doc loop; four of the reference's own unit tests (tests/golden/agg_terms_hist_reference.json) hold through the model
and through the binding's merge and finalize; the plan's arithmetic at its edges and every refusal through the host
library; the C ABI is declared, bound and exported.  No device compute here, and no tolerance: every comparison is ==."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import agg_model as AM
from tests import terms_hist_model as HM
from tests import terms_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
ORDER_NAMES = {"count_desc": TM.COUNT_DESC, "count_asc": TM.COUNT_ASC, "key_asc": TM.KEY_ASC, "key_desc": TM.KEY_DESC}


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def _h_info(col, gcd=1):
    return dict(col.info, gcd=gcd)


def _random_cases():
    """name -> (t_u64, t_has, h Column, value_type, histogram, match docs)"""
    rng = np.random.default_rng(20261120)
    md = 700
    every = np.ones(md, bool)
    some_t, some_h = rng.random(md) < 0.8, rng.random(md) < 0.6
    most = np.nonzero(rng.random(md) < 0.7)[0]
    out = {}

    def add(name, t_vals, t_has, h_vals, h_has, vt, histogram, match):
        t = np.zeros(md, np.uint64)
        t[t_has] = t_vals
        out[name] = (t, t_has, AM.Column(h_vals, None if h_has is None else h_has, md), vt, histogram, match)

    status = (rng.zipf(1.4, size=md) % 7).astype(np.uint64) * np.uint64(100) + np.uint64(200)
    ts = np.sort(rng.integers(0, 36000, size=md)).astype(np.uint64)
    add("full x full u64", status, every, ts, None, AM.U64, {"interval": 3600.0}, most)
    add("hard bounds bind", status, every, ts, None, AM.U64, {"interval": 3600.0, "hard_bounds": (7200.0, 20000.0)}, most)
    add("hard bounds do not bind", status, every, ts, None, AM.U64, {"interval": 3600.0, "hard_bounds": (-1.0, 1e9)}, most)
    add("optional key", status[: int(some_t.sum())], some_t, ts, None, AM.U64, {"interval": 1000.0, "offset": 250.0}, most)
    add("optional histogram column", status, every, ts[: int(some_h.sum())], some_h, AM.U64, {"interval": 5000.0}, most)
    add("both optional, bounds", status[: int(some_t.sum())], some_t, ts[: int(some_h.sum())], some_h, AM.U64,
        {"interval": 5000.0, "hard_bounds": (6000.0, 19999.0)}, most)
    i64 = np.array([AM.to_u64(int(x), AM.I64) for x in rng.integers(-50000, 50000, size=md)], np.uint64)
    add("i64 dates", status, every, i64, None, AM.I64, {"interval": 10000.0}, most)
    f64 = np.array([AM.to_u64(float(x), AM.F64) for x in rng.normal(0.0, 3.0, size=md)], np.uint64)
    add("f64", status, every, f64, None, AM.F64, {"interval": 0.5, "offset": 0.25}, most)
    add("no value in bounds", status, every, ts, None, AM.U64, {"interval": 10.0, "hard_bounds": (1e6, 2e6)}, most)
    add("histogram column without a value", status, every, np.zeros(0, np.uint64), np.zeros(md, bool), AM.U64, {"interval": 10.0}, most)
    add("key column without a value", np.zeros(0, np.uint64), np.zeros(md, bool), ts, None, AM.U64, {"interval": 3600.0}, most)
    add("empty match", status, every, ts, None, AM.U64, {"interval": 3600.0}, np.zeros(0, np.int64))
    add("one key, one bucket", np.full(md, 9, np.uint64), every, np.full(md, 5, np.uint64), None, AM.U64, {"interval": 10.0}, most)
    add("the histogram column is the key column", status, every, status, None, AM.U64, {"interval": 250.0}, most)
    return out


CASES = _random_cases()


def _plan_of(case, order=TM.COUNT_DESC, size=10):
    t, t_has, h, vt, histogram, match = case
    return HM.plan(TM.column_info(t[t_has]), _h_info(h), vt, histogram, order, size)


@pytest.mark.parametrize("order", TM.ORDERS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_models_agree(name, order):
    t, t_has, h, vt, histogram, match = CASES[name]
    p = _plan_of(CASES[name], order)
    distinct = HM.closed_form(t, t_has, h, vt, match, p, order, 1)[0]["distinct"]
    assert (distinct == 0) == (name in ("key column without a value", "empty match"))
    assert (p["hist"]["n_buckets"] == 0) == (name in ("no value in bounds", "histogram column without a value"))
    for size in sorted({1, max(1, distinct - 1), max(1, distinct), distinct + 1}):
        rec, keys, counts, rows = HM.closed_form(t, t_has, h, vt, match, p, order, size)
        ref = HM.reference_segment(t, t_has, h, vt, match, p, order, size)
        where = (name, order, size)
        assert keys == ref["order"], where
        assert [(c, r) for c, r in zip(counts, rows)] == [ref["entries"][k] for k in keys], where
        assert rec["sum_other_doc_count"] == ref["sum_other_doc_count"], where
        assert rec["doc_count_error_upper_bound"] == ref["doc_count_error_upper_bound"], where
        assert rec["distinct"] == ref["distinct"] == distinct and rec["n_returned"] == len(keys) == min(size, distinct), where
        assert rec["count"] == sum(counts) + rec["sum_other_doc_count"] == int(t_has[match].sum()) and rec["matches"] == match.size
        assert all(len(r) == p["hist"]["n_buckets"] and sum(r) <= c for c, r in zip(counts, rows)), where
        # the terms half is the terms model's, whatever the histogram does
        trec, tkeys, tcounts = TM.closed_form(t, t_has, match, TM.column_info(t[t_has]), order, size)
        assert (trec, tkeys, tcounts) == (rec, keys, counts), where
    if "bounds bind" not in name and "optional histogram" not in name and "both optional" not in name and p["hist"]["n_buckets"]:
        rec, keys, counts, rows = HM.closed_form(t, t_has, h, vt, match, p, order, 1000)
        assert [sum(r) for r in rows] == counts  # every counted doc has a bucket


def test_the_column_sums_are_the_plain_histogram():
    for name in ("full x full u64", "hard bounds bind", "i64 dates", "f64", "optional histogram column"):
        t, t_has, h, vt, histogram, match = CASES[name]
        p = _plan_of(CASES[name])
        rows = HM.closed_form(t, t_has, h, vt, match, p, TM.KEY_ASC, 1000)[3]
        _, want = AM.expected(match, h, vt, p["hist"])
        assert [sum(col) for col in zip(*rows)] == want, name


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "agg_terms_hist_reference.json")) as f:
        return json.load(f)["cases"]


def _golden_segment(case, lo, hi):
    """docs [lo, hi) of a golden case as one segment: -> (t_u64, t_has, h Column, match docs)"""
    i = np.arange(lo, hi, dtype=np.uint64)
    t = i % np.uint64(case["n_terms"])
    vals = np.array([AM.to_u64(float(int(x) % case["value_mod"]), AM.F64) for x in i], np.uint64)
    return t, np.ones(i.size, bool), AM.Column(vals, None, i.size), np.arange(i.size)


@pytest.mark.parametrize("case", _golden(), ids=lambda c: c["name"])
def test_the_references_own_cases(case, B):
    order = ORDER_NAMES[case["terms"]["order"]]
    size = case["terms"]["size"]
    histogram = dict(case["histogram"])
    if "hard_bounds" in histogram:
        histogram["hard_bounds"] = tuple(histogram["hard_bounds"])
    want = case["expect"]
    splits = {tuple(case["segments"]), (case["n_docs"],), (case["n_docs"] // 2, case["n_docs"] - case["n_docs"] // 2), (7, case["n_docs"] - 7)}
    assert sum(case["segments"]) == case["n_docs"]
    for split in sorted(splits):
        parts, lo = [], 0
        for n in split:
            t, t_has, h, match = _golden_segment(case, lo, lo + n)
            lo += n
            p = HM.plan(TM.column_info(t), _h_info(h), AM.F64, histogram, order, min(size * 10, TM.MAX_SIZE))
            # the plan through the host library is the model's
            assert B.agg_terms_hist_plan(TM.column_info(t), _h_info(h), AM.F64, histogram, order, min(size * 10, TM.MAX_SIZE)) == p
            rec, keys, counts, rows = HM.closed_form(t, t_has, h, AM.F64, match, p, order, min(size * 10, TM.MAX_SIZE))
            ref = HM.reference_segment(t, t_has, h, AM.F64, match, p, order, min(size * 10, TM.MAX_SIZE))
            assert keys == ref["order"] and [(c, r) for c, r in zip(counts, rows)] == [ref["entries"][k] for k in keys]
            if len(split) == 1:  # the segment's own answer
                assert keys == list(range(want["n_term_buckets"])) and counts == [want["doc_count"]] * len(keys)
                assert rows == [[want["bucket_doc_count"]] * len(want["bucket_keys"])] * len(keys)
                assert [(p["hist"]["base_pos"] + b) * p["hist"]["interval"] + p["hist"]["offset"] for b in range(p["hist"]["n_buckets"])] == want["bucket_keys"]
                if case["name"].endswith("non_binding_hard_bounds"):
                    assert (p["hist"]["bounds_min"], p["hist"]["bounds_max"]) == (-AM.F64_MAX, AM.F64_MAX)
                if case["name"].endswith("with_hard_bounds"):
                    assert (p["hist"]["bounds_min"], p["hist"]["bounds_max"]) == (5.0, 14.0) and p["n_cells"] == 3 * 11
            parts.append((np.array(keys, np.uint64), np.array(counts, np.uint32), np.array(rows, np.uint32).reshape(len(keys), -1), rec, p["hist"]))
        merged = B.merge_terms_hist(parts)
        assert B.merge_terms_hist([merged, B.merge_terms_hist([])])["entries"] == merged["entries"]
        assert B.merge_terms_hist([B.merge_terms_hist(parts[:1]), B.merge_terms_hist(parts[1:])]) == merged
        final = B.terms_hist_finalize(merged, size=size, order=order)
        assert final["bucket_keys"] == want["bucket_keys"], split
        assert [k for k, _, _ in final["buckets"]] == list(range(want["n_term_buckets"])), split
        assert all(c == want["doc_count"] for _, c, _ in final["buckets"]), split
        assert all(row == [want["bucket_doc_count"]] * len(want["bucket_keys"]) for _, _, row in final["buckets"]), split
        assert final["sum_other_doc_count"] == 0 and final["doc_count_error_upper_bound"] == 0


def test_merge_aligns_rows_by_base_pos_and_finalize_cuts(B):
    hp = {"interval": 10.0, "offset": 5.0}
    a = (np.array([7, 3], np.uint64), np.array([9, 4], np.uint32), np.array([[1, 2, 3], [0, 4, 0]], np.uint32),
         {"n_returned": 2, "sum_other_doc_count": 2, "doc_count_error_upper_bound": 1}, dict(hp, base_pos=2, n_buckets=3))
    b = (np.array([3, 8, 99], np.uint64), np.array([5, 1, 77], np.uint32), np.array([[5, 0], [0, 1], [9, 9]], np.uint32),
         {"n_returned": 2, "sum_other_doc_count": 0, "doc_count_error_upper_bound": 0}, dict(hp, base_pos=-1, n_buckets=2))
    c = (np.array([3], np.uint64), np.array([6], np.uint32), np.zeros((1, 0), np.uint32),
         {"n_returned": 1, "sum_other_doc_count": 0, "doc_count_error_upper_bound": 0}, dict(hp, base_pos=0, n_buckets=0))
    m = B.merge_terms_hist([a, b, c])
    assert m["base_pos"] == -1 and m["bucket_keys"] == [-5.0, 5.0, 15.0, 25.0, 35.0, 45.0]
    assert m["entries"] == {7: (9, [0, 0, 0, 1, 2, 3]), 3: (15, [5, 0, 0, 0, 4, 0]), 8: (1, [0, 1, 0, 0, 0, 0])}
    assert (m["sum_other_doc_count"], m["doc_count_error_upper_bound"]) == (2, 1)
    f = B.terms_hist_finalize(m, size=2)
    assert f["buckets"] == [(3, 15, [5, 0, 0, 0, 4, 0]), (7, 9, [0, 0, 0, 1, 2, 3])] and f["sum_other_doc_count"] == 3
    assert B.terms_hist_finalize(m, size=10, min_doc_count=2, order=B.TERMS_KEY_DESC)["buckets"] == \
        [(7, 9, [0, 0, 0, 1, 2, 3]), (3, 15, [5, 0, 0, 0, 4, 0])]
    # the terms half of the merge is merge_terms'
    flat = B.merge_terms([(p[0], p[1], p[3]) for p in (a, b, c)])
    assert {k: v[0] for k, v in m["entries"].items()} == flat["entries"]


def _info(lo, hi, gcd=1, rows=10):
    return {"min_value": lo, "max_value": hi, "gcd": gcd, "num_rows": rows}


def test_the_plan_and_its_refusals(B):
    h1 = {"interval": 1.0}
    # the grid's arithmetic: n_keys x (n_buckets + 1) at 65 536 and at 65 537
    for t, h, cells in ((_info(0, 255), _info(0, 254), 65536), (_info(10, 10 + 3 * 65535, 3), _info(5, 5, 1, 0), 65536),
                        (_info(0, 0), _info(0, 65534), 65536), (_info(0, 4095), _info(100, 114), 65536)):
        want = HM.plan(t, h, AM.U64, h1)
        assert B.agg_terms_hist_plan(t, h, AM.U64, h1) == want and want["n_cells"] == cells, (t, h)
    for t, h, nk, nb in ((_info(0, 256), _info(0, 254), 257, 255), (_info(0, 0), _info(0, 65535), 1, 65536),
                         (_info(0, 65535), _info(7, 7), 65536, 1), (_info(0, 4096), _info(100, 114), 4097, 15)):
        with pytest.raises(HM.Refused) as mi:
            HM.plan(t, h, AM.U64, h1)
        with pytest.raises(B.TantivyAmdError) as ei:
            B.agg_terms_hist_plan(t, h, AM.U64, h1)
        assert mi.value.kind == "unsupported" and ei.value.code == 4, (t, h)
        msg = str(ei.value)
        assert "tq_agg_terms_hist_plan" in msg and "n_keys = %d" % nk in msg and "n_buckets = %d" % nb in msg, msg
    assert nk * (nb + 1) == 65552 and 257 * 256 == 65792 and 1 * 65537 == 65537
    # n_buckets == 0 is served: bounds that hold no value, a histogram column without a row
    p = B.agg_terms_hist_plan(_info(3, 9, 3), _info(0, 100), AM.U64, {"interval": 1.0, "hard_bounds": (200.0, 300.0)})
    assert p == HM.plan(_info(3, 9, 3), _info(0, 100), AM.U64, {"interval": 1.0, "hard_bounds": (200.0, 300.0)})
    assert p["hist"]["n_buckets"] == 0 and p["terms"]["n_keys"] == 3 and p["n_cells"] == 3
    p = B.agg_terms_hist_plan(_info(3, 9, 3), _info(0, 0, 1, 0), AM.U64, h1)
    assert p["hist"]["n_buckets"] == 0 and p["n_cells"] == 3
    # n_keys == 0: a key column without a row
    p = B.agg_terms_hist_plan(_info(0, 0, 1, 0), _info(0, 100), AM.U64, h1)
    assert p == HM.plan(_info(0, 0, 1, 0), _info(0, 100), AM.U64, h1)
    assert p["terms"]["n_keys"] == 0 and p["hist"]["n_buckets"] == 101 and p["n_cells"] == 0
    # non-binding hard bounds drop out; the plans are the two existing calls' plans
    p = B.agg_terms_hist_plan(_info(0, 2), _info(0, 19), AM.U64, {"interval": 1.0, "hard_bounds": (-0.5, 19.5)})
    assert p["hist"] == B.agg_histogram_plan(_info(0, 19), AM.U64, 1.0, 0.0, (-0.5, 19.5)) and p["terms"] == B.agg_terms_plan(_info(0, 2))
    assert p["hist"]["bounds_max"] == AM.F64_MAX and p["n_cells"] == 3 * 21
    # every refusal: the code, and this function's name
    t, h = _info(0, 5), _info(0, 50)
    invalid = [({"segment_size": 0}, "segment_size"), ({"segment_size": 1025}, "segment_size"), ({"order": 4}, "order"),
               ({"reserved": (1, 0)}, "reserved"), ({"reserved": (0, 1)}, "reserved"), ({"histogram_flag": 0}, "histogram"),
               ({"histogram_flag": 2}, "histogram"), ({"histogram": {"interval": 0.0}}, "interval"),
               ({"histogram": {"interval": float("nan")}}, "interval"), ({"histogram": {"interval": 1.0, "offset": float("inf")}}, "offset"),
               ({"histogram": {"interval": 1.0, "hard_bounds": (3.0, 2.0)}}, "hard_m"),
               ({"histogram": {"interval": 1.0, "hard_bounds": (0.0, float("inf"))}}, "hard bounds"), ({"value_type": 3}, "value_type")]
    for kw, word in invalid:
        args = {"value_type": AM.U64, "histogram": h1}
        args.update(kw)
        with pytest.raises(HM.Refused) as mi:
            HM.plan(t, h, args.pop("value_type"), args.pop("histogram"), **args)
        args = {"value_type": AM.U64, "histogram": h1}
        args.update(kw)
        with pytest.raises(B.TantivyAmdError) as ei:
            B.agg_terms_hist_plan(t, h, args.pop("value_type"), args.pop("histogram"), **args)
        assert mi.value.kind == "invalid" and ei.value.code == 1, kw
        assert "tq_agg_terms_hist_plan:" in str(ei.value) and word in str(ei.value), (kw, str(ei.value))
    unsupported = [((_info(0, 65536), h), "n_keys"), ((t, _info(0, 70000)), "buckets"), ((_info(0, M64), h), "n_keys")]
    for (ti, hi), word in unsupported:
        with pytest.raises(HM.Refused) as mi:
            HM.plan(ti, hi, AM.U64, h1)
        with pytest.raises(B.TantivyAmdError) as ei:
            B.agg_terms_hist_plan(ti, hi, AM.U64, h1)
        assert mi.value.kind == "unsupported" and ei.value.code == 4
        assert "tq_agg_terms_hist_plan:" in str(ei.value) and word in str(ei.value), str(ei.value)
    with pytest.raises(B.TantivyAmdError) as ei:
        B.agg_terms_hist_plan(_info(5, 4), h, AM.U64, h1)  # (a column whose max is below its min)
    assert ei.value.code == 1 and "tq_agg_terms_hist_plan:" in str(ei.value)
    # a refused plan is all zeros
    L = B.lib()
    req = B._agg_terms_hist_request(0, 0, AM.U64, h1, 0, 10)
    plan = B.TqAggTermsHistPlan()
    C.memset(C.byref(plan), 0xFF, C.sizeof(plan))
    ct, ch = B.TqColumnInfo(**_info(0, 65535)), B.TqColumnInfo(**_info(0, 1))
    assert L.tq_agg_terms_hist_plan(C.byref(ct), C.byref(ch), C.byref(req), C.byref(plan)) == 4
    assert bytes(plan) == bytes(C.sizeof(plan))


def _header():
    return open(os.path.join(ROOT, "include", "tantivy_amd.h")).read()


def test_header_declares_the_feature_and_the_binding_agrees(B):
    from tantivy_amd import build

    src = _header()
    masks = {name: int(v, 16) for name, v in re.findall(r"#define\s+(TQ_KERNEL_[A-Z_]+)\s+(0x[0-9a-fA-F]+)u", src)}
    assert B.KERNEL_AGG_TERMS_HIST == masks["TQ_KERNEL_AGG_TERMS_HIST"] == 0x2000000 == 2 * masks["TQ_KERNEL_AGG_RANGE"]
    assert masks["TQ_KERNEL_AGG_TERMS_HIST"] not in [v for n, v in masks.items() if n != "TQ_KERNEL_AGG_TERMS_HIST"]
    assert B.kernel_names(B.KERNEL_AGG_TERMS_HIST) == ["agg_terms_hist"] and sorted(B.KERNEL_NAMES) == sorted(masks.values())
    assert C.sizeof(B.TqAggTermsHistRequest) == 56 and C.sizeof(B.TqAggTermsHistPlan) == 64
    assert re.search(r"\}\s*tq_agg_terms_hist_request\s*;\s*/\* 56 bytes \*/", src)
    assert re.search(r"\}\s*tq_agg_terms_hist_plan_t\s*;\s*/\* 64 bytes \*/", src)
    assert B.TqAggTermsHistRequest.hist.offset == 16 and B.TqAggTermsHistPlan.hist.offset == 24 and B.TqAggTermsHistPlan.n_cells.offset == 56
    assert HM.MAX_CELLS == B.AGG_MAX_BUCKETS == 65536
    for k in ("agg_terms_hist_count_kernel", "agg_terms_hist_rowsum_kernel", "agg_terms_hist_gather_kernel", "agg_terms_hist_init_kernel"):
        assert build.KERNEL_FILES[k] == "tq_agg_terms_hist.hip", k
    assert "tq_agg_terms_hist.hip" in build.WALK_FILES
    names = [os.path.basename(p) for p in build.SOURCES]
    assert "tq_agg_terms_hist.hip" in names and "tq_agg_terms_hist.cpp" in names
    assert all(os.path.exists(p) for p in build.SOURCES)
    # the kernel file is made of the shared parts, not of copies of them
    hip = open(os.path.join(ROOT, "tantivy_amd", "csrc", "tq_agg_terms_hist.hip")).read()
    for part in ("docset_walk(", "col_key_index(", "col_value(", "tq_agg_f64(", "tq_agg_sat_i64(", "rg_row<"):
        assert part in hip, part
    cpp = open(os.path.join(ROOT, "tantivy_amd", "csrc", "tq_agg_terms_hist.cpp")).read()
    assert "tqk_launch_agg_terms_select(" in cpp and "agg_terms_plan_checked(" in cpp and "agg_histogram_plan_checked(" in cpp


def test_library_exports_the_entry_points(B):
    L = B.lib()
    declared = set(re.findall(r"\b(tq_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for name in ("tq_agg_terms_hist_plan", "tq_agg_terms_hist_batch", "tq_agg_terms_hist_batch_device", "tq_agg_terms_hist_lds_capacities"):
        assert name in declared and name in B.EXPORTS and hasattr(L, name), name
    # null arguments are errors, not crashes; the message names the function
    assert L.tq_agg_terms_hist_batch(None, None, 1, None, None, None, None, None, 0, 0) != 0
    assert b"tq_agg_terms_hist_batch:" in L.tq_last_error()
    assert L.tq_agg_terms_hist_batch_device(None, None, 1, None, None, None, None, None, 0, 0, None) != 0
    assert b"tq_agg_terms_hist_batch_device:" in L.tq_last_error()
    assert L.tq_agg_terms_hist_plan(None, None, None, None) != 0 and b"tq_agg_terms_hist_plan:" in L.tq_last_error()
    small, large = B.agg_terms_hist_lds_capacities()
    assert (small, large) == B.agg_terms_lds_capacities()  # (the terms kernel's capacities: same entry size, same walk)
    assert 16 < small < large and 4 * large + 16640 <= 65536  # (the table beside the slabs in the static 64 KB)
