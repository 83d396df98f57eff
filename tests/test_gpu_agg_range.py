"""GPU parity of the range aggregation (tq_agg_range_batch*: tantivy_amd/csrc/tq_agg_range.cpp, tq_agg_range.hip — doc counts
per range of a bucket column A and, with a metric, the stats of a column B per range, per query of a batch).

Expectations never come from the device: the column bytes are written by tests/column_model.py from values the test
chose, the match sets come from the oracle's decode / tests/all_model.py / tests/slop_model.py, the buckets are
tests/range_agg_model.plan and the record, the row of counts and the bucket records are range_agg_model.expected_range —
exact integers that tests/test_agg_range_model_cpu.py ties to the reference's collect.  Every comparison is exact (there is
no tolerance in this file).  Segments, columns and queries are those of tests/test_gpu_agg.py, by import."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import agg_model as GM
from tests import all_model as AM
from tests import column_model as CM
from tests import phrase_model as PM
from tests import range_agg_model as RM
from tests.test_column_model_cpu import bitpacked_values
from tests.test_gpu_agg import (EVENS, FIELDS, AggLists, _edge_columns, _err, _typed_columns, _walk_queries, _walk_segment, small,
                                ta)  # noqa: F401 (ta, small: fixtures)
from tests.test_gpu_agg_sub import _assert_records
from tests.test_gpu_all import STAR, T, _flat, _model_clauses
from tests.test_gpu_docset import ERR_INVALID, ERR_UNSUPPORTED
from tests.test_gpu_range import _query_columns, _upload
from tests.test_gpu_round3 import _alive_bytes
from tests.test_gpu_sort import EDGE_COLUMNS
from tests.test_gpu_term_set import _prepare_all_terms, _synth_segment
from tests.tree_shapes import to_device

pytestmark = pytest.mark.gpu

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
TOP = RM.TOP


def _assert_range(got, want, plan, where):
    """got = (stats, counts, bucket_stats | None, plan) of raw_agg_range; want = [(record, counts, records | None)] of
    RM.expected_range; plan = the model's buckets."""
    stats, rows, recs, got_plan = got
    assert got_plan == plan, (where, got_plan[:4], plan[:4])
    assert len(stats) == len(rows) == len(want) and rows.shape == (len(want), len(plan)), (where, rows.shape)
    for i, (rec, counts, _) in enumerate(want):
        g = {k: int(stats[i][k]) for k in FIELDS}
        assert g == rec, (where, i, g, rec)
        assert g["out_of_range"] == 0 and g["in_bounds"] == g["count"] == sum(counts)
        bad = np.nonzero(rows[i] != np.array(counts, np.uint32))[0]
        assert bad.size == 0, (where, "query", i, "bucket", int(bad[0]), int(rows[i][bad[0]]), counts[bad[0]])
    if want and want[0][2] is not None:
        _assert_records(recs, [w[2] for w in want], where)
    else:
        assert recs is None


def _cut(values, n, rng=None):
    """n user ranges through a column's u64 values as f64 bounds of a U64 column: quantiles of the distinct values, every
    second range followed by a hole, unsorted when rng is given.  (A constant or empty column: one range around 0.)"""
    d = np.unique(np.asarray(values, np.uint64))
    if d.size < 2:
        return [(1.0, 50.0)]
    qs = [float(int(d[int(i * (d.size - 1) / (2 * n))])) for i in range(2 * n + 1)]
    out = [(qs[2 * i], qs[2 * i + 1] if i % 2 else qs[2 * i + 2]) for i in range(n)]
    out = [(lo, hi) for lo, hi in out if lo <= hi]
    return [out[i] for i in rng.permutation(len(out))] if rng is not None else out


def _uniform_ranges(n_buckets, width=8.0):
    """n_buckets buckets over a 13-bit U64 column: adjacent ranges `width` wide from 0, the last one open"""
    if n_buckets == 1:
        return [(None, None)]
    return [(width * i, width * (i + 1)) for i in range(n_buckets - 1)] + [(width * (n_buckets - 1), None)]


# ---- 1. the walk and the readers of A and B at their edges
@pytest.mark.parametrize("column", EDGE_COLUMNS)
def test_walk_and_readers_at_the_edges(ta, column):
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    codec, vals, present = _edge_columns(md)[column]
    a_model = GM.Column(vals, present, md)
    ranges = _cut(vals, 6, np.random.default_rng(1))
    plan = RM.plan(GM.U64, ranges)
    b_vals = bitpacked_values(np.random.default_rng(2), md, 33, 7, 3)
    b_model = GM.Column(b_vals, None, md)
    queries = _walk_queries(ta, sparse)
    batch = [q for q, _ in queries]
    want = [RM.expected_range(m, a_model, plan) for _, m in queries]
    want_m = [RM.expected_range(m, a_model, plan, b_model, GM.U64) for _, m in queries]
    assert want[2][1] == [0] * len(plan) and all(r == RM.empty_record() for r in want_m[2][2])
    if column == "bitpacked 13 bits":
        assert len(plan) >= 8 and sum(1 for c in want[0][1] if c) >= 6  # (the ranges do cut through the values)
    if column == "bitpacked 64 bits":
        assert want[0][1][-1] >= 1  # (2^64 - 1 lands in the last bucket)
    if column == "optional bitpacked none":
        assert want[0][0]["count"] == 0 and want[0][0]["matches"] == md
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        _, col = _upload(dev, codec, vals, present)
        col_b = dev.add_column(CM.write_bitpacked(b_vals))
        for slices in (1, 3, 256, 0):
            dev.set_option("agg_slices", slices)
            _assert_range(dev.raw_agg_range(batch, col, B.VALUE_U64, ranges), want, plan, (column, "counts", slices))
            assert dev.last_batch_match_counts(len(batch)).tolist() == [m.size for _, m in queries]
            _assert_range(dev.raw_agg_range(batch, col, B.VALUE_U64, ranges, col_b, B.VALUE_U64), want_m, plan, (column, "metric", slices))
    finally:
        dev.close()


# ---- 2. boundaries
def test_boundaries_holes_and_an_empty_range(ta):
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    # unsorted; holes [50, 100), [300, 1000); both outer buckets; 10.2 .. 10.9 is the empty range [10, 10) beside [10, 50)
    # (the empty range stands in front of the range that shares its start: the sort is stable, and the other way round the
    # pair is refused as overlapping — by the reference too)
    ranges = [(100.0, 300.0), (5.0, 10.2), (1000.0, 2.0 ** 63), (10.2, 10.9), (10.9, 50.0)]
    plan = RM.plan(GM.U64, ranges)
    assert [(b["start"], b["end"], b["source"]) for b in plan] == [
        (0, 5, None), (5, 10, 1), (10, 10, 3), (10, 50, 4), (50, 100, None), (100, 300, 0), (300, 1000, None), (1000, 1 << 63, 2),
        (1 << 63, TOP, None)]
    edge = sorted({x for b in plan for x in (max(b["start"] - 1, 0), b["start"], max(b["end"] - 1, 0))} | {0, TOP, TOP - 1})
    rng = np.random.default_rng(12)
    vals = rng.integers(0, 1200, size=md).astype(np.uint64)
    vals[: len(edge)] = np.array(edge, np.uint64)          # docs 0 .. : one per boundary value (`*` sees them all)
    vals[sparse[: len(edge)]] = np.array(edge, np.uint64)  # ... and again under the sparse term
    a_model = GM.Column(vals, None, md)
    b_model = GM.Column(np.arange(md, dtype=np.uint64) * np.uint64(3), None, md)
    queries = _walk_queries(ta, sparse)[:2]
    want = [RM.expected_range(m, a_model, plan) for _, m in queries]
    want_m = [RM.expected_range(m, a_model, plan, b_model, GM.U64) for _, m in queries]
    for w in want:
        assert w[1][2] == 0 and all(c > 0 for i, c in enumerate(w[1]) if i != 2)  # the empty range alone counts 0
        assert w[1][-1] >= 3  # 2^63, 2^64 - 2 and 2^64 - 1: the last lands in the last bucket
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        col = dev.add_column(CM.write_bitpacked(vals))
        col_b = dev.add_column(CM.write_bitpacked(b_model.u64))
        batch = [q for q, _ in queries]
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_range(dev.raw_agg_range(batch, col, B.VALUE_U64, ranges), want, plan, ("boundaries", slices))
            _assert_range(dev.raw_agg_range(batch, col, B.VALUE_U64, ranges, col_b, B.VALUE_U64), want_m, plan, ("boundaries, metric", slices))
    finally:
        dev.close()


# ---- 3. value types
TYPED_RANGES = {
    "i64 straddling zero": [(-5000.0, -100.5), (-100.5, 0.0), (0.0, 1.0), (250.0, None)],
    "f64 with infinities and a nan": [(-math.inf, -2.5), (-2.5, 0.0), (0.0, 12.5), (50.0, math.inf)],
    "date-like nanoseconds": [(1.7e18, 1.7e18 + 3.6e12), (1.7e18 + 3.6e12, 1.7e18 + 4.0e13), (1.7e18 + 8.0e13, None)],
    "fractional bounds on u64": [(0.5, 2.5), (2.5, 2.75), (2.75, 100.9)],
}


@pytest.mark.parametrize("which", sorted(TYPED_RANGES))
def test_value_types(ta, which):
    seg, sparse = _walk_segment()
    md = seg.max_doc
    typed = _typed_columns(md)
    if which == "fractional bounds on u64":
        vt_a, a_vals = GM.U64, np.random.default_rng(4).integers(0, 120, size=md).astype(np.uint64)
        vt_b, b_vals, _ = typed["i64 straddling zero"]  # a metric of another type than A
    else:
        vt_a, a_vals, _ = typed[which]
        vt_b, b_vals, _ = typed["f64 with infinities and a nan" if which.startswith("i64") else "i64 straddling zero"]
    ranges = TYPED_RANGES[which]
    plan = RM.plan(vt_a, ranges)
    a_model, b_model = GM.Column(a_vals, None, md), GM.Column(b_vals, None, md)
    queries = _walk_queries(ta, sparse)[:2] + [((O.MODE_OR, [EVENS]), np.arange(0, md, 2, dtype=np.uint32))]
    want = [RM.expected_range(m, a_model, plan, b_model, vt_b, vt_a=vt_a) for _, m in queries]
    star = want[0]
    if which == "i64 straddling zero":  # docs 0..3 hold -5000, -1, 0, 4999
        assert [b["source"] for b in plan] == [None, 0, 1, 2, None, 3] and all(star[1][1:])
        assert star[1][0] == 0 and star[1][3] == int((GM.f64_array(a_vals, vt_a) == 0.0).sum())  # [0, 1) holds the zeros alone
        assert all(r["sum_lo"] == r["sum_hi"] == 0 for r in star[2])  # (an F64 metric: no sums)
    elif which == "f64 with infinities and a nan":
        # docs 4, 5, 6 hold inf, -inf and a NaN; the positive NaN sits above +inf in the mapped order: the last bucket
        # [inf, MAX) holds inf and the NaN, the first [0, -inf) nothing, [-inf, -2.5) the -inf
        assert plan[0]["source"] is None and plan[-1]["source"] is None and plan[-1]["start"] == GM.to_u64(math.inf, GM.F64)
        assert star[1][0] == 0 and star[1][-1] == 2 and star[0]["sum_lo"] == star[0]["sum_hi"] == 0
        # docs 0 and 1 hold 0.0 and -0.0: the bound 0.0 parts them, as the mapped order does
        assert RM.bucket_of(RM.starts_of(plan), int(a_vals[0])) == 3 and RM.bucket_of(RM.starts_of(plan), int(a_vals[1])) == 2
    elif which == "date-like nanoseconds":
        assert len(plan) == 5 and all(star[1][1:]) and star[1][0] == 0
    else:
        assert [(b["start"], b["end"]) for b in plan] == [(0, 2), (2, 2), (2, 100), (100, TOP)]
        assert star[1][1] == 0 and star[1][0] > 0 and star[1][2] > 0 and star[1][3] > 0
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        col_a = dev.add_column(CM.write_bitpacked(a_vals))
        col_b = dev.add_column(CM.write_bitpacked(b_vals))
        got = dev.raw_agg_range([q for q, _ in queries], col_a, vt_a, ranges, col_b, vt_b)
        _assert_range(got, want, plan, which)
        _assert_range(dev.raw_agg_range([q for q, _ in queries], col_a, vt_a, ranges), [(w[0], w[1], None) for w in want], plan, which)
    finally:
        dev.close()


# ---- 4. table sizes
SIZE_CASES = ["1", "2", "3", "64", "65", "small", "small + 1", "large", "large + 1", "1024"]


def _size_of(case, caps):
    # (one past a capacity that is the most buckets a plan can have: that many)
    return {"small": caps[0], "small + 1": caps[0] + 1, "large": caps[1], "large + 1": min(caps[1] + 1, RM.MAX_BUCKETS)}.get(case) or int(case)


@pytest.mark.parametrize("lds_buckets", [None, 16])
@pytest.mark.parametrize("case", SIZE_CASES)
def test_table_sizes(ta, case, lds_buckets):
    """n_buckets at and one past each capacity of the record table, at 1 024 (every start and every record in LDS), and small
    counts; each with "agg_lds_buckets" at its default and at 16 (every row above 16 buckets goes straight to the row and
    the records: the global path)."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    caps = B.agg_range_lds_capacities()
    assert 16 < caps[0] < caps[1] <= RM.MAX_BUCKETS
    n_buckets = _size_of(case, caps)
    ranges = _uniform_ranges(n_buckets)
    plan = RM.plan(GM.U64, ranges)
    assert len(plan) == n_buckets
    rng = np.random.default_rng(5)
    a_model = GM.Column(bitpacked_values(rng, md, 13, 0, 1), None, md)
    has_b = rng.random(md) < 0.6
    b_model = GM.Column(bitpacked_values(rng, int(has_b.sum()), 33, 7, 3), has_b, md)
    queries = _walk_queries(ta, sparse)
    want = [RM.expected_range(m, a_model, plan) for _, m in queries]
    want_m = [RM.expected_range(m, a_model, plan, b_model, GM.U64) for _, m in queries]
    assert want[0][1][-1] > 0 and (n_buckets < 3 or want[0][1][n_buckets // 2] > 0)
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        col_a = dev.add_column(CM.write_bitpacked(a_model.u64))
        _, col_b = _upload(dev, CM.BITPACKED, b_model.u64[has_b], has_b)
        if lds_buckets is not None:
            dev.set_option("agg_lds_buckets", lds_buckets)
        batch = [q for q, _ in queries]
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_range(dev.raw_agg_range(batch, col_a, GM.U64, ranges), want, plan, (case, lds_buckets, slices, "counts"))
            _assert_range(dev.raw_agg_range(batch, col_a, GM.U64, ranges, col_b, GM.U64), want_m, plan, (case, lds_buckets, slices, "metric"))
    finally:
        dev.close()


# ---- 5. presence
def test_presence_of_both_columns_and_the_same_column_twice(ta):
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    rng = np.random.default_rng(52)
    has_a, has_b = rng.random(md) < 0.7, rng.random(md) < 0.5
    a_model = GM.Column(rng.integers(0, 60, size=int(has_a.sum())).astype(np.uint64), has_a, md)
    b_model = GM.Column(bitpacked_values(rng, int(has_b.sum()), 13, 1 << 40, 1000), has_b, md)
    ranges = [(10.0, 20.0), (20.0, 45.0)]
    plan = RM.plan(GM.U64, ranges)
    assert len(plan) == 4
    queries = _walk_queries(ta, sparse)[:2]
    for _, m in queries:
        assert {(bool(has_a[d]), bool(has_b[d])) for d in m.tolist()} == {(False, False), (False, True), (True, False), (True, True)}
    want = [RM.expected_range(m, a_model, plan, b_model, GM.U64) for _, m in queries]
    assert all(0 < sum(r["count"] for r in w[2]) < w[0]["count"] < w[0]["matches"] for w in want)
    same = [RM.expected_range(m, a_model, plan, a_model, GM.U64) for _, m in queries]
    assert all([r["count"] for r in w[2]] == w[1] and w[2][1]["min_value"] >= 10 and w[2][1]["max_value"] < 20 for w in same)
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        _, col_a = _upload(dev, CM.BITPACKED, a_model.u64[has_a], has_a)
        _, col_b = _upload(dev, CM.BITPACKED, b_model.u64[has_b], has_b)
        full_b = dev.add_column(CM.write_bitpacked(b_model.u64))  # (the values of B with a zero where it has none: a Full column)
        fb_model = GM.Column(b_model.u64, None, md)
        full_a = dev.add_column(CM.write_bitpacked(a_model.u64))
        fa_model = GM.Column(a_model.u64, None, md)
        batch = [q for q, _ in queries]
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_range(dev.raw_agg_range(batch, col_a, B.VALUE_U64, ranges, col_b, B.VALUE_U64), want, plan, ("optional A, optional B", slices))
            _assert_range(dev.raw_agg_range(batch, col_a, B.VALUE_U64, ranges, full_b, B.VALUE_U64),
                          [RM.expected_range(m, a_model, plan, fb_model, GM.U64) for _, m in queries], plan, ("optional A, full B", slices))
            _assert_range(dev.raw_agg_range(batch, full_a, B.VALUE_U64, ranges, col_b, B.VALUE_U64),
                          [RM.expected_range(m, fa_model, plan, b_model, GM.U64) for _, m in queries], plan, ("full A, optional B", slices))
            _assert_range(dev.raw_agg_range(batch, col_a, B.VALUE_U64, ranges, col_a, B.VALUE_U64), same, plan, ("B == A", slices))
    finally:
        dev.close()


# ---- 6. query shapes against the models
@pytest.mark.parametrize("with_deletes", [False, True])
def test_query_shapes_against_the_model(ta, with_deletes):
    seg = _synth_segment()
    md = seg.max_doc
    cols = _query_columns(md)
    codec, vals, _ = cols["full bitpacked"]
    b_codec, b_vals, b_present = cols["optional blockwise"]
    by_df = sorted(range(len(seg.terms)), key=lambda t: seg.terms[t].doc_freq)
    a, b = by_df[len(by_df) // 2], by_df[-3]
    B = ta.binding
    alive = None
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        if with_deletes:
            deleted = np.random.default_rng(11).choice(md, size=md // 6, replace=False)
            alive = np.ones(md, bool)
            alive[deleted] = False
            dev.set_alive_bitset(_alive_bytes(md, deleted.tolist()))
        blob, col = _upload(dev, codec, vals, None)
        _, col_b = _upload(dev, b_codec, b_vals, b_present)
        h = CM.read_header(blob)
        srt = np.sort(vals)
        q1, q3 = int(srt[vals.size // 4]), int(srt[3 * vals.size // 4])
        L = AggLists(seg)

        def new_range(lower, upper):
            kind, mask, weight = CM.expected_range(vals, None, lower, upper, 1.0)
            got, got_w = dev.range_prepare(col, lower, upper, 1.0)
            assert kind == "set" and isinstance(got, B.RawHandle)
            return L.add_range(got, mask, got_w)

        r = new_range(("in", q1), ("ex", q3))
        r_empty = new_range(("in", h["max_value"]), ("ex", h["max_value"]))
        for t in (a, b):
            L.need(t)
        cases = [
            ([(M, T(a)), (M, T(b))], 0),        # flat AND
            ([(S, T(a)), (S, T(b))], 0),        # flat OR
            ([(M, T(a)), (M, T(r))], 0),        # +a +range, bucketing the range's own column
            ([(M, STAR), (N, T(r))], 0),        # * -range
            ([(M, T(a)), (M, T(r_empty))], 0),  # the empty result
        ]
        match = [AM.expect(_model_clauses(cl, L), m, L.lists, md, alive)[0].astype(np.uint32) for cl, m in cases]
        assert match[4].size == 0 and all(match[i].size for i in range(4))
        a_model, b_model = GM.Column(vals, None, md), GM.Column(b_vals, b_present, md)
        # the clause's own range [q1, q3) as one bucket, a band below it and one above
        ranges = [(float(q1), float(q3)), (float(h["min_value"]), float(q1)), (float(q3), float(q3 + (h["max_value"] - q3) // 2))]
        plan = RM.plan(GM.U64, ranges)
        assert float(q3) < 2.0 ** 53 and [bk["source"] for bk in plan] == [None, 1, 0, 2, None]
        want = [RM.expected_range(m, a_model, plan, b_model, GM.U64) for m in match]
        batch = [_flat(ta, cl, m) for cl, m in cases]
        _assert_range(dev.raw_agg_range(batch, col, B.VALUE_U64, ranges, col_b, B.VALUE_U64), want, plan, with_deletes)
        assert dev.last_batch_match_counts(len(batch)).tolist() == [m.size for m in match]
        _assert_range(dev.raw_agg_range(batch, col, B.VALUE_U64, ranges), [(w[0], w[1], None) for w in want], plan, with_deletes)
        # the range clause as seen through the rows: +a +range fills bucket 2 alone, * -range leaves it empty
        assert want[2][1][2] == match[2].size > 0 and want[3][1][2] == 0 and want[3][2][2] == RM.empty_record()
    finally:
        dev.close()


# ---- 7. trees
def test_trees_take_the_docset_option(ta):
    """A phrase, a sloppy phrase and a nested query: refused without "docset_trees" naming the first such query, exact with it."""
    from tests.test_gpu_phrase_slop import _expect as slop_expect

    corp = PM.corpus("P")
    seg = corp.segment()
    md = corp.max_doc
    assert corp.alive is None
    B = ta.binding
    rng = np.random.default_rng(8)
    vals = bitpacked_values(rng, md, 13, 1 << 40, 1000)
    b_vals = bitpacked_values(rng, md, 20, 0, 1)
    _, terms, offs = corp.queries[0]
    e = slop_expect(corp, 0, 1)
    assert e.longest <= B.SLOP_CARRY_CAP
    spec = [(M, 2), (M, [(S, [0, 1]), (S, 3)], 0)]  # +c +((+a +b) d)
    flat_q = (O.MODE_OR, [4])
    queries = [flat_q, (O.MODE_PHRASE, list(terms), list(offs)), (O.MODE_PHRASE, list(terms), list(offs), 1), to_device(ta, spec, 0),
               flat_q]
    match = [O.decode_postings(seg, 4)[0].astype(np.uint32),
             np.sort(O.match_all(seg, list(terms), O.MODE_PHRASE, phrase_offsets=list(offs))[0]).astype(np.uint32),
             np.asarray(e.exists_docs, np.uint32), np.asarray(O.tree_match_all(seg, spec, 0)[0], np.uint32),
             O.decode_postings(seg, 4)[0].astype(np.uint32)]
    assert all(m.size for m in match)
    a_model, b_model = GM.Column(vals, None, md), GM.Column(b_vals, None, md)
    ranges = _cut(vals, 5)
    plan = RM.plan(GM.U64, ranges)
    want = [RM.expected_range(m, a_model, plan, b_model, GM.U64) for m in match]
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_budget_x", 256)
        _prepare_all_terms(dev, seg)
        col = dev.add_column(CM.write_bitpacked(vals))
        col_b = dev.add_column(CM.write_bitpacked(b_vals))
        with pytest.raises(ta.TantivyAmdError) as ei:
            dev.raw_agg_range(queries, col, B.VALUE_U64, ranges, col_b, B.VALUE_U64)
        assert ei.value.code == ERR_UNSUPPORTED and "query 1" in str(ei.value) and "tq_agg_range_batch" in str(ei.value)
        dev.set_option("docset_trees", 1)
        _assert_range(dev.raw_agg_range(queries, col, B.VALUE_U64, ranges, col_b, B.VALUE_U64), want, plan, "trees")
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == B.KERNEL_AGG_RANGE | B.KERNEL_DOCSET_TREE | B.KERNEL_PHRASE_SLOP, st
        assert int(dev.last_batch_slop_overflows(len(queries)).sum()) == 0
    finally:
        dev.close()


# ---- 8. sub-batches
def test_sub_batches_keep_the_callers_index(ta):
    """"docset_temp_lists" = 16: a batch that names 40 distinct lists without a bitmap runs as three sub-batches."""
    seg = _synth_segment()
    md = seg.max_doc
    rng = np.random.default_rng(9)
    vals = bitpacked_values(rng, md, 13, 1 << 40, 1000)
    b_vals = bitpacked_values(rng, md, 20, 0, 1)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 2)  # a bitmap only for the lists that hold half of the docs
        _prepare_all_terms(dev, seg)
        bare = [t for t in range(len(seg.terms)) if dev.term_table(dev.term_handle(t), "dense").size == 0]
        assert len(bare) >= 40
        bare = bare[:40]
        dev.set_option("docset_temp_lists", 16)
        assert -(-len(bare) // 16) == 3  # one fresh list per query, 16 slots per sub-batch
        col = dev.add_column(CM.write_bitpacked(vals))
        col_b = dev.add_column(CM.write_bitpacked(b_vals))
        queries = [(O.MODE_OR, [t]) for t in bare]
        match = [O.decode_postings(seg, t)[0].astype(np.uint32) for t in bare]
        a_model, b_model = GM.Column(vals, None, md), GM.Column(b_vals, None, md)
        ranges = _cut(vals, 7)
        plan = RM.plan(GM.U64, ranges)
        want = [RM.expected_range(m, a_model, plan, b_model, GM.U64) for m in match]
        # (a row under another query's index would show: every query's records differ)
        assert len({tuple(r["sum_lo"] for r in w[2]) for w in want}) == len(want)
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_range(dev.raw_agg_range(queries, col, ta.binding.VALUE_U64, ranges, col_b, ta.binding.VALUE_U64), want, plan,
                          ("sub-batches", slices))
            assert dev.last_batch_match_counts(len(bare)).tolist() == [m.size for m in match]
    finally:
        dev.close()


# ---- 9. device outputs; 10. refusals; 11. the byte model and the mask
def test_device_rows_strides_and_guards(ta, small):
    import torch

    dev, queries, match, model, omodel = small["dev"], small["queries"], small["match"], small["model"], small["omodel"]
    B = ta.binding
    n = len(queries)
    ranges = _cut(model.u64, 6)
    plan = RM.plan(GM.U64, ranges)
    nb = len(plan)
    stride = nb + 7
    want = [RM.expected_range(m, model, plan, omodel, GM.U64) for m in match]
    plain = [(w[0], w[1], None) for w in want]
    args = (queries, small["col"], B.VALUE_U64, ranges, small["ocol"], B.VALUE_U64)
    _assert_range(dev.raw_agg_range(*args, stride=stride), want, plan, "host rows, a wider stride")
    _assert_range(dev.raw_agg_range(*args, stride=stride, device=True), want, plan, "device rows")
    _assert_range(dev.raw_agg_range(*args[:4], stride=stride, device=True), plain, plan, "device rows, counts alone")
    # two rows of each kind and two records more than the batch has queries; everything pre-filled
    fill = 0x5A5A5A5A5A5A5A5A
    d_stats = torch.full(((n + 2) * 8,), fill, dtype=torch.int64, device="cuda:0")
    d_rows = torch.full(((n + 2) * stride,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    d_recs = torch.full(((n + 2) * stride * 5,), fill, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    seen = []
    for call in (0, 1):  # the second call accumulates into the same buffers: the call zeroes what it adds to
        rc = dev.raw_agg_range_device(*args, stride, d_stats, d_rows, d_recs)
        assert rc == 0, _err(ta)
        dev.last_batch_stats()  # (waits for the batch)
        torch.cuda.synchronize()
        stats = d_stats.cpu().numpy().view(np.uint64)
        rows = d_rows.cpu().numpy().view(np.uint32).reshape(n + 2, stride)
        recs = d_recs.cpu().numpy().view(np.uint64).reshape(n + 2, stride, 5)
        got_recs = np.ascontiguousarray(recs[:n, :nb]).reshape(-1).view(B.AGG_BUCKET_STATS_DTYPE).reshape(n, nb)
        _assert_range((stats[: n * 8].view(B.AGG_STATS_DTYPE), rows[:n, :nb], got_recs, plan), want, plan, ("device buffers", call))
        assert np.all(rows[:n, nb:] == 0x5A5A5A5A) and np.all(rows[n:] == 0x5A5A5A5A)
        assert np.all(recs[:n, nb:] == fill) and np.all(recs[n:] == fill)
        assert np.all(stats[n * 8:] == fill)
        seen.append((stats.tobytes(), rows.tobytes(), recs.tobytes()))
    assert seen[0] == seen[1]  # two identical calls: identical bytes
    # counts alone: the records' buffer is not touched at all
    d_recs.fill_(0x77)
    rc = dev.raw_agg_range_device(*args[:4], None, None, stride, d_stats, d_rows, None)
    assert rc == 0, _err(ta)
    dev.last_batch_stats()
    torch.cuda.synchronize()
    rows = d_rows.cpu().numpy().view(np.uint32).reshape(n + 2, stride)
    assert [rows[i, :nb].tolist() for i in range(n)] == [w[1] for w in want] and np.all(rows[:n, nb:] == 0x5A5A5A5A)
    assert np.all(d_recs.cpu().numpy() == 0x77)


def test_refusals_leave_the_segment_usable(ta, small):
    import torch

    dev, queries, match, col, ocol = small["dev"], small["queries"], small["match"], small["col"], small["ocol"]
    model, omodel = small["model"], small["omodel"]
    B = ta.binding
    ranges = _cut(model.u64, 3)
    plan = RM.plan(GM.U64, ranges)
    nb = len(plan)
    want = [RM.expected_range(match[0], model, plan, omodel, GM.U64)]

    def still_good():
        _assert_range(dev.raw_agg_range(queries[:1], col, B.VALUE_U64, ranges, ocol, B.VALUE_U64), want, plan, "after a refusal")
        rc, docs, starts = dev.raw_docset(queries[:1], match[0].size)
        assert rc == 0 and np.array_equal(docs[: int(starts[1])], match[0]), _err(ta)

    def refused(call, code, *words):
        with pytest.raises(ta.TantivyAmdError) as ei:
            call()
        assert ei.value.code == code and all(w in str(ei.value) for w in words), ei.value
        still_good()

    still_good()
    fn = "tq_agg_range_batch"
    # what the plan refuses, under this function's name
    refused(lambda: dev.raw_agg_range(queries, col, 0, []), ERR_INVALID, fn, "n_ranges")
    refused(lambda: dev.raw_agg_range(queries, col, 3, ranges), ERR_INVALID, fn, "value_type 3")
    refused(lambda: dev.raw_agg_range(queries, col, 0, [(1.0, math.nan)]), ERR_INVALID, fn, "NaN")
    refused(lambda: dev.raw_agg_range(queries, col, 0, [(0.0, 10.0), (5.0, 20.0)]), ERR_INVALID, fn, "overlapping ranges 0 and 1")
    refused(lambda: dev.raw_agg_range(queries, col, 0, [(10.0, 5.0)]), ERR_INVALID, fn, "range 0", "above its end")
    refused(lambda: dev.raw_agg_range(queries, col, 0, [(10.0 * (i + 1), 10.0 * (i + 1) + 7.0) for i in range(512)]), ERR_UNSUPPORTED, fn, "1025")
    # the call's own
    refused(lambda: dev.raw_agg_range(queries, 7, 0, ranges), ERR_INVALID, fn, "column 7")  # (no such upload)
    refused(lambda: dev.raw_agg_range(queries, B.MAX_COLUMNS, 0, ranges), ERR_INVALID, fn, "column")
    refused(lambda: dev.raw_agg_range(queries, col, 0, ranges, B.MAX_COLUMNS, 0), ERR_INVALID, fn, "metric column")
    refused(lambda: dev.raw_agg_range(queries, col, 0, ranges, 7, 0), ERR_INVALID, fn, "metric column")
    refused(lambda: dev.raw_agg_range(queries, col, 0, ranges, ocol, 3), ERR_INVALID, fn, "metric value_type")
    refused(lambda: dev.raw_agg_range(queries, col, 0, ranges, ocol, 0, stride=nb - 1), ERR_INVALID, fn, "bucket_stride")
    refused(lambda: dev.raw_agg_range(queries[:2] + [(O.MODE_PHRASE, [1, 2], [0, 1])], col, 0, ranges, ocol, 0), ERR_UNSUPPORTED, fn, "query 2")
    # null rows (the device variant takes the pointers as they are)
    n = len(queries)
    d_stats = torch.zeros(n * 8, dtype=torch.int64, device="cuda:0")
    d_rows = torch.zeros(n * nb, dtype=torch.int32, device="cuda:0")
    rc = dev.raw_agg_range_device(queries, col, 0, ranges, ocol, 0, nb, d_stats, d_rows, None)
    assert rc == ERR_INVALID and "tq_agg_range_batch_device" in _err(ta) and "null bucket records" in _err(ta)
    still_good()
    rc = dev.raw_agg_range_device(queries, col, 0, ranges, None, None, nb, d_stats, None, None)
    assert rc == ERR_INVALID and "tq_agg_range_batch_device" in _err(ta) and "null count rows" in _err(ta)
    still_good()
    # a column released after a successful call
    extra = dev.add_column(CM.write_bitpacked(bitpacked_values(np.random.default_rng(2), small["seg"].max_doc, 5, 0, 1)))
    assert int(dev.raw_agg_range(queries[:1], col, 0, ranges, extra, 0)[2][0]["count"].sum()) == match[0].size
    assert int(dev.raw_agg_range(queries[:1], extra, 0, [(3.0, 9.0)])[1][0].sum()) == match[0].size
    dev.column_release(extra)
    refused(lambda: dev.raw_agg_range(queries[:1], col, 0, ranges, extra, 0), ERR_INVALID, fn, "metric column")
    refused(lambda: dev.raw_agg_range(queries[:1], extra, 0, ranges), ERR_INVALID, fn, "column")


@pytest.mark.parametrize("optional", [False, True])
def test_stats_follow_the_byte_model(ta, small, optional):
    dev, queries, match, lists = small["dev"], small["queries"], small["match"], small["lists"]
    B = ta.binding
    n_words = (small["seg"].max_doc + 31) // 32
    n = len(queries)
    sizes = [m.size for m in match]
    # Full: A the 13-bit column, B the Optional one.  Optional: the other way round
    (col_a, a_model), (col_b, b_model) = ((small["col"], small["model"]), (small["ocol"], small["omodel"]))
    if optional:
        (col_a, a_model), (col_b, b_model) = (col_b, b_model), (col_a, a_model)
    ranges = _cut(a_model.u64[a_model.has], 5)
    plan = RM.plan(GM.U64, ranges)
    nb = len(plan)
    want = [RM.expected_range(m, a_model, plan, b_model, GM.U64) for m in match]
    valued = sum(w[0]["count"] for w in want)
    with_b = sum(r["count"] for w in want for r in w[2])
    assert (valued < sum(sizes)) == optional and (with_b < valued) == (not optional) and with_b > 0
    for slices in (1, 2):
        dev.set_option("agg_slices", slices)
        got = dev.raw_agg_range(queries, col_a, B.VALUE_U64, ranges, col_b, B.VALUE_U64)
        _assert_range(got, want, plan, ("stats", optional, slices))
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == B.KERNEL_AGG_RANGE and st["kernels"] == ["agg_range"]
        assert dev.last_batch_match_counts(n).tolist() == sizes and st["matches"] == sum(sizes)
        # tq_agg_batch's figure with this n_buckets, the starts once per call; every valued doc is bucketed
        agg_bytes = sum(lists) * n_words * 4 + 8 * valued + (8 * sum(sizes) if optional else 0) + n * (64 + 4 * nb) + 8 * nb
        assert st["algorithmic_bytes"] == agg_bytes + 8 * with_b + (0 if optional else 8 * valued) + n * 40 * nb
        plain = dev.raw_agg_range(queries, col_a, B.VALUE_U64, ranges)
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == B.KERNEL_AGG_RANGE and st["algorithmic_bytes"] == agg_bytes
        assert plain[0].tobytes() == got[0].tobytes() and np.array_equal(plain[1], got[1]) and plain[2] is None
        # the record is tq_agg_batch's of column A, bit for bit but for in_bounds (a histogram's; here == count)
        rec = dev.raw_agg(queries, col_a, B.VALUE_U64)[0]
        for k in FIELDS:
            assert k == "in_bounds" or np.array_equal(rec[k], got[0][k]), k
    dev.set_option("agg_slices", 0)
