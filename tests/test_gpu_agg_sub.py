"""GPU parity of the sub-aggregations (tq_agg_sub_batch*: tantivy_amd/csrc/tq_agg.cpp, tq_agg_sub.hip — a histogram over a
bucket column A with the stats of a metric column B per bucket, per query of a batch).

Expectations never come from the device: the column bytes are written by tests/column_model.py from values the test
chose, the match sets come from the oracle's decode / tests/all_model.py / tests/slop_model.py, and the record, the row of
counts and the bucket records are tests/agg_sub_model.expected_sub — exact integers that tests/test_agg_sub_model_cpu.py
ties to the reference's nested path.  Every comparison is exact (there is no tolerance in this file), and out_of_range is 0
in every case.  Segments, columns and queries are those of tests/test_gpu_agg.py, by import."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import agg_model as GM
from tests import agg_sub_model as SM
from tests import all_model as AM
from tests import column_model as CM
from tests import phrase_model as PM
from tests.test_column_model_cpu import bitpacked_values
from tests.test_gpu_agg import (EVENS, AggLists, _assert_agg, _edge_columns, _err, _typed_columns, _walk_queries,
                                _walk_segment, small, ta)  # noqa: F401 (ta, small: fixtures)
from tests.test_gpu_all import STAR, T, _flat, _model_clauses
from tests.test_gpu_docset import ERR_INVALID, ERR_UNSUPPORTED
from tests.test_gpu_range import _query_columns, _upload
from tests.test_gpu_round3 import _alive_bytes
from tests.test_gpu_sort import EDGE_COLUMNS
from tests.test_gpu_term_set import _prepare_all_terms, _synth_segment
from tests.tree_shapes import to_device

pytestmark = pytest.mark.gpu

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT


def _assert_records(recs, want_rows, where):
    """recs [n, n_buckets] of AGG_BUCKET_STATS_DTYPE against [[record dict per bucket] per query]"""
    assert recs.shape == (len(want_rows), len(want_rows[0]) if want_rows else 0), (where, recs.shape)
    for i, records in enumerate(want_rows):
        for k in SM.RECORD_FIELDS:
            want = np.array([r[k] for r in records], np.uint64)
            bad = np.nonzero(recs[i][k] != want)[0]
            assert bad.size == 0, (where, "query", i, k, "bucket", int(bad[0]), int(recs[i][k][bad[0]]), int(want[bad[0]]))


def _assert_sub(got, want, plan, where):
    """got = (stats, rows, bucket_stats, plan) of raw_agg_sub; want = [(record, counts, bucket records)] of SM.expected_sub."""
    stats, rows, recs, got_plan = got
    _assert_agg((stats, rows, got_plan), [(w[0], w[1]) for w in want], plan, where)
    _assert_records(recs, [w[2] for w in want], where)


def _ramp_a(md):
    """A = doc // 128 as a Linear column: 129 buckets of interval 1 on the walk segment, docs 100 and 101 share bucket 0."""
    vals = (np.arange(md, dtype=np.uint64) // np.uint64(128)).astype(np.uint64)
    model = GM.Column(vals, None, md)
    plan = GM.histogram_plan(model.info, GM.U64, 1.0)
    assert plan["n_buckets"] == (md - 1) // 128 + 1
    return vals, model, plan


# ---- 1. the walk and B's readers at their edges
@pytest.mark.parametrize("column", EDGE_COLUMNS)
def test_walk_and_metric_readers_at_the_edges(ta, column):
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    codec, vals, present = _edge_columns(md)[column]
    b_model = GM.Column(vals, present, md)
    a_vals, a_model, plan = _ramp_a(md)
    assert plan["n_buckets"] == 129
    queries = _walk_queries(ta, sparse)
    batch = [q for q, _ in queries]
    want = [SM.expected_sub(m, a_model, GM.U64, plan, b_model, GM.U64) for _, m in queries]
    assert all(r == SM.empty_record() for r in want[2][2]) and want[2][1] == [0] * 129
    if column == "bitpacked 64 bits":  # docs 100 and 101 sit near 2^64 - 1 and share bucket 0: its sum passes 2^64
        assert want[0][2][0]["sum_hi"] >= 1 and want[1][2][0]["sum_hi"] >= 1
    if column == "optional bitpacked none":
        assert all(r == SM.empty_record() for r in want[0][2]) and want[0][0]["in_bounds"] == md
    if column == "optional bitpacked one doc":
        assert sum(r["count"] for r in want[0][2]) == 1
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        col_a = dev.add_column(CM.write_linear(a_vals))
        _, col_b = _upload(dev, codec, vals, present)
        for slices in (1, 3, 256, 0):
            dev.set_option("agg_slices", slices)
            _assert_sub(dev.raw_agg_sub(batch, col_a, B.VALUE_U64, {"interval": 1.0}, col_b, B.VALUE_U64), want, plan, (column, slices))
            assert dev.last_batch_match_counts(len(batch)).tolist() == [m.size for _, m in queries]
    finally:
        dev.close()


# ---- 2. presence
def test_presence_of_both_columns_and_the_same_column_twice(ta):
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    rng = np.random.default_rng(52)
    has_a, has_b = rng.random(md) < 0.7, rng.random(md) < 0.5
    a_model = GM.Column(rng.integers(0, 60, size=int(has_a.sum())).astype(np.uint64), has_a, md)
    b_model = GM.Column(bitpacked_values(rng, int(has_b.sum()), 13, 1 << 40, 1000), has_b, md)
    hist = {"interval": 10.0}
    plan = GM.histogram_plan(a_model.info, GM.U64, 10.0)
    assert plan["n_buckets"] == 6
    queries = _walk_queries(ta, sparse)[:2]
    # independent presence: with and without A, with and without B — and both kinds of bucketed doc inside bucket 0
    for _, m in queries:
        assert {(bool(has_a[d]), bool(has_b[d])) for d in m.tolist()} == {(False, False), (False, True), (True, False), (True, True)}
        docs, idx = SM.bucket_of_docs(m, a_model, GM.U64, plan)
        assert {bool(has_b[d]) for d in docs[idx == 0].tolist()} == {False, True}
    want = [SM.expected_sub(m, a_model, GM.U64, plan, b_model, GM.U64) for _, m in queries]
    assert all(0 < sum(r["count"] for r in w[2]) < w[0]["in_bounds"] == w[0]["count"] < w[0]["matches"] for w in want)
    same = [SM.expected_sub(m, a_model, GM.U64, plan, a_model, GM.U64) for _, m in queries]
    assert all([r["count"] for r in w[2]] == w[1] and w[2][1]["min_value"] >= 10 and w[2][1]["max_value"] < 20 for w in same)
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        _, col_a = _upload(dev, CM.BITPACKED, a_model.u64[has_a], has_a)
        _, col_b = _upload(dev, CM.BITPACKED, b_model.u64[has_b], has_b)
        batch = [q for q, _ in queries]
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_sub(dev.raw_agg_sub(batch, col_a, B.VALUE_U64, hist, col_b, B.VALUE_U64), want, plan, ("presence", slices))
            _assert_sub(dev.raw_agg_sub(batch, col_a, B.VALUE_U64, hist, col_a, B.VALUE_U64), same, plan, ("B == A", slices))
    finally:
        dev.close()


# ---- 3. value types of B, chosen apart from A's
@pytest.mark.parametrize("which", ["i64 straddling zero", "f64 with infinities and a nan", "date-like nanoseconds",
                                   "i64 A with u64 B"])
def test_value_types_of_the_metric_column(ta, which):
    seg, sparse = _walk_segment()
    md = seg.max_doc
    a_vals, a_model, plan = _ramp_a(md)
    vt_a, hist = GM.U64, {"interval": 1.0}
    if which == "i64 A with u64 B":
        vt_a, a_vals, hist = _typed_columns(md)["i64 straddling zero"]
        a_model = GM.Column(a_vals, None, md)
        plan = GM.histogram_plan(a_model.info, vt_a, hist["interval"])
        assert plan["base_pos"] == -50 and plan["n_buckets"] == 100
        vt_b, b_vals = GM.U64, bitpacked_values(np.random.default_rng(6), md, 13, 1 << 40, 1000)
    else:
        vt_b, b_vals, _ = _typed_columns(md)[which]
    b_model = GM.Column(b_vals, None, md)
    queries = _walk_queries(ta, np.union1d(sparse, np.arange(8)).astype(np.uint32))[:1] + \
        [((O.MODE_OR, [EVENS]), np.arange(0, md, 2, dtype=np.uint32))]
    want = [SM.expected_sub(m, a_model, vt_a, plan, b_model, vt_b) for _, m in queries]
    first = GM.finalize(want[0][2][0], vt_b)  # bucket 0 of `*`
    if which == "i64 straddling zero":
        assert first["min"] < 0 < first["max"] and first["sum"] == int(GM.f64_array(b_vals[:128], vt_b).sum())
    elif which == "f64 with infinities and a nan":  # docs 4, 5 and 6 hold inf, -inf and a NaN: all in bucket 0
        assert first["min"] == -math.inf and math.isnan(first["max"]) and first["sum"] is None and first["count"] == 128
        assert all(r["sum_lo"] == r["sum_hi"] == 0 for w in want for r in w[2])
    elif which == "date-like nanoseconds":
        assert first["count"] == 128 and want[0][2][0]["sum_hi"] >= 1  # (128 values near 2^63 + 1.7e18)
    else:
        assert sum(r["count"] for r in want[0][2]) == md and want[0][2][50]["count"] > 0  # (entry 50: bucket [0, 100))
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        col_a = dev.add_column(CM.write_linear(a_vals) if vt_a == GM.U64 else CM.write_bitpacked(a_vals))
        col_b = dev.add_column(CM.write_bitpacked(b_vals))
        got = dev.raw_agg_sub([q for q, _ in queries], col_a, vt_a, hist, col_b, vt_b)
        _assert_sub(got, want, plan, which)
        assert ta.binding.agg_stats_finalize(got[2][0][0], vt_b) == first or which.startswith("f64")  # (nan != nan)
    finally:
        dev.close()


# ---- 4. the LDS capacities
def _capacity_cases(caps):
    """name -> (histogram over a 13-bit A of values 0..8191, n_buckets)"""
    small_cap, large_cap = caps
    cases = {"one bucket": ({"interval": 1e6}, 1), "8192 buckets": ({"interval": 1.0}, 8192),
             "hard bounds cut both ends": ({"interval": 128.0, "hard_bounds": (1000.0, 5000.0)}, 33)}
    for name, c in (("small", small_cap), ("large", large_cap)):
        cases[name] = ({"interval": 1.0, "hard_bounds": (0.0, float(c - 1))}, c)
        cases[name + " + 1"] = ({"interval": 1.0, "hard_bounds": (0.0, float(c))}, c + 1)
    return cases


CAPACITY_CASES = ["one bucket", "small", "small + 1", "large", "large + 1", "8192 buckets", "hard bounds cut both ends"]


@pytest.mark.parametrize("lds_buckets", [None, 16])
@pytest.mark.parametrize("case", CAPACITY_CASES)
def test_lds_capacities(ta, case, lds_buckets):
    """n_buckets at and one past the capacity of each instantiation's LDS table (interval 1 under hard bounds), one bucket,
    8 192 buckets (at 40 bytes a bucket past any LDS table: always the global path); each with "agg_lds_buckets" at its
    default and at 16 (every row but the one-bucket one goes straight to the row and the records)."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    caps = B.agg_sub_lds_capacities()
    assert sorted(_capacity_cases(caps)) == sorted(CAPACITY_CASES) and 16 < caps[0] < caps[1] < 8192
    hist, n_buckets = _capacity_cases(caps)[case]
    rng = np.random.default_rng(5)
    a_model = GM.Column(bitpacked_values(rng, md, 13, 0, 1), None, md)
    has_b = rng.random(md) < 0.6
    b_model = GM.Column(bitpacked_values(rng, int(has_b.sum()), 33, 7, 3), has_b, md)
    plan = GM.histogram_plan(a_model.info, GM.U64, hist["interval"], 0.0, hist.get("hard_bounds"))
    assert plan["n_buckets"] == n_buckets
    queries = _walk_queries(ta, sparse)
    want = [SM.expected_sub(m, a_model, GM.U64, plan, b_model, GM.U64) for _, m in queries]
    star = want[0]
    if case == "one bucket":
        assert star[1] == [md] and star[2][0]["count"] == int(has_b.sum())
    elif case != "8192 buckets":
        assert 0 < sum(star[1]) == star[0]["in_bounds"] < star[0]["count"]  # (the bounds cut: fewer docs bucketed than valued)
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        col_a = dev.add_column(CM.write_bitpacked(a_model.u64))
        _, col_b = _upload(dev, CM.BITPACKED, b_model.u64[has_b], has_b)
        if lds_buckets is not None:
            dev.set_option("agg_lds_buckets", lds_buckets)
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_sub(dev.raw_agg_sub([q for q, _ in queries], col_a, GM.U64, hist, col_b, GM.U64), want, plan,
                        (case, lds_buckets, slices))
    finally:
        dev.close()


# ---- 5. query shapes against the models
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
        hist = {"interval": float((h["max_value"] - h["min_value"]) // 300 + 1), "offset": 0.5}
        plan = GM.histogram_plan(a_model.info, GM.U64, hist["interval"], hist["offset"])
        assert 250 < plan["n_buckets"] <= 302
        want = [SM.expected_sub(m, a_model, GM.U64, plan, b_model, GM.U64) for m in match]
        batch = [_flat(ta, cl, m) for cl, m in cases]
        _assert_sub(dev.raw_agg_sub(batch, col, B.VALUE_U64, hist, col_b, B.VALUE_U64), want, plan, with_deletes)
        assert dev.last_batch_match_counts(len(batch)).tolist() == [m.size for m in match]
        # the range as seen through the rows: * -range leaves the buckets strictly inside [q1, q3) empty
        lo_i, hi_i = (GM.bucket_pos(float(x), hist["interval"], hist["offset"]) - plan["base_pos"] for x in (q1, q3))
        assert hi_i - lo_i > 100 and not any(want[3][1][lo_i + 1: hi_i]) and all(rec == SM.empty_record() for rec in want[3][2][lo_i + 1: hi_i])
    finally:
        dev.close()


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
    hist = {"interval": 250_000.0}
    plan = GM.histogram_plan(a_model.info, GM.U64, 250_000.0)
    want = [SM.expected_sub(m, a_model, GM.U64, plan, b_model, GM.U64) for m in match]
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_budget_x", 256)
        _prepare_all_terms(dev, seg)
        col = dev.add_column(CM.write_bitpacked(vals))
        col_b = dev.add_column(CM.write_bitpacked(b_vals))
        with pytest.raises(ta.TantivyAmdError) as ei:
            dev.raw_agg_sub(queries, col, B.VALUE_U64, hist, col_b, B.VALUE_U64)
        assert ei.value.code == ERR_UNSUPPORTED and "query 1" in str(ei.value) and "tq_agg_sub_batch" in str(ei.value)
        dev.set_option("docset_trees", 1)
        _assert_sub(dev.raw_agg_sub(queries, col, B.VALUE_U64, hist, col_b, B.VALUE_U64), want, plan, "trees")
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == B.KERNEL_AGG_SUB | B.KERNEL_DOCSET_TREE | B.KERNEL_PHRASE_SLOP, st
        assert int(dev.last_batch_slop_overflows(len(queries)).sum()) == 0
    finally:
        dev.close()


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
        hist = {"interval": 100_000.0, "offset": 7.0}
        plan = GM.histogram_plan(a_model.info, GM.U64, 100_000.0, 7.0)
        want = [SM.expected_sub(m, a_model, GM.U64, plan, b_model, GM.U64) for m in match]
        # (a row under another query's index would show: every query's records differ)
        assert len({tuple(r["sum_lo"] for r in w[2]) for w in want}) == len(want)
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_sub(dev.raw_agg_sub(queries, col, ta.binding.VALUE_U64, hist, col_b, ta.binding.VALUE_U64), want, plan,
                        ("sub-batches", slices))
            assert dev.last_batch_match_counts(len(bare)).tolist() == [m.size for m in match]
    finally:
        dev.close()


# ---- 6. device outputs; 7. refusals; 8. the byte model and the mask
def test_device_rows_strides_and_guards(ta, small):
    import torch

    dev, queries, match, model, omodel = small["dev"], small["queries"], small["match"], small["model"], small["omodel"]
    B = ta.binding
    n = len(queries)
    hist = {"interval": 200_000.0, "offset": 0.5}
    plan = GM.histogram_plan(model.info, GM.U64, 200_000.0, 0.5)
    nb = plan["n_buckets"]
    stride = nb + 7
    want = [SM.expected_sub(m, model, GM.U64, plan, omodel, GM.U64) for m in match]
    args = (queries, small["col"], B.VALUE_U64, hist, small["ocol"], B.VALUE_U64)
    _assert_sub(dev.raw_agg_sub(*args, stride=stride), want, plan, "host rows, a wider stride")
    _assert_sub(dev.raw_agg_sub(*args, stride=stride, device=True), want, plan, "device rows")
    # two rows of each kind and two records more than the batch has queries; everything pre-filled
    fill = 0x5A5A5A5A5A5A5A5A
    d_stats = torch.full(((n + 2) * 8,), fill, dtype=torch.int64, device="cuda:0")
    d_rows = torch.full(((n + 2) * stride,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    d_recs = torch.full(((n + 2) * stride * 5,), fill, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for call in (0, 1):  # the second call accumulates into the same buffers: the call zeroes what it adds to
        rc = dev.raw_agg_sub_device(*args, stride, d_stats, d_rows, d_recs)
        assert rc == 0, _err(ta)
        dev.last_batch_stats()  # (waits for the batch)
        torch.cuda.synchronize()
        stats = d_stats.cpu().numpy().view(np.uint64)
        rows = d_rows.cpu().numpy().view(np.uint32).reshape(n + 2, stride)
        recs = d_recs.cpu().numpy().view(np.uint64).reshape(n + 2, stride, 5)
        got_recs = np.ascontiguousarray(recs[:n, :nb]).reshape(-1).view(B.AGG_BUCKET_STATS_DTYPE).reshape(n, nb)
        _assert_sub((stats[: n * 8].view(B.AGG_STATS_DTYPE), rows[:n, :nb], got_recs, plan), want, plan, ("device buffers", call))
        assert np.all(rows[:n, nb:] == 0x5A5A5A5A) and np.all(rows[n:] == 0x5A5A5A5A)
        assert np.all(recs[:n, nb:] == fill) and np.all(recs[n:] == fill)
        assert np.all(stats[n * 8:] == fill)


def test_refusals_leave_the_segment_usable(ta, small):
    import torch

    dev, queries, match, col, ocol = small["dev"], small["queries"], small["match"], small["col"], small["ocol"]
    model, omodel = small["model"], small["omodel"]
    B = ta.binding
    hist = {"interval": 500_000.0}
    plan = GM.histogram_plan(model.info, GM.U64, 500_000.0)
    nb = plan["n_buckets"]
    want = [SM.expected_sub(match[0], model, GM.U64, plan, omodel, GM.U64)]

    def still_good():
        _assert_sub(dev.raw_agg_sub(queries[:1], col, B.VALUE_U64, hist, ocol, B.VALUE_U64), want, plan, "after a refusal")
        _assert_agg(dev.raw_agg(queries[:1], col, B.VALUE_U64, hist), [want[0][:2]], plan, "raw_agg after a refusal")
        rc, docs, starts = dev.raw_docset(queries[:1], match[0].size)
        assert rc == 0 and np.array_equal(docs[: int(starts[1])], match[0]), _err(ta)

    def refused(call, code, *words):
        with pytest.raises(ta.TantivyAmdError) as ei:
            call()
        assert ei.value.code == code and all(w in str(ei.value) for w in words), ei.value
        still_good()

    still_good()
    fn = "tq_agg_sub_batch"
    refused(lambda: dev.raw_agg_sub(queries, col, 0, None, ocol, 0), ERR_INVALID, fn, "histogram")
    refused(lambda: dev.raw_agg_sub(queries, col, 0, hist, B.MAX_COLUMNS, 0), ERR_INVALID, fn, "metric column")
    refused(lambda: dev.raw_agg_sub(queries, col, 0, hist, 7, 0), ERR_INVALID, fn, "metric column")  # (no such upload)
    refused(lambda: dev.raw_agg_sub(queries, col, 0, hist, ocol, 3), ERR_INVALID, fn, "metric value_type")
    refused(lambda: dev.raw_agg_sub(queries, col, 0, hist, ocol, 0, stride=nb - 1), ERR_INVALID, fn, "bucket_stride")
    # what tq_agg_batch refuses, under this function's name
    refused(lambda: dev.raw_agg_sub(queries, 7, 0, hist, ocol, 0), ERR_INVALID, fn, "column 7")
    refused(lambda: dev.raw_agg_sub(queries, col, 0, {"interval": 0.0}, ocol, 0), ERR_INVALID, fn, "interval")
    refused(lambda: dev.raw_agg_sub(queries, col, 0, {"interval": 1.0}, ocol, 0), ERR_UNSUPPORTED, fn, "buckets")
    refused(lambda: dev.raw_agg_sub(queries[:2] + [(O.MODE_PHRASE, [1, 2], [0, 1])], col, 0, hist, ocol, 0), ERR_UNSUPPORTED, fn, "query 2")
    # null bucket records with n_buckets > 0 (the device variant takes the pointers as they are)
    n = len(queries)
    d_stats = torch.zeros(n * 8, dtype=torch.int64, device="cuda:0")
    d_rows = torch.zeros(n * nb, dtype=torch.int32, device="cuda:0")
    rc = dev.raw_agg_sub_device(queries, col, 0, hist, ocol, 0, nb, d_stats, d_rows, None)
    assert rc == ERR_INVALID and "tq_agg_sub_batch_device" in _err(ta) and "null bucket records" in _err(ta)
    still_good()
    # a metric column released after a successful call
    extra = dev.add_column(CM.write_bitpacked(bitpacked_values(np.random.default_rng(2), small["seg"].max_doc, 5, 0, 1)))
    assert int(dev.raw_agg_sub(queries[:1], col, 0, hist, extra, 0)[2][0]["count"].sum()) == match[0].size
    dev.column_release(extra)
    refused(lambda: dev.raw_agg_sub(queries[:1], col, 0, hist, extra, 0), ERR_INVALID, fn, "metric column")


@pytest.mark.parametrize("optional", [False, True])
def test_stats_follow_the_byte_model(ta, small, optional):
    dev, queries, match, lists = small["dev"], small["queries"], small["match"], small["lists"]
    B = ta.binding
    model = small["model"]
    col_b, b_model = (small["ocol"], small["omodel"]) if optional else (small["col"], small["model"])
    n_words = (small["seg"].max_doc + 31) // 32
    span = model.info["max_value"] - model.info["min_value"]
    hist = {"interval": float(span // 40 + 1), "hard_bounds": (float(model.info["min_value"] + span // 4), float(model.info["max_value"]))}
    plan = GM.histogram_plan(model.info, GM.U64, hist["interval"], 0.0, hist["hard_bounds"])
    nb = plan["n_buckets"]
    want = [SM.expected_sub(m, model, GM.U64, plan, b_model, GM.U64) for m in match]
    sizes = [m.size for m in match]
    bucketed = sum(w[0]["in_bounds"] for w in want)
    with_b = sum(r["count"] for w in want for r in w[2])
    assert 0 < bucketed < sum(sizes) and (with_b < bucketed) == optional
    for slices in (1, 2):
        dev.set_option("agg_slices", slices)
        got = dev.raw_agg_sub(queries, small["col"], B.VALUE_U64, hist, col_b, B.VALUE_U64)
        _assert_sub(got, want, plan, ("stats", optional, slices))
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == B.KERNEL_AGG_SUB and st["kernels"] == ["agg_sub"]
        assert dev.last_batch_match_counts(len(queries)).tolist() == sizes
        assert st["matches"] == sum(sizes)
        agg_bytes = sum(lists) * n_words * 4 + 8 * sum(sizes) + len(queries) * (64 + 4 * nb)  # (A is Full: every match valued)
        assert st["algorithmic_bytes"] == agg_bytes + 8 * with_b + (8 * bucketed if optional else 0) + len(queries) * 40 * nb
        # the same request without the metric: the same records and rows, from agg_kernel
        plain = dev.raw_agg(queries, small["col"], B.VALUE_U64, hist)
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == B.KERNEL_AGG and st["kernels"] == ["agg"] and st["algorithmic_bytes"] == agg_bytes
        assert plain[0].tobytes() == got[0].tobytes() and np.array_equal(plain[1], got[1]) and plain[2] == got[3]
    dev.set_option("agg_slices", 0)
