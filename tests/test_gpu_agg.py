"""GPU parity of the aggregations over a fast field (tq_agg_batch*: tantivy_amd/csrc/tq_agg.cpp, tq_agg.hip — a stats metric
and a histogram / fixed-interval date histogram over a resident u64 column, per query of a batch).

Expectations never come from the device: the column bytes are written by tests/column_model.py from values the test
chose, the match sets come from the oracle's decode / tests/all_model.py / tests/slop_model.py, and a record with its row
of counts is tests/agg_model.expected — exact integers, and IEEE double arithmetic that tests/test_agg_model_cpu.py ties to
the reference's.  Every comparison is exact (there is no tolerance in this file), and out_of_range is 0 in every case.

Shapes: a 16 421-doc segment (2 x 8 192 + 37: 514 bitmap words — an aggregation workgroup takes 256 per step: two full
steps of four 64-word chunks and a ragged tail of two words, the last of 5 docs; "agg_slices" 3 and 256 cut it into slices
of 172 and of 3 words, the last 84 of the 256 empty) for the walk, the value types and the histogram paths; the 20 000-doc
synthetic segment for the query shapes; the 4 500-doc phrase corpus P for phrases, sloppy phrases and nested queries."""
import functools
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import agg_model as GM
from tests import all_model as AM
from tests import column_model as CM
from tests import phrase_model as PM
from tests.test_column_model_cpu import bitpacked_values, blockwise_values, ramp_values
from tests.test_gpu_all import STAR, T, _flat, _model_clauses
from tests.test_gpu_docset import ERR_INVALID, ERR_UNSUPPORTED
from tests.test_gpu_range import RangeLists, _query_columns, _upload, _values
from tests.test_gpu_round3 import _alive_bytes
from tests.test_gpu_sort import EDGE_COLUMNS
from tests.test_gpu_term_set import SetLists, _prepare_all_terms, _synth_segment
from tests.tree_shapes import to_device

pytestmark = pytest.mark.gpu

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
WALK_MAX_DOC = 2 * 8192 + 37
TOP = (1 << 64) - 1
SPARSE, EVENS, ODDS = 0, 1, 2  # the walk segment's terms
FIELDS = ("matches", "count", "min_value", "max_value", "sum_lo", "sum_hi", "in_bounds", "out_of_range")


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def _err(ta):
    return ta.binding.lib().tq_last_error().decode()


def _assert_agg(got, want, plan, where):
    """got = (stats, rows, plan) of raw_agg; want = [(record, counts)] of GM.expected; plan = the model's (or None)."""
    stats, rows, got_plan = got
    assert len(stats) == len(rows) == len(want), where
    nb = plan["n_buckets"] if plan else 0
    if plan:
        assert got_plan == plan, (where, got_plan, plan)
    assert rows.shape == (len(want), nb), (where, rows.shape)
    for i, (rec, counts) in enumerate(want):
        g = {k: int(stats[i][k]) for k in FIELDS}
        assert g == rec, (where, i, g, rec)
        assert g["out_of_range"] == 0
        assert rows[i].tolist() == counts, (where, i)
        assert sum(counts) == rec["in_bounds"]


# ---- 1. the walk at its edges
@functools.lru_cache(maxsize=None)
def _walk_segment():
    md = WALK_MAX_DOC
    assert (md + 31) // 32 == 2 * 256 + 2 and md % 32 == 5
    rng = np.random.default_rng(20261021)
    pinned = [0, 31, 32, 100, 101, 200, 2047, 2048, 8191, 8192, 16383, 16384, md - 1]
    sparse = np.union1d(rng.choice(md, size=300, replace=False), pinned)
    lists = [sparse.tolist(), list(range(0, md, 2)), list(range(1, md, 2))]
    norms = rng.integers(1, 40, size=md).tolist()
    return O.build_segment(md, [[(int(d), 1) for d in l] for l in lists], norms), sparse.astype(np.uint32)


def _wide_values(rng, md):
    """64 bits wide with 0 and 2^64 - 1; docs 100, 101 and 200 — three docs of the sparse term — near 2^64 - 1."""
    v = bitpacked_values(rng, md, 64, 0, 1)
    v[100], v[101], v[200] = TOP - 2, TOP - 3, TOP - (1 << 30)
    assert int(v.min()) == 0 and int(v.max()) == TOP
    return v


def _edge_columns(md):
    """tests/test_gpu_sort._edge_columns at this segment's size: name -> (codec, values, present | None)"""
    rng = np.random.default_rng(20261020)
    some = rng.random(md) < 0.3
    some[md - 1] = True
    one = np.zeros(md, bool)
    one[8192] = True
    some_b = rng.random(md) < 0.3
    cols = {
        "bitpacked 1 bit": (CM.BITPACKED, bitpacked_values(rng, md, 1, 0, 1), None),
        "bitpacked 0 bits": (CM.BITPACKED, bitpacked_values(rng, md, 0, 77, 1), None),
        "bitpacked 13 bits": (CM.BITPACKED, bitpacked_values(rng, md, 13, 1 << 40, 1000), None),
        "bitpacked 64 bits": (CM.BITPACKED, _wide_values(rng, md), None),
        "linear descending": (CM.LINEAR, ramp_values(rng, md, True), None),
        "blockwise": (CM.BLOCKWISE, blockwise_values(rng, md), None),
        "optional bitpacked none": (CM.BITPACKED, _values(rng, CM.BITPACKED, 0), np.zeros(md, bool)),
        "optional bitpacked one doc": (CM.BITPACKED, _values(rng, CM.BITPACKED, 1), one),
        "optional bitpacked random": (CM.BITPACKED, _values(rng, CM.BITPACKED, int(some.sum())), some),
        "optional blockwise random": (CM.BLOCKWISE, blockwise_values(rng, int(some_b.sum())), some_b),
    }
    assert list(cols) == EDGE_COLUMNS
    return cols


def _walk_queries(ta, sparse):
    md = WALK_MAX_DOC
    return [((ta.MODE_BOOL, [ta.binding.TERM_ALL], [M], [0], 0), np.arange(md, dtype=np.uint32)),
            ((O.MODE_OR, [SPARSE]), sparse),
            ((O.MODE_AND, [EVENS, ODDS]), np.zeros(0, np.uint32))]   # matches nothing


@pytest.mark.parametrize("column", EDGE_COLUMNS)
def test_walk_at_the_edges(ta, column):
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    codec, vals, present = _edge_columns(md)[column]
    col_model = GM.Column(vals, present, md)
    queries = _walk_queries(ta, sparse)
    batch = [q for q, _ in queries]
    # about 50 buckets over the column's range whatever it is (a constant column: one bucket holds every doc)
    span = col_model.info["max_value"] - col_model.info["min_value"]
    hist = {"interval": float(span // 50 + 1), "offset": 0.25}
    plan = GM.histogram_plan(col_model.info, GM.U64, hist["interval"], hist["offset"])
    if column == "bitpacked 0 bits":
        assert plan["n_buckets"] == 1
    if column == "optional bitpacked none":
        assert plan["n_buckets"] == 0
    want_stats = [GM.expected(m, col_model, GM.U64) for _, m in queries]
    want_hist = [GM.expected(m, col_model, GM.U64, plan) for _, m in queries]
    nothing = want_stats[2][0]
    assert (nothing["matches"], nothing["count"], nothing["min_value"], nothing["max_value"]) == (0, 0, TOP, 0)
    if column == "bitpacked 64 bits":  # the sum passes 2^64 on three docs alone
        assert want_stats[1][0]["sum_hi"] >= 2 and want_stats[0][0]["sum_hi"] > 1000
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        _, col = _upload(dev, codec, vals, present)
        for slices in (1, 3, 256, 0):
            dev.set_option("agg_slices", slices)
            _assert_agg(dev.raw_agg(batch, col, B.VALUE_U64), want_stats, None, (column, "stats", slices))
            assert dev.last_batch_match_counts(len(batch)).tolist() == [m.size for _, m in queries]
            _assert_agg(dev.raw_agg(batch, col, B.VALUE_U64, hist), want_hist, plan, (column, "histogram", slices))
    finally:
        dev.close()


# ---- 2. value types
def _f64_to_u64(f):
    bits = np.asarray(f, np.float64).view(np.uint64)
    return np.where(bits >> np.uint64(63) != 0, ~bits, bits ^ np.uint64(GM.HIGH)).astype(np.uint64)


def _typed_columns(md):
    """name -> (value type, u64-space values, histogram request)"""
    rng = np.random.default_rng(31)
    i64 = rng.integers(-5000, 5000, size=md)
    i64[:4] = (-5000, -1, 0, 4999)
    f64 = np.round(rng.uniform(-100.0, 100.0, size=md), 2)
    f64[:8] = (0.0, -0.0, -99.75, 12.5, math.inf, -math.inf, math.nan, -2.5)
    date = 1_700_000_000_000_000_000 + rng.integers(0, 86_400_000_000_000, size=md)
    date[:2] = (1_700_000_000_123_456_789, 1_700_086_399_987_654_321)
    as_u64 = lambda a: (a.astype(np.int64).view(np.uint64) ^ np.uint64(GM.HIGH))  # noqa: E731
    return {"i64 straddling zero": (GM.I64, as_u64(i64), {"interval": 100.0}),
            "f64 with infinities and a nan": (GM.F64, _f64_to_u64(f64), {"interval": 2.5, "offset": 0.5, "hard_bounds": (-150.0, 150.0)}),
            "date-like nanoseconds": (GM.I64, as_u64(date), {"interval": 3.6e12})}


@pytest.mark.parametrize("which", ["i64 straddling zero", "f64 with infinities and a nan", "date-like nanoseconds"])
def test_value_types(ta, which):
    seg, sparse = _walk_segment()
    md = seg.max_doc
    vt, vals, hist = _typed_columns(md)[which]
    col_model = GM.Column(vals, None, md)
    plan = GM.histogram_plan(col_model.info, vt, hist["interval"], hist.get("offset", 0.0), hist.get("hard_bounds"))
    queries = _walk_queries(ta, np.union1d(sparse, np.arange(8)).astype(np.uint32))[:1] + \
        [((O.MODE_OR, [EVENS]), np.arange(0, md, 2, dtype=np.uint32))]
    want = [GM.expected(m, col_model, vt, plan) for _, m in queries]
    star = want[0][0]
    fin = GM.finalize(star, vt)
    if which == "i64 straddling zero":
        assert plan["base_pos"] == -50 and fin["min"] == -5000 and fin["max"] == 4999 and fin["sum"] == int(GM.f64_array(vals, vt).sum())
    elif which == "date-like nanoseconds":
        assert plan["n_buckets"] == 25 and float(int(fin["min"])) != int(fin["min"])  # (the value rounds on its way to f64)
    else:
        assert star["in_bounds"] == star["count"] - 3 and star["sum_lo"] == star["sum_hi"] == 0 and fin["sum"] is None
        assert fin["min"] == -math.inf and math.isnan(fin["max"])  # (the mapped order: a NaN sits at its end)
        zero_bucket = GM.bucket_pos(0.0, 2.5, 0.5) - plan["base_pos"]
        assert GM.bucket_pos(-0.0, 2.5, 0.5) - plan["base_pos"] == zero_bucket
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        col = dev.add_column(CM.write_bitpacked(vals))
        got = dev.raw_agg([q for q, _ in queries], col, vt, hist)
        _assert_agg(got, want, plan, which)
        assert ta.binding.agg_stats_finalize(got[0][0], vt) == fin or which.startswith("f64")  # (nan != nan)
        _assert_agg(dev.raw_agg([q for q, _ in queries], col, vt), [GM.expected(m, col_model, vt) for _, m in queries], None, which)
    finally:
        dev.close()


# ---- 3. histogram paths
HIST_CASES = {
    "interval 1": ({"interval": 1.0}, 8192),
    "interval 128": ({"interval": 128.0}, 64),
    "one bucket": ({"interval": 1e6}, 1),
    "hard bounds cut both ends": ({"interval": 128.0, "hard_bounds": (1000.0, 5000.0)}, 33),
    "fractional offset": ({"interval": 100.0, "offset": 33.25}, 83),
}


@pytest.mark.parametrize("lds_buckets", [None, 16])
@pytest.mark.parametrize("case", sorted(HIST_CASES))
def test_histogram_paths(ta, case, lds_buckets):
    """A 13-bit column (values 0..8191); each request with "agg_lds_buckets" at its default (the LDS table: every row here
    fits the kernel's capacity of 8 192) and at 16 (every row but the one-bucket one goes straight to the row)."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    vals = bitpacked_values(np.random.default_rng(5), md, 13, 0, 1)
    col_model = GM.Column(vals, None, md)
    hist, n_buckets = HIST_CASES[case]
    plan = GM.histogram_plan(col_model.info, GM.U64, hist["interval"], hist.get("offset", 0.0), hist.get("hard_bounds"))
    assert plan["n_buckets"] == n_buckets
    queries = _walk_queries(ta, sparse)
    want = [GM.expected(m, col_model, GM.U64, plan) for _, m in queries]
    if case == "one bucket":
        assert want[0][1] == [md]
    if case == "hard bounds cut both ends":
        assert 0 < want[0][0]["in_bounds"] < want[0][0]["count"]
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        col = dev.add_column(CM.write_bitpacked(vals))
        if lds_buckets is not None:
            dev.set_option("agg_lds_buckets", lds_buckets)
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_agg(dev.raw_agg([q for q, _ in queries], col, GM.U64, hist), want, plan, (case, lds_buckets, slices))
    finally:
        dev.close()


# ---- 4. query shapes against the models
class AggLists(RangeLists, SetLists):
    pass


@pytest.mark.parametrize("which,with_deletes", [("full bitpacked", False), ("full bitpacked", True),
                                                ("optional blockwise", False), ("optional blockwise", True)])
def test_query_shapes_against_the_model(ta, which, with_deletes):
    """The case list of tests/test_gpu_sort.py::test_query_shapes_against_the_model: flat AND / OR / boolean, +a +range, a
    term set, m-of-n; match sets from AM.expect."""
    seg = _synth_segment()
    md = seg.max_doc
    codec, vals, present = _query_columns(md)[which]
    by_df = sorted(range(len(seg.terms)), key=lambda t: seg.terms[t].doc_freq)
    a, b, c = by_df[len(by_df) // 2], by_df[-3], by_df[-5]
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
        blob, col = _upload(dev, codec, vals, present)
        h = CM.read_header(blob)
        srt = np.sort(vals)
        q1, q3 = int(srt[vals.size // 4]), int(srt[3 * vals.size // 4])
        L = AggLists(seg)

        def new_range(lower, upper):
            kind, mask, weight = CM.expected_range(vals, present, lower, upper, 1.0)
            got, got_w = dev.range_prepare(col, lower, upper, 1.0)
            assert kind == "set" and isinstance(got, B.RawHandle)
            return L.add_range(got, mask, got_w)

        r = new_range(("in", q1), ("ex", q3))
        r_empty = new_range(("in", h["max_value"]), ("ex", h["max_value"]))
        members = [by_df[3], by_df[10], by_df[20]]
        ts = L.add_set(dev.term_set_prepare(members), members, 1.0)
        for t in (a, b, c):
            L.need(t)
        cases = [
            ([(M, T(a)), (M, T(b))], 0),                   # flat AND
            ([(S, T(a)), (S, T(b))], 0),                   # flat OR
            ([(M, T(a)), (N, T(b)), (S, T(c))], 0),        # boolean
            ([(M, T(a)), (M, T(r))], 0),                   # +a +range, aggregating the range's own column
            ([(M, T(a)), (M, ("union", [b, r]))], 0),      # +a +(b OR range)
            ([(M, STAR), (N, T(r))], 0),                   # * -range
            ([(M, T(a)), (M, T(r_empty))], 0),             # the empty result
            ([(S, T(a)), (S, T(b)), (S, T(c))], 2),        # 2 of 3 Should clauses
            ([(M, T(ts)), (N, T(a))], 0),                  # a term-set handle
        ]
        match = [AM.expect(_model_clauses(cl, L), m, L.lists, md, alive)[0].astype(np.uint32) for cl, m in cases]
        assert match[6].size == 0 and all(match[i].size for i in (0, 1, 2, 3, 4, 5, 7, 8))
        col_model = GM.Column(vals, present, md)
        assert (col_model.info["min_value"], col_model.info["max_value"]) == (h["min_value"], h["max_value"])
        hist = {"interval": float((h["max_value"] - h["min_value"]) // 300 + 1), "offset": 0.5}
        plan = GM.histogram_plan(col_model.info, GM.U64, hist["interval"], hist["offset"])
        assert 250 < plan["n_buckets"] <= 302
        want = [GM.expected(m, col_model, GM.U64, plan) for m in match]
        batch = [_flat(ta, cl, m) for cl, m in cases]
        _assert_agg(dev.raw_agg(batch, col, B.VALUE_U64, hist), want, plan, (which, with_deletes))
        assert dev.last_batch_match_counts(len(batch)).tolist() == [m.size for m in match]
        # a range as seen through the stats: every value of +a +range lies inside it
        assert q1 <= want[3][0]["min_value"] and want[3][0]["max_value"] < q3
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
    vals = bitpacked_values(np.random.default_rng(8), md, 13, 1 << 40, 1000)
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
    assert all(m.size for m in match) and match[2].size >= match[1].size
    col_model = GM.Column(vals, None, md)
    hist = {"interval": 250_000.0}
    plan = GM.histogram_plan(col_model.info, GM.U64, 250_000.0)
    want = [GM.expected(m, col_model, GM.U64, plan) for m in match]
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_budget_x", 256)
        _prepare_all_terms(dev, seg)
        col = dev.add_column(CM.write_bitpacked(vals))
        with pytest.raises(ta.TantivyAmdError) as ei:
            dev.raw_agg(queries, col, B.VALUE_U64, hist)
        assert ei.value.code == ERR_UNSUPPORTED and "query 1" in str(ei.value) and "tq_agg_batch" in str(ei.value)
        dev.set_option("docset_trees", 1)
        _assert_agg(dev.raw_agg(queries, col, B.VALUE_U64, hist), want, plan, "trees")
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == B.KERNEL_AGG | B.KERNEL_DOCSET_TREE | B.KERNEL_PHRASE_SLOP, st
        assert int(dev.last_batch_slop_overflows(len(queries)).sum()) == 0
    finally:
        dev.close()


def test_sub_batches_keep_the_callers_index(ta):
    """"docset_temp_lists" = 16: a batch that names 40 distinct lists without a bitmap runs as three sub-batches."""
    seg = _synth_segment()
    md = seg.max_doc
    vals = bitpacked_values(np.random.default_rng(9), md, 13, 1 << 40, 1000)
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
        queries = [(O.MODE_OR, [t]) for t in bare]
        match = [O.decode_postings(seg, t)[0].astype(np.uint32) for t in bare]
        col_model = GM.Column(vals, None, md)
        hist = {"interval": 100_000.0, "offset": 7.0}
        plan = GM.histogram_plan(col_model.info, GM.U64, 100_000.0, 7.0)
        want = [GM.expected(m, col_model, GM.U64, plan) for m in match]
        assert len({w[0]["sum_lo"] for w in want}) == len(want)  # (a row under another query's index would show)
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_agg(dev.raw_agg(queries, col, ta.binding.VALUE_U64, hist), want, plan, ("sub-batches", slices))
            assert dev.last_batch_match_counts(len(bare)).tolist() == [m.size for m in match]
    finally:
        dev.close()


# ---- 5. device outputs and bounds; 6. refusals; 7. stats
@pytest.fixture(scope="module")
def small(ta):
    """The synthetic segment with a 13-bit Full column, an Optional one, and four queries with their match sets."""
    seg = _synth_segment()
    md = seg.max_doc
    rng = np.random.default_rng(21)
    vals = bitpacked_values(rng, md, 13, 1 << 40, 1000)
    present = rng.random(md) < 0.5
    ovals = bitpacked_values(rng, int(present.sum()), 9, 5, 3)
    by_df = sorted(range(len(seg.terms)), key=lambda t: seg.terms[t].doc_freq)
    a, b = by_df[-2], by_df[len(by_df) // 2]
    da, db = (O.decode_postings(seg, t)[0].astype(np.uint32) for t in (a, b))
    queries = [(O.MODE_OR, [b]), (O.MODE_AND, [a, b]), (ta.MODE_BOOL, [a, b], [M, N], [0, 1], 0),
               (ta.MODE_BOOL, [ta.binding.TERM_ALL], [M], [0], 0)]
    match = [db, np.intersect1d(da, db), np.setdiff1d(da, db), np.arange(md, dtype=np.uint32)]
    lists = [1, 2, 2, 0]
    dev = ta.DeviceIndex([seg])
    _prepare_all_terms(dev, seg)
    col = dev.add_column(CM.write_bitpacked(vals))
    ocol = dev.add_column(CM.write_bitpacked(ovals), CM.OPTIONAL, CM.presence_words(present))
    yield {"dev": dev, "seg": seg, "queries": queries, "match": match, "lists": lists, "col": col, "ocol": ocol,
           "model": GM.Column(vals, None, md), "omodel": GM.Column(ovals, present, md)}
    dev.close()


def test_device_rows_strides_and_guards(ta, small):
    import torch

    dev, queries, match, model = small["dev"], small["queries"], small["match"], small["model"]
    B = ta.binding
    n = len(queries)
    hist = {"interval": 200_000.0, "offset": 0.5}
    plan = GM.histogram_plan(model.info, GM.U64, 200_000.0, 0.5)
    nb = plan["n_buckets"]
    stride = nb + 7
    want = [GM.expected(m, model, GM.U64, plan) for m in match]
    host = dev.raw_agg(queries, small["col"], B.VALUE_U64, hist, stride=stride)
    _assert_agg(host, want, plan, "host rows, a wider stride")
    _assert_agg(dev.raw_agg(queries, small["col"], B.VALUE_U64, hist, stride=stride, device=True), want, plan, "device rows")
    # two rows and two records more than the batch has queries; everything pre-filled
    d_stats = torch.full(((n + 2) * 8,), 0x5A5A5A5A, dtype=torch.int64, device="cuda:0")
    d_rows = torch.full(((n + 2) * stride,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for call in (0, 1):  # the second call accumulates into the same buffers: the call zeroes what it adds to
        rc = dev.raw_agg_device(queries, small["col"], B.VALUE_U64, hist, stride, d_stats, d_rows)
        assert rc == 0, _err(ta)
        dev.last_batch_stats()  # (waits for the batch)
        torch.cuda.synchronize()
        stats = d_stats.cpu().numpy().view(np.uint64)
        rows = d_rows.cpu().numpy().view(np.uint32).reshape(n + 2, stride)
        _assert_agg((stats[: n * 8].view(B.AGG_STATS_DTYPE), rows[:n, :nb], plan), want, plan, ("device buffers", call))
        assert np.all(rows[:n, nb:] == 0x5A5A5A5A) and np.all(rows[n:] == 0x5A5A5A5A)
        assert np.all(stats[n * 8:] == 0x5A5A5A5A)
    # stats alone: no bucket rows at all
    rc = dev.raw_agg_device(queries, small["col"], B.VALUE_U64, None, 0, d_stats, None)
    assert rc == 0, _err(ta)
    dev.last_batch_stats()
    torch.cuda.synchronize()
    stats = d_stats.cpu().numpy().view(np.uint64)
    _assert_agg((stats[: n * 8].view(B.AGG_STATS_DTYPE), np.zeros((n, 0), np.uint32), None), [GM.expected(m, model, GM.U64) for m in match],
                None, "device stats alone")
    assert np.all(stats[n * 8:] == 0x5A5A5A5A)


def test_refusals_leave_the_segment_usable(ta, small):
    dev, queries, match, col, model = small["dev"], small["queries"], small["match"], small["col"], small["model"]
    B = ta.binding
    hist = {"interval": 500_000.0}
    plan = GM.histogram_plan(model.info, GM.U64, 500_000.0)
    want = [GM.expected(match[0], model, GM.U64, plan)]

    def still_good():
        _assert_agg(dev.raw_agg(queries[:1], col, B.VALUE_U64, hist), want, plan, "after a refusal")
        rc, docs, starts = dev.raw_docset(queries[:1], match[0].size)
        assert rc == 0 and np.array_equal(docs[: int(starts[1])], match[0]), _err(ta)

    def refused(call, code, *words):
        with pytest.raises(ta.TantivyAmdError) as ei:
            call()
        assert ei.value.code == code and all(w in str(ei.value) for w in words), ei.value
        still_good()

    still_good()
    fn = "tq_agg_batch"
    refused(lambda: dev.raw_agg(queries, B.MAX_COLUMNS, 0, hist), ERR_INVALID, fn, "column")
    refused(lambda: dev.raw_agg(queries, 7, 0), ERR_INVALID, fn, "column")  # (no such upload)
    refused(lambda: dev.raw_agg(queries, col, 3), ERR_INVALID, fn, "value_type")
    refused(lambda: dev.raw_agg(queries, col, 0, hist, stride=plan["n_buckets"] - 1), ERR_INVALID, fn, "bucket_stride")
    refused(lambda: dev.raw_agg(queries, col, 0, {"interval": 0.0}), ERR_INVALID, fn, "interval")
    refused(lambda: dev.raw_agg(queries, col, 0, {"interval": 1.0, "offset": math.nan}), ERR_INVALID, fn, "offset")
    refused(lambda: dev.raw_agg(queries, col, 0, {"interval": 1.0, "hard_bounds": (2.0, 1.0)}), ERR_INVALID, fn, "hard_min")
    refused(lambda: dev.raw_agg(queries, col, 0, {"interval": 1.0}), ERR_UNSUPPORTED, fn, "buckets")  # 8 191 001 of them
    # the doc-set path's refusals under this function's name: a phrase without "docset_trees", a malformed query
    refused(lambda: dev.raw_agg(queries[:2] + [(O.MODE_PHRASE, [1, 2], [0, 1])], col, 0, hist), ERR_UNSUPPORTED, fn, "query 2")
    refused(lambda: dev.raw_agg(queries[:1] + [(ta.MODE_BOOL, [1, 2], [M, 3], [0, 1], 0)], col, 0, hist), ERR_INVALID, fn, "query 1")
    # a column released after a successful call
    extra = dev.add_column(CM.write_bitpacked(bitpacked_values(np.random.default_rng(2), small["seg"].max_doc, 5, 0, 1)))
    assert int(dev.raw_agg(queries[:1], extra, 0)[0][0]["count"]) == match[0].size
    dev.column_release(extra)
    refused(lambda: dev.raw_agg(queries[:1], extra, 0), ERR_INVALID, fn, "column")


@pytest.mark.parametrize("optional", [False, True])
def test_stats_follow_the_byte_model(ta, small, optional):
    dev, queries, match, lists = small["dev"], small["queries"], small["match"], small["lists"]
    B = ta.binding
    col, model = (small["ocol"], small["omodel"]) if optional else (small["col"], small["model"])
    n_words = (small["seg"].max_doc + 31) // 32
    span = model.info["max_value"] - model.info["min_value"]
    for hist in (None, {"interval": float(span // 40 + 1)}):
        plan = GM.histogram_plan(model.info, GM.U64, hist["interval"]) if hist else None
        nb = plan["n_buckets"] if plan else 0
        for slices in (1, 2):
            dev.set_option("agg_slices", slices)
            want = [GM.expected(m, model, GM.U64, plan) for m in match]
            _assert_agg(dev.raw_agg(queries, col, B.VALUE_U64, hist), want, plan, ("stats", optional, slices))
            st = dev.last_batch_stats()
            sizes = [m.size for m in match]
            assert st["kernel_mask"] == B.KERNEL_AGG and st["kernels"] == ["agg"]
            assert dev.last_batch_match_counts(len(queries)).tolist() == sizes
            assert st["matches"] == sum(sizes)
            valued = sum(w[0]["count"] for w in want)
            assert (valued < sum(sizes)) == optional
            assert st["algorithmic_bytes"] == (sum(lists) * n_words * 4 + 8 * valued + (8 * sum(sizes) if optional else 0) +
                                               len(queries) * (64 + 4 * nb))
    dev.set_option("agg_slices", 0)
