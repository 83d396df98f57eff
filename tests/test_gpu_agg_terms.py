"""GPU parity of the terms aggregation (tq_agg_terms_batch*: tantivy_amd/csrc/tq_agg_terms.cpp, tq_agg_terms.hip — the top
segment_size values of a fast-field column by doc count or by key, per query of a batch).

Expectations never come from the device: the column bytes are written by tests/column_model.py from values the test
chose, the match sets come from the oracle's decode / tests/all_model.py / tests/slop_model.py, and the record with its
rows of keys and counts is tests/terms_model.closed_form — exact integers that tests/test_agg_terms_model_cpu.py ties to the
reference's segment collector.  Every comparison is exact (rows, order and record; there is no tolerance in this file),
and out_of_range is 0 in every case.  Segments and queries are those of tests/test_gpu_agg.py, by import."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import agg_model as GM
from tests import all_model as AM
from tests import column_model as CM
from tests import phrase_model as PM
from tests import terms_model as TM
from tests.test_column_model_cpu import bitpacked_values
from tests.test_gpu_agg import AggLists, _err, _walk_queries, _walk_segment, small, ta  # noqa: F401 (ta, small: fixtures)
from tests.test_gpu_all import STAR, T, _flat, _model_clauses
from tests.test_gpu_docset import ERR_INVALID, ERR_UNSUPPORTED
from tests.test_gpu_range import _upload
from tests.test_gpu_round3 import _alive_bytes
from tests.test_gpu_term_set import _prepare_all_terms, _synth_segment
from tests.tree_shapes import to_device

pytestmark = pytest.mark.gpu

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
FILL64, FILL32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


class Col:
    """A column's model: GM.Column's per-doc arrays and the info a plan needs (min, max, gcd, rows)."""

    def __init__(self, values, present, max_doc):
        self.c = GM.Column(values, present, max_doc)
        self.info = TM.column_info(values)

    def want(self, match, order, size):
        return TM.closed_form(self.c.u64, self.c.has, match, self.info, order, size)


def _assert_terms(got, want, plan, where):
    """got = (terms, keys, counts, plan) of raw_agg_terms; want = [(record, keys, counts)] of TM.closed_form."""
    terms, keys, counts, got_plan = got
    assert got_plan == plan, (where, got_plan, plan)
    assert len(terms) == len(keys) == len(counts) == len(want), where
    for i, (rec, wkeys, wcounts) in enumerate(want):
        g = {k: int(terms[i][k]) for k in TM.FIELDS}
        assert g == rec, (where, i, g, rec)
        assert g["out_of_range"] == 0
        n = rec["n_returned"]
        assert n <= keys.shape[1], (where, i)
        assert keys[i, :n].tolist() == wkeys, (where, i, keys[i, :n].tolist()[:8], wkeys[:8])
        assert counts[i, :n].tolist() == wcounts, (where, i)
        assert rec["count"] == sum(wcounts) + rec["sum_other_doc_count"]


def _random_keys(rng, rows, n_keys, vmin=0, gcd=1):
    """min + gcd * n, n uniform below n_keys, row 0 and the last row pinned to the extremes."""
    n = rng.integers(0, n_keys, size=rows).astype(np.uint64)
    n[0], n[-1] = 0, n_keys - 1
    return np.uint64(vmin) + np.uint64(gcd) * n


def _columns(md):
    """name -> (codec, values, present | None, n_keys): the three codecs, gcd 1 / a power of two / 1 000, a min near 2^63,
    keys above 2^53, presence none / one doc / half."""
    rng = np.random.default_rng(20261102)
    ramp = np.arange(md, dtype=np.uint64)
    half = rng.random(md) < 0.5
    half[md - 1] = True
    one = np.zeros(md, bool)
    one[8192] = True
    i64 = rng.integers(-50, 50, size=md)
    i64[0], i64[-1] = -50, 49
    nh = int(half.sum())
    cols = {
        "bitpacked 1 bit": (CM.BITPACKED, bitpacked_values(rng, md, 1, 0, 1), None, 2),
        "bitpacked 0 bits, one key holds every doc": (CM.BITPACKED, bitpacked_values(rng, md, 0, 77, 1), None, 1),
        "bitpacked 13 bits gcd 1000": (CM.BITPACKED, bitpacked_values(rng, md, 13, 1 << 40, 1000), None, 8192),
        "bitpacked above 2^53 gcd 8": (CM.BITPACKED, _random_keys(rng, md, 300, (1 << 60) + 3, 8), None, 300),
        "bitpacked i64 straddling zero": (CM.BITPACKED, np.array([GM.to_u64(int(x), GM.I64) for x in i64], np.uint64), None, 100),
        "linear gcd 1": (CM.LINEAR, np.uint64(1_000_000) + ramp * np.uint64(3) + rng.integers(0, 64, size=md).astype(np.uint64), None, None),
        "linear gcd 1000 above 2^53": (CM.LINEAR, np.uint64((1 << 61) + 5) + np.uint64(1000) * (ramp // np.uint64(4) + rng.integers(0, 16, size=md).astype(np.uint64)), None, None),
        "linear descending gcd 8": (CM.LINEAR, np.uint64(64) + np.uint64(8) * (ramp[::-1] // np.uint64(16) + rng.integers(0, 4, size=md).astype(np.uint64)), None, None),
        "blockwise gcd 3": (CM.BLOCKWISE, np.uint64(500) + np.uint64(3) * (ramp * np.uint64(2) + rng.integers(0, 8, size=md).astype(np.uint64)), None, None),
        "optional bitpacked none": (CM.BITPACKED, np.zeros(0, np.uint64), np.zeros(md, bool), 0),
        "optional bitpacked one doc": (CM.BITPACKED, np.array([1 << 40], np.uint64), one, 1),
        "optional bitpacked half": (CM.BITPACKED, _random_keys(rng, nh, 700, 1 << 40, 1000), half, 700),
        "optional blockwise half": (CM.BLOCKWISE, np.uint64(9) + np.uint64(3) * (np.arange(nh, dtype=np.uint64) + rng.integers(0, 8, size=nh).astype(np.uint64)), half, None),
        "optional, every count equal": (CM.BITPACKED, np.arange(16384, dtype=np.uint64) % np.uint64(128), np.arange(md) < 16384, 128),
    }
    assert list(cols) == EDGE_COLUMNS
    return cols


EDGE_COLUMNS = ["bitpacked 1 bit", "bitpacked 0 bits, one key holds every doc", "bitpacked 13 bits gcd 1000", "bitpacked above 2^53 gcd 8",
                "bitpacked i64 straddling zero", "linear gcd 1", "linear gcd 1000 above 2^53", "linear descending gcd 8", "blockwise gcd 3",
                "optional bitpacked none", "optional bitpacked one doc", "optional bitpacked half", "optional blockwise half",
                "optional, every count equal"]


# ---- 1. the walk, the codecs and the key arithmetic at their edges
@pytest.mark.parametrize("column", EDGE_COLUMNS)
def test_walk_codecs_and_keys_at_the_edges(ta, column):
    """The walk segment (16 421 docs: 514 bitmap words, the last of 5 docs; the sparse term has the first and the last doc,
    `*` the last doc of every slice) under 1, 3, 256 slices and the host's choice; `*`, the sparse term, and a query
    matching nothing; the four orders, with a cut below the number of entries wherever the column has more than 8 keys."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    assert md % 64 and md % 32 and {0, md - 1} <= set(sparse.tolist())
    B = ta.binding
    codec, vals, present, n_keys = _columns(md)[column]
    col = Col(vals, present, md)
    plan = TM.terms_plan(col.info)
    assert n_keys is None or plan["n_keys"] == n_keys
    assert plan["n_keys"] <= TM.MAX_KEYS
    if "gcd" in column:
        assert col.info["gcd"] == int(column.split("gcd ")[1].split()[0])
    if "2^53" in column:
        assert col.info["min_value"] > 1 << 53 and col.info["min_value"] % 2 == 1  # (no f64 holds these keys)
    if "i64" in column:
        assert col.info["min_value"] == (1 << 63) - 50 and col.info["max_value"] == (1 << 63) + 49
    queries = _walk_queries(ta, sparse)
    batch = [q for q, _ in queries]
    size = 8
    want = {o: [col.want(m, o, size) for _, m in queries] for o in TM.ORDERS}
    star = want[TM.COUNT_DESC][0]
    assert want[TM.COUNT_DESC][2][0] == {"matches": 0, "count": 0, "sum_other_doc_count": 0, "distinct": 0, "n_returned": 0,
                                         "doc_count_error_upper_bound": 0, "out_of_range": 0}
    if plan["n_keys"] > 8:
        assert star[0]["distinct"] > size and star[0]["sum_other_doc_count"] > 0 and star[0]["doc_count_error_upper_bound"] > 0
    if column == "bitpacked 0 bits, one key holds every doc":
        assert star[1:] == ([77], [md]) and star[0]["distinct"] == 1
    if column == "optional bitpacked none":
        assert star[0]["matches"] == md and star[0]["count"] == 0 and star[1] == []
    if column == "optional bitpacked half":
        assert md * 0.4 < star[0]["count"] < md * 0.6
    if column == "optional, every count equal":  # all counts equal across the cut: the eight smallest keys survive
        assert star[1:] == (list(range(8)), [128] * 8) and star[0]["doc_count_error_upper_bound"] == 128
        assert want[TM.COUNT_ASC][0][1] == list(range(8))
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        _, handle = _upload(dev, codec, vals, present)
        assert dev.agg_terms_plan(handle) == plan
        for slices in (1, 3, 256, 0):
            dev.set_option("agg_slices", slices)
            for order in TM.ORDERS:
                _assert_terms(dev.raw_agg_terms(batch, handle, order, size), want[order], plan, (column, slices, order))
                assert dev.last_batch_match_counts(len(batch)).tolist() == [m.size for _, m in queries]
    finally:
        dev.close()


# ---- 2. the LDS capacities and the global path
N_KEYS_CASES = ["1", "64", "65", "small", "small + 1", "large", "large + 1", "65536"]


@pytest.mark.parametrize("lds_buckets", [None, 16])
@pytest.mark.parametrize("case", N_KEYS_CASES)
def test_n_keys_around_the_lds_capacities(ta, case, lds_buckets):
    """n_keys at and one past each instantiation's LDS table, 1, 64, 65 and the most served; each with "agg_lds_buckets" at
    its default and at 16 (all but n_keys = 1 are then counted with atomics on the scratch row): the same rows."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    caps = B.agg_terms_lds_capacities()
    assert 65 < caps[0] < caps[1] < 65536
    n_keys = {"small": caps[0], "small + 1": caps[0] + 1, "large": caps[1], "large + 1": caps[1] + 1}.get(case) or int(case)
    rng = np.random.default_rng(5)
    vals = _random_keys(rng, md, n_keys, 1 << 40, 1)
    vals[1:md // 3] = vals[1]  # (one heavy key, so that counts differ at the top)
    col = Col(vals, None, md)
    plan = TM.terms_plan(col.info)
    assert plan["n_keys"] == n_keys
    queries = _walk_queries(ta, sparse)
    size = 65
    want = {o: [col.want(m, o, size) for _, m in queries] for o in TM.ORDERS}
    if n_keys == 65536:  # thousands of keys hold one doc: the cut falls inside a long tie
        star = want[TM.COUNT_DESC][0]
        assert star[0]["distinct"] > 5000 and star[2][0] > md // 4 and star[2][-1] == star[0]["doc_count_error_upper_bound"]
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        handle = dev.add_column(CM.write_bitpacked(vals))
        if lds_buckets is not None:
            dev.set_option("agg_lds_buckets", lds_buckets)
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            for order in TM.ORDERS:
                _assert_terms(dev.raw_agg_terms([q for q, _ in queries], handle, order, size), want[order], plan, (case, lds_buckets, slices, order))
    finally:
        dev.close()


# ---- 3. the cut
@pytest.mark.parametrize("order", TM.ORDERS)
def test_segment_sizes(ta, order):
    """segment_size 1, 64, 65 and 1 024 below the number of entries, and at, one below and above it."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    rng = np.random.default_rng(6)
    wide = Col((rng.zipf(1.3, size=md) % 3000).astype(np.uint64) * np.uint64(7) + np.uint64(11), None, md)
    few = Col(_random_keys(rng, md, 40, 1000, 5), None, md)
    queries = _walk_queries(ta, sparse)
    batch = [q for q, _ in queries]
    assert wide.want(queries[0][1], order, 1)[0]["distinct"] > 1024 and few.want(queries[0][1], order, 1)[0]["distinct"] == 40
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        h_wide, h_few = dev.add_column(CM.write_bitpacked(wide.c.u64)), dev.add_column(CM.write_bitpacked(few.c.u64))
        for size in (1, 64, 65, 1024):
            want = [wide.want(m, order, size) for _, m in queries]
            assert want[0][0]["n_returned"] == size
            _assert_terms(dev.raw_agg_terms(batch, h_wide, order, size), want, TM.terms_plan(wide.info), ("wide", order, size))
        for size in (39, 40, 41, 1024):
            want = [few.want(m, order, size) for _, m in queries]
            assert want[0][0]["n_returned"] == min(size, 40) and (want[0][0]["sum_other_doc_count"] == 0) == (size >= 40)
            _assert_terms(dev.raw_agg_terms(batch, h_few, order, size), want, TM.terms_plan(few.info), ("few", order, size))
    finally:
        dev.close()


# ---- 4. query shapes against the models
def _optional_blockwise(md):
    rng = np.random.default_rng(78)
    present = rng.random(md) < 0.4
    present[md - 1] = True
    n = int(present.sum())
    return CM.BLOCKWISE, np.uint64(9) + np.uint64(3) * (np.arange(n, dtype=np.uint64) // np.uint64(4) + rng.integers(0, 8, size=n).astype(np.uint64)), present


@pytest.mark.parametrize("which,with_deletes", [("full bitpacked", False), ("full bitpacked", True),
                                                ("optional blockwise", False), ("optional blockwise", True)])
def test_query_shapes_against_the_model(ta, which, with_deletes):
    """The case list of tests/test_gpu_agg.py::test_query_shapes_against_the_model: flat AND / OR / boolean, +a +range, a
    term set, m-of-n; match sets from AM.expect."""
    seg = _synth_segment()
    md = seg.max_doc
    rng = np.random.default_rng(77)
    codec, vals, present = (CM.BITPACKED, bitpacked_values(rng, md, 9, 1 << 40, 1000), None) if which == "full bitpacked" else _optional_blockwise(md)
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
        blob, handle = _upload(dev, codec, vals, present)
        h = CM.read_header(blob)
        srt = np.sort(vals)
        q1, q3 = int(srt[vals.size // 4]), int(srt[3 * vals.size // 4])
        L = AggLists(seg)

        def new_range(lower, upper):
            kind, mask, weight = CM.expected_range(vals, present, lower, upper, 1.0)
            got, got_w = dev.range_prepare(handle, lower, upper, 1.0)
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
        col = Col(vals, present, md)
        plan = TM.terms_plan(col.info)
        assert (plan["min_value"], plan["gcd"]) == (h["min_value"], h["gcd"]) and 300 < plan["n_keys"] <= TM.MAX_KEYS
        batch = [_flat(ta, cl, m) for cl, m in cases]
        for order, size in ((TM.COUNT_DESC, 10), (TM.KEY_ASC, 100), (TM.COUNT_ASC, 33), (TM.KEY_DESC, 1)):
            want = [col.want(m, order, size) for m in match]
            _assert_terms(dev.raw_agg_terms(batch, handle, order, size), want, plan, (which, with_deletes, order))
            assert dev.last_batch_match_counts(len(batch)).tolist() == [m.size for m in match]
        # a range as seen through the keys: every key of +a +range lies inside it
        keys = col.want(match[3], TM.KEY_ASC, 1024)[1]
        assert keys and q1 <= keys[0] and keys[-1] < q3
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
    col = Col(bitpacked_values(np.random.default_rng(8), md, 6, 1 << 40, 1000), None, md)
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
    plan = TM.terms_plan(col.info)
    want = [col.want(m, TM.COUNT_DESC, 10) for m in match]
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_budget_x", 256)
        _prepare_all_terms(dev, seg)
        handle = dev.add_column(CM.write_bitpacked(col.c.u64))
        with pytest.raises(ta.TantivyAmdError) as ei:
            dev.raw_agg_terms(queries, handle, TM.COUNT_DESC, 10)
        assert ei.value.code == ERR_UNSUPPORTED and "query 1" in str(ei.value) and "tq_agg_terms_batch" in str(ei.value)
        dev.set_option("docset_trees", 1)
        _assert_terms(dev.raw_agg_terms(queries, handle, TM.COUNT_DESC, 10), want, plan, "trees")
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == B.KERNEL_AGG_TERMS | B.KERNEL_DOCSET_TREE | B.KERNEL_PHRASE_SLOP, st
        assert int(dev.last_batch_slop_overflows(len(queries)).sum()) == 0
    finally:
        dev.close()


def test_sub_batches_keep_the_callers_index(ta):
    """"docset_temp_lists" = 16: a batch that names 40 distinct lists without a bitmap runs as three sub-batches, the
    selection once behind the last."""
    seg = _synth_segment()
    md = seg.max_doc
    col = Col(bitpacked_values(np.random.default_rng(9), md, 13, 1 << 40, 1000), None, md)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 2)  # a bitmap only for the lists that hold half of the docs
        _prepare_all_terms(dev, seg)
        bare = [t for t in range(len(seg.terms)) if dev.term_table(dev.term_handle(t), "dense").size == 0]
        assert len(bare) >= 40
        bare = bare[:40]
        dev.set_option("docset_temp_lists", 16)
        assert -(-len(bare) // 16) == 3  # one fresh list per query, 16 slots per sub-batch
        handle = dev.add_column(CM.write_bitpacked(col.c.u64))
        queries = [(O.MODE_OR, [t]) for t in bare]
        match = [O.decode_postings(seg, t)[0].astype(np.uint32) for t in bare]
        plan = TM.terms_plan(col.info)
        want = [col.want(m, TM.COUNT_DESC, 20) for m in match]
        assert len({tuple(w[1]) for w in want}) == len(want)  # (a row under another query's index would show)
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_terms(dev.raw_agg_terms(queries, handle, TM.COUNT_DESC, 20), want, plan, ("sub-batches", slices))
            assert dev.last_batch_match_counts(len(bare)).tolist() == [m.size for m in match]
    finally:
        dev.close()


# ---- 5. device outputs; 6. refusals; 7. the byte model and the mask
def _small_col(small, optional):
    """the `small` fixture's Full (8 192 keys) or Optional (512 keys) column with its model"""
    model = small["omodel"] if optional else small["model"]
    col = Col(model.u64[model.has], model.has if optional else None, small["seg"].max_doc)
    return (small["ocol"] if optional else small["col"]), col


def test_device_rows_strides_and_guards(ta, small):
    import torch

    dev, queries, match = small["dev"], small["queries"], small["match"]
    B = ta.binding
    n = len(queries)
    handle, col = _small_col(small, False)
    plan = TM.terms_plan(col.info)
    size, stride = 50, 57
    for order in (TM.COUNT_DESC, TM.KEY_DESC):
        want = [col.want(m, order, size) for m in match]
        assert max(w[0]["n_returned"] for w in want) == size
        host = dev.raw_agg_terms(queries, handle, order, size, stride=stride)
        _assert_terms(host, want, plan, "host rows, a wider stride")
        on_dev = dev.raw_agg_terms(queries, handle, order, size, stride=stride, device=True)
        _assert_terms(on_dev, want, plan, "device rows")
        # the host and the device variant agree bit for bit
        assert host[0].tobytes() == on_dev[0].tobytes()
        for i, w in enumerate(want):
            r = w[0]["n_returned"]
            assert host[1][i, :r].tobytes() == on_dev[1][i, :r].tobytes() and host[2][i, :r].tobytes() == on_dev[2][i, :r].tobytes()
    # device buffers a caller owns, used twice: entries at or past n_returned are not touched — with a stride above
    # segment_size, and with a cut above the entries of some queries —; two rows of each kind and two records more than the
    # batch has queries; everything pre-filled
    ocol, omodel = _small_col(small, True)
    oplan = TM.terms_plan(omodel.info)
    assert oplan["n_keys"] == 512
    for c_handle, c_col, c_plan, order, size, stride in ((handle, col, plan, TM.COUNT_DESC, 50, 57), (ocol, omodel, oplan, TM.COUNT_ASC, 600, 520)):
        want = [c_col.want(m, order, size) for m in match]
        returned = [w[0]["n_returned"] for w in want]
        if size == 600:
            assert min(returned) < 512 <= stride and all(w[0]["sum_other_doc_count"] == 0 for w in want)
        else:
            assert max(returned) == size < stride
        d_terms = torch.full(((n + 2) * 5,), FILL64, dtype=torch.int64, device="cuda:0")
        d_keys = torch.full(((n + 2) * stride,), FILL64, dtype=torch.int64, device="cuda:0")
        d_counts = torch.full(((n + 2) * stride,), FILL32, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        for call in (0, 1):  # the second call accumulates into the same buffers: the call zeroes what it adds to
            rc = dev.raw_agg_terms_device(queries, c_handle, order, size, stride, d_terms, d_keys, d_counts)
            assert rc == 0, _err(ta)
            dev.last_batch_stats()  # (waits for the batch)
            torch.cuda.synchronize()
            terms = d_terms.cpu().numpy().view(np.uint64)
            keys = d_keys.cpu().numpy().view(np.uint64).reshape(n + 2, stride)
            counts = d_counts.cpu().numpy().view(np.uint32).reshape(n + 2, stride)
            _assert_terms((terms[: n * 5].view(B.AGG_TERMS_DTYPE), keys[:n], counts[:n], c_plan), want, c_plan, ("device buffers", size, call))
            for i, r in enumerate(returned):
                assert np.all(keys[i, r:] == FILL64) and np.all(counts[i, r:] == FILL32), (size, call, i)
            assert np.all(keys[n:] == FILL64) and np.all(counts[n:] == FILL32) and np.all(terms[n * 5:] == FILL64)
    # the host variant writes zeros from n_returned to min(segment_size, n_keys) and nothing past them
    host = dev.raw_agg_terms(queries, ocol, TM.COUNT_ASC, size, stride=stride)
    _assert_terms(host, want, oplan, "host rows above the entries")
    for i, r in enumerate(returned):
        assert np.all(host[1][i, r:] == 0) and np.all(host[2][i, r:] == 0) and host[1].shape == (n, 512)


def test_refusals_leave_the_segment_usable(ta, small):
    import torch

    dev, queries, match = small["dev"], small["queries"], small["match"]
    B = ta.binding
    handle, col = _small_col(small, False)
    plan = TM.terms_plan(col.info)
    want = [col.want(match[0], TM.COUNT_DESC, 10)]

    def still_good():
        _assert_terms(dev.raw_agg_terms(queries[:1], handle, TM.COUNT_DESC, 10), want, plan, "after a refusal")
        rc, docs, starts = dev.raw_docset(queries[:1], match[0].size)
        assert rc == 0 and np.array_equal(docs[: int(starts[1])], match[0]), _err(ta)

    def refused(call, code, *words):
        with pytest.raises(ta.TantivyAmdError) as ei:
            call()
        assert ei.value.code == code and all(w in str(ei.value) for w in words), ei.value
        still_good()

    still_good()
    fn = "tq_agg_terms_batch"
    refused(lambda: dev.raw_agg_terms(queries, B.MAX_COLUMNS, 0, 10), ERR_INVALID, fn, "column")
    refused(lambda: dev.raw_agg_terms(queries, 7, 0, 10), ERR_INVALID, fn, "column 7")  # (no such upload)
    refused(lambda: dev.raw_agg_terms(queries, handle, 0, 0), ERR_INVALID, fn, "segment_size")
    refused(lambda: dev.raw_agg_terms(queries, handle, 0, B.agg_terms_max_size() + 1), ERR_INVALID, fn, "segment_size")
    refused(lambda: dev.raw_agg_terms(queries, handle, 4, 10), ERR_INVALID, fn, "order")
    refused(lambda: dev.raw_agg_terms(queries, handle, 0, 10, stride=9), ERR_INVALID, fn, "out_stride")
    # more keys than the count rows are sized for: 8 191 001 of them without the gcd
    wide = bitpacked_values(np.random.default_rng(3), small["seg"].max_doc, 17, 5, 1)
    extra = dev.add_column(CM.write_bitpacked(wide))
    refused(lambda: dev.raw_agg_terms(queries, extra, 0, 10), ERR_UNSUPPORTED, fn, "n_keys", "131072")
    dev.column_release(extra)
    # the doc-set path's refusals under this function's name: a phrase without "docset_trees", a malformed query
    refused(lambda: dev.raw_agg_terms(queries[:2] + [(O.MODE_PHRASE, [1, 2], [0, 1])], handle, 0, 10), ERR_UNSUPPORTED, fn, "query 2")
    refused(lambda: dev.raw_agg_terms(queries[:1] + [(ta.MODE_BOOL, [1, 2], [M, 3], [0, 1], 0)], handle, 0, 10), ERR_INVALID, fn, "query 1")
    # null outputs (the device variant takes the pointers as they are)
    n = len(queries)
    d_terms = torch.zeros(n * 5, dtype=torch.int64, device="cuda:0")
    d_keys = torch.zeros(n * 10, dtype=torch.int64, device="cuda:0")
    d_counts = torch.zeros(n * 10, dtype=torch.int32, device="cuda:0")
    for args in ((d_terms, None, d_counts), (d_terms, d_keys, None), (None, d_keys, d_counts)):
        rc = dev.raw_agg_terms_device(queries, handle, 0, 10, 10, *args)
        assert rc == ERR_INVALID and "tq_agg_terms_batch_device" in _err(ta) and "null" in _err(ta)
        still_good()
    # a column released after a successful call
    extra = dev.add_column(CM.write_bitpacked(bitpacked_values(np.random.default_rng(2), small["seg"].max_doc, 5, 0, 1)))
    assert int(dev.raw_agg_terms(queries[:1], extra, 0, 10)[0][0]["count"]) == match[0].size
    dev.column_release(extra)
    refused(lambda: dev.raw_agg_terms(queries[:1], extra, 0, 10), ERR_INVALID, fn, "column")


@pytest.mark.parametrize("optional", [False, True])
def test_stats_follow_the_byte_model(ta, small, optional):
    dev, queries, match, lists = small["dev"], small["queries"], small["match"], small["lists"]
    B = ta.binding
    handle, col = _small_col(small, optional)
    plan = TM.terms_plan(col.info)
    n_words = (small["seg"].max_doc + 31) // 32
    sizes = [m.size for m in match]
    for size in (7, 1024):
        for slices in (1, 2):
            dev.set_option("agg_slices", slices)
            want = [col.want(m, TM.COUNT_DESC, size) for m in match]
            _assert_terms(dev.raw_agg_terms(queries, handle, TM.COUNT_DESC, size), want, plan, ("stats", optional, size, slices))
            st = dev.last_batch_stats()
            assert st["kernel_mask"] == B.KERNEL_AGG_TERMS and st["kernels"] == ["agg_terms"]
            assert dev.last_batch_match_counts(len(queries)).tolist() == sizes
            assert st["matches"] == sum(sizes)
            valued = sum(w[0]["count"] for w in want)
            returned = sum(w[0]["n_returned"] for w in want)
            assert (valued < sum(sizes)) == optional and returned > 0
            assert st["algorithmic_bytes"] == (sum(lists) * n_words * 4 + 8 * valued + (8 * sum(sizes) if optional else 0) +
                                               len(queries) * (40 + 4 * plan["n_keys"]) + 12 * returned)
    dev.set_option("agg_slices", 0)
    # the other aggregation calls enqueue what they did: the same column through tq_agg_batch, stats alone
    stats = dev.raw_agg(queries, handle, B.VALUE_U64)[0]
    st = dev.last_batch_stats()
    assert st["kernel_mask"] == B.KERNEL_AGG and [int(s["count"]) for s in stats] == [w[0]["count"] for w in want]
