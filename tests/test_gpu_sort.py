"""GPU parity of sort by fast field (tq_search_sorted_batch*: tantivy_amd/csrc/tq_sort.cpp, tq_sort.hip —
TopDocs::order_by_fast_field / order_by_u64_field / order_by((SortByStaticFastValue, ComparatorEnum)) on one segment).

Expectations never come from the device: the column bytes are written by tests/column_model.py from values the test
chose, the match sets come from the oracle's decode / tests/all_model.py / tests/slop_model.py, and a row is
tests/sort_model.expected_sorted_docs — the closed form tests/test_sort_model_cpu.py shows to be what the reference's
TopNComputer yields.  Every comparison is exact: docs, values, flags, counts and padding.

Shapes: tests/test_gpu_term_set._edge_segment — 131 113 docs, 4 098 bitmap words (a selection workgroup takes 256 per step:
16 steps and 2 words; "sort_slices" 3 and 200 cut it into slices of 1 366 and of 21 words, the last four of the 200
empty), a last word of 9 docs, 257 BlockwiseLinear blocks — for the selection; a 20 000-doc synthetic segment for the
query shapes; the 4 500-doc phrase corpus P for phrases, sloppy phrases and nested queries."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import all_model as AM
from tests import column_model as CM
from tests import phrase_model as PM
from tests import sort_model as SM
from tests.test_column_model_cpu import bitpacked_values, blockwise_values, ramp_values
from tests.test_gpu_all import STAR, T, _flat, _model_clauses
from tests.test_gpu_docset import ERR_INVALID, ERR_UNSUPPORTED
from tests.test_gpu_range import RangeLists, _query_columns, _upload, _values
from tests.test_gpu_round3 import _alive_bytes
from tests.test_gpu_term_set import EVEN, SetLists, _edge_segment, _prepare_all_terms, _synth_segment
from tests.tree_shapes import to_device

pytestmark = pytest.mark.gpu

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
TERMINATED = 0x7FFFFFFF
COMBOS = [(order, nulls) for order in (SM.DESC, SM.ASC) for nulls in (SM.NULLS_LAST, SM.NULLS_FIRST)]
KS = (1, 10, 64, 65, 1024)


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def _err(ta):
    return ta.binding.lib().tq_last_error().decode()


class Orders:
    """The full expected order of a match set under every (order, nulls), computed once and cut to k."""

    def __init__(self, per_doc):
        self.per_doc, self.cache = per_doc, {}

    def row(self, name, match, k, order, nulls):
        key = (name, order, nulls)
        if key not in self.cache:
            self.cache[key] = SM.expected_sorted_docs(match, self.per_doc, len(match), order, nulls)
        return self.cache[key][:k]

    def full(self, name, order, nulls):
        return self.cache[(name, order, nulls)]


def _assert_rows(got, want_rows, where):
    """got = (docs, values, has_value, counts) with any stride; want_rows[i] = [(doc, value | None)]."""
    docs, vals, has, counts = got
    assert docs.shape == vals.shape == has.shape and docs.shape[0] == counts.shape[0] == len(want_rows)
    for i, want in enumerate(want_rows):
        c = int(counts[i])
        assert c == len(want), (where, i, c, len(want))
        wd = np.array([d for d, _ in want], np.uint32)
        wv = np.array([0 if v is None else v for _, v in want], np.uint64)
        wh = np.array([v is not None for _, v in want], np.uint8)
        assert np.array_equal(docs[i, :c], wd), (where, i, docs[i, :c][:8], wd[:8])
        assert np.array_equal(vals[i, :c], wv), (where, i, vals[i, :c][:8], wv[:8])
        assert np.array_equal(has[i, :c], wh), (where, i, has[i, :c][:8], wh[:8])
        assert np.all(docs[i, c:] == TERMINATED) and np.all(vals[i, c:] == 0) and np.all(has[i, c:] == 0), (where, i)


# ---- 1. selection at the edges
def _wide_values(rng, md):
    """64 bits wide with 0 and 2^64 - 1, and near both ends pairs that differ only below bit 30 / only at or above it."""
    v = bitpacked_values(rng, md, 64, 0, 1)
    top = (1 << 64) - 1
    for doc, x in ((100, top - 2), (101, top - 3), (200, top - (1 << 30)), (201, top - (1 << 31)),
                   (300, 1), (301, 2), (400, 1 << 30), (401, 1 << 31)):
        v[doc] = x
    assert int(v[100]) ^ int(v[101]) < 1 << 30 and (int(v[200]) ^ int(v[201])) & ((1 << 30) - 1) == 0
    assert int(v[300]) ^ int(v[301]) < 1 << 30 and (int(v[400]) ^ int(v[401])) & ((1 << 30) - 1) == 0
    assert int(v.min()) == 0 and int(v.max()) == top
    return v


def _edge_columns(md):
    """name -> (codec, values, present | None)"""
    rng = np.random.default_rng(20261020)
    some = rng.random(md) < 0.3
    some[md - 1] = True
    one = np.zeros(md, bool)
    one[65536] = True
    some_b = rng.random(md) < 0.3
    return {
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


EDGE_COLUMNS = ["bitpacked 1 bit", "bitpacked 0 bits", "bitpacked 13 bits", "bitpacked 64 bits", "linear descending", "blockwise",
                "optional bitpacked none", "optional bitpacked one doc", "optional bitpacked random", "optional blockwise random"]


@pytest.mark.parametrize("column", EDGE_COLUMNS)
def test_selection_at_the_edges(ta, column):
    seg = _edge_segment()
    md = seg.max_doc
    assert (md + 31) // 32 == 4098 and md % 32 == 9
    B = ta.binding
    codec, vals, present = _edge_columns(md)[column]
    by_df = sorted(range(len(seg.terms)), key=lambda t: seg.terms[t].doc_freq)
    mid, big = by_df[len(by_df) // 2], by_df[-3]
    d_mid, d_even, d_big = (O.decode_postings(seg, t)[0].astype(np.uint32) for t in (mid, EVEN, big))
    queries = {"*": ((ta.MODE_BOOL, [B.TERM_ALL], [M], [0], 0), np.arange(md, dtype=np.uint32)),
               "mid term": ((O.MODE_OR, [mid]), d_mid),
               "+a -b": ((ta.MODE_BOOL, [EVEN, big], [M, N], [0, 1], 0), np.setdiff1d(d_even, d_big))}
    names = list(queries)
    assert 1 < d_mid.size < 1024 < queries["+a -b"][1].size  # (some query has fewer matches than k)
    orders = Orders(SM.per_doc_values(vals, present))
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        _, col = _upload(dev, codec, vals, present)
        info = dev.column_info(col)
        if column == "bitpacked 0 bits":
            assert info["num_bits"] == 0
        if column == "bitpacked 64 bits":
            assert info["num_bits"] == 64
        batch = [queries[n][0] for n in names for _ in KS]
        ks = [k for _ in names for k in KS]
        filled = False
        for order, nulls in COMBOS:
            want = [orders.row(n, queries[n][1], k, order, nulls) for n in names for k in KS]
            # the preconditions this column is here for
            full = orders.full("*", order, nulls)
            if column in ("bitpacked 1 bit", "bitpacked 0 bits"):  # the doc-id tie-break decides at every k
                for k in KS:
                    assert SM.rank_key(full[k - 1][1], order, nulls) == SM.rank_key(full[k][1], order, nulls)
            for n in names:
                valued = sum(1 for _, v in orders.full(n, order, nulls) if v is not None)
                filled = filled or any(valued < min(k, queries[n][1].size) for k in KS)
            for slices in (1, 3, 200, 0):
                dev.set_option("sort_slices", slices)
                got = dev.raw_search_sorted(batch, col, order, nulls, ks)
                _assert_rows(got, want, (column, order, nulls, slices))
                assert dev.last_batch_match_counts(len(batch)).tolist() == [queries[n][1].size for n in names for _ in KS]
        if present is not None:
            assert filled  # some k exceeds the number of valued matches: docs without a value fill the row
    finally:
        dev.close()


# ---- 2. query shapes against the models
class SortLists(RangeLists, SetLists):
    pass


@pytest.mark.parametrize("which,with_deletes", [("full bitpacked", False), ("full bitpacked", True),
                                                ("optional blockwise", False), ("optional blockwise", True)])
def test_query_shapes_against_the_model(ta, which, with_deletes):
    """The case list of tests/test_gpu_range.py::test_every_entry_point_against_the_model (ranges over the SORT column), an
    m-of-n Should query and a term-set handle; match sets from AM.expect."""
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
        L = SortLists(seg)

        def new_range(lower, upper):
            kind, mask, weight = CM.expected_range(vals, present, lower, upper, 1.0)
            got, got_w = dev.range_prepare(col, lower, upper, 1.0)
            assert kind == "set" and isinstance(got, B.RawHandle)
            return L.add_range(got, mask, got_w)

        r = new_range(("in", q1), ("ex", q3))
        r_narrow = new_range(("in", q1), ("in", int(srt[vals.size // 4 + 40])))
        r_empty = new_range(("in", h["max_value"]), ("ex", h["max_value"]))
        members = [by_df[3], by_df[10], by_df[20]]
        ts = L.add_set(dev.term_set_prepare(members), members, 1.0)
        for t in (a, b, c):
            L.need(t)
        cases = [
            ([(S, T(r))], 0),                              # range
            ([(M, T(a)), (M, T(r))], 0),                   # +a +range, sorted by the range's own column
            ([(S, T(a)), (S, T(r))], 0),                   # a range
            ([(M, T(a)), (N, T(r))], 0),                   # +a -range
            ([(M, T(a)), (M, ("union", [b, r]))], 0),      # +a +(b OR range)
            ([(M, STAR), (N, T(r))], 0),                   # * -range
            ([(M, T(b)), (M, T(r_narrow))], 0),
            ([(M, T(a)), (M, T(r_empty))], 0),             # the empty result
            ([(S, T(a)), (S, T(r_empty))], 0),
            ([(S, T(a)), (S, T(b)), (S, T(c))], 2),        # 2 of 3 Should clauses
            ([(M, T(ts)), (N, T(a))], 0),                  # a term-set handle
        ]
        match = [AM.expect(_model_clauses(cl, L), m, L.lists, md, alive)[0].astype(np.uint32) for cl, m in cases]
        assert match[0].size > 1000 and match[7].size == 0 and 0 < match[9].size and 0 < match[10].size
        flat = [_flat(ta, cl, m) for cl, m in cases]
        orders = Orders(SM.per_doc_values(vals, present))
        batch = [q for q in flat for _ in (0, 1)]
        ks = [k for _ in flat for k in (10, 300)]
        for order, nulls in COMBOS:
            want = [orders.row(i, match[i], k, order, nulls) for i in range(len(cases)) for k in (10, 300)]
            got = dev.raw_search_sorted(batch, col, order, nulls, ks)
            _assert_rows(got, want, (which, with_deletes, order, nulls))
            assert dev.last_batch_match_counts(len(batch)).tolist() == [match[i].size for i in range(len(cases)) for _ in (0, 1)]
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
    orders = Orders(SM.per_doc_values(vals, None))
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_budget_x", 256)
        _prepare_all_terms(dev, seg)
        col = dev.add_column(CM.write_bitpacked(vals))
        with pytest.raises(ta.TantivyAmdError) as ei:
            dev.raw_search_sorted(queries, col, SM.DESC, SM.NULLS_LAST, 10)
        assert ei.value.code == ERR_UNSUPPORTED and "query 1" in str(ei.value) and "tq_search_sorted_batch" in str(ei.value)
        dev.set_option("docset_trees", 1)
        for order, nulls in COMBOS[:2]:
            want = [orders.row(i, match[i], 50, order, nulls) for i in range(len(queries))]
            got = dev.raw_search_sorted(queries, col, order, nulls, 50)
            _assert_rows(got, want, ("trees", order, nulls))
            st = dev.last_batch_stats()
            assert st["kernel_mask"] == B.KERNEL_SORT | B.KERNEL_DOCSET_TREE | B.KERNEL_PHRASE_SLOP, st
            assert int(dev.last_batch_slop_overflows(len(queries)).sum()) == 0
    finally:
        dev.close()


def test_sub_batches_keep_the_callers_index(ta):
    """"docset_temp_lists" = 16: a batch that names 40 distinct lists without a bitmap runs as three sub-batches."""
    seg = _synth_segment()
    md = seg.max_doc
    rng = np.random.default_rng(9)
    vals = bitpacked_values(rng, md, 13, 1 << 40, 1000)
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
        orders = Orders(SM.per_doc_values(vals, None))
        ks = [(5, 70, 300)[i % 3] for i in range(len(bare))]
        for slices in (1, 3):
            dev.set_option("sort_slices", slices)
            want = [orders.row(i, match[i], ks[i], SM.ASC, SM.NULLS_LAST) for i in range(len(bare))]
            got = dev.raw_search_sorted(queries, col, SM.ASC, SM.NULLS_LAST, ks)
            _assert_rows(got, want, ("sub-batches", slices))
            assert dev.last_batch_match_counts(len(bare)).tolist() == [m.size for m in match]
    finally:
        dev.close()


# ---- 3. device outputs and bounds; 4. refusals; 5. stats
@pytest.fixture(scope="module")
def small(ta):
    """The synthetic segment with a 13-bit Full column, an Optional one, and three queries with their match sets."""
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
           "orders": Orders(SM.per_doc_values(vals, None)), "oorders": Orders(SM.per_doc_values(ovals, present)),
           "present": present}
    dev.close()


def test_device_rows_padding_and_guards(ta, small):
    import torch

    dev, queries, match = small["dev"], small["queries"], small["match"]
    n, k = len(queries), 20
    stride = k + 5
    want = [small["orders"].row(i, match[i], k, SM.DESC, SM.NULLS_LAST) for i in range(n)]
    host = dev.raw_search_sorted(queries, small["col"], SM.DESC, SM.NULLS_LAST, k, stride=stride)
    assert host[0].shape == (n, stride)
    _assert_rows(host, want, "host rows")
    _assert_rows(dev.raw_search_sorted(queries, small["col"], SM.DESC, SM.NULLS_LAST, k, stride=stride, device=True), want, "device rows")
    # one buffer: [values | guard | docs | guard | flags | guard | counts | guard], 64 guard bytes each
    G = 64
    ent = n * stride
    sizes = [ent * 8, ent * 4, (ent + 63) // 64 * 64, n * 4]
    offs = np.cumsum([0] + [s + G for s in sizes])
    buf = torch.full((int(offs[-1]),), 0xA5, dtype=torch.uint8, device="cuda:0")
    part = lambda i, nbytes: buf[int(offs[i]): int(offs[i]) + nbytes]  # noqa: E731
    torch.cuda.synchronize()
    rc = dev.raw_search_sorted_device(queries, small["col"], SM.DESC, SM.NULLS_LAST, k, stride, part(1, ent * 4), part(0, ent * 8),
                                      part(2, ent), part(3, n * 4))
    assert rc == 0, _err(ta)
    dev.last_batch_stats()  # (waits for the batch)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    got = (raw[offs[1]: offs[1] + ent * 4].view(np.uint32).reshape(n, stride), raw[offs[0]: offs[0] + ent * 8].view(np.uint64).reshape(n, stride),
           raw[offs[2]: offs[2] + ent].reshape(n, stride), raw[offs[3]: offs[3] + n * 4].view(np.uint32))
    _assert_rows(got, want, "device rows in one buffer")
    for i, s in enumerate(sizes):  # between the arrays and behind the last one (and the flags' tail up to 64 bytes)
        used = ent if i == 2 else s
        assert np.all(raw[offs[i] + used: offs[i + 1]] == 0xA5), i


def test_refusals_leave_the_segment_usable(ta, small):
    dev, queries, match, col = small["dev"], small["queries"], small["match"], small["col"]
    B = ta.binding
    want = [small["orders"].row(0, match[0], 10, SM.ASC, SM.NULLS_LAST)]

    def still_good():
        _assert_rows(dev.raw_search_sorted(queries[:1], col, SM.ASC, SM.NULLS_LAST, 10), want, "after a refusal")
        rc, docs, starts = dev.raw_docset(queries[:1], match[0].size)
        assert rc == 0 and np.array_equal(docs[: int(starts[1])], match[0]), _err(ta)

    def refused(call, code, *words):
        with pytest.raises(ta.TantivyAmdError) as ei:
            call()
        assert ei.value.code == code and all(w in str(ei.value) for w in words), ei.value
        still_good()

    still_good()
    fn = "tq_search_sorted_batch"
    refused(lambda: dev.raw_search_sorted(queries, B.MAX_COLUMNS, 0, 0, 10), ERR_INVALID, fn, "column")
    refused(lambda: dev.raw_search_sorted(queries, 7, 0, 0, 10), ERR_INVALID, fn, "column")  # (no such upload)
    refused(lambda: dev.raw_search_sorted(queries, col, 2, 0, 10), ERR_INVALID, fn, "order")
    refused(lambda: dev.raw_search_sorted(queries, col, 0, 2, 10), ERR_INVALID, fn, "nulls")
    refused(lambda: dev.raw_search_sorted(queries, col, 0, 0, [10, 0, 10, 10]), ERR_INVALID, fn, "query 1", "k 0")
    refused(lambda: dev.raw_search_sorted(queries, col, 0, 0, [10, 10, B.MAX_K + 1, 10], stride=2000), ERR_INVALID, fn, "query 2")
    refused(lambda: dev.raw_search_sorted(queries, col, 0, 0, [10, 40, 10, 10], stride=39), ERR_INVALID, fn, "out_stride")
    # the doc-set path's refusals under this function's name: a phrase without "docset_trees", a malformed query
    refused(lambda: dev.raw_search_sorted(queries[:2] + [(O.MODE_PHRASE, [1, 2], [0, 1])], col, 0, 0, 10), ERR_UNSUPPORTED, fn, "query 2")
    refused(lambda: dev.raw_search_sorted(queries[:1] + [(ta.MODE_BOOL, [1, 2], [M, 3], [0, 1], 0)], col, 0, 0, 10), ERR_INVALID, fn, "query 1")
    # a column released after a successful sorted call
    extra = dev.add_column(CM.write_bitpacked(bitpacked_values(np.random.default_rng(2), small["seg"].max_doc, 5, 0, 1)))
    assert int(dev.raw_search_sorted(queries[:1], extra, 0, 0, 10)[3][0]) == 10
    dev.column_release(extra)
    refused(lambda: dev.raw_search_sorted(queries[:1], extra, 0, 0, 10), ERR_INVALID, fn, "column")


@pytest.mark.parametrize("optional", [False, True])
def test_stats_follow_the_byte_model(ta, small, optional):
    dev, queries, match, lists = small["dev"], small["queries"], small["match"], small["lists"]
    B = ta.binding
    col, orders = (small["ocol"], small["oorders"]) if optional else (small["col"], small["orders"])
    n_words = (small["seg"].max_doc + 31) // 32
    ks = [10, 1024, 300, 64]
    for slices in (1, 2):
        dev.set_option("sort_slices", slices)
        want = [orders.row(i, match[i], ks[i], SM.DESC, SM.NULLS_FIRST) for i in range(len(queries))]
        _assert_rows(dev.raw_search_sorted(queries, col, SM.DESC, SM.NULLS_FIRST, ks), want, ("stats", optional, slices))
        st = dev.last_batch_stats()
        sizes = [m.size for m in match]
        assert st["kernel_mask"] == B.KERNEL_SORT and st["kernels"] == ["sort"]
        assert dev.last_batch_match_counts(len(queries)).tolist() == sizes
        assert st["matches"] == sum(sizes)
        valued = sum(int(small["present"][m].sum()) for m in match) if optional else sum(sizes)
        entries = sum(len(w) for w in want)
        assert entries == sum(min(k, s) for k, s in zip(ks, sizes))
        assert st["algorithmic_bytes"] == sum(lists) * n_words * 4 + 8 * valued + (8 * sum(sizes) if optional else 0) + 13 * entries
    dev.set_option("sort_slices", 0)
