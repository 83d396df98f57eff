"""One mixed batch through every consumer of the doc-set route (tantivy_amd/csrc/tq_docset.cpp: rows on the host and on the
device, the count pass of tq_count_batch, the selection of tq_sort.cpp, the aggregation of tq_agg.cpp, scored rows),
cut into sub-batches whose boundaries fall on a tree and on a sloppy phrase — where a sub-batch's first query, first tree
record and first sloppy-phrase record meet.

60 queries over tests/test_gpu_docset_tree.py's 60 000-doc segment, cycling through six kinds: a one-list OR over a list
without a bitmap, an AND of the bitmap list and a list without one, a two-term phrase, a nested shape of
tests/tree_shapes.py, a phrase with slop 1, `+* -t`.  Term 0 is prepared before "dense_ratio" 2 is set and is the only
list with a bitmap of its own; every query then takes exactly one slot of the scratch (a distinct list without a bitmap,
or the result of its tree / sloppy phrase), so under "docset_temp_lists" 16 the batch runs as [0, 16), [16, 32), [32, 48),
[48, 60): the second sub-batch begins with a sloppy phrase, the third with a phrase.  The test restates the cut from the
slot demand and asserts both before it trusts a run.

Expectations never come from the device: match sets from the oracle (flat, phrase, nested), tests/slop_model.py (the
non-scoring verdict) and set arithmetic (`+* -t`); rows from tests/sort_model.py, records and buckets from
tests/agg_model.py.  Every comparison is exact.  tq_count_batch hands the doc-set route only its sloppy phrases and
`+* -t` queries (20 of the 60, `+* -t` first): their cut is restated the same way.  tq_last_batch_match_counts is compared
after the calls whose batch is the caller's (not tq_count_batch: its last pass ran a sub-array)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import agg_model as GM
from tests import column_model as CM
from tests import slop_model as SLM
from tests import sort_model as SM
from tests.test_column_model_cpu import bitpacked_values
from tests.test_gpu_agg import _assert_agg
from tests.test_gpu_docset_tree import _assert_rows, _dev_query, _rows, _synth, _want
from tests.test_gpu_docset_tree_scored import _cache, _tw
from tests.test_gpu_sort import Orders
from tests.test_gpu_sort import _assert_rows as _assert_sorted
from tests.tree_shapes import SHAPES

pytestmark = pytest.mark.gpu

M, S, N = O.MUST, O.SHOULD, O.MUST_NOT
KINDS = ("or", "and", "phrase", "nested", "slop", "all-not")
N_QUERIES = 60
TEMP = 16
BITMAP_TERM = 0
KS = (5, 70, 300)


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def _err(ta):
    return ta.binding.lib().tq_last_error().decode()


def _term_positions(seg, terms):
    """tests/phrase_model.py's term_positions ({doc: [positions]} per term id) of the named terms, from the oracle's decode."""
    tp = [{} for _ in seg.terms]
    for t in terms:
        docs, tfs = O.decode_postings(seg, t)
        total = int(tfs.sum())
        flat, n = O.decode_positions(seg, t, total)
        assert n == total
        ends = np.cumsum(tfs.astype(np.int64))
        tp[t] = {int(d): flat[e - f: e].tolist() for d, f, e in zip(docs, tfs.astype(np.int64), ends)}
    return tp


@functools.lru_cache(maxsize=None)
def _batch():
    """-> (segment, queries, match sets).  A query: tests/test_gpu_docset_tree.py's ("flat" | "phrase" | "tree", ...) forms,
    ("slop", term ids, offsets, slop), or ("all-not", t) for `+* -t`."""
    seg = _synth(60_000, 48)
    md = seg.max_doc
    bare = iter(range(47, 0, -1))  # a list without a bitmap of its own per flat query: 30 distinct ones, rare first
    queries = []
    for qi in range(N_QUERIES):
        kind, r = KINDS[qi % len(KINDS)], qi // len(KINDS)
        if kind == "or":
            queries.append(("flat", (O.MODE_OR, [next(bare)])))
        elif kind == "and":
            queries.append(("flat", (O.MODE_AND, [BITMAP_TERM, next(bare)])))
        elif kind == "phrase":
            queries.append(("phrase", [r % 6, r % 6 + 1], [0, 1]))
        elif kind == "nested":
            spec, msm = SHAPES[r % len(SHAPES)]
            queries.append(("tree", spec([1 + (r + j) % 8 for j in range(8)]), msm))
        elif kind == "slop":
            queries.append(("slop", [1 + r % 5, 2 + r % 5], [0, 1], 1))
        else:
            queries.append(("all-not", next(bare)))
    tp = _term_positions(seg, range(1, 7))
    match = []
    for q in queries:
        if q[0] == "slop":
            v = SLM.verdicts(tp, q[1], q[2], q[3])
            match.append(np.array(sorted(d for d, x in v.items() if x.exists), np.uint32))
        elif q[0] == "all-not":
            match.append(np.setdiff1d(np.arange(md, dtype=np.uint32), O.decode_postings(seg, q[1])[0].astype(np.uint32)))
        else:
            match.append(_want(seg, q))
    return seg, queries, match


def _slots(q, qi):
    """What the query takes of a sub-batch's scratch: its lists without a bitmap, or the one result of a tree / sloppy phrase."""
    if q[0] == "flat":
        return {t for t in q[1][1] if t != BITMAP_TERM}
    if q[0] == "all-not":
        return {q[1]}
    return {("result", qi)}


def _expected_cut(queries, max_temp):
    """First queries of the sub-batches: a query joins the current one while its fresh slots still fit."""
    firsts, cur = [0], set()
    for qi, q in enumerate(queries):
        need = _slots(q, qi)
        if qi > firsts[-1] and len(cur | need) > max_temp:
            firsts.append(qi)
            cur = set()
        cur |= need
    return firsts


def _device_query(ta, q):
    if q[0] == "slop":
        return (O.MODE_PHRASE, list(q[1]), list(q[2]), q[3])
    if q[0] == "all-not":
        return (ta.MODE_BOOL, [ta.binding.TERM_ALL, q[1]], [M, N], [0, 1], 0)
    return _dev_query(ta, q)


def test_the_cut_lands_on_a_tree_and_on_a_sloppy_phrase():
    _, queries, match = _batch()
    firsts = _expected_cut(queries, TEMP)
    assert firsts == [0, 16, 32, 48]
    assert queries[16][0] == "slop" and queries[32][0] == "phrase"
    assert _expected_cut(queries, 4096) == [0]
    # the sub-array tq_count_batch hands over: the `+* -t` queries, then the sloppy phrases
    counted = [q for q in queries if q[0] == "all-not"] + [q for q in queries if q[0] == "slop"]
    assert _expected_cut(counted, TEMP) == [0, 16] and counted[16][0] == "slop"
    assert all(m.size for m in match) and len({m.size for m in match}) > 40  # (a row under another index would show)


@pytest.fixture(scope="module")
def mixed(ta):
    seg, queries, match = _batch()
    md = seg.max_doc
    vals = bitpacked_values(np.random.default_rng(12), md, 13, 1 << 40, 1000)
    dev = ta.DeviceIndex([seg])
    try:
        dev.term_handle(BITMAP_TERM)  # (prepared under the default "dense_ratio": the batch's one bitmap list)
        dev.set_option("dense_ratio", 2)
        for t in range(len(seg.terms)):
            dev.term_handle(t)
        own = [t for t in range(len(seg.terms)) if dev.term_table(dev.term_handle(t), "dense").size]
        assert own == [BITMAP_TERM], own
        col = dev.add_column(CM.write_bitpacked(vals))
        dev.set_option("docset_trees", 1)
        yield {"dev": dev, "seg": seg, "queries": queries, "match": match, "vals": vals, "col": col,
               "raw": [_device_query(ta, q) for q in queries]}
    finally:
        dev.close()


def _mask(ta, consumer):
    B = ta.binding
    return consumer | B.KERNEL_DOCSET_TREE | B.KERNEL_PHRASE_SLOP


def _after(ta, dev, match, consumer):
    n = len(match)
    assert dev.last_batch_match_counts(n).tolist() == [m.size for m in match]
    assert int(dev.last_batch_slop_overflows(n).sum()) == 0
    assert dev.last_batch_stats()["kernel_mask"] == _mask(ta, consumer)


@pytest.mark.parametrize("temp", [0, TEMP])
def test_rows_on_the_host_and_on_the_device(ta, mixed, temp):
    import torch

    dev, queries, match, raw = mixed["dev"], mixed["queries"], mixed["match"], mixed["raw"]
    md, n = mixed["seg"].max_doc, len(queries)
    total = sum(m.size for m in match)
    dev.set_option("docset_temp_lists", temp)
    rc, docs, starts = dev.raw_docset(raw, total, guard=8)
    assert rc == 0, _err(ta)
    assert int(starts[0]) == 0 and int(starts[-1]) == total
    _assert_rows(queries, _rows(docs, starts), match, md)
    assert np.all(docs[total:] == 0xDEADBEEF)
    _after(ta, dev, match, ta.binding.KERNEL_DOCSET)
    d_docs = torch.full((total + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert dev.raw_docset_device(raw, d_docs, total, d_starts) == 0, _err(ta)
    _after(ta, dev, match, ta.binding.KERNEL_DOCSET)  # (waits for the batch)
    torch.cuda.synchronize()
    got, got_starts = d_docs.cpu().numpy().view(np.uint32), d_starts.cpu().numpy().view(np.uint64)
    assert int(got_starts[0]) == 0 and int(got_starts[-1]) == total
    _assert_rows(queries, _rows(got, got_starts), match, md)
    assert np.all(got[total:] == 0x5A5A5A5A)


@pytest.mark.parametrize("temp", [0, TEMP])
def test_counts(ta, mixed, temp):
    dev, match, raw = mixed["dev"], mixed["match"], mixed["raw"]
    B = ta.binding
    dev.set_option("docset_temp_lists", temp)
    assert dev.count(raw).tolist() == [m.size for m in match]
    assert int(dev.last_batch_slop_overflows(len(raw)).sum()) == 0
    want = B.KERNEL_DOCSET | B.KERNEL_PHRASE_SLOP  # (the count pass takes no tree: phrases and nested queries are scanned)
    assert dev.last_batch_stats()["kernel_mask"] & (want | B.KERNEL_DOCSET_TREE) == want


@pytest.mark.parametrize("temp", [0, TEMP])
def test_sorted_rows(ta, mixed, temp):
    dev, match, raw = mixed["dev"], mixed["match"], mixed["raw"]
    orders = Orders(SM.per_doc_values(mixed["vals"], None))
    ks = [KS[i % 3] for i in range(len(raw))]
    want = [orders.row(i, match[i], ks[i], SM.ASC, SM.NULLS_LAST) for i in range(len(raw))]
    dev.set_option("docset_temp_lists", temp)
    try:
        for slices in (1, 3):
            dev.set_option("sort_slices", slices)
            _assert_sorted(dev.raw_search_sorted(raw, mixed["col"], SM.ASC, SM.NULLS_LAST, ks), want, ("sorted", temp, slices))
            _after(ta, dev, match, ta.binding.KERNEL_SORT)
    finally:
        dev.set_option("sort_slices", 0)


@pytest.mark.parametrize("temp", [0, TEMP])
def test_aggregations(ta, mixed, temp):
    dev, match, raw = mixed["dev"], mixed["match"], mixed["raw"]
    B = ta.binding
    col_model = GM.Column(mixed["vals"], None, mixed["seg"].max_doc)
    hist = {"interval": 128_000.0, "offset": float(1 << 40)}
    plan = GM.histogram_plan(col_model.info, GM.U64, hist["interval"], hist["offset"])
    assert plan["n_buckets"] == 64
    want = [GM.expected(m, col_model, GM.U64, plan) for m in match]
    assert len({w[0]["sum_lo"] for w in want}) > 40
    dev.set_option("docset_temp_lists", temp)
    try:
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_agg(dev.raw_agg(raw, mixed["col"], B.VALUE_U64, hist), want, plan, ("agg", temp, slices))
            _after(ta, dev, match, B.KERNEL_AGG)
    finally:
        dev.set_option("agg_slices", 0)


def test_scored_rows_do_not_depend_on_the_cut(ta, mixed):
    """The batch without its sloppy phrases (scored doc sets refuse them) under "docset_score_trees": the docs are the match
    sets, and the scores of the four sub-batches are bit for bit those of the one."""
    dev, seg = mixed["dev"], mixed["seg"]
    B = ta.binding
    keep = [i for i, q in enumerate(mixed["queries"]) if q[0] != "slop"]
    queries, match = [mixed["queries"][i] for i in keep], [mixed["match"][i] for i in keep]
    assert len(_expected_cut(queries, TEMP)) == 4
    raw = [mixed["raw"][i] for i in keep]
    weights = [[1.0, 1.0] if q[0] == "all-not" else _tw(ta, seg, q) for q in queries]
    total = sum(m.size for m in match)
    dev.set_option("docset_score_trees", 1)
    got = {}
    try:
        for temp in (0, TEMP):
            dev.set_option("docset_temp_lists", temp)
            rc, docs, scores, starts = dev.raw_docset_scored(raw, total, guard=8, weights=weights, cache=_cache(seg))
            assert rc == 0, _err(ta)
            assert int(starts[-1]) == total
            _assert_rows(queries, _rows(docs, starts), match, seg.max_doc)
            assert np.all(docs[total:] == 0xDEADBEEF) and np.all(scores[total:].view(np.uint32) == 0xDEADBEEF)
            assert dev.last_batch_stats()["kernel_mask"] == (B.KERNEL_DOCSET | B.KERNEL_DOCSET_SCORE | B.KERNEL_DOCSET_TREE |
                                                             B.KERNEL_DOCSET_TREE_SCORE)
            got[temp] = scores[:total].view(np.uint32).copy()
        assert np.array_equal(got[0], got[TEMP])
        assert np.all(np.isfinite(got[0].view(np.float32)))
    finally:
        dev.set_option("docset_score_trees", 0)
        dev.set_option("docset_temp_lists", 0)
