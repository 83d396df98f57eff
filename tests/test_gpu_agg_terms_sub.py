"""GPU parity of the terms aggregation with a metric (tq_agg_terms_sub_batch*: tantivy_amd/csrc/tq_agg_terms_sub.cpp,
tq_agg_terms_sub.hip — per key of a column its doc count and a stats record of a second column, the top segment_size
entries by doc count, by key or by one metric of the record, per query of a batch).

Expectations never come from the device: the column bytes are written by tests/column_model.py from values the test
chose, the match sets come from the oracle's decode / tests/all_model.py / tests/slop_model.py, and the record with its
rows of keys, counts and per-entry records is tests/terms_sub_model.closed_form — exact integers that
tests/test_agg_terms_sub_model_cpu.py ties to the reference's nested segment collector and
tests/test_agg_terms_metric_image_cpu.py to the order value the kernel computes.  Every comparison is exact (there is no
tolerance in this file), and out_of_range is 0 in every case.  Segments and queries are those of tests/test_gpu_agg.py and
tests/test_gpu_agg_terms.py, by import."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
from tests import agg_model as GM
from tests import all_model as AM
from tests import column_model as CM
from tests import phrase_model as PM
from tests import terms_model as TM
from tests import terms_sub_model as SM
from tests.test_column_model_cpu import bitpacked_values
from tests.test_gpu_agg import _err, _walk_queries, _walk_segment, small, ta  # noqa: F401 (ta, small: fixtures)
from tests.test_gpu_agg_terms import _columns, _random_keys
from tests.test_gpu_docset import ERR_INVALID, ERR_UNSUPPORTED
from tests.test_gpu_range import _upload
from tests.test_gpu_term_set import _prepare_all_terms
from tests.tree_shapes import to_device

pytestmark = pytest.mark.gpu

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
FILL64, FILL32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
OLD_ORDERS = TM.ORDERS
METRIC_ORDERS = (SM.METRIC_DESC, SM.METRIC_ASC)


class Pair:
    """The models of a key column A and a metric column B (None: B is A) with the closed form over them."""

    def __init__(self, a_vals, a_present, b_vals, b_present, vt_b, md):
        self.a = GM.Column(a_vals, a_present, md)
        self.b = self.a if b_vals is None else GM.Column(b_vals, b_present, md)
        self.info = TM.column_info(a_vals)
        self.vt = vt_b
        self.plan = TM.terms_plan(self.info)
        self._tables = {}

    def table(self, match):
        key = np.asarray(match, np.uint32).tobytes()
        if key not in self._tables:
            self._tables[key] = SM.per_key(self.a.u64, self.a.has, match, self.info, self.b.u64, self.b.has, self.vt)
        return self._tables[key]

    def want(self, match, order, size, metric=SM.AVG):
        return SM.select(self.table(match), int(np.asarray(match).size), self.vt, order, size, metric)


def _recs_as_dicts(rows):
    return [{k: int(r[k]) for k in SM.RECORD_FIELDS} for r in rows]


def _assert_sub(got, want, plan, where):
    """got = (terms, keys, counts, records, plan) of raw_agg_terms_sub; want = [(record, keys, counts, records)] of the closed form."""
    terms, keys, counts, recs, got_plan = got
    assert got_plan == plan, (where, got_plan, plan)
    assert len(terms) == len(keys) == len(counts) == len(recs) == len(want), where
    for i, (rec, wkeys, wcounts, wrecs) in enumerate(want):
        g = {k: int(terms[i][k]) for k in TM.FIELDS}
        assert g == rec, (where, i, g, rec)
        assert g["out_of_range"] == 0
        n = rec["n_returned"]
        assert n <= keys.shape[1], (where, i)
        assert keys[i, :n].tolist() == wkeys, (where, i, keys[i, :n].tolist()[:8], wkeys[:8])
        assert counts[i, :n].tolist() == wcounts, (where, i)
        assert _recs_as_dicts(recs[i, :n]) == wrecs, (where, i)
        assert rec["count"] == sum(wcounts) + rec["sum_other_doc_count"]


def _i64_col(rng, n, lo, hi):
    typed = rng.integers(lo, hi, size=n)
    return np.array([GM.to_u64(int(x), GM.I64) for x in typed], np.uint64)


# ---- 1. the walk, the codecs and the two columns at their edges
WALK_CASES = {
    # name: (A of test_gpu_agg_terms._columns, B)
    "bitpacked 13 bits gcd 1000 | B full u64": ("bitpacked 13 bits gcd 1000", "full u64"),
    "bitpacked above 2^53 gcd 8 | B optional half i64": ("bitpacked above 2^53 gcd 8", "optional half i64"),
    "linear gcd 1000 above 2^53 | B full i64": ("linear gcd 1000 above 2^53", "full i64"),
    "blockwise gcd 3 | B is A": ("blockwise gcd 3", "A"),
    "optional bitpacked half | B optional half i64": ("optional bitpacked half", "optional half i64"),
    "optional blockwise half | B full blockwise": ("optional blockwise half", "full blockwise"),
    "optional bitpacked none | B full u64": ("optional bitpacked none", "full u64"),
    "bitpacked 1 bit | B linear": ("bitpacked 1 bit", "linear"),
    "bitpacked i64 straddling zero | B is A": ("bitpacked i64 straddling zero", "A"),
}


def _metric_column(which, md):
    """-> (codec, values, present | None, value type)"""
    rng = np.random.default_rng(20261203)
    half = rng.random(md) < 0.5
    half[0] = True
    if which == "full u64":
        return CM.BITPACKED, bitpacked_values(rng, md, 20, 1 << 33, 3), None, GM.U64
    if which == "full i64":
        return CM.BITPACKED, _i64_col(rng, md, -5000, 5000), None, GM.I64
    if which == "optional half i64":
        return CM.BITPACKED, _i64_col(rng, int(half.sum()), -(1 << 40), 1 << 40), half, GM.I64
    if which == "full blockwise":
        return CM.BLOCKWISE, np.uint64(77) + np.uint64(5) * (np.arange(md, dtype=np.uint64) + rng.integers(0, 9, size=md).astype(np.uint64)), None, GM.U64
    assert which == "linear"
    return CM.LINEAR, np.uint64(10) + np.arange(md, dtype=np.uint64) * np.uint64(7) + rng.integers(0, 32, size=md).astype(np.uint64), None, GM.U64


@pytest.mark.parametrize("case", sorted(WALK_CASES))
def test_walk_codecs_and_columns_at_the_edges(ta, case):
    """The walk segment (16 421 docs: 514 bitmap words, the last of 5 docs; the sparse term has the first and the last doc)
    under 1, 3, 256 slices and the host's choice; `*`, the sparse term, and a query matching nothing; A across the codecs,
    with gcd > 1, Optional, keys above 2^53; B Full and Optional-half, U64 and I64 straddling zero, and B = A."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    a_name, b_name = WALK_CASES[case]
    codec_a, vals_a, present_a, _ = _columns(md)[a_name]
    if b_name == "A":
        codec_b, vals_b, present_b, vt = None, None, None, GM.I64 if "i64" in a_name else GM.U64
    else:
        codec_b, vals_b, present_b, vt = _metric_column(b_name, md)
    pair = Pair(vals_a, present_a, vals_b, present_b, vt, md)
    queries = _walk_queries(ta, sparse)
    batch = [q for q, _ in queries]
    size = 8
    combos = [(o, SM.AVG) for o in OLD_ORDERS] + [(SM.METRIC_DESC, SM.AVG), (SM.METRIC_ASC, SM.MAX), (SM.METRIC_DESC, SM.SUM), (SM.METRIC_ASC, SM.VALUE_COUNT)]
    want = {c: [pair.want(m, c[0], size, c[1]) for _, m in queries] for c in combos}
    star = want[(SM.METRIC_DESC, SM.AVG)][0]
    assert want[combos[0]][2][0]["matches"] == 0 and want[combos[0]][2][1] == []
    if pair.plan["n_keys"] > 8:
        assert star[0]["distinct"] > size and star[0]["sum_other_doc_count"] > 0
    if "optional half" in b_name:
        assert any(r["count"] < c for r, c in zip(star[3], star[2]))  # (docs counted under a key without a value in B)
    if vt == GM.I64:
        typed = [SM.typed_sum(r, vt) for r in pair.table(queries[0][1])[2] if r["count"]]
        assert b_name == "A" or (min(typed) < 0 < max(typed))
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        _, ha = _upload(dev, codec_a, vals_a, present_a)
        hb = ha if b_name == "A" else _upload(dev, codec_b, vals_b, present_b)[1]
        for slices in (1, 3, 256, 0):
            dev.set_option("agg_slices", slices)
            for order, metric in combos:
                got = dev.raw_agg_terms_sub(batch, ha, hb, vt, order, size, metric)
                _assert_sub(got, want[(order, metric)], pair.plan, (case, slices, order, metric))
                assert dev.last_batch_match_counts(len(batch)).tolist() == [m.size for _, m in queries]
    finally:
        dev.close()


# ---- 2. the four old orders are tq_agg_terms_batch's, bit for bit
def test_old_orders_equal_the_terms_call(ta, small):
    dev, queries, match = small["dev"], small["queries"], small["match"]
    md = small["seg"].max_doc
    a, b = small["model"], small["omodel"]
    pair = Pair(a.u64, None, b.u64[b.has], b.has, GM.U64, md)
    for order in OLD_ORDERS:
        for size in (7, 300):
            plain = dev.raw_agg_terms(queries, small["col"], order, size)
            got = dev.raw_agg_terms_sub(queries, small["col"], small["ocol"], GM.U64, order, size, SM.SUM)
            assert got[0].tobytes() == plain[0].tobytes() and got[4] == plain[3], (order, size)
            for i in range(len(queries)):
                n = int(plain[0][i]["n_returned"])
                assert got[1][i, :n].tobytes() == plain[1][i, :n].tobytes() and got[2][i, :n].tobytes() == plain[2][i, :n].tobytes()
            _assert_sub(got, [pair.want(m, order, size) for m in match], pair.plan, ("old orders", order, size))


# ---- 3. the metric orders
def _metric_case(which, md):
    """-> (A values, A present, B values, B present, value type of B)"""
    rng = np.random.default_rng(20261204)
    docs = np.arange(md, dtype=np.uint64)
    if which == "every metric ties across the cut":
        present = np.arange(md) < 16400  # 50 keys x 328 docs; key k holds B = 0..327, whatever k
        return (docs[:16400] % np.uint64(50)) * np.uint64(3) + np.uint64(100), present, docs // np.uint64(50), None, GM.U64
    if which == "keys with docs but no value in B":
        idx = rng.integers(0, 60, size=md)
        idx[:60] = np.arange(60)
        has_b = idx % 5 != 0
        return np.uint64(1000) + np.uint64(2) * idx.astype(np.uint64), None, _i64_col(rng, int(has_b.sum()), -3000, 3000), has_b, GM.I64
    if which == "sums above 2^64":
        idx = rng.integers(0, 40, size=md)
        return idx.astype(np.uint64), None, np.uint64(1 << 63) + rng.integers(0, 1 << 62, size=md).astype(np.uint64), None, GM.U64
    assert which == "averages one f64 apart"
    idx = 3 + rng.integers(0, 37, size=md)
    b = np.uint64(1 << 59) + rng.integers(0, 1 << 40, size=md).astype(np.uint64)
    # keys 0, 1, 2: three docs each around 2^60, where f64 are 256 apart: the averages are 2^60, 2^60 + 256 (the next
    # f64; its sum 3 * 2^60 + 768 is no f64) and 2^60 + 128 (halfway: to even, 2^60 — a tie with key 0)
    idx[:9] = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    b[:9] = [1 << 60] * 5 + [(1 << 60) + 768] + [1 << 60] * 2 + [(1 << 60) + 384]
    return idx.astype(np.uint64), None, b, None, GM.U64


METRIC_CASES = ["every metric ties across the cut", "keys with docs but no value in B", "sums above 2^64", "averages one f64 apart"]


@pytest.mark.parametrize("which", METRIC_CASES)
def test_metric_orders(ta, which):
    """Every order_metric x DESC / ASC with a cut below the number of entries."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    vals_a, present_a, vals_b, present_b, vt = _metric_case(which, md)
    pair = Pair(vals_a, present_a, vals_b, present_b, vt, md)
    queries = _walk_queries(ta, sparse)
    batch = [q for q, _ in queries]
    size = 7
    want = {(o, m): [pair.want(mt, o, size, m) for _, mt in queries] for o in METRIC_ORDERS for m in SM.METRICS}
    star = {k: w[0] for k, w in want.items()}
    assert all(w[0]["distinct"] > size for w in star.values())
    if which == "every metric ties across the cut":
        for w in star.values():  # the smallest keys survive, under both orders
            assert w[1] == [100 + 3 * k for k in range(size)] and w[2] == [328] * size and w[0]["doc_count_error_upper_bound"] == 328
    if which == "keys with docs but no value in B":
        full = pair.want(queries[0][1], SM.METRIC_DESC, 1024, SM.AVG)
        at = [i for i, r in enumerate(full[3]) if r["count"] == 0]
        assert len(at) == 12 and at == list(range(at[0], at[0] + 12)) and 0 < at[0] and at[-1] < len(full[3]) - 1  # typed 0: in the middle
        assert [full[1][i] for i in at] == sorted(full[1][i] for i in at)
    if which == "sums above 2^64":
        assert all(r["sum_hi"] > 0 for r in star[(SM.METRIC_DESC, SM.SUM)][3])
    if which == "averages one f64 apart":
        table = pair.table(queries[0][1])
        img = [SM.image(table[2][k], vt, SM.AVG) for k in range(3)]
        assert img[1] == img[0] + 1 and img[2] == img[0]
        assert star[(SM.METRIC_DESC, SM.AVG)][1][:3] == [1, 0, 2]  # the larger by one bit first, then the tie by ascending key
        s1 = SM.typed_sum(table[2][1], vt)
        assert float(s1) != s1  # (f64 arithmetic on a rounded sum would start from another number)
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        _, ha = _upload(dev, CM.BITPACKED, vals_a, present_a)
        _, hb = _upload(dev, CM.BITPACKED, vals_b, present_b)
        for (order, metric), w in want.items():
            _assert_sub(dev.raw_agg_terms_sub(batch, ha, hb, vt, order, size, metric), w, pair.plan, (which, order, metric))
    finally:
        dev.close()


# ---- 4. the LDS capacities and the global path
N_KEYS_CASES = ["1", "64", "65", "small", "small + 1", "large", "large + 1", "65536"]


@pytest.mark.parametrize("lds_buckets", [None, 16])
@pytest.mark.parametrize("case", N_KEYS_CASES)
def test_n_keys_around_the_lds_capacities(ta, case, lds_buckets):
    """n_keys at and one past each instantiation's LDS table, 1, 64, 65 and the most served; each with "agg_lds_buckets" at
    its default and at 16 (all but n_keys = 1 are then accumulated with atomics on the scratch rows): the same rows."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    caps = B.agg_terms_sub_lds_capacities()
    assert 65 < caps[0] < caps[1] < 65536
    n_keys = {"small": caps[0], "small + 1": caps[0] + 1, "large": caps[1], "large + 1": caps[1] + 1}.get(case) or int(case)
    rng = np.random.default_rng(5)
    vals = _random_keys(rng, md, n_keys, 1 << 40, 1)
    vals[1:md // 3] = vals[1]  # (one heavy key)
    half = rng.random(md) < 0.5
    pair = Pair(vals, None, _i64_col(rng, int(half.sum()), -(1 << 50), 1 << 50), half, GM.I64, md)
    assert pair.plan["n_keys"] == n_keys
    queries = _walk_queries(ta, sparse)
    size = 65
    combos = [(SM.COUNT_DESC, SM.AVG), (SM.METRIC_DESC, SM.AVG), (SM.METRIC_ASC, SM.SUM), (SM.METRIC_DESC, SM.MIN)]
    want = {c: [pair.want(m, c[0], size, c[1]) for _, m in queries] for c in combos}
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        ha = dev.add_column(CM.write_bitpacked(vals))
        _, hb = _upload(dev, CM.BITPACKED, pair.b.u64[pair.b.has], half)
        if lds_buckets is not None:
            dev.set_option("agg_lds_buckets", lds_buckets)
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            for order, metric in combos:
                got = dev.raw_agg_terms_sub([q for q, _ in queries], ha, hb, GM.I64, order, size, metric)
                _assert_sub(got, want[(order, metric)], pair.plan, (case, lds_buckets, slices, order, metric))
    finally:
        dev.close()


# ---- 5. the cut
@pytest.mark.parametrize("order,metric", [(SM.COUNT_DESC, SM.AVG), (SM.METRIC_DESC, SM.AVG), (SM.METRIC_ASC, SM.MAX), (SM.METRIC_DESC, SM.SUM)])
def test_segment_sizes(ta, order, metric):
    """segment_size 1, 1 023 and 1 024 below the number of entries, and at, one below and above it."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    rng = np.random.default_rng(6)
    b = bitpacked_values(rng, md, 30, 5, 1)
    wide = Pair((rng.zipf(1.3, size=md) % 3000).astype(np.uint64) * np.uint64(7) + np.uint64(11), None, b, None, GM.U64, md)
    few = Pair(_random_keys(rng, md, 40, 1000, 5), None, b, None, GM.U64, md)
    queries = _walk_queries(ta, sparse)
    batch = [q for q, _ in queries]
    assert wide.want(queries[0][1], order, 1, metric)[0]["distinct"] > 1024 and few.want(queries[0][1], order, 1, metric)[0]["distinct"] == 40
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        h_wide, h_few, hb = (dev.add_column(CM.write_bitpacked(v)) for v in (wide.a.u64, few.a.u64, b))
        for size in (1, 1023, 1024):
            want = [wide.want(m, order, size, metric) for _, m in queries]
            assert want[0][0]["n_returned"] == size
            _assert_sub(dev.raw_agg_terms_sub(batch, h_wide, hb, GM.U64, order, size, metric), want, wide.plan, ("wide", order, size))
        for size in (39, 40, 41):
            want = [few.want(m, order, size, metric) for _, m in queries]
            assert want[0][0]["n_returned"] == min(size, 40) and (want[0][0]["sum_other_doc_count"] == 0) == (size >= 40)
            _assert_sub(dev.raw_agg_terms_sub(batch, h_few, hb, GM.U64, order, size, metric), want, few.plan, ("few", order, size))
    finally:
        dev.close()


# ---- 6. host and device rows
def _small_pair(small, a_optional):
    """the `small` fixture's columns: A the Optional (512 keys) or the Full (8 192 keys) one, B the other"""
    md = small["seg"].max_doc
    full, opt = small["model"], small["omodel"]
    if a_optional:
        return small["ocol"], small["col"], Pair(opt.u64[opt.has], opt.has, full.u64, None, GM.U64, md)
    return small["col"], small["ocol"], Pair(full.u64, None, opt.u64[opt.has], opt.has, GM.U64, md)


def test_host_and_device_rows_strides_and_guards(ta, small):
    import torch

    dev, queries, match = small["dev"], small["queries"], small["match"]
    B = ta.binding
    n = len(queries)
    ha, hb, pair = _small_pair(small, True)
    assert pair.plan["n_keys"] == 512
    order, metric, size, stride = SM.METRIC_DESC, SM.AVG, 600, 520
    want = [pair.want(m, order, size, metric) for m in match]
    returned = [w[0]["n_returned"] for w in want]
    assert min(returned) < 512 <= stride and all(w[0]["sum_other_doc_count"] == 0 for w in want)
    # the host variant, a stride wider than needed: entries past n_returned read 0
    host = dev.raw_agg_terms_sub(queries, ha, hb, GM.U64, order, size, metric, stride=stride)
    _assert_sub(host, want, pair.plan, "host rows, a wider stride")
    assert host[1].shape == (n, stride)
    for i, r in enumerate(returned):
        assert np.all(host[1][i, r:512] == 0) and np.all(host[2][i, r:512] == 0), i
        assert all(int(host[3][i, r:512][f].max(initial=0)) == 0 for f in SM.RECORD_FIELDS), i
        assert np.all(host[1][i, 512:] == 0xDEADBEEF) and np.all(host[2][i, 512:] == 0xDEADBEEF)  # (nothing past the width)
    # device buffers a caller owns, used twice: entries at or past n_returned keep the fill; two rows more than queries
    d_terms = torch.full(((n + 2) * 5,), FILL64, dtype=torch.int64, device="cuda:0")
    d_keys = torch.full(((n + 2) * stride,), FILL64, dtype=torch.int64, device="cuda:0")
    d_counts = torch.full(((n + 2) * stride,), FILL32, dtype=torch.int32, device="cuda:0")
    d_recs = torch.full(((n + 2) * stride * 5,), FILL64, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for call in (0, 1):  # the second call accumulates into the same buffers: the call zeroes what it adds to
        rc = dev.raw_agg_terms_sub_device(queries, ha, hb, GM.U64, order, size, metric, stride, d_terms, d_keys, d_counts, d_recs)
        assert rc == 0, _err(ta)
        dev.last_batch_stats()  # (waits for the batch)
        torch.cuda.synchronize()
        terms = d_terms.cpu().numpy().view(np.uint64)
        keys = d_keys.cpu().numpy().view(np.uint64).reshape(n + 2, stride)
        counts = d_counts.cpu().numpy().view(np.uint32).reshape(n + 2, stride)
        words = d_recs.cpu().numpy().view(np.uint64).reshape(n + 2, stride, 5)
        recs = words.reshape(-1).view(B.AGG_BUCKET_STATS_DTYPE).reshape(n + 2, stride)
        _assert_sub((terms[: n * 5].view(B.AGG_TERMS_DTYPE), keys[:n], counts[:n], recs[:n], pair.plan), want, pair.plan, ("device buffers", call))
        for i, r in enumerate(returned):
            assert np.all(keys[i, r:] == FILL64) and np.all(counts[i, r:] == FILL32) and np.all(words[i, r:] == FILL64), (call, i)
        assert np.all(keys[n:] == FILL64) and np.all(counts[n:] == FILL32) and np.all(words[n:] == FILL64) and np.all(terms[n * 5:] == FILL64)
        # the host and the device variant agree bit for bit
        assert host[0].tobytes() == terms[: n * 5].tobytes()
    on_dev = dev.raw_agg_terms_sub(queries, ha, hb, GM.U64, order, size, metric, device=True)
    _assert_sub(on_dev, want, pair.plan, "device rows through the binding")


# ---- 7. nested and phrase queries
def test_trees_take_the_docset_option(ta):
    """A phrase, a sloppy phrase and a nested query: refused without "docset_trees" naming the first such query, exact with it."""
    from tests.test_gpu_phrase_slop import _expect as slop_expect

    corp = PM.corpus("P")
    seg = corp.segment()
    md = corp.max_doc
    assert corp.alive is None
    B = ta.binding
    rng = np.random.default_rng(8)
    pair = Pair(bitpacked_values(rng, md, 6, 1 << 40, 1000), None, _i64_col(rng, md, -1000, 1000), None, GM.I64, md)
    _, terms, offs = corp.queries[0]
    e = slop_expect(corp, 0, 1)
    assert e.longest <= B.SLOP_CARRY_CAP
    spec = [(M, 2), (M, [(S, [0, 1]), (S, 3)], 0)]  # +c +((+a +b) d)
    flat_q = (O.MODE_OR, [4])
    queries = [flat_q, (O.MODE_PHRASE, list(terms), list(offs)), (O.MODE_PHRASE, list(terms), list(offs), 1), to_device(ta, spec, 0), flat_q]
    match = [O.decode_postings(seg, 4)[0].astype(np.uint32),
             np.sort(O.match_all(seg, list(terms), O.MODE_PHRASE, phrase_offsets=list(offs))[0]).astype(np.uint32),
             np.asarray(e.exists_docs, np.uint32), np.asarray(O.tree_match_all(seg, spec, 0)[0], np.uint32),
             O.decode_postings(seg, 4)[0].astype(np.uint32)]
    assert all(m.size for m in match)
    want = [pair.want(m, SM.METRIC_DESC, 10, SM.AVG) for m in match]
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_budget_x", 256)
        _prepare_all_terms(dev, seg)
        ha, hb = dev.add_column(CM.write_bitpacked(pair.a.u64)), dev.add_column(CM.write_bitpacked(pair.b.u64))
        with pytest.raises(ta.TantivyAmdError) as ei:
            dev.raw_agg_terms_sub(queries, ha, hb, GM.I64, SM.METRIC_DESC, 10, SM.AVG)
        assert ei.value.code == ERR_UNSUPPORTED and "query 1" in str(ei.value) and "tq_agg_terms_sub_batch" in str(ei.value)
        dev.set_option("docset_trees", 1)
        _assert_sub(dev.raw_agg_terms_sub(queries, ha, hb, GM.I64, SM.METRIC_DESC, 10, SM.AVG), want, pair.plan, "trees")
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == B.KERNEL_AGG_TERMS_SUB | B.KERNEL_DOCSET_TREE | B.KERNEL_PHRASE_SLOP, st
        assert int(dev.last_batch_slop_overflows(len(queries)).sum()) == 0
    finally:
        dev.close()


# ---- 8. refusals
def test_refusals_leave_the_segment_usable(ta, small):
    import torch

    dev, queries, match = small["dev"], small["queries"], small["match"]
    B = ta.binding
    ha, hb, pair = _small_pair(small, False)
    want = [pair.want(match[0], SM.METRIC_DESC, 10, SM.AVG)]

    def still_good():
        _assert_sub(dev.raw_agg_terms_sub(queries[:1], ha, hb, GM.U64, SM.METRIC_DESC, 10, SM.AVG), want, pair.plan, "after a refusal")
        rc, docs, starts = dev.raw_docset(queries[:1], match[0].size)
        assert rc == 0 and np.array_equal(docs[: int(starts[1])], match[0]), _err(ta)

    def refused(call, code, *words):
        with pytest.raises(ta.TantivyAmdError) as ei:
            call()
        assert ei.value.code == code and all(w in str(ei.value) for w in words), ei.value
        still_good()

    def call(column=ha, metric_column=hb, vt=GM.U64, order=SM.METRIC_DESC, size=10, metric=SM.AVG, qs=queries, **kw):
        return lambda: dev.raw_agg_terms_sub(qs, column, metric_column, vt, order, size, metric, **kw)

    still_good()
    fn = "tq_agg_terms_sub_batch"
    # everything tq_agg_terms_batch refuses
    refused(call(column=B.MAX_COLUMNS), ERR_INVALID, fn, "column")
    refused(call(column=7), ERR_INVALID, fn, "column 7")  # (no such upload)
    refused(call(size=0), ERR_INVALID, fn, "segment_size")
    refused(call(size=B.agg_terms_max_size() + 1), ERR_INVALID, fn, "segment_size")
    refused(call(stride=9), ERR_INVALID, fn, "out_stride")
    wide = bitpacked_values(np.random.default_rng(3), small["seg"].max_doc, 17, 5, 1)
    extra = dev.add_column(CM.write_bitpacked(wide))
    refused(call(column=extra), ERR_UNSUPPORTED, fn, "n_keys", "131072")
    # ... and its own
    refused(call(order=6), ERR_INVALID, fn, "order")
    refused(call(metric=5), ERR_INVALID, fn, "order_metric")
    refused(call(reserved=(0, 1)), ERR_INVALID, fn, "reserved")
    refused(call(reserved=(1, 0)), ERR_INVALID, fn, "reserved")
    refused(call(metric_column=B.MAX_COLUMNS), ERR_INVALID, fn, "metric column")
    refused(call(metric_column=7), ERR_INVALID, fn, "metric column 7")
    refused(call(vt=3), ERR_INVALID, fn, "metric value_type")
    refused(call(vt=GM.F64, metric=SM.SUM), ERR_UNSUPPORTED, fn, "SUM", "F64")
    refused(call(vt=GM.F64, metric=SM.AVG, order=SM.METRIC_ASC), ERR_UNSUPPORTED, fn, "AVG", "F64")
    # an order_metric above AVG is read under the metric orders alone; F64 min / max / count and the old orders are served
    dev.raw_agg_terms_sub(queries, ha, hb, GM.U64, SM.COUNT_DESC, 10, 9)
    dev.raw_agg_terms_sub(queries, ha, hb, GM.F64, SM.METRIC_DESC, 10, SM.MAX)
    dev.raw_agg_terms_sub(queries, ha, hb, GM.F64, SM.KEY_ASC, 10, SM.AVG)
    # the wide column as the METRIC is fine: only the key column is planned
    assert int(dev.raw_agg_terms_sub(queries[:1], ha, extra, GM.U64, SM.METRIC_DESC, 10, SM.MAX)[0][0]["count"]) == match[0].size
    dev.column_release(extra)
    refused(call(metric_column=extra), ERR_INVALID, fn, "metric column")
    # the doc-set path's refusals under this function's name
    refused(call(qs=queries[:2] + [(O.MODE_PHRASE, [1, 2], [0, 1])]), ERR_UNSUPPORTED, fn, "query 2")
    refused(call(qs=queries[:1] + [(ta.MODE_BOOL, [1, 2], [M, 3], [0, 1], 0)]), ERR_INVALID, fn, "query 1")
    # the terms call keeps refusing the metric orders
    with pytest.raises(ta.TantivyAmdError) as ei:
        dev.raw_agg_terms(queries, ha, SM.METRIC_DESC, 10)
    assert ei.value.code == ERR_INVALID and "tq_agg_terms_batch" in str(ei.value) and "order" in str(ei.value)
    still_good()
    # null outputs (the device variant takes the pointers as they are)
    n = len(queries)
    d_terms = torch.zeros(n * 5, dtype=torch.int64, device="cuda:0")
    d_keys = torch.zeros(n * 10, dtype=torch.int64, device="cuda:0")
    d_counts = torch.zeros(n * 10, dtype=torch.int32, device="cuda:0")
    d_recs = torch.zeros(n * 50, dtype=torch.int64, device="cuda:0")
    for args in ((d_terms, None, d_counts, d_recs), (d_terms, d_keys, None, d_recs), (None, d_keys, d_counts, d_recs), (d_terms, d_keys, d_counts, None)):
        rc = dev.raw_agg_terms_sub_device(queries, ha, hb, GM.U64, SM.METRIC_DESC, 10, SM.AVG, 10, *args)
        assert rc == ERR_INVALID and "tq_agg_terms_sub_batch_device" in _err(ta) and "null" in _err(ta)
        still_good()


# ---- 9. the byte model and the mask
@pytest.mark.parametrize("b_optional", [False, True])
def test_stats_follow_the_byte_model(ta, small, b_optional):
    dev, queries, match, lists = small["dev"], small["queries"], small["match"], small["lists"]
    B = ta.binding
    ha, hb, pair = _small_pair(small, not b_optional)  # (A Optional with B Full, A Full with B Optional)
    a_optional = not b_optional
    n_words = (small["seg"].max_doc + 31) // 32
    sizes = [m.size for m in match]
    for size, order in ((7, SM.METRIC_DESC), (1024, SM.COUNT_DESC)):
        for slices in (1, 2):
            dev.set_option("agg_slices", slices)
            want = [pair.want(m, order, size, SM.AVG) for m in match]
            _assert_sub(dev.raw_agg_terms_sub(queries, ha, hb, GM.U64, order, size, SM.AVG), want, pair.plan, ("stats", b_optional, size, slices))
            st = dev.last_batch_stats()
            assert st["kernel_mask"] == B.KERNEL_AGG_TERMS_SUB and st["kernels"] == ["agg_terms_sub"]
            assert dev.last_batch_match_counts(len(queries)).tolist() == sizes
            assert st["matches"] == sum(sizes)
            valued = sum(w[0]["count"] for w in want)  # docs with a value in A = the counted docs
            returned = sum(w[0]["n_returned"] for w in want)
            with_b = sum(r["count"] for m in match for r in pair.table(m)[2])
            assert (valued < sum(sizes)) == a_optional and (with_b < valued) == b_optional and returned > 0
            assert st["algorithmic_bytes"] == (sum(lists) * n_words * 4 + 8 * valued + (8 * sum(sizes) if a_optional else 0) +
                                               len(queries) * (40 + 4 * pair.plan["n_keys"]) + 12 * returned +
                                               8 * with_b + (8 * valued if b_optional else 0) +
                                               len(queries) * 40 * pair.plan["n_keys"] + 40 * returned)
    dev.set_option("agg_slices", 0)
    # the other aggregation calls enqueue what they did
    plain = dev.raw_agg_terms(queries, ha, TM.COUNT_DESC, 7)
    st = dev.last_batch_stats()
    assert st["kernel_mask"] == B.KERNEL_AGG_TERMS and [int(t["count"]) for t in plain[0]] == [pair.table(m)[3] for m in match]


# ---- 10. two segments through the host merge
def test_two_segments_merge_and_finalize(ta):
    """The walk segment twice, with other columns: merge_terms_sub + terms_sub_finalize against the model over the
    concatenation.  segment_size holds every entry, so the merged result is exact; key 0 has docs in both segments and a
    value in B in neither: it sorts as f64::MIN at the final stage, last under DESC and first under ASC, though other
    averages are negative (at the segment stage it ordered as 0, in the middle)."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    rng = np.random.default_rng(20261205)
    parts = []
    for s in range(2):
        idx = rng.integers(0, 30 + 5 * s, size=md)
        idx[:40] = np.arange(40) % (30 + 5 * s)
        has_b = idx != 0
        typed = rng.integers(-900, 1000, size=md) + (idx - 15) * 100  # (a key's average follows its index: both signs)
        b_vals = np.array([GM.to_u64(int(x), GM.I64) for x in typed[has_b]], np.uint64)
        parts.append(Pair(np.uint64(500) + np.uint64(10) * idx.astype(np.uint64), None, b_vals, has_b, GM.I64, md))
    queries = _walk_queries(ta, sparse)[:2]
    batch = [q for q, _ in queries]
    dev = ta.DeviceIndex([seg, seg])
    try:
        for s in range(2):
            for t in range(len(seg.terms)):
                dev.term_handle(t, segment_ord=s)
        got = []
        for s, pair in enumerate(parts):
            ha = dev.add_column(CM.write_bitpacked(pair.a.u64), segment_ord=s)
            hb = dev.add_column(CM.write_bitpacked(pair.b.u64[pair.b.has]), CM.OPTIONAL, CM.presence_words(pair.b.has), segment_ord=s)
            out = dev.raw_agg_terms_sub(batch, ha, hb, GM.I64, SM.METRIC_DESC, 100, SM.AVG, segment_ord=s)
            _assert_sub(out, [pair.want(m, SM.METRIC_DESC, 100, SM.AVG) for _, m in queries], pair.plan, ("segment", s))
            got.append(out)
            # at the segment stage the key without a value orders as 0, inside the range
            row = _recs_as_dicts(out[3][0, : int(out[0][0]["n_returned"])])
            at = [i for i, r in enumerate(row) if r["count"] == 0]
            assert len(at) == 1 and 0 < at[0] < len(row) - 1 and int(out[1][0, at[0]]) == 500
        for qi, (_, match) in enumerate(queries):
            merged = B.merge_terms_sub([(g[1][qi], g[2][qi], g[3][qi], g[0][qi]) for g in got])
            assert merged["sum_other_doc_count"] == 0 and merged["doc_count_error_upper_bound"] == 0
            # the model over the concatenation
            a = np.concatenate([p.a.u64 for p in parts])
            b = np.concatenate([p.b.u64 for p in parts])
            has_b = np.concatenate([p.b.has for p in parts])
            docs = np.concatenate([match.astype(np.int64), match.astype(np.int64) + md])
            info = TM.column_info(a)
            plan, per, records, _ = SM.per_key(a, np.ones(2 * md, bool), docs, info, b, has_b, GM.I64)
            entries = {plan["min_value"] + plan["gcd"] * i: (int(per[i]), records[i]) for i in np.nonzero(per)[0].tolist()}
            assert {k: (c, {f: r[f] for f in SM.RECORD_FIELDS}) for k, (c, r) in merged["entries"].items()} == entries
            for order in METRIC_ORDERS:
                for metric in SM.METRICS:
                    fin = B.terms_sub_finalize(merged, GM.I64, size=12, order=order, order_metric=metric)

                    def final_value(r):  # get_value_from_aggregation(..).unwrap_or(f64::MIN)
                        if metric in (SM.MIN, SM.MAX, SM.AVG) and not r["count"]:
                            return Fraction(-GM.F64_MAX)
                        v = SM.metric_rational(r, GM.I64, metric)
                        return Fraction(float(v)) if metric == SM.AVG else v

                    ordered = sorted(entries, key=lambda k: (-final_value(entries[k][1]) if order == SM.METRIC_DESC else final_value(entries[k][1]), k))
                    assert [k for k, _, _ in fin["buckets"]] == ordered[:12], (qi, order, metric)
                    assert [c for _, c, _ in fin["buckets"]] == [entries[k][0] for k in ordered[:12]]
                    assert fin["sum_other_doc_count"] == sum(entries[k][0] for k in ordered[12:])
                    if metric in (SM.MIN, SM.MAX, SM.AVG):
                        full = [k for k, _, _ in B.terms_sub_finalize(merged, GM.I64, size=1000, order=order, order_metric=metric)["buckets"]]
                        assert full.index(500) == (len(full) - 1 if order == SM.METRIC_DESC else 0)
                        assert any(final_value(r) < 0 for _, r in entries.values() if r["count"])
    finally:
        dev.close()
