"""GPU parity of the terms x histogram aggregation (tq_agg_terms_hist_batch*: tantivy_amd/csrc/tq_agg_terms_hist.cpp,
tq_agg_terms_hist.hip — per key of a column T its doc count and a dense histogram of a column H, the top segment_size keys
by doc count or by key, per query of a batch).

Expectations never come from the device: the column bytes are written by tests/column_model.py from values the test
chose, the match sets come from the oracle's decode / tests/all_model.py / tests/slop_model.py, and the record with its
rows of keys, counts and histogram rows is tests/terms_hist_model.closed_form — exact integers and IEEE double arithmetic
that tests/test_agg_terms_hist_model_cpu.py ties to the literal per-doc loop and to the reference's own unit tests.  Every
comparison is exact (there is no tolerance in this file), and out_of_range is 0 in every case.  Segments and queries are
those of tests/test_gpu_agg.py and tests/test_gpu_agg_terms.py, by import."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import agg_model as GM
from tests import all_model as AM
from tests import column_model as CM
from tests import phrase_model as PM
from tests import terms_hist_model as HM
from tests import terms_model as TM
from tests.test_column_model_cpu import bitpacked_values
from tests.test_gpu_agg import AggLists, _err, _walk_queries, _walk_segment, small, ta  # noqa: F401 (ta, small: fixtures)
from tests.test_gpu_agg_terms import _random_keys
from tests.test_gpu_all import STAR, T, _flat, _model_clauses
from tests.test_gpu_docset import ERR_INVALID, ERR_UNSUPPORTED
from tests.test_gpu_range import _query_columns, _upload
from tests.test_gpu_round3 import _alive_bytes
from tests.test_gpu_term_set import _prepare_all_terms, _synth_segment
from tests.tree_shapes import to_device

pytestmark = pytest.mark.gpu

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
FILL64, FILL32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
HOUR_NS = 3_600_000_000_000


class Grid:
    """The models of a key column T and a histogram column H (h_vals None: H is T) with the closed form over them."""

    def __init__(self, t_vals, t_present, h_vals, h_present, vt, md, histogram):
        self.t = GM.Column(t_vals, t_present, md)
        self.h = self.t if h_vals is None else GM.Column(h_vals, h_present, md)
        self.vt, self.histogram = vt, histogram
        self.plan = HM.plan(TM.column_info(t_vals), dict(self.h.info, gcd=1), vt, histogram)
        self._grids = {}

    def grid(self, match):
        key = np.asarray(match, np.uint32).tobytes()
        if key not in self._grids:
            self._grids[key] = HM.grid(self.t.u64, self.t.has, self.h, self.vt, match, self.plan)
        return self._grids[key]

    def want(self, match, order, size):
        return HM.closed_form(self.t.u64, self.t.has, self.h, self.vt, match, self.plan, order, size, self.grid(match))

    def with_h(self, match):
        """the counted docs with a value in H"""
        m = np.asarray(match, np.int64)
        return int((self.t.has[m] & self.h.has[m]).sum())


def _assert_hist(got, want, plan, where):
    """got = (terms, keys, counts, rows, plan) of raw_agg_terms_hist; want = [(record, keys, counts, rows)] of the closed form."""
    terms, keys, counts, rows, got_plan = got
    assert got_plan == plan, (where, got_plan, plan)
    nb = plan["hist"]["n_buckets"]
    assert len(terms) == len(keys) == len(counts) == len(rows) == len(want), where
    for i, (rec, wkeys, wcounts, wrows) in enumerate(want):
        g = {k: int(terms[i][k]) for k in TM.FIELDS}
        assert g == rec, (where, i, g, rec)
        assert g["out_of_range"] == 0
        n = rec["n_returned"]
        assert n <= keys.shape[1], (where, i)
        assert keys[i, :n].tolist() == wkeys, (where, i, keys[i, :n].tolist()[:8], wkeys[:8])
        assert counts[i, :n].tolist() == wcounts, (where, i)
        assert rows[i, :n, :nb].tolist() == wrows, (where, i)
        assert rec["count"] == sum(wcounts) + rec["sum_other_doc_count"]
        assert all(sum(r) <= c for r, c in zip(wrows, wcounts))


def _i64_col(typed):
    return np.array([GM.to_u64(int(x), GM.I64) for x in typed], np.uint64)


def _f64_col(typed):
    return np.array([GM.to_u64(float(x), GM.F64) for x in typed], np.uint64)


# ---- 1. the codecs, the value types and the grid at its edges (and 6.: several slices per query)
def _edge_case(name, md):
    """-> (T codec, values, present | None, H codec | None, values | None, present | None, value type of H, histogram)"""
    rng = np.random.default_rng(20261121)
    half = rng.random(md) < 0.5
    half[0] = half[md - 1] = True
    third = rng.random(md) < 0.35
    third[0] = True
    nh, n3 = int(half.sum()), int(third.sum())
    ts = np.sort(rng.integers(1_700_000_000, 1_700_000_000 + 120 * 3600, size=md)).astype(np.uint64)
    ts[5::97] = (ts[5::97] // np.uint64(3600)) * np.uint64(3600)  # values on a bucket boundary, without and with the offset
    ts[6::97] = (ts[6::97] // np.uint64(3600)) * np.uint64(3600) + np.uint64(1800)
    dates = np.sort(rng.integers(-40 * HOUR_NS, 80 * HOUR_NS, size=md))
    dates[3::50] = (dates[3::50] // HOUR_NS) * HOUR_NS  # on a boundary, below and above zero
    dates = _i64_col(dates)
    floats = rng.normal(0.0, 3.0, size=md)
    floats[7::40] = np.floor(floats[7::40] * 2.0) / 2.0 + 0.25  # k * interval + offset exactly
    floats = _f64_col(floats)
    status = _random_keys(rng, md, 7, 200, 100)
    skew = np.uint64(5) + np.uint64(10) * (rng.zipf(1.4, size=md) % 12).astype(np.uint64)
    skew[0], skew[-1] = 5, 5 + 10 * 11
    many = _random_keys(rng, md, 300, (1 << 60) + 3, 8)
    hour, hour_ns = {"interval": 3600.0}, {"interval": float(HOUR_NS)}
    cases = {
        "T bitpacked | H bitpacked u64": (CM.BITPACKED, status, None, CM.BITPACKED, ts, None, GM.U64, hour),
        "T linear gcd 10 | H linear i64 dates": (CM.LINEAR, skew, None, CM.LINEAR, dates, None, GM.I64, hour_ns),
        "T blockwise above 2^53 gcd 8 | H blockwise u64, offset": (CM.BLOCKWISE, many, None, CM.BLOCKWISE, ts, None, GM.U64,
                                                                  {"interval": 3600.0, "offset": 1800.0}),
        "T bitpacked | H bitpacked f64": (CM.BITPACKED, status, None, CM.BITPACKED, floats, None, GM.F64, {"interval": 0.5, "offset": 0.25}),
        "T optional bitpacked | H optional blockwise u64": (CM.BITPACKED, status[:nh], half, CM.BLOCKWISE, ts[:n3], third, GM.U64, hour),
        "T optional linear | H optional linear i64 dates, hard bounds": (CM.LINEAR, skew[:nh], half, CM.LINEAR, dates[:n3], third, GM.I64,
                                                                        {"interval": float(HOUR_NS), "hard_bounds": (-10.0 * HOUR_NS, 30.0 * HOUR_NS)}),
        "T optional blockwise | H optional bitpacked f64": (CM.BLOCKWISE, many[:nh], half, CM.BITPACKED, floats[:n3], third, GM.F64,
                                                           {"interval": 0.25}),
        "one key": (CM.BITPACKED, np.full(md, 77, np.uint64), None, CM.BITPACKED, ts, None, GM.U64, hour),
        "one bucket": (CM.BITPACKED, status, None, CM.BITPACKED, ts, None, GM.U64, {"interval": 1e12}),
        "no bucket: hard bounds that hold no value": (CM.BITPACKED, status, None, CM.BITPACKED, ts, None, GM.U64,
                                                      {"interval": 3600.0, "hard_bounds": (0.0, 10.0)}),
        "no bucket: H without a value": (CM.BITPACKED, status, None, CM.BITPACKED, np.zeros(0, np.uint64), np.zeros(md, bool), GM.U64, hour),
        "H is T": (CM.BITPACKED, status, None, None, None, None, GM.U64, {"interval": 250.0}),
    }
    return cases[name]


EDGE_CASES = ["T bitpacked | H bitpacked u64", "T linear gcd 10 | H linear i64 dates", "T blockwise above 2^53 gcd 8 | H blockwise u64, offset",
              "T bitpacked | H bitpacked f64", "T optional bitpacked | H optional blockwise u64",
              "T optional linear | H optional linear i64 dates, hard bounds", "T optional blockwise | H optional bitpacked f64", "one key",
              "one bucket", "no bucket: hard bounds that hold no value", "no bucket: H without a value", "H is T"]


@pytest.mark.parametrize("case", EDGE_CASES)
def test_codecs_value_types_and_the_grid_at_its_edges(ta, case):
    """The walk segment (16 421 docs: 514 bitmap words, the last of 5 docs) under 1, 3, 256 slices — cells then take adds
    from several workgroups — and the host's choice; `*`, the sparse term, and a query matching nothing; T and H across the
    three codecs, Full and Optional; H as U64, I64 dates and F64 with values on bucket boundaries; keys at index 0 and
    n_keys - 1; one key, one bucket, no bucket, and H = T."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    codec_t, vals_t, present_t, codec_h, vals_h, present_h, vt, histogram = _edge_case(case, md)
    grid = Grid(vals_t, present_t, vals_h, present_h, vt, md, histogram)
    plan = grid.plan
    nk, nb = plan["terms"]["n_keys"], plan["hist"]["n_buckets"]
    queries = _walk_queries(ta, sparse)
    batch = [q for q, _ in queries]
    size = 5
    want = {o: [grid.want(m, o, size) for _, m in queries] for o in TM.ORDERS}
    star = grid.want(queries[0][1], TM.KEY_ASC, 1024)
    assert want[TM.COUNT_DESC][2][0]["matches"] == 0 and want[TM.COUNT_DESC][2][1] == []
    assert star[1][0] == plan["terms"]["min_value"] and star[1][-1] == plan["terms"]["min_value"] + plan["terms"]["gcd"] * (nk - 1)
    assert (nk == 1) == (case == "one key") and (nb == 1) == (case == "one bucket") and (nb == 0) == case.startswith("no bucket")
    if nk > size:
        assert want[TM.COUNT_DESC][0][0]["sum_other_doc_count"] > 0
    if nb > 1 and case != "H is T":  # a value on a boundary: the bucket's key itself
        f = GM.f64_array(grid.h.u64[grid.h.has], vt)
        on = (f - histogram.get("offset", 0.0)) / histogram["interval"]
        assert int((on == np.floor(on)).sum()) > 20
    if present_h is not None or "hard_bounds" in histogram:
        assert any(sum(r) < c for r, c in zip(star[3], star[2]))  # (docs counted under a key and in no bucket)
    else:
        assert all(sum(r) == c for r, c in zip(star[3], star[2]))
    if nb > 1 and present_t is None:
        assert sum(r[0] for r in star[3]) > 0 and sum(r[-1] for r in star[3]) > 0  # (the first and the last bucket hold docs)
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        _, ht = _upload(dev, codec_t, vals_t, present_t)
        hh = ht if codec_h is None else _upload(dev, codec_h, vals_h, present_h)[1]
        for slices in (1, 3, 256, 0):
            dev.set_option("agg_slices", slices)
            for order in TM.ORDERS:
                got = dev.raw_agg_terms_hist(batch, ht, hh, vt, histogram, order, size)
                _assert_hist(got, want[order], plan, (case, slices, order))
                assert dev.last_batch_match_counts(len(batch)).tolist() == [m.size for _, m in queries]
        _assert_hist(dev.raw_agg_terms_hist(batch[:1], ht, hh, vt, histogram, TM.KEY_ASC, 1024), [star], plan, (case, "every key"))
    finally:
        dev.close()


# ---- 2. the LDS capacities and the global path
GRID_CASES = {"small": (64, 31), "small + 1": (3, 682), "small + 1, short rows": (683, 2), "large": (128, 63), "large + 1": (3, 2730),
              "large + 1, short rows": (2731, 2), "the largest grid": (256, 255), "one cell": (1, 0)}


@pytest.mark.parametrize("lds_buckets", [None, 16])
@pytest.mark.parametrize("case", sorted(GRID_CASES))
def test_grids_around_the_lds_capacities(ta, case, lds_buckets):
    """n_cells = n_keys x (n_buckets + 1) at and one past each instantiation's LDS table, with long and with short rows, the
    largest grid served (65 536 cells) and the smallest; each with "agg_lds_buckets" at its default and at 16 (all but the
    one-cell grid are then counted with atomics on the scratch row): the same rows.  One heavy cell."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    caps = B.agg_terms_hist_lds_capacities()
    nk, nb = GRID_CASES[case]
    cells = {"small": caps[0], "small + 1": caps[0] + 1, "small + 1, short rows": caps[0] + 1, "large": caps[1], "large + 1": caps[1] + 1,
             "large + 1, short rows": caps[1] + 1, "the largest grid": B.AGG_MAX_BUCKETS, "one cell": 1}[case]
    assert nk * (nb + 1) == cells
    rng = np.random.default_rng(5)
    vals_t = _random_keys(rng, md, nk, 1 << 40, 1)
    vals_h = _random_keys(rng, md, nb, 50, 1) if nb else None
    if nb:
        vals_t[1:md // 3], vals_h[1:md // 3] = vals_t[1], vals_h[1]  # (one heavy cell)
        grid = Grid(vals_t, None, vals_h, None, GM.U64, md, {"interval": 1.0})
    else:  # the one-cell grid: one key, and bounds that hold no value
        grid = Grid(vals_t, None, None, None, GM.U64, md, {"interval": 1.0, "hard_bounds": (0.0, 1.0)})
    assert (grid.plan["terms"]["n_keys"], grid.plan["hist"]["n_buckets"], grid.plan["n_cells"]) == (nk, nb, cells)
    queries = _walk_queries(ta, sparse)
    size = 65
    want = {o: [grid.want(m, o, size) for _, m in queries] for o in (TM.COUNT_DESC, TM.KEY_DESC)}
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        ht = dev.add_column(CM.write_bitpacked(vals_t))
        hh = dev.add_column(CM.write_bitpacked(vals_h)) if nb else ht
        if lds_buckets is not None:
            dev.set_option("agg_lds_buckets", lds_buckets)
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            for order in want:
                got = dev.raw_agg_terms_hist([q for q, _ in queries], ht, hh, GM.U64, grid.histogram, order, size)
                _assert_hist(got, want[order], grid.plan, (case, lds_buckets, slices, order))
    finally:
        dev.close()


# ---- 3. binding hard bounds and an Optional H
def test_outside_docs_keep_the_doc_counts(ta, small):
    """T the fixture's Optional column (512 keys), H its Full one under hard bounds that cut both ends, then H = an Optional
    column: a key's doc_count is every doc with that key, its row the in-bounds docs alone; a doc without a value in T
    enters nothing.  Checked against plain numpy counts beside the model."""
    dev, queries, match = small["dev"], small["queries"], small["match"]
    md = small["seg"].max_doc
    t, h = small["omodel"], small["model"]
    lo, hi = float((1 << 40) + 2_000_000), float((1 << 40) + 6_000_000)
    histogram = {"interval": 100_000.0, "hard_bounds": (lo, hi)}
    grid = Grid(t.u64[t.has], t.has, h.u64, None, GM.U64, md, histogram)
    assert grid.plan["hist"]["n_buckets"] == 41 and grid.plan["terms"]["n_keys"] == 512
    want = [grid.want(m, TM.KEY_ASC, 1024) for m in match]
    got = dev.raw_agg_terms_hist(queries, small["ocol"], small["col"], GM.U64, histogram, TM.KEY_ASC, 1024)
    _assert_hist(got, want, grid.plan, "hard bounds that bind")
    for i, m in enumerate(match):
        with_key = m[t.has[m]]
        n = int(got[0][i]["n_returned"])
        assert int(got[0][i]["matches"]) == m.size and int(got[0][i]["count"]) == with_key.size < m.size
        keys, per_key = np.unique(t.u64[with_key], return_counts=True)
        assert got[1][i, :n].tolist() == keys.tolist() and got[2][i, :n].tolist() == per_key.tolist()
        f = h.u64[with_key].astype(np.float64)
        inb = (lo <= f) & (f <= hi)
        assert 0 < int(inb.sum()) < with_key.size
        assert int(got[3][i, :n].sum()) == int(inb.sum())
        for j in (0, n // 2, n - 1):
            mine = t.u64[with_key] == got[1][i, j]
            assert int(got[3][i, j].sum()) == int((mine & inb).sum()) <= int(got[2][i, j]) == int(mine.sum())
    # an Optional H: a new column over the same docs
    rng = np.random.default_rng(31)
    some = rng.random(md) < 0.4
    ovals = bitpacked_values(rng, int(some.sum()), 10, 0, 1)
    extra = dev.add_column(CM.write_bitpacked(ovals), CM.OPTIONAL, CM.presence_words(some))
    try:
        g2 = Grid(t.u64[t.has], t.has, ovals, some, GM.U64, md, {"interval": 64.0})
        got = dev.raw_agg_terms_hist(queries, small["ocol"], extra, GM.U64, {"interval": 64.0}, TM.COUNT_DESC, 1024)
        _assert_hist(got, [g2.want(m, TM.COUNT_DESC, 1024) for m in match], g2.plan, "an Optional H")
        for i, m in enumerate(match):
            n = int(got[0][i]["n_returned"])
            assert int(got[3][i, :n].sum()) == int((t.has[m] & some[m]).sum()) < int(got[2][i, :n].sum()) == int(t.has[m].sum())
    finally:
        dev.column_release(extra)


# ---- 4. the cut
def _tie_columns(md):
    """T: Optional, docs below 16 400 hold key 100 + 3 x (doc % 40): `*` gives every key 410 docs; H = 7 x doc"""
    docs = np.arange(md, dtype=np.uint64)
    present = np.arange(md) < 16400
    return (docs[:16400] % np.uint64(40)) * np.uint64(3) + np.uint64(100), present, docs * np.uint64(7)


def test_the_cut_under_the_four_orders(ta):
    """40 keys with equal counts under `*`, segment_size 7: the ties at the cut go to the ascending key under both count
    orders; the record fields; the rows returned are the survivors', in order."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    vals_t, present_t, vals_h = _tie_columns(md)
    histogram = {"interval": 1000.0}
    grid = Grid(vals_t, present_t, vals_h, None, GM.U64, md, histogram)
    assert grid.plan["terms"]["n_keys"] == 40 and grid.plan["hist"]["n_buckets"] == 115
    queries = _walk_queries(ta, sparse)
    batch = [q for q, _ in queries]
    want = {o: [grid.want(m, o, 7) for _, m in queries] for o in TM.ORDERS}
    for order, first in ((TM.COUNT_DESC, 0), (TM.COUNT_ASC, 0), (TM.KEY_ASC, 0), (TM.KEY_DESC, 33)):
        rec, keys, counts, rows = want[order][0]
        assert sorted(keys) == [100 + 3 * k for k in range(first, first + 7)] and counts == [410] * 7, order
        assert rec == {"matches": md, "count": 16400, "sum_other_doc_count": 33 * 410, "distinct": 40, "n_returned": 7,
                       "doc_count_error_upper_bound": 410, "out_of_range": 0}
        # a key's docs are 40 apart: a row holds all of them, and the rows differ
        assert all(sum(r) == 410 for r in rows) and len({tuple(r) for r in rows}) > 1
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        _, ht = _upload(dev, CM.BITPACKED, vals_t, present_t)
        hh = dev.add_column(CM.write_bitpacked(vals_h))
        for order in TM.ORDERS:
            _assert_hist(dev.raw_agg_terms_hist(batch, ht, hh, GM.U64, histogram, order, 7), want[order], grid.plan, ("the cut", order))
        for size in (39, 40, 41, 1024):
            for order in (TM.COUNT_ASC, TM.KEY_DESC):
                w = [grid.want(m, order, size) for _, m in queries]
                assert w[0][0]["n_returned"] == min(size, 40) and (w[0][0]["sum_other_doc_count"] == 0) == (size >= 40)
                _assert_hist(dev.raw_agg_terms_hist(batch, ht, hh, GM.U64, histogram, order, size), w, grid.plan, ("sizes", order, size))
    finally:
        dev.close()


def test_host_and_device_rows_strides_and_guards(ta):
    """Strides above need, host and device: the host variant writes zeros from n_returned to min(segment_size, n_keys) and
    nothing past them; the device variant touches nothing at or past n_returned of a row set, nor at or past n_buckets of a
    histogram row — keys, counts and histogram rows alike —, in buffers that are used twice."""
    import torch

    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    vals_t, present_t, vals_h = _tie_columns(md)
    histogram = {"interval": 1000.0}
    grid = Grid(vals_t, present_t, vals_h, None, GM.U64, md, histogram)
    nb = grid.plan["hist"]["n_buckets"]
    queries = _walk_queries(ta, sparse)
    batch = [q for q, _ in queries]
    n = len(batch)
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        _, ht = _upload(dev, CM.BITPACKED, vals_t, present_t)
        hh = dev.add_column(CM.write_bitpacked(vals_h))
        for order, size, stride, hist_stride in ((TM.COUNT_DESC, 7, 12, nb + 5), (TM.KEY_DESC, 45, 43, nb), (TM.COUNT_ASC, 7, 7, nb + 1)):
            width = min(size, 40)
            want = [grid.want(m, order, size) for _, m in queries]
            returned = [w[0]["n_returned"] for w in want]
            assert returned[0] == width and 0 < returned[1] <= width and returned[2] == 0
            host = dev.raw_agg_terms_hist(batch, ht, hh, GM.U64, histogram, order, size, stride=stride, hist_stride=hist_stride)
            _assert_hist(host, want, grid.plan, ("host rows", order, size))
            assert host[1].shape == (n, stride) and host[3].shape == (n, stride, hist_stride)
            for i, r in enumerate(returned):
                assert np.all(host[1][i, r:width] == 0) and np.all(host[2][i, r:width] == 0) and np.all(host[3][i, r:width, :nb] == 0), i
                assert np.all(host[1][i, width:] == 0xDEADBEEF) and np.all(host[2][i, width:] == 0xDEADBEEF)  # (nothing past the width)
                assert np.all(host[3][i, width:] == 0xDEADBEEF) and np.all(host[3][i, :, nb:] == 0xDEADBEEF)
            # device buffers a caller owns, used twice; two row sets and two records more than the batch has queries
            d_terms = torch.full(((n + 2) * 5,), FILL64, dtype=torch.int64, device="cuda:0")
            d_keys = torch.full(((n + 2) * stride,), FILL64, dtype=torch.int64, device="cuda:0")
            d_counts = torch.full(((n + 2) * stride,), FILL32, dtype=torch.int32, device="cuda:0")
            d_rows = torch.full(((n + 2) * stride * hist_stride,), FILL32, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            for call in (0, 1):  # the second call accumulates into the same scratch: the call zeroes what it adds to
                rc = dev.raw_agg_terms_hist_device(batch, ht, hh, GM.U64, histogram, order, size, stride, hist_stride, d_terms, d_keys,
                                                   d_counts, d_rows)
                assert rc == 0, _err(ta)
                dev.last_batch_stats()  # (waits for the batch)
                torch.cuda.synchronize()
                terms = d_terms.cpu().numpy().view(np.uint64)
                keys = d_keys.cpu().numpy().view(np.uint64).reshape(n + 2, stride)
                counts = d_counts.cpu().numpy().view(np.uint32).reshape(n + 2, stride)
                rows = d_rows.cpu().numpy().view(np.uint32).reshape(n + 2, stride, hist_stride)
                _assert_hist((terms[: n * 5].view(B.AGG_TERMS_DTYPE), keys[:n], counts[:n], rows[:n], grid.plan), want, grid.plan,
                             ("device buffers", order, size, call))
                for i, r in enumerate(returned):
                    assert np.all(keys[i, r:] == FILL64) and np.all(counts[i, r:] == FILL32), (order, call, i)
                    assert np.all(rows[i, r:] == FILL32) and np.all(rows[i, :, nb:] == FILL32), (order, call, i)
                assert np.all(keys[n:] == FILL64) and np.all(counts[n:] == FILL32) and np.all(rows[n:] == FILL32)
                assert np.all(terms[n * 5:] == FILL64)
                assert host[0].tobytes() == terms[: n * 5].tobytes()  # the host and the device variant agree bit for bit
            on_dev = dev.raw_agg_terms_hist(batch, ht, hh, GM.U64, histogram, order, size, device=True)
            _assert_hist(on_dev, want, grid.plan, ("device rows through the binding", order, size))
    finally:
        dev.close()


# ---- 5. two identities against the calls that exist
def test_the_terms_half_is_the_terms_call_and_the_column_sums_are_the_histogram(ta, small):
    dev, queries, match = small["dev"], small["queries"], small["match"]
    md = small["seg"].max_doc
    B = ta.binding
    histogram = {"interval": 82_000.0, "offset": 11.0}
    # T Optional (512 keys), H Full: record, keys and counts are raw_agg_terms', bit for bit
    for order in TM.ORDERS:
        for size in (7, 600):
            plain = dev.raw_agg_terms(queries, small["ocol"], order, size)
            got = dev.raw_agg_terms_hist(queries, small["ocol"], small["col"], GM.U64, histogram, order, size)
            assert got[0].tobytes() == plain[0].tobytes() and got[4]["terms"] == plain[3], (order, size)
            for i in range(len(queries)):
                n = int(plain[0][i]["n_returned"])
                assert n > 0 and got[1][i, :n].tobytes() == plain[1][i, :n].tobytes() and got[2][i, :n].tobytes() == plain[2][i, :n].tobytes()
    # a Full T with segment_size >= n_keys: the column sums of the rows are raw_agg's histogram row of H
    vals_t = _random_keys(np.random.default_rng(41), md, 300, 9, 4)
    extra = dev.add_column(CM.write_bitpacked(vals_t))
    try:
        for h_col, h_hist in ((small["col"], histogram), (small["ocol"], {"interval": 100.0})):
            got = dev.raw_agg_terms_hist(queries, extra, h_col, GM.U64, h_hist, TM.KEY_ASC, 300)
            stats, rows, plan = dev.raw_agg(queries, h_col, B.VALUE_U64, h_hist)
            assert got[4]["hist"] == plan and got[4]["terms"]["n_keys"] == 300 and plan["n_buckets"] > 10
            for i, m in enumerate(match):
                n = int(got[0][i]["n_returned"])
                assert got[3][i, :n].sum(axis=0, dtype=np.uint64).tolist() == rows[i].tolist(), (h_col, i)
                assert int(rows[i].sum()) == int(stats[i]["in_bounds"]) == int(stats[i]["count"]) > 0
                assert int(got[0][i]["count"]) == m.size == int(got[2][i, :n].sum())
    finally:
        dev.column_release(extra)


# ---- 6. several slices per query
def test_slices_add_into_the_same_cells(ta, small):
    """"agg_slices" 1, 2, 7 and 64, through the LDS table and straight to the grid row: the same bytes."""
    dev, queries = small["dev"], small["queries"]
    histogram = {"interval": 1_000_000.0}
    base = None
    try:
        for lds in (8192, 16):
            dev.set_option("agg_lds_buckets", lds)
            for slices in (1, 2, 7, 64):
                dev.set_option("agg_slices", slices)
                got = dev.raw_agg_terms_hist(queries, small["ocol"], small["col"], GM.U64, histogram, TM.COUNT_DESC, 1024)
                blob = [a.tobytes() for a in got[:4]]
                base = blob if base is None else base
                assert blob == base, (lds, slices)
        assert got[4]["n_cells"] == 512 * 10
    finally:
        dev.set_option("agg_slices", 0)
        dev.set_option("agg_lds_buckets", 8192)
    md = small["seg"].max_doc
    t, h = small["omodel"], small["model"]
    grid = Grid(t.u64[t.has], t.has, h.u64, None, GM.U64, md, histogram)
    _assert_hist(got, [grid.want(m, TM.COUNT_DESC, 1024) for m in small["match"]], grid.plan, "slices")


# ---- 7. sub-batches
def test_sub_batches_keep_the_callers_index(ta):
    """"docset_temp_lists" = 16: a batch that names 40 distinct lists without a bitmap runs as three sub-batches; the finish
    launches run once behind the last."""
    seg = _synth_segment()
    md = seg.max_doc
    rng = np.random.default_rng(9)
    vals_t = _random_keys(rng, md, 60, 1 << 40, 1000)
    vals_h = bitpacked_values(rng, md, 13, 0, 1)
    histogram = {"interval": 100.0, "offset": 7.0}
    grid = Grid(vals_t, None, vals_h, None, GM.U64, md, histogram)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 2)  # a bitmap only for the lists that hold half of the docs
        _prepare_all_terms(dev, seg)
        bare = [t for t in range(len(seg.terms)) if dev.term_table(dev.term_handle(t), "dense").size == 0]
        assert len(bare) >= 40
        bare = bare[:40]
        dev.set_option("docset_temp_lists", 16)
        ht, hh = dev.add_column(CM.write_bitpacked(vals_t)), dev.add_column(CM.write_bitpacked(vals_h))
        queries = [(O.MODE_OR, [t]) for t in bare]
        match = [O.decode_postings(seg, t)[0].astype(np.uint32) for t in bare]
        want = [grid.want(m, TM.COUNT_DESC, 9) for m in match]
        assert len({(tuple(w[1]), tuple(w[2])) for w in want}) == len(want)  # (a row under another query's index would show)
        for slices in (1, 3):
            dev.set_option("agg_slices", slices)
            _assert_hist(dev.raw_agg_terms_hist(queries, ht, hh, GM.U64, histogram, TM.COUNT_DESC, 9), want, grid.plan, ("sub-batches", slices))
            assert dev.last_batch_match_counts(len(bare)).tolist() == [m.size for m in match]
    finally:
        dev.close()


# ---- 8. query shapes against the models
@pytest.mark.parametrize("which,with_deletes", [("full bitpacked", False), ("full bitpacked", True),
                                                ("optional blockwise", False), ("optional blockwise", True)])
def test_query_shapes_against_the_model(ta, which, with_deletes):
    """The case list of tests/test_gpu_agg.py::test_query_shapes_against_the_model: flat AND / OR / boolean, +a +range over
    H's own column, `*`, a term set, m-of-n; match sets from AM.expect.  T is an Optional column of 50 keys."""
    seg = _synth_segment()
    md = seg.max_doc
    codec, vals, present = _query_columns(md)[which]
    by_df = sorted(range(len(seg.terms)), key=lambda t: seg.terms[t].doc_freq)
    a, b, c = by_df[len(by_df) // 2], by_df[-3], by_df[-5]
    B = ta.binding
    rng = np.random.default_rng(12)
    present_t = rng.random(md) < 0.8
    present_t[0] = present_t[md - 1] = True
    vals_t = _random_keys(rng, int(present_t.sum()), 50, 1 << 33, 5)
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
        _, tcol = _upload(dev, CM.BITPACKED, vals_t, present_t)
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
            ([(M, T(a)), (M, T(r))], 0),                   # +a +range, the histogram over the range's own column
            ([(M, T(a)), (M, ("union", [b, r]))], 0),      # +a +(b OR range)
            ([(M, STAR), (N, T(r))], 0),                   # * -range
            ([(M, T(a)), (M, T(r_empty))], 0),             # the empty result
            ([(S, T(a)), (S, T(b)), (S, T(c))], 2),        # 2 of 3 Should clauses
            ([(M, T(ts)), (N, T(a))], 0),                  # a term-set handle
            ([(M, STAR)], 0),                              # TQ_TERM_ALL alone
        ]
        match = [AM.expect(_model_clauses(cl, L), m, L.lists, md, alive)[0].astype(np.uint32) for cl, m in cases]
        assert match[6].size == 0 and all(match[i].size for i in (0, 1, 2, 3, 4, 5, 7, 8, 9))
        histogram = {"interval": float((h["max_value"] - h["min_value"]) // 300 + 1), "offset": 0.5}
        grid = Grid(vals_t, present_t, vals, present, GM.U64, md, histogram)
        assert 250 < grid.plan["hist"]["n_buckets"] <= 302 and grid.plan["terms"]["n_keys"] == 50
        batch = [_flat(ta, cl, m) for cl, m in cases]
        for order, size in ((TM.COUNT_DESC, 10), (TM.KEY_ASC, 50)):
            want = [grid.want(m, order, size) for m in match]
            _assert_hist(dev.raw_agg_terms_hist(batch, tcol, col, B.VALUE_U64, histogram, order, size), want, grid.plan, (which, with_deletes, order))
            assert dev.last_batch_match_counts(len(batch)).tolist() == [m.size for m in match]
        # +a +range as seen through the rows: only the buckets of the range hold docs
        rows = np.array(want[3][3])
        keys = (grid.plan["hist"]["base_pos"] + np.nonzero(rows.sum(axis=0))[0]) * histogram["interval"] + histogram["offset"]
        assert q1 - histogram["interval"] < keys.min() and keys.max() < q3
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
    histogram = {"interval": 250_000.0}
    grid = Grid(_random_keys(rng, md, 6, 1 << 40, 1000), None, bitpacked_values(rng, md, 13, 1 << 40, 1000), None, GM.U64, md, histogram)
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
    want = [grid.want(m, TM.COUNT_DESC, 4) for m in match]
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_budget_x", 256)
        _prepare_all_terms(dev, seg)
        ht, hh = dev.add_column(CM.write_bitpacked(grid.t.u64)), dev.add_column(CM.write_bitpacked(grid.h.u64))
        with pytest.raises(ta.TantivyAmdError) as ei:
            dev.raw_agg_terms_hist(queries, ht, hh, GM.U64, histogram, TM.COUNT_DESC, 4)
        assert ei.value.code == ERR_UNSUPPORTED and "query 1" in str(ei.value) and "tq_agg_terms_hist_batch" in str(ei.value)
        dev.set_option("docset_trees", 1)
        _assert_hist(dev.raw_agg_terms_hist(queries, ht, hh, GM.U64, histogram, TM.COUNT_DESC, 4), want, grid.plan, "trees")
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == B.KERNEL_AGG_TERMS_HIST | B.KERNEL_DOCSET_TREE | B.KERNEL_PHRASE_SLOP, st
        assert int(dev.last_batch_slop_overflows(len(queries)).sum()) == 0
    finally:
        dev.close()


# ---- 9. refusals
def test_refusals_leave_the_segment_usable(ta, small):
    import torch

    dev, queries, match = small["dev"], small["queries"], small["match"]
    md = small["seg"].max_doc
    B = ta.binding
    ht, hh = small["ocol"], small["col"]
    t, h = small["omodel"], small["model"]
    histogram = {"interval": 500_000.0}
    grid = Grid(t.u64[t.has], t.has, h.u64, None, GM.U64, md, histogram)
    want = [grid.want(match[0], TM.COUNT_DESC, 10)]

    def still_good():
        _assert_hist(dev.raw_agg_terms_hist(queries[:1], ht, hh, GM.U64, histogram, TM.COUNT_DESC, 10), want, grid.plan, "after a refusal")
        rc, docs, starts = dev.raw_docset(queries[:1], match[0].size)
        assert rc == 0 and np.array_equal(docs[: int(starts[1])], match[0]), _err(ta)

    def refused(call, code, *words):
        with pytest.raises(ta.TantivyAmdError) as ei:
            call()
        assert ei.value.code == code and all(w in str(ei.value) for w in words), ei.value
        still_good()

    def call(column=ht, hist_column=hh, vt=GM.U64, hist=histogram, order=TM.COUNT_DESC, size=10, qs=queries, **kw):
        return lambda: dev.raw_agg_terms_hist(qs, column, hist_column, vt, hist, order, size, **kw)

    still_good()
    fn = "tq_agg_terms_hist_batch"
    # everything tq_agg_terms_batch refuses
    refused(call(column=B.MAX_COLUMNS), ERR_INVALID, fn, "column")
    refused(call(column=7), ERR_INVALID, fn, "column 7")  # (no such upload)
    refused(call(size=0), ERR_INVALID, fn, "segment_size")
    refused(call(size=B.agg_terms_max_size() + 1), ERR_INVALID, fn, "segment_size")
    refused(call(order=4), ERR_INVALID, fn, "order")
    refused(call(stride=9), ERR_INVALID, fn, "out_stride")
    wide = bitpacked_values(np.random.default_rng(3), md, 17, 5, 1)
    extra = dev.add_column(CM.write_bitpacked(wide))
    refused(call(column=extra), ERR_UNSUPPORTED, fn, "n_keys", "131072")
    # everything tq_agg_batch refuses of a histogram
    refused(call(hist_column=B.MAX_COLUMNS), ERR_INVALID, fn, "histogram column")
    refused(call(hist_column=7), ERR_INVALID, fn, "histogram column 7")
    refused(call(vt=3), ERR_INVALID, fn, "value_type")
    refused(call(hist={"interval": 0.0}), ERR_INVALID, fn, "interval")
    refused(call(hist={"interval": 1.0, "offset": float("nan")}), ERR_INVALID, fn, "offset")
    refused(call(hist={"interval": 1.0, "hard_bounds": (2.0, 1.0)}), ERR_INVALID, fn, "hard_min")
    refused(call(hist={"interval": 1.0}), ERR_UNSUPPORTED, fn, "buckets")  # (8 191 001 of them)
    # ... and its own
    refused(call(histogram_flag=0), ERR_INVALID, fn, "histogram == 1")
    refused(call(reserved=(1, 0)), ERR_INVALID, fn, "reserved")
    refused(call(reserved=(0, 1)), ERR_INVALID, fn, "reserved")
    too_many = GM.histogram_plan(h.info, GM.U64, 64_500.0)["n_buckets"]
    assert 512 * too_many <= B.AGG_MAX_BUCKETS < 512 * (too_many + 1)  # (the outside entries take it over)
    refused(call(hist={"interval": 64_500.0}), ERR_UNSUPPORTED, fn, "n_keys = 512", "n_buckets = %d" % too_many, "TQ_AGG_MAX_BUCKETS")
    refused(call(hist_stride=16), ERR_INVALID, fn, "hist_stride")
    # the wide column as H is fine under an interval that keeps the grid small; released, it is refused
    assert int(dev.raw_agg_terms_hist(queries[:1], ht, extra, GM.U64, {"interval": 2000.0}, TM.COUNT_DESC, 10)[0][0]["matches"]) == match[0].size
    dev.column_release(extra)
    refused(call(hist_column=extra, hist={"interval": 2000.0}), ERR_INVALID, fn, "histogram column")
    refused(call(column=extra), ERR_INVALID, fn, "column")
    # the doc-set path's refusals under this function's name
    refused(call(qs=queries[:2] + [(O.MODE_PHRASE, [1, 2], [0, 1])]), ERR_UNSUPPORTED, fn, "query 2")
    refused(call(qs=queries[:1] + [(ta.MODE_BOOL, [1, 2], [M, 3], [0, 1], 0)]), ERR_INVALID, fn, "query 1")
    # null outputs (the device variant takes the pointers as they are)
    n = len(queries)
    nb = grid.plan["hist"]["n_buckets"]
    d_terms = torch.zeros(n * 5, dtype=torch.int64, device="cuda:0")
    d_keys = torch.zeros(n * 10, dtype=torch.int64, device="cuda:0")
    d_counts = torch.zeros(n * 10, dtype=torch.int32, device="cuda:0")
    d_rows = torch.zeros(n * 10 * nb, dtype=torch.int32, device="cuda:0")
    for args in ((d_terms, None, d_counts, d_rows), (d_terms, d_keys, None, d_rows), (None, d_keys, d_counts, d_rows), (d_terms, d_keys, d_counts, None)):
        rc = dev.raw_agg_terms_hist_device(queries, ht, hh, GM.U64, histogram, TM.COUNT_DESC, 10, 10, nb, *args)
        assert rc == ERR_INVALID and "tq_agg_terms_hist_batch_device" in _err(ta) and "null" in _err(ta)
        still_good()
    # without a bucket the histogram rows may be null
    none = {"interval": 1.0, "hard_bounds": (0.0, 5.0)}
    rc = dev.raw_agg_terms_hist_device(queries, ht, hh, GM.U64, none, TM.COUNT_DESC, 10, 10, 0, d_terms, d_keys, d_counts, None)
    assert rc == 0, _err(ta)
    dev.last_batch_stats()
    torch.cuda.synchronize()
    g0 = Grid(t.u64[t.has], t.has, h.u64, None, GM.U64, md, none)
    assert g0.plan["hist"]["n_buckets"] == 0
    for i, m in enumerate(match):
        rec, keys, counts, _ = g0.want(m, TM.COUNT_DESC, 10)
        assert d_keys.cpu().numpy().view(np.uint64).reshape(n, 10)[i, : rec["n_returned"]].tolist() == keys
        assert d_counts.cpu().numpy().view(np.uint32).reshape(n, 10)[i, : rec["n_returned"]].tolist() == counts
    still_good()


# ---- 10. the byte model and the mask
@pytest.mark.parametrize("h_optional", [False, True])
def test_stats_follow_the_byte_model(ta, small, h_optional):
    dev, queries, match, lists = small["dev"], small["queries"], small["match"], small["lists"]
    md = small["seg"].max_doc
    B = ta.binding
    full, opt = small["model"], small["omodel"]
    extra = None
    try:
        if h_optional:  # T Full (a new column of 300 keys), H the Optional column
            vals_t = _random_keys(np.random.default_rng(43), md, 300, 9, 4)
            extra = dev.add_column(CM.write_bitpacked(vals_t))
            ht, hh, histogram = extra, small["ocol"], {"interval": 100.0}
            grid = Grid(vals_t, None, opt.u64[opt.has], opt.has, GM.U64, md, histogram)
        else:  # T the Optional column, H the Full one
            ht, hh, histogram = small["ocol"], small["col"], {"interval": 82_000.0}
            grid = Grid(opt.u64[opt.has], opt.has, full.u64, None, GM.U64, md, histogram)
        t_optional = not h_optional
        nk, nb, cells = grid.plan["terms"]["n_keys"], grid.plan["hist"]["n_buckets"], grid.plan["n_cells"]
        assert cells == nk * (nb + 1) and nb > 10
        n_words = (md + 31) // 32
        sizes = [m.size for m in match]
        for size in (7, 1024):
            for slices in (1, 2):
                dev.set_option("agg_slices", slices)
                want = [grid.want(m, TM.COUNT_DESC, size) for m in match]
                _assert_hist(dev.raw_agg_terms_hist(queries, ht, hh, GM.U64, histogram, TM.COUNT_DESC, size), want, grid.plan,
                             ("stats", h_optional, size, slices))
                st = dev.last_batch_stats()
                assert st["kernel_mask"] == B.KERNEL_AGG_TERMS_HIST and st["kernels"] == ["agg_terms_hist"]
                assert dev.last_batch_match_counts(len(queries)).tolist() == sizes
                assert st["matches"] == sum(sizes)
                valued = sum(w[0]["count"] for w in want)  # docs with a value in T = the counted docs
                returned = sum(w[0]["n_returned"] for w in want)
                with_h = sum(grid.with_h(m) for m in match)
                assert (valued < sum(sizes)) == t_optional and (with_h < valued) == h_optional and returned > 0
                assert st["algorithmic_bytes"] == (sum(lists) * n_words * 4 + 8 * valued + (8 * sum(sizes) if t_optional else 0) +
                                                   len(queries) * (40 + 4 * nk) + 12 * returned +
                                                   8 * with_h + (8 * valued if h_optional else 0) +
                                                   len(queries) * 4 * cells + 4 * nb * returned)
        dev.set_option("agg_slices", 0)
        # the other aggregation calls account for what they did
        plain = dev.raw_agg_terms(queries, ht, TM.COUNT_DESC, 7)
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == B.KERNEL_AGG_TERMS and [int(t["count"]) for t in plain[0]] == [w[0]["count"] for w in want]
        assert st["algorithmic_bytes"] == (sum(lists) * n_words * 4 + 8 * valued + (8 * sum(sizes) if t_optional else 0) +
                                           len(queries) * (40 + 4 * nk) + 12 * sum(int(t["n_returned"]) for t in plain[0]))
    finally:
        dev.set_option("agg_slices", 0)
        if extra is not None:
            dev.column_release(extra)


# ---- 11. two segments through the host merge
def test_two_segments_merge_and_finalize(ta):
    """The walk segment twice, with other columns whose key ranges and bucket ranges only overlap: merge_terms_hist +
    terms_hist_finalize against the model over the concatenation.  segment_size holds every entry, so the merged result is
    exact."""
    seg, sparse = _walk_segment()
    md = seg.max_doc
    B = ta.binding
    rng = np.random.default_rng(20261206)
    histogram = {"interval": 3600.0, "offset": 600.0, "hard_bounds": (20_000.0, 700_000.0)}
    parts = []
    for s in range(2):
        vals_t = _random_keys(rng, md, 20 + 10 * s, 500 + 40 * s, 10)
        some = rng.random(md) < 0.7
        vals_h = np.sort(rng.integers(300_000 * s, 300_000 * s + 450_000, size=int(some.sum()))).astype(np.uint64)
        parts.append(Grid(vals_t, None, vals_h, some, GM.U64, md, histogram))
    assert parts[0].plan["hist"]["base_pos"] < parts[1].plan["hist"]["base_pos"] < parts[0].plan["hist"]["base_pos"] + parts[0].plan["hist"]["n_buckets"]
    queries = _walk_queries(ta, sparse)[:2]
    batch = [q for q, _ in queries]
    dev = ta.DeviceIndex([seg, seg])
    try:
        for s in range(2):
            for t in range(len(seg.terms)):
                dev.term_handle(t, segment_ord=s)
        got = []
        for s, grid in enumerate(parts):
            ht = dev.add_column(CM.write_bitpacked(grid.t.u64), segment_ord=s)
            hh = dev.add_column(CM.write_bitpacked(grid.h.u64[grid.h.has]), CM.OPTIONAL, CM.presence_words(grid.h.has), segment_ord=s)
            out = dev.raw_agg_terms_hist(batch, ht, hh, GM.U64, histogram, TM.COUNT_DESC, 100, segment_ord=s)
            _assert_hist(out, [grid.want(m, TM.COUNT_DESC, 100) for _, m in queries], grid.plan, ("segment", s))
            got.append(out)
        t_all = np.concatenate([p.t.u64 for p in parts])
        h_has = np.concatenate([p.h.has for p in parts])
        h_all = GM.Column(np.concatenate([p.h.u64[p.h.has] for p in parts]), h_has, 2 * md)
        whole = HM.plan(TM.column_info(t_all), dict(h_all.info, gcd=1), GM.U64, histogram)
        for qi, (_, match) in enumerate(queries):
            merged = B.merge_terms_hist([(g[1][qi], g[2][qi], g[3][qi], g[0][qi], g[4]["hist"]) for g in got])
            assert merged["sum_other_doc_count"] == 0 and merged["doc_count_error_upper_bound"] == 0
            docs = np.concatenate([match.astype(np.int64), match.astype(np.int64) + md])
            rec, keys, counts, rows = HM.closed_form(t_all, np.ones(2 * md, bool), h_all, GM.U64, docs, whole, TM.KEY_ASC, 1024)
            assert rec["sum_other_doc_count"] == 0 and len(keys) == rec["distinct"] > 30
            assert merged["base_pos"] == whole["hist"]["base_pos"] and len(merged["bucket_keys"]) == whole["hist"]["n_buckets"]
            assert merged["bucket_keys"] == [(whole["hist"]["base_pos"] + b) * 3600.0 + 600.0 for b in range(whole["hist"]["n_buckets"])]
            assert merged["entries"] == {k: (c, r) for k, c, r in zip(keys, counts, rows)}
            assert any(sum(r) < c for c, r in merged["entries"].values())
            for order in TM.ORDERS:
                fin = B.terms_hist_finalize(merged, size=12, order=order)
                w = HM.closed_form(t_all, np.ones(2 * md, bool), h_all, GM.U64, docs, whole, order, 12)
                assert fin["buckets"] == list(zip(w[1], w[2], w[3])), (qi, order)
                assert fin["sum_other_doc_count"] == w[0]["sum_other_doc_count"] and fin["bucket_keys"] == merged["bucket_keys"]
    finally:
        dev.close()
