"""GPU parity of fast-field range clauses (tq_column_upload / tq_range_prepare: tantivy_amd/csrc/tq_column.cpp,
tq_range.hip — what FastFieldRangeWeight::scorer leaves for a RangeQuery on a u64-mapped fast field: RangeDocSet over a
Column<u64> under a ConstScorer) through tq_column_decode, tq_term_table_read, tq_term_set_info, tq_count_batch,
tq_docset_batch, tq_docset_scored_batch, tq_search_batch and tq_search_one.

Expectations never come from the device: the column bytes are written by tests/column_model.py, a column's values are
the ones the writer was given (and what the model's reader makes of the bytes), a range's decision, doc mask and weight
are column_model.expected_range, its table column_model.expected_table; scores and top-k rows come from the literal model of
tests/all_model.py, whose `lists` dict takes a range as (present = the mask, score = full(weight)).  Comparison rule
(tests/test_gpu_term_set.py): docs, counts, tables and decoded values exact; scores bit for bit with at most two scoring
lists, within 1e-5 relative otherwise; top-k rows exact (score, doc) sequences with at most two scoring lists.

Shapes: tests/test_gpu_term_set._edge_segment — 131 113 docs, 4 098 bitmap words (two borders of the rank scan's tile, a
last word of 9 docs), 257 blocks of a BlockwiseLinear column, the last of 41 rows — for the build; a 20 000-doc synthetic
segment for the query shapes (625 words: the last wavefront of the fill owns one word, not two)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import all_model as AM
from tests import column_model as CM
from tests.test_column_model_cpu import bitpacked_grid, bitpacked_values, blockwise_values, ramp_values
from tests.test_gpu_all import STAR, Lists, T, _entries, _weights_of, check_cases
from tests.test_gpu_docset import ERR_INVALID, ERR_UNSUPPORTED
from tests.test_gpu_round3 import _alive_bytes
from tests.test_gpu_term_set import _edge_segment, _prepare_all_terms, _synth_segment

pytestmark = pytest.mark.gpu

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
ERR_FORMAT = 3


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def _err(ta):
    return ta.binding.lib().tq_last_error()


def _values(rng, codec, rows, grid=(13, 1 << 40, 1000)):
    if rows == 0:
        return np.zeros(0, np.uint64)
    if codec == CM.BITPACKED:
        return bitpacked_values(rng, rows, *grid)
    if codec == CM.LINEAR:
        return ramp_values(rng, rows, False)
    return blockwise_values(rng, rows)


def _presence_patterns(rng, md):
    """none, one doc, every doc, about 30 % with doc max_doc - 1 present."""
    one = np.zeros(md, bool)
    one[65536] = True
    some = rng.random(md) < 0.3
    some[md - 1] = True
    return {"none": np.zeros(md, bool), "one doc": one, "every doc": np.ones(md, bool), "random": some}


def _column_groups(md):
    """name -> [(name, codec, values, present | None)]: the columns of one parametrised case each."""
    rng = np.random.default_rng(20261019)
    groups = {}
    for bits, vmin, gcd in bitpacked_grid():
        key = "bitpacked min %s gcd %d" % ("0" if vmin == 0 else "2^40", gcd)
        groups.setdefault(key, []).append(("%d bits" % bits, CM.BITPACKED, bitpacked_values(rng, md, bits, vmin, gcd), None))
    groups["linear"] = [("ascending", CM.LINEAR, ramp_values(rng, md, False), None),
                        ("descending", CM.LINEAR, ramp_values(rng, md, True), None)]
    groups["blockwise"] = [("ramp with per-block noise", CM.BLOCKWISE, blockwise_values(rng, md), None)]
    for codec, cname in ((CM.BITPACKED, "bitpacked"), (CM.LINEAR, "linear"), (CM.BLOCKWISE, "blockwise")):
        groups["optional " + cname] = [(pname, codec, _values(rng, codec, int(p.sum())), p)
                                       for pname, p in _presence_patterns(rng, md).items()]
    return groups


GROUPS = ["bitpacked min 0 gcd 1", "bitpacked min 0 gcd 1000", "bitpacked min 2^40 gcd 1", "bitpacked min 2^40 gcd 1000",
          "linear", "blockwise", "optional bitpacked", "optional linear", "optional blockwise"]


def _upload(dev, codec, vals, present, junk_bits=True):
    blob = CM.WRITERS[codec](vals)
    if present is None:
        return blob, dev.add_column(blob)
    words = CM.presence_words(present)
    if junk_bits and present.size % 32:
        words[-1] |= np.uint32((0xFFFFFFFF << (present.size % 32)) & 0xFFFFFFFF)  # bits at and above max_doc: ignored
    return blob, dev.add_column(blob, CM.OPTIONAL, words)


def _mids(vals, lo, hi):
    if vals.size < 4:
        return lo, hi
    srt = np.sort(vals)
    return int(srt[vals.size // 4]), int(srt[3 * vals.size // 4])


def _check_column(ta, dev, md, label, codec, vals, present, cache):
    B = ta.binding
    n_words = (md + 31) // 32
    blob, col = _upload(dev, codec, vals, present)
    try:
        h = CM.read_header(blob)
        info = dev.column_info(col)
        for key in ("codec", "min_value", "max_value", "gcd", "num_rows", "num_bits"):
            assert info[key] == h[key], (label, key, info, h)
        assert info["cardinality"] == (CM.FULL if present is None else CM.OPTIONAL)
        presence_bytes = 0 if present is None else (n_words + 1) * 8
        if codec == CM.BITPACKED:  # the payload rounded up to a dword + 16 zero bytes (+ the presence table)
            assert info["resident_bytes"] == (len(blob) - h["at"] + 3) // 4 * 4 + 16 + presence_bytes, (label, info)
        else:
            assert info["resident_bytes"] >= 16 + presence_bytes, (label, info)
        # 1. the codec readers: the whole column, and a window that starts and ends inside a dword
        assert np.array_equal(CM.read_column(blob), vals), label
        assert np.array_equal(dev.column_decode(col), vals), label
        if vals.size > 600:
            for first, n in ((3, 70), (509, 7), (vals.size - 45, 44), (vals.size - 1, 1)):
                assert np.array_equal(dev.column_decode(col, first, n), vals[first: first + n]), (label, first, n)
        with pytest.raises(ta.TantivyAmdError) as e:
            dev.column_decode(col, vals.size, 1)
        assert e.value.code == ERR_INVALID
        # 2. the bound table
        lo, hi = h["min_value"], h["max_value"]
        mid_a, mid_b = _mids(vals, lo, hi)
        handles, sizes, weights = [], [], []
        for name, lower, upper, boost in CM.bound_table(lo, hi, h["gcd"], mid_a, mid_b):
            kind, mask, weight = CM.expected_range(vals, present, lower, upper, boost)
            got, got_w = dev.range_prepare(col, lower, upper, boost)
            where = (label, name)
            if kind == "all":
                assert got == B.STAR and not isinstance(got, B.RawHandle) and got_w == 1.0, where
                continue
            assert isinstance(got, B.RawHandle) and np.float32(got_w) == np.float32(weight), (where, got, got_w)
            table = dev.term_table(got, "dense")
            want = CM.expected_table(mask)
            assert table.shape == want.shape, (where, table.shape, want.shape)
            bad = np.nonzero((table != want).any(axis=1))[0]
            assert bad.size == 0, (where, bad[:4], table[bad[:4]], want[bad[:4]])
            assert dev.term_set_info(got) == (int(mask.sum()), n_words * 8), where
            handles.append(got), sizes.append(int(mask.sum())), weights.append([float(weight)])
        assert handles
        counts = dev.raw_count([(O.MODE_OR, [x]) for x in handles], weights, cache)
        assert counts.tolist() == sizes, label
        for x in handles:
            dev.term_set_release(x)
        return sizes
    finally:
        dev.column_release(col)


@pytest.mark.parametrize("group", GROUPS)
def test_build_at_the_edges(ta, group):
    seg = _edge_segment()
    md = seg.max_doc
    assert (md + 31) // 32 == 4098 and md % 32 == 9 and (md + 511) // 512 == 257 and md % 512 == 41
    columns = _column_groups(md)[group]
    dev = ta.DeviceIndex([seg])
    try:
        cache = np.ones(256, np.float32)
        before = dev.segment_stats()
        all_sizes = []
        for name, codec, vals, present in columns:
            all_sizes += _check_column(ta, dev, md, "%s: %s" % (group, name), codec, vals, present, cache)
        assert 0 in all_sizes and max(all_sizes) > md // 4
        if group == "blockwise":
            widths = set(CM.block_widths(CM.write_blockwise(columns[0][2])))
            assert 0 in widths and any(w > 32 for w in widths) and len(widths) >= 4, widths
        after = dev.segment_stats()  # columns are not part of tq_segment_stats; every handle was released
        assert after["bitmap_bytes"] == before["bitmap_bytes"] and after["n_dense_lists"] == before["n_dense_lists"]
    finally:
        dev.close()


# ---- 3. query level
class RangeLists(Lists):
    """tests/test_gpu_all.Lists, plus ranges: key = the handle, present = the mask, score = full(weight)."""

    def add_range(self, h, mask, weight):
        self.lists[h] = (mask.copy(), np.full(self.seg.max_doc, np.float32(weight), np.float32))
        self.weights[h] = float(np.float32(weight))
        return h


def _query_columns(md):
    rng = np.random.default_rng(77)
    present = rng.random(md) < 0.4
    present[md - 1] = True
    return {"full bitpacked": (CM.BITPACKED, bitpacked_values(rng, md, 13, 1 << 40, 1000), None),
            "full linear": (CM.LINEAR, ramp_values(rng, md, True), None),
            "optional blockwise": (CM.BLOCKWISE, blockwise_values(rng, int(present.sum())), present)}


@pytest.mark.parametrize("which,with_deletes", [("full bitpacked", False), ("full bitpacked", True), ("full linear", False),
                                                ("optional blockwise", False), ("optional blockwise", True)])
def test_every_entry_point_against_the_model(ta, which, with_deletes):
    seg = _synth_segment()
    md = seg.max_doc
    codec, vals, present = _query_columns(md)[which]
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
        blob, col = _upload(dev, codec, vals, present)
        h = CM.read_header(blob)
        lo, hi = h["min_value"], h["max_value"]
        srt = np.sort(vals)
        q1, q3 = int(srt[vals.size // 4]), int(srt[3 * vals.size // 4])
        L = RangeLists(seg)

        def new_range(lower, upper, boost):
            kind, mask, weight = CM.expected_range(vals, present, lower, upper, boost)
            got, got_w = dev.range_prepare(col, lower, upper, boost)
            assert kind == "set" and isinstance(got, B.RawHandle) and int(got) >= len(seg.terms), (kind, got)
            assert np.float32(got_w) == np.float32(weight)
            return L.add_range(got, mask, got_w)

        r = new_range(("in", q1), ("ex", q3), 1.0)
        r2 = new_range(("in", q1), ("ex", q3), 2.0)
        r_narrow = new_range(("in", q1), ("in", int(srt[vals.size // 4 + 40])), 1.0)
        r_empty = new_range(("in", hi), ("ex", hi), 1.0)
        assert 40 <= int(L.lists[r_narrow][0].sum()) < int(L.lists[r][0].sum()) and not L.lists[r_empty][0].any()
        for t in (a, b):
            L.need(t)
        cases = [
            ([(S, T(r))], 0),                              # range
            ([(M, T(a)), (M, T(r))], 0),                   # +a +range
            ([(S, T(a)), (S, T(r2))], 0),                  # a range^2
            ([(M, T(a)), (N, T(r))], 0),                   # +a -range
            ([(M, T(a)), (M, ("union", [b, r]))], 0),      # +a +(b OR range)
            ([(M, STAR), (N, T(r))], 0),                   # * -range
            ([(M, T(b)), (M, T(r_narrow))], 0),
            ([(M, T(a)), (M, T(r_empty))], 0),
            ([(S, T(a)), (S, T(r_empty))], 0),
        ]
        # a covering range with boost 1.0 is TQ_TERM_ALL: `+range +a` scores bm25(a) alone
        cover, cover_w = dev.range_prepare(col, ("in", lo), ("in", hi), 1.0)
        kind, _, weight = CM.expected_range(vals, present, ("in", lo), ("in", hi), 1.0)
        if present is None:
            assert kind == "all" and cover == B.STAR and cover_w == 1.0 and STAR == ("all", 1.0)
            cases.append(([(M, STAR), (M, T(a))], 0))
        else:  # (an Optional column never takes the shortcut: the set of the docs with a value)
            assert kind == "set" and isinstance(cover, B.RawHandle)
            L.add_range(cover, present, cover_w)
            cases.append(([(M, T(cover)), (M, T(a))], 0))
        want, rows = check_cases(ta, dev, L, cases, alive=alive, ks=(10,))
        assert want[0][0].size > 1000 and want[7][0].size == 0 and any(0 < w[0].size for w in want[1:5])
        # tq_search_one gives the batch's row
        sc, dc, ct = rows[(10, 0)]
        for i, (c, m) in enumerate(cases):
            terms, occurs, cof, whats = _entries(c)
            s1, d1, c1 = dev.raw_search_one((ta.MODE_BOOL, terms, occurs, cof, m), _weights_of(whats, L), L.cache, 10)
            assert c1 == int(ct[i]), (c, c1, int(ct[i]))
            assert np.array_equal(d1[:c1], dc[i, :c1]) and np.array_equal(s1[:c1].view(np.uint32), sc[i, :c1].view(np.uint32)), c
        # the flat spellings
        flat = [(O.MODE_AND, [a, r]), (O.MODE_OR, [a, r2]), (O.MODE_OR, [r])]
        flat_cases = [cases[1], cases[2], cases[0]]
        sizes = [AM.expect(c, 0, L.lists, md, alive)[0].size for c, _ in flat_cases]
        assert dev.raw_count(flat, [[L.weights[t] for t in q[1]] for q in flat], L.cache).tolist() == sizes
    finally:
        dev.close()


# ---- 4. refusals, lifetime, timing
def test_refusals_leave_the_segment_usable(ta):
    seg = _synth_segment()
    md = seg.max_doc
    B = ta.binding
    lib = B.lib()
    rng = np.random.default_rng(3)
    vals = bitpacked_values(rng, md, 8, 100, 1)
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        cache = np.array(list(O.bm25_for_one_term(1, md, 10.0).cache), np.float32)
        blob = CM.write_bitpacked(vals)
        col = dev.add_column(blob)
        _, mask, _ = CM.expected_range(vals, None, ("in", 120), ("in", 180), 1.5)
        want = np.nonzero(mask)[0].astype(np.uint32)
        h, w = dev.range_prepare(col, ("in", 120), ("in", 180), 1.5)
        good = (O.MODE_OR, [h])

        def still_good():
            rc, docs, starts = dev.raw_docset([good], want.size)
            assert rc == 0 and np.array_equal(docs[: int(starts[1])], want), _err(ta)
            assert dev.raw_count([good], [[w]], cache).tolist() == [want.size]
            sc, dc, ct = dev.raw_search([(O.MODE_OR, [h], None)], [[w]], cache, 5)
            assert int(ct[0]) == 5 and dc[0].tolist() == want[:5].tolist() and np.all(sc[0] == np.float32(1.5))
            h2, _ = dev.range_prepare(col2, ("in", 120), ("in", 180), 1.0)
            assert dev.term_set_info(h2)[0] == want.size
            dev.term_set_release(h2)

        def raises(code, call, word=None):
            with pytest.raises(ta.TantivyAmdError) as e:
                call()
            assert e.value.code == code and (word is None or word in str(e.value)), e.value
            still_good()

        col2 = dev.add_column(blob)
        still_good()
        # a multivalued upload; a Full column with presence words or the wrong number of rows; an Optional one whose
        # popcount is not its row count; malformed bytes
        raises(ERR_UNSUPPORTED, lambda: dev.add_column(blob, CM.MULTIVALUED), "multivalued")
        raises(ERR_FORMAT, lambda: dev.add_column(blob, CM.FULL, np.zeros((md + 31) // 32, np.uint32)))
        raises(ERR_FORMAT, lambda: dev.add_column(CM.write_bitpacked(vals[:-1])))
        raises(ERR_FORMAT, lambda: dev.add_column(blob, CM.OPTIONAL, np.zeros((md + 31) // 32, np.uint32)))
        raises(ERR_FORMAT, lambda: dev.add_column(blob[:-1]))
        # a 17th column
        extra = [dev.add_column(blob) for _ in range(B.MAX_COLUMNS - 2)]
        assert sorted([col, col2] + extra) == list(range(B.MAX_COLUMNS))
        raises(ERR_INVALID, lambda: dev.add_column(blob), "columns")
        for c in extra:
            dev.column_release(c)
        # a released column in tq_range_prepare / info / decode / a second release; a column out of range; a bad bound kind
        gone = extra[0]
        raises(ERR_INVALID, lambda: dev.range_prepare(gone, ("in", 120), None), "column")
        raises(ERR_INVALID, lambda: dev.column_info(gone))
        raises(ERR_INVALID, lambda: dev.column_decode(gone, 0, 1))
        raises(ERR_INVALID, lambda: dev.column_release(gone))
        raises(ERR_INVALID, lambda: dev.range_prepare(B.MAX_COLUMNS, ("in", 120), None))
        out, ow = B.C.c_uint32(), B.C.c_float()
        assert lib.tq_range_prepare(dev.segment_raw(), col, 3, 0, 1, 5, 1.0, B.C.byref(out), B.C.byref(ow)) == ERR_INVALID
        still_good()
        assert dev.range_prepare(gone, None, None, 2.0) == (B.STAR, 1.0)  # (an AllScorer before the column is looked at)

        def refused(fn, code, index, word):
            rc = fn()
            msg = lib.tq_last_error().decode()
            assert rc == code and ("query %d" % index) in msg and word in msg, (rc, msg)
            still_good()

        def rc_of(call):
            def run():
                try:
                    call()
                except ta.TantivyAmdError as e:
                    return e.code
                return 0
            return run

        ok = (O.MODE_AND, [1, 2])
        # a range handle in a phrase
        refused(lambda: dev.raw_docset([ok, (O.MODE_PHRASE, [1, h], [0, 1])], 1 << 16)[0], ERR_INVALID, 1, "phrase")
        refused(rc_of(lambda: dev.raw_search([(O.MODE_PHRASE, [1, h], [0, 1])], [[1.0, 1.0]], cache, 5)), ERR_INVALID, 0, "phrase")
        # ... in a nested query: `+a +(+b +range)`
        nested = (ta.MODE_BOOL, [1, 2, h], [M, M, M], [0, 1, 1], 0, {"nested_occurs": [M, M, M]})
        for option in ("docset_trees", "docset_score_trees"):
            dev.set_option(option, 1)
        refused(lambda: dev.raw_docset([ok, ok, nested], 1 << 16)[0], ERR_UNSUPPORTED, 2, "nested")
        refused(rc_of(lambda: dev.raw_search_trees([nested], [[1.0] * 3], cache, 5)), ERR_UNSUPPORTED, 0, "nested")
        for option in ("docset_trees", "docset_score_trees"):
            dev.set_option(option, 0)
        # `* range` through top-k
        star_range = (ta.MODE_BOOL, [B.TERM_ALL, h], None, [S, S], None, 0)
        refused(rc_of(lambda: dev.raw_search([(O.MODE_AND, [1, 2], None), star_range], [[1.0, 1.0]] * 2, cache, 5)), ERR_UNSUPPORTED, 1, "match-all")
        # releasing the column leaves the handles built from it valid
        h_before, _ = dev.range_prepare(col, ("in", 120), ("in", 180), 1.0)
        dev.column_release(col)
        rc, docs, starts = dev.raw_docset([good, (O.MODE_OR, [h_before])], 2 * want.size)
        assert rc == 0 and np.array_equal(docs[: want.size], want) and np.array_equal(docs[want.size: 2 * want.size], want)
        assert dev.raw_count([good], [[w]], cache).tolist() == [want.size]
        assert dev.term_set_info(h) == (want.size, (md + 31) // 32 * 8)
        dev.term_set_release(h_before)
        still_good()
        # a released range handle is a released term set
        dev.term_set_release(h)
        rc, _, _ = dev.raw_docset([ok, good], 1 << 16)
        assert rc == ERR_INVALID and "released" in lib.tq_last_error().decode()
    finally:
        dev.close()


def test_timing_leaves_the_build_figures(ta):
    """Option "timing": tq_range_prepare leaves the HIP-event time of the build and the byte model — the payload once, 16 B per
    32 docs of table, 8 B per 32 docs of presence table — in the batch statistics; an empty range runs no kernel: 0 bytes."""
    seg = _edge_segment()
    md = seg.max_doc
    n_words = (md + 31) // 32
    rng = np.random.default_rng(4)
    present = rng.random(md) < 0.5
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("timing", 1)
        full = bitpacked_values(rng, md, 13, 0, 1)
        opt = bitpacked_values(rng, int(present.sum()), 7, 0, 1)
        for vals, p in ((full, None), (opt, present)):
            blob, col = _upload(dev, CM.BITPACKED, vals, p)
            payload = len(blob) - CM.read_header(blob)["at"]
            h, _ = dev.range_prepare(col, ("in", 10), ("in", 50), 1.0)
            st = dev.last_batch_stats()
            assert st["algorithmic_bytes"] == payload + 16 * n_words + (0 if p is None else 8 * n_words)
            assert st["kernel_ms"] > 0.0 and st["batches_averaged"] == 1 and st["matches"] == 0
            assert dev.term_set_info(h)[0] == int(((vals >= 10) & (vals <= 50)).sum())
            h0, _ = dev.range_prepare(col, ("in", 50), ("ex", 50), 1.0)
            assert dev.last_batch_stats()["algorithmic_bytes"] == 0 and dev.term_set_info(h0)[0] == 0
    finally:
        dev.close()
