"""CPU-only checks of fast-field columns (include/tantivy_amd.h "fast-field ranges", tantivy_amd/csrc/tq_column.cpp): the
model of the reference's u64_based column bytes (tests/column_model.py) round-trips every column the GPU tests upload and
reproduces the one byte-level fact the reference pins; tq_column_parse — the library's host-side parse, which needs no
device — agrees with the model's header fields on the same blobs and answers every malformed blob with TQ_ERR_FORMAT;
and expected_range, the model of search_on_u64_ff + bound_to_value_range, gives hand-written answers on the bound
table.  No device compute here."""
import ctypes as C

import numpy as np
import pytest

from tests import column_model as CM

OK, ERR_INVALID, ERR_FORMAT = 0, 1, 3
M64 = CM.M64


@pytest.fixture(scope="module")
def B():
    from tantivy_amd import binding

    binding.lib()
    return binding


def bitpacked_values(rng, rows, bits, vmin, gcd):
    """min + gcd * n, n uniform below 2^bits, row 0 and the last row pinned to the extremes."""
    n = rng.integers(0, (1 << bits) - 1, size=rows, dtype=np.uint64, endpoint=True) if bits else np.zeros(rows, np.uint64)
    n[0], n[-1] = 0, (1 << bits) - 1
    return np.uint64(vmin) + np.uint64(gcd) * n


def bitpacked_grid():
    """(bits, min, gcd) of the Bitpacked columns: every width x {0, 2^40} x {1, 1000} whose largest value fits 64 bits."""
    out = []
    for bits in (0, 1, 3, 7, 8, 13, 31, 32, 33, 56, 64):
        for vmin in (0, 1 << 40):
            for gcd in (1, 1000):
                if bits == 0 and gcd != 1:
                    continue  # (a constant column's gcd is 1)
                if vmin + gcd * ((1 << bits) - 1) <= M64:
                    out.append((bits, vmin, gcd))
    return out


def ramp_values(rng, rows, descending):
    """A noisy ramp for the Linear codec: about 9 per row with noise below 64, rising or falling."""
    base = np.arange(rows, dtype=np.uint64) * np.uint64(9)
    if descending:
        base = base[::-1].copy()
    return np.uint64(1_000_000) + base + rng.integers(0, 64, size=rows).astype(np.uint64)


def blockwise_values(rng, rows):
    """A ramp with per-block noise for BlockwiseLinear: block 0 exact (width 0), block 1 noise above 2^32 (a width above
    32), then alternating small and large noise (differing neighbours)."""
    vals = np.arange(rows, dtype=np.uint64) * np.uint64(21) * np.uint64(3)
    for b in range(0, rows, CM.BLOCK):
        n = min(CM.BLOCK, rows - b)
        k = b // CM.BLOCK
        amp = 0 if k == 0 else (1 << 37) if k == 1 else (5, 1 << 11, 1 << 20)[k % 3]
        if amp:
            vals[b: b + n] += rng.integers(0, amp, size=n).astype(np.uint64) * np.uint64(3)
    return vals + np.uint64(500)


def small_cases():
    """(name, codec, values) — the GPU tests' columns at 1 400 rows (three blockwise blocks, the last partial)."""
    rng = np.random.default_rng(20261019)
    rows = 1400
    cases = [("bitpacked %d bits min %d gcd %d" % g, CM.BITPACKED, bitpacked_values(rng, rows, *g)) for g in bitpacked_grid()]
    cases.append(("linear ascending", CM.LINEAR, ramp_values(rng, rows, False)))
    cases.append(("linear descending", CM.LINEAR, ramp_values(rng, rows, True)))
    cases.append(("blockwise", CM.BLOCKWISE, blockwise_values(rng, rows)))
    cases.append(("blockwise one row", CM.BLOCKWISE, np.array([77], np.uint64)))
    cases.append(("bitpacked no rows", CM.BITPACKED, np.zeros(0, np.uint64)))
    return cases


def test_reference_pins_1_2_5():
    """u64_based/tests.rs:5-21: [1, 2, 5] as Bitpacked is 7 bytes — codec, min 1, gcd 1, amplitude 4, 3 rows, 9 bits of payload."""
    blob = CM.write_bitpacked([1, 2, 5])
    assert len(blob) == 7
    assert blob[:5] == bytes([0, 0x81, 0x81, 0x84, 0x83])
    assert CM.read_column(blob).tolist() == [1, 2, 5]
    assert [CM.read_one(blob, r) for r in range(3)] == [1, 2, 5]


def test_model_primitives():
    assert [CM.compute_num_bits(n) for n in (0, 1, 2, 255, 256, (1 << 56) - 1, 1 << 56, M64)] == [0, 1, 2, 8, 9, 56, 64, 64]
    assert CM.vint(0) == b"\x80" and CM.vint(127) == b"\xff" and CM.vint(128) == b"\x00\x81"
    assert CM.read_vint(CM.vint(M64) + b"\x01", 0) == (M64, 10)
    # Line::eval: bits 32..63 of the product, truncated to 32 bits, sign-extended
    assert CM.line_eval(3 << 32, 10, 5) == 25
    assert CM.line_eval(M64 - (3 << 32), 100, 5) == 84  # the complement of a slope of 3 falls by 3 per row, rounded down
    assert CM.line_eval(1 << 63, 0, 1) == M64 - (1 << 31) + 1  # 0x80000000 sign-extends
    xs = np.arange(0, 600, 7)
    for slope, intercept in ((3 << 32, 10), (M64 - (3 << 32) - 12345, M64 - 5), ((1 << 40) + 99, 1 << 63)):
        assert line_eval_all(slope, intercept, xs) == CM.line_eval_np(slope, intercept, xs).tolist()
    assert CM.pack([5, 2, 7], 3) == bytes([0b11010101, 0b1])
    assert CM.unpack(bytes([0b11010101, 0b1]), 3, 3).tolist() == [5, 2, 7]
    assert [CM.unpack_one(bytes([0b11010101, 0b1]), i, 3) for i in range(3)] == [5, 2, 7]


def line_eval_all(slope, intercept, xs):
    return [CM.line_eval(slope, intercept, int(x)) for x in xs]


def test_write_then_read_round_trips_and_the_library_parses_the_same_header(B):
    widths_seen = set()
    for name, codec, vals in small_cases():
        blob = CM.WRITERS[codec](vals)
        got = CM.read_column(blob)
        assert np.array_equal(got, vals), name
        for r in sorted({0, 1, 7, 511, 512, 513, 1023, 1024, vals.size - 1} & set(range(vals.size))):
            assert CM.read_one(blob, r) == int(vals[r]), (name, r)
        h = CM.read_header(blob)
        info = B.column_parse(blob)
        for key in ("codec", "min_value", "max_value", "gcd", "num_rows", "num_bits"):
            assert info[key] == h[key], (name, key, info, h)
        if vals.size:
            assert (h["min_value"], h["max_value"]) == (int(vals.min()), int(vals.max())), name
        if codec == CM.BLOCKWISE:
            widths_seen |= set(CM.block_widths(blob))
        assert info["resident_bytes"] >= 16 and info["cardinality"] == 0, name
    assert 0 in widths_seen and any(w > 32 for w in widths_seen) and len(widths_seen) >= 3, widths_seen


def test_gcd_and_min_of_the_grid_reach_the_header(B):
    rng = np.random.default_rng(5)
    for bits, vmin, gcd in bitpacked_grid():
        info = B.column_parse(CM.write_bitpacked(bitpacked_values(rng, 300, bits, vmin, gcd)))
        assert (info["num_bits"], info["min_value"]) == (bits, vmin), (bits, vmin, gcd)
        if bits > 1:
            assert info["gcd"] == gcd, (bits, vmin, gcd, info)
        assert info["max_value"] == vmin + gcd * ((1 << bits) - 1)


def _parse_rc(B, blob):
    info = B.TqColumnInfo()
    a = np.frombuffer(bytes(blob) + b"\0", dtype=np.uint8)  # (an empty blob is still a pointer)
    rc = B.lib().tq_column_parse(a.ctypes.data, a.size - 1, C.byref(info))
    return rc, B.lib().tq_last_error().decode()


def test_malformed_blobs_are_format_errors(B):
    rng = np.random.default_rng(9)
    good = {c: CM.WRITERS[c](v) for c, v in ((CM.BITPACKED, bitpacked_values(rng, 700, 13, 5, 1)),
                                             (CM.LINEAR, ramp_values(rng, 700, False)),
                                             (CM.BLOCKWISE, blockwise_values(rng, 1400)))}
    for blob in good.values():
        assert _parse_rc(B, blob)[0] == OK
    stats = CM.stats_bytes(5, 5 + 8191, 1, 700)
    bad = {
        "empty": b"",
        "codec byte alone": b"\x00",
        "unknown codec byte": bytes([3]) + good[CM.BITPACKED][1:],
        "codec byte 255": bytes([255]) + good[CM.BITPACKED][1:],
        "stats cut inside a vint": good[CM.BITPACKED][:3],
        "stats without rows": bytes([0]) + CM.vint(5) + CM.vint(1) + CM.vint(8191),
        "a vint that never stops": bytes([0]) + b"\x01" * 12,
        "gcd 0": bytes([0]) + CM.vint(5) + CM.vint(0) + CM.vint(8191) + CM.vint(700) + bytes(2000),
        "min + amplitude past u64": bytes([0]) + CM.vint(M64) + CM.vint(2) + CM.vint(3) + CM.vint(1) + bytes(8),
        "bitpacked payload one byte short": good[CM.BITPACKED][:-1],
        "bitpacked payload missing": bytes([0]) + stats,
        "linear without parameters": bytes([1]) + stats,
        "linear without its width byte": bytes([1]) + stats + CM.vint(1 << 32) + CM.vint(0),
        "linear width 57": bytes([1]) + stats + CM.vint(1 << 32) + CM.vint(0) + bytes([57]) + bytes(8000),
        "linear width 63": bytes([1]) + stats + CM.vint(1 << 32) + CM.vint(0) + bytes([63]) + bytes(8000),
        "linear width 65": bytes([1]) + stats + CM.vint(1 << 32) + CM.vint(0) + bytes([65]) + bytes(8000),
        "linear payload one byte short": good[CM.LINEAR][:-1],
        "blockwise without a footer length": bytes([2]) + stats + b"\x00\x00",
        "blockwise footer longer than the blob": good[CM.BLOCKWISE][:-4] + (1 << 20).to_bytes(4, "little"),
        "blockwise footer too short for its blocks": bytes([2]) + stats + bytes(4000) + CM.vint(0) + CM.vint(0) + bytes([3]) + (3).to_bytes(4, "little"),
        "blockwise footer cut inside a block": bytes([2]) + stats + bytes(4000) + (CM.vint(0) + CM.vint(0) + bytes([3])) + CM.vint(0) + b"\x01\x01" + (6).to_bytes(4, "little"),
        "blockwise width 60": bytes([2]) + stats + bytes(9000) + (CM.vint(0) + CM.vint(0) + bytes([60])) * 2 + (6).to_bytes(4, "little"),
        "blockwise data shorter than its blocks": bytes([2]) + stats + bytes(100) + (CM.vint(0) + CM.vint(0) + bytes([8])) * 2 + (6).to_bytes(4, "little"),
    }
    for name, blob in bad.items():
        rc, msg = _parse_rc(B, blob)
        assert rc == ERR_FORMAT and msg, (name, rc, msg)
    assert B.lib().tq_column_parse(None, 0, None) == ERR_INVALID
    with pytest.raises(B.TantivyAmdError) as e:
        B.column_parse(bad["gcd 0"])
    assert e.value.code == ERR_FORMAT and "gcd" in str(e.value)


def test_null_arguments_are_errors_not_crashes(B):
    L = B.lib()
    info = B.TqColumnInfo()
    out, w = C.c_uint32(123), C.c_float(9.0)
    blob = np.frombuffer(CM.write_bitpacked([1, 2, 5]), np.uint8)
    assert L.tq_column_upload(None, blob.ctypes.data, blob.size, 0, None, C.byref(out)) == ERR_INVALID
    assert b"tq_column_upload" in L.tq_last_error()
    assert L.tq_column_info(None, 0, C.byref(info)) == ERR_INVALID
    assert L.tq_column_release(None, 0) == ERR_INVALID
    assert L.tq_column_decode(None, 0, 0, 1, None) == ERR_INVALID
    assert L.tq_range_prepare(None, 0, 1, 0, 1, 5, 1.0, C.byref(out), C.byref(w)) == ERR_INVALID
    assert b"tq_range_prepare" in L.tq_last_error()
    assert out.value == 123 and w.value == 9.0
    for name in ("add_column", "column_info", "column_release", "column_decode", "range_prepare"):
        assert callable(getattr(B.DeviceIndex, name)), name
    assert B.STAR == B.TERM_ALL and B.MAX_COLUMNS == 16


# ---- the bound table against hand-written expectations
VALS = [10, 13, 16, 40, 10, 37, 40, 22]  # min 10, max 40, gcd 3


def _docs(kind_mask_weight):
    kind, mask, weight = kind_mask_weight
    return kind, np.nonzero(mask)[0].tolist(), weight


def test_bound_table_by_hand():
    E = lambda lo, hi, boost=1.0, present=None: _docs(CM.expected_range(VALS, present, lo, hi, boost))  # noqa: E731
    every = list(range(8))
    assert CM.stats_of(VALS) == (10, 40, 3, 8)
    assert E(None, None, 2.0) == ("all", every, 1.0)               # AllScorer before the column: the boost is dropped
    assert E(("ex", M64), None) == ("set", [], 1.0)                 # checked_add overflows
    assert E(None, ("ex", 0), 3.0) == ("set", [], 3.0)              # checked_sub underflows
    assert E(("in", 0), ("in", 9)) == ("set", [], 1.0)              # end < min (the packed transform would saturate to 0)
    assert E(None, ("ex", 10)) == ("set", [], 1.0)                  # end = 9 < min
    assert E(("in", 41), None) == ("set", [], 1.0)                  # start > max
    assert E(("ex", 40), ("in", M64)) == ("set", [], 1.0)
    assert E(("in", 16), ("in", 16)) == ("set", [2], 1.0)           # lo == hi
    assert E(("in", 10), ("in", 10), 0.5) == ("set", [0, 4], 0.5)
    assert E(("in", 17), ("in", 17)) == ("set", [], 1.0)            # lo == hi between two multiples of the gcd
    assert E(("in", 16), ("ex", 16)) == ("set", [], 1.0)            # start > end
    assert E(("in", 11), ("in", 38)) == ("set", [1, 2, 5, 7], 1.0)  # ends off the gcd grid: div_ceil up, floor down
    assert E(("ex", 12), ("ex", 38)) == ("set", [1, 2, 5, 7], 1.0)
    assert E(("ex", 13), ("ex", 37), 2.5) == ("set", [2, 7], 2.5)
    assert E(("in", 10), ("in", 40), 1.0) == ("all", every, 1.0)    # coverage, boost 1: AllScorer
    assert E(("in", 10), ("in", 40), 2.0) == ("set", every, 2.0)    # coverage, boost 2: ConstScorer(AllScorer, 2) is a set
    assert E(("in", 0), ("in", M64), 1.0) == ("all", every, 1.0)    # start raised to min, end not clamped
    assert E(None, ("in", 40), 1.0) == ("all", every, 1.0)
    assert E(("ex", 10), None) == ("set", [1, 2, 3, 5, 6, 7], 1.0)
    # an Optional column never takes the coverage shortcut; its rows are the present docs in order
    present = np.zeros(13, bool)
    present[[0, 2, 3, 5, 8, 9, 11, 12]] = True
    assert E(("in", 10), ("in", 40), 1.0, present) == ("set", [0, 2, 3, 5, 8, 9, 11, 12], 1.0)
    assert E(("in", 11), ("in", 38), 1.0, present) == ("set", [2, 3, 9, 12], 1.0)
    assert E(None, None, 2.0, present) == ("all", list(range(13)), 1.0)
    # no rows at all
    assert _docs(CM.expected_range([], np.zeros(5, bool), ("in", 0), None, 1.5)) == ("set", [], 1.5)
    # numpy columns take the same path
    arr = np.array(VALS, np.uint64)
    for _, lo, hi, boost in CM.bound_table(10, 40, 3, 16, 37):
        a, b = CM.expected_range(VALS, None, lo, hi, boost), CM.expected_range(arr, None, lo, hi, boost)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2], (lo, hi, boost)


def test_expected_table_layout():
    mask = np.zeros(70, bool)
    mask[[0, 31, 32, 69]] = True
    assert CM.expected_table(mask).tolist() == [[0x80000001, 0], [1, 2], [1 << 5, 3], [0, 4]]
    assert CM.presence_words(mask).tolist() == [0x80000001, 1, 1 << 5]
