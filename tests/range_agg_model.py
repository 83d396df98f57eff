"""Model of a range bucket aggregation with at most ONE stats sub-aggregation on one segment, on top of tests/agg_model.py,
written from the reference's sources (read, not copied):

* f64_to_fastfield_u64 (src/aggregation/mod.rs:394-402) with Rust's saturating `as u64` / `as i64`;
* to_u64_range and extend_validate_ranges (src/aggregation/bucket/range.rs:451-519): the bounds in u64 space, a stable sort
  by start, the two outer buckets, the holes filled, overlapping neighbours refused;
* get_bucket_pos (:431-437): slice::binary_search_by_key(..).unwrap_or_else(|p| p - 1), here with core's binary_search_by
  transliterated (size halving, `base = if cmp == Greater { base } else { mid }`);
* SegmentRangeCollector::collect (:276-305) in doc order, the sub-aggregation's IntermediateStats per bucket
  (metric/stats.rs:282-306, missing = None);
* range_to_string (:521-543) with f64's Display.

What the project decides where the reference leaves it open: a range whose converted start is above its
converted end is refused; a value's bucket is THE LAST BUCKET WHOSE START IS <= THE VALUE, so an empty range [s, s) counts
nothing.  `expected_range` is the closed form tests/test_gpu_agg_range.py holds the device to; `reference_range` is the
transliteration; tests/test_agg_range_model_cpu.py shows where the two agree (strictly increasing starts)."""
import decimal
import math

import numpy as np

from tests import agg_model as GM
from tests.agg_model import Refused  # noqa: F401 (kind = "invalid" / "unsupported")

MAX_BUCKETS = 1024  # TQ_AGG_RANGE_MAX_BUCKETS
TOP = GM.MASK


def convert_bound(val, value_type):
    """f64_to_fastfield_u64: `val as u64` / `(val as i64).to_u64()` / `val.to_u64()`, the casts saturating, NaN -> 0."""
    val = float(val)
    if value_type == GM.I64:
        return (GM.sat_i64(val) & GM.MASK) ^ GM.HIGH
    if value_type == GM.F64:
        return GM.to_u64(val, GM.F64)
    if val != val or val <= 0.0:
        return 0
    if val >= 18446744073709551616.0:
        return TOP
    return int(val)


def _bounds(r):
    return (r.get("from"), r.get("to")) if isinstance(r, dict) else tuple(r)


def plan(value_type, ranges):
    """-> [{"start", "end", "source"}] in bucket order (source: index of the caller's range, None = inserted); raises
    Refused.  ranges: (from, to) pairs or dicts, None = that end is open."""
    if len(ranges) == 0:
        raise Refused("invalid", "no range")
    if value_type > GM.F64:
        raise Refused("invalid", "value_type")
    conv = []
    for i, r in enumerate(ranges):
        lo, hi = _bounds(r)
        if any(x is not None and float(x) != float(x) for x in (lo, hi)):
            raise Refused("invalid", "range %d has a NaN bound" % i)
    for i, r in enumerate(ranges):
        lo, hi = _bounds(r)
        start = 0 if lo is None else convert_bound(lo, value_type)
        end = TOP if hi is None else convert_bound(hi, value_type)
        if start > end:
            raise Refused("invalid", "range %d starts above its end" % i)
        conv.append({"start": start, "end": end, "source": i})
    conv.sort(key=lambda b: b["start"])  # (stable, as sort_by_key)
    if conv[0]["start"] != 0:
        conv.insert(0, {"start": 0, "end": conv[0]["start"], "source": None})
    if conv[-1]["end"] != TOP:
        conv.append({"start": conv[-1]["end"], "end": TOP, "source": None})
    while True:  # find_hole, one at a time as the reference does
        hole = None
        for pos in range(len(conv) - 1):
            if conv[pos]["end"] > conv[pos + 1]["start"]:
                raise Refused("invalid", "overlapping ranges %r and %r" % (conv[pos]["source"], conv[pos + 1]["source"]))
            if conv[pos]["end"] != conv[pos + 1]["start"]:
                hole = pos
                break
        if hole is None:
            break
        conv.insert(hole + 1, {"start": conv[hole]["end"], "end": conv[hole + 1]["start"], "source": None})
    if len(conv) > MAX_BUCKETS:
        raise Refused("unsupported", "%d buckets" % len(conv))
    return conv


def starts_of(buckets):
    return [b["start"] for b in buckets]


def bucket_of(starts, v):
    """the last bucket whose start <= v"""
    pos = 0
    for i, s in enumerate(starts):
        if s <= v:
            pos = i
    return pos


def rust_binary_search_by_key(keys, target):
    """core::slice::binary_search_by as of Rust 1.52+ restated: -> ("ok", index) or ("err", insertion point)."""
    size = len(keys)
    if size == 0:
        return "err", 0
    base = 0
    while size > 1:
        half = size // 2
        mid = base + half
        base = base if keys[mid] > target else mid
        size -= half
    if keys[base] == target:
        return "ok", base
    return "err", base + (1 if keys[base] < target else 0)


def reference_bucket_pos(starts, v):
    """get_bucket_pos: binary_search_by_key(&val, start).unwrap_or_else(|pos| pos - 1)"""
    kind, pos = rust_binary_search_by_key(starts, v)
    return pos if kind == "ok" else pos - 1


def empty_record():
    return {"count": 0, "min_value": GM.MASK, "max_value": 0, "sum_lo": 0, "sum_hi": 0}


def expected_range(match_docs, col_a, buckets, col_b=None, vt_b=None, vt_a=GM.U64):
    """-> (record, counts, bucket_records or None): tq_agg_stats_t of column A as agg_model.expected gives it with in_bounds
    == count, the doc counts per bucket, and per bucket a dict of Python ints as tq_agg_bucket_stats_t of column B over the
    docs counted there (col_b None: no metric)."""
    rec, _ = GM.expected(match_docs, col_a, vt_a)
    rec["in_bounds"] = rec["count"]
    starts = np.array(starts_of(buckets), np.uint64)
    nb = len(buckets)
    docs = np.sort(np.asarray(match_docs, np.int64))
    docs = docs[col_a.has[docs]]
    idx = np.searchsorted(starts, col_a.u64[docs], "right").astype(np.int64) - 1
    assert idx.size == 0 or (0 <= int(idx.min()) and int(idx.max()) < nb)
    counts = np.bincount(idx, minlength=nb).tolist()
    if col_b is None:
        return rec, counts, None
    has_b = col_b.has[docs]
    vals, at = col_b.u64[docs][has_b], idx[has_b]
    order = np.argsort(at, kind="stable")
    vals, at = vals[order], at[order]
    cuts = np.searchsorted(at, np.arange(nb + 1))
    records = []
    for i in range(nb):
        ints = vals[cuts[i]: cuts[i + 1]].tolist()
        total = 0 if vt_b == GM.F64 else sum(ints)
        records.append({"count": len(ints), "min_value": min(ints) if ints else GM.MASK, "max_value": max(ints) if ints else 0,
                        "sum_lo": total & GM.MASK, "sum_hi": total >> 64})
    return rec, counts, records


def reference_range(match_docs, col_a, buckets, col_b=None, vt_b=None):
    """collect, doc by doc in doc order -> (doc counts, [IntermediateStats per bucket] or None, the partial sums' largest
    magnitude)."""
    starts = starts_of(buckets)
    counts = [0] * len(buckets)
    stats = [GM.IntermediateStats() for _ in buckets] if col_b is not None else None
    largest = 0.0
    for doc in np.sort(np.asarray(match_docs, np.int64)).tolist():
        if not col_a.has[doc]:
            continue
        pos = reference_bucket_pos(starts, int(col_a.u64[doc]))
        counts[pos] += 1
        if stats is not None and col_b.has[doc]:
            stats[pos].collect(GM.f64_from_u64(col_b.u64[doc], vt_b))
            largest = max(largest, abs(stats[pos].sum))
    return counts, stats, largest


def f64_display(x):
    """Rust's Display of an f64: shortest round-trip digits, never an exponent, no trailing ".0"."""
    x = float(x)
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    t = format(decimal.Decimal(repr(x)), "f")
    return t.rstrip("0").rstrip(".") if "." in t else t


def key_of(bucket, value_type):
    """range_to_string for U64 / I64 / F64"""
    lo = "*" if bucket["start"] == 0 else f64_display(GM.f64_from_u64(bucket["start"], value_type))
    hi = "*" if bucket["end"] == TOP else f64_display(GM.f64_from_u64(bucket["end"], value_type))
    return "%s-%s" % (lo, hi)
