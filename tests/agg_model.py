"""Model of a stats metric and a histogram bucket aggregation on one segment, written from the reference's sources (read,
not copied):

* f64_from_fastfield_u64 (src/aggregation/mod.rs:351-383; common/src/lib.rs:108-114 u64_to_f64 / f64_to_u64, i64's
  MonotonicallyMappableToU64): U64 `v as f64`, I64 `(v ^ 1 << 63) as i64 as f64`, F64 `from_bits(v & HIGH ? v ^ HIGH : !v)`;
* IntermediateStats::collect / finalize (src/aggregation/metric/stats.rs:86-176): count, Kahan sum, f64::min / max;
* HistogramBounds::contains, get_bucket_pos_f64, normalize_histogram_req, compute_dense_range
  (src/aggregation/bucket/histogram/histogram.rs:468-518, 672-699, 738-769), with Rust's saturating `as i64`.

`expected` is the closed form tests/test_gpu_agg.py holds the device to: exact integer stats in the column's u64 space and
a dense row of counts.  tests/test_agg_model_cpu.py shows where the exact sums ARE the reference's Kahan sums.

Python floats and numpy float64 are IEEE doubles with round-to-nearest-even and no contraction: every figure here is bit
for bit what the C++ host code and the kernel compute."""
import math

import numpy as np

U64, I64, F64 = 0, 1, 2  # tq_value_type
HIGH = 1 << 63
MASK = (1 << 64) - 1
F64_MAX = float(np.finfo(np.float64).max)
MAX_BUCKETS = 65536      # TQ_AGG_MAX_BUCKETS
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


class Refused(Exception):
    """what tq_agg_histogram_plan refuses: kind = "invalid" (TQ_ERR_INVALID) or "unsupported" (TQ_ERR_UNSUPPORTED)"""

    def __init__(self, kind, why):
        Exception.__init__(self, why)
        self.kind = kind


# ---- the three conversions, both ways
def _bits_to_f64(bits):
    return float(np.array([bits & MASK], np.uint64).view(np.float64)[0])


def _f64_to_bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def f64_from_u64(v, value_type):
    v = int(v)
    if value_type == I64:
        s = v ^ HIGH
        return float(s - (1 << 64) if s >> 63 else s)   # (int -> float: round to nearest even, as `as f64`)
    if value_type == F64:
        return _bits_to_f64(v ^ HIGH if v & HIGH else ~v)
    return float(v)


def to_u64(x, value_type):
    """MonotonicallyMappableToU64::to_u64 of a typed value (int for U64 / I64, float for F64)."""
    if value_type == I64:
        return (int(x) & MASK) ^ HIGH
    if value_type == F64:
        bits = _f64_to_bits(float(x))
        return (~bits) & MASK if bits & HIGH else bits ^ HIGH
    return int(x)


def typed_from_u64(v, value_type):
    """The typed value: exact int for U64 / I64, float for F64."""
    v = int(v)
    if value_type == I64:
        s = v ^ HIGH
        return s - (1 << 64) if s >> 63 else s
    if value_type == F64:
        return f64_from_u64(v, F64)
    return v


def f64_array(values, value_type):
    """f64_from_u64 over a uint64 array."""
    v = np.asarray(values, np.uint64)
    if value_type == I64:
        return (v ^ np.uint64(HIGH)).view(np.int64).astype(np.float64)
    if value_type == F64:
        neg = (v & np.uint64(HIGH)) != 0
        return np.where(neg, v ^ np.uint64(HIGH), ~v).astype(np.uint64).view(np.float64)
    return v.astype(np.float64)


# ---- stats: the reference's f64 accumulator
class IntermediateStats:
    def __init__(self):
        self.count, self.sum, self.delta = 0, 0.0, 0.0
        self.min, self.max = F64_MAX, -F64_MAX

    def collect(self, value):
        self.count += 1
        y = value - self.delta       # Kahan
        t = self.sum + y
        self.delta = (t - self.sum) - y
        self.sum = t
        # f64::min / f64::max: the other operand when one is NaN
        self.min = value if (self.min != self.min or value < self.min) else self.min
        self.max = value if (self.max != self.max or value > self.max) else self.max

    def merge_fruits(self, other):
        self.count += other.count
        y = other.sum - (self.delta + other.delta)
        t = self.sum + y
        self.delta = (t - self.sum) - y
        self.sum = t
        self.min, self.max = min(self.min, other.min), max(self.max, other.max)

    def finalize(self):
        none = self.count == 0
        return {"count": self.count, "sum": self.sum, "min": None if none else self.min, "max": None if none else self.max,
                "avg": None if none else self.sum / float(self.count)}


def reference_stats(values_u64, value_type):
    """collect over the values in the given (doc) order -> finalize()"""
    st = IntermediateStats()
    for v in values_u64:
        st.collect(f64_from_u64(v, value_type))
    return st.finalize()


# ---- histogram
def sat_i64(x):
    """Rust's `f64 as i64`."""
    if x != x:
        return 0
    if x >= 9223372036854775808.0:
        return I64_MAX
    if x <= -9223372036854775808.0:
        return I64_MIN
    return int(x)


def bucket_pos(val, interval, offset):
    """get_bucket_pos_f64(...) as i64"""
    f = (val - offset) / interval
    return sat_i64(f if (f != f or math.isinf(f)) else math.floor(f))


def contains(bounds, val):
    return bounds[0] <= val <= bounds[1]


def _fmax(a, b):  # f64::max
    return b if a != a else a if b != b else max(a, b)


def _fmin(a, b):
    return b if a != a else a if b != b else min(a, b)


def normalize_bounds(col_min, col_max, value_type, hard_bounds):
    """normalize_histogram_req's bounds: the hard bounds, the sentinel without them or when they cannot exclude a value."""
    sentinel = (-F64_MAX, F64_MAX)
    if hard_bounds is None:
        return sentinel
    lo, hi = f64_from_u64(col_min, value_type), f64_from_u64(col_max, value_type)
    if lo >= hard_bounds[0] and hi <= hard_bounds[1]:
        return sentinel
    return (float(hard_bounds[0]), float(hard_bounds[1]))


def dense_range(col_min, col_max, value_type, interval, offset, bounds):
    """compute_dense_range -> (base_pos, len) or None"""
    lo = _fmax(f64_from_u64(col_min, value_type), bounds[0])
    hi = _fmin(f64_from_u64(col_max, value_type), bounds[1])
    if lo > hi:
        return None
    base, top = bucket_pos(lo, interval, offset), bucket_pos(hi, interval, offset)
    n = top - base + 1
    return (base, n) if n > 0 else None


def histogram_plan(info, value_type, interval, offset=0.0, hard_bounds=None):
    """tq_agg_histogram_plan: info = {"min_value", "max_value", "num_rows"} -> the plan dict of the binding, or Refused."""
    if value_type not in (U64, I64, F64):
        raise Refused("invalid", "value_type")
    if not (math.isfinite(interval) and interval > 0.0):
        raise Refused("invalid", "interval")
    if not math.isfinite(offset):
        raise Refused("invalid", "offset")
    if hard_bounds is not None:
        if not (math.isfinite(hard_bounds[0]) and math.isfinite(hard_bounds[1])) or hard_bounds[0] > hard_bounds[1]:
            raise Refused("invalid", "hard bounds")
    bounds = normalize_bounds(info["min_value"], info["max_value"], value_type, hard_bounds)
    rng = dense_range(info["min_value"], info["max_value"], value_type, interval, offset, bounds) if info["num_rows"] else None
    if rng is not None and rng[1] > MAX_BUCKETS:
        raise Refused("unsupported", "%d buckets" % rng[1])
    return {"base_pos": rng[0] if rng else 0, "n_buckets": rng[1] if rng else 0, "bounds_min": bounds[0], "bounds_max": bounds[1],
            "interval": float(interval), "offset": float(offset)}


# ---- the closed form over a column
class Column:
    """Column<u64>::first(doc) of every doc: values[row] for row = the rank of the doc among the docs with a value
    (present: bool per doc, or None: every doc has a value)."""

    def __init__(self, values, present, max_doc):
        values = np.asarray(values, np.uint64)
        self.has = np.ones(max_doc, bool) if present is None else np.asarray(present, bool)
        self.u64 = np.zeros(max_doc, np.uint64)
        self.u64[self.has] = values
        self.info = {"min_value": int(values.min()) if values.size else 0, "max_value": int(values.max()) if values.size else 0,
                     "num_rows": int(values.size)}


def expected(match_docs, column, value_type, plan=None):
    """-> (record: dict of Python ints as tq_agg_stats_t, counts: list of plan["n_buckets"] ints)."""
    docs = np.asarray(match_docs, np.int64)
    vals = column.u64[docs][column.has[docs]]
    ints = vals.tolist()
    total = 0 if value_type == F64 else sum(ints)
    rec = {"matches": int(docs.size), "count": len(ints), "min_value": min(ints) if ints else MASK, "max_value": max(ints) if ints else 0,
           "sum_lo": total & MASK, "sum_hi": total >> 64, "in_bounds": 0, "out_of_range": 0}
    nb = plan["n_buckets"] if plan else 0
    counts = [0] * nb
    if nb:
        f = f64_array(vals, value_type)
        inb = f[(plan["bounds_min"] <= f) & (f <= plan["bounds_max"])]
        rec["in_bounds"] = int(inb.size)
        for val, c in zip(*np.unique(inb, return_counts=True)):
            i = bucket_pos(float(val), plan["interval"], plan["offset"]) - plan["base_pos"]
            assert 0 <= i < nb, (val, i, nb)   # (the dense range holds every counted value)
            counts[i] += int(c)
    return rec, counts


def finalize(rec, value_type):
    """The record in the typed space, as the binding's agg_stats_finalize gives it."""
    count = rec["count"]
    total = None if value_type == F64 else rec["sum_lo"] + (rec["sum_hi"] << 64) - (count << 63 if value_type == I64 else 0)
    if count == 0:
        return {"count": 0, "sum": total, "min": None, "max": None, "avg": None}
    return {"count": count, "sum": total, "min": typed_from_u64(rec["min_value"], value_type),
            "max": typed_from_u64(rec["max_value"], value_type), "avg": None if total is None else total / count}
