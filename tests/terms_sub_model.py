"""Models of a terms bucket aggregation with ONE stats sub-aggregation on one segment (tq_agg_terms_sub_batch*), on top of
tests/terms_model.py and tests/agg_model.py, written from the reference's sources (read, not copied):
src/aggregation/bucket/term_agg/mod.rs — SegmentTermCollector::collect with a sub-aggregation (836-899),
into_intermediate_bucket_result with OrderTarget::SubAggregation (1040-1083), cut_off_buckets (1328-1353) — and
src/aggregation/metric/stats.rs — IntermediateStats::collect (164-175), compute_metric_value (325-357).

* `closed_form` is what tests/test_gpu_agg_terms_sub.py holds the device to: np.bincount over the key indices, per key a
  record of Python ints over the docs counted under it, the order value (`image`) as Python ints / fractions, a lexsort
  with ascending key as the tie-break, the cut at segment_size.
* `reference_segment` is the transliteration: a map from value to (count, IntermediateStats) filled doc by doc with the
  Kahan f64 sum, compute_metric_value(..).unwrap_or(0.0), the select (Python's sort where the reference uses
  select_nth_unstable_by — which of several equal entries survive the cut is unspecified there), cut_off_buckets.

Every figure of closed_form is an exact integer."""
from fractions import Fraction

import numpy as np

from tests import agg_model as GM
from tests import terms_model as TM

COUNT_DESC, COUNT_ASC, KEY_ASC, KEY_DESC, METRIC_DESC, METRIC_ASC = 0, 1, 2, 3, 4, 5  # tq_terms_order
ORDERS = (COUNT_DESC, COUNT_ASC, KEY_ASC, KEY_DESC, METRIC_DESC, METRIC_ASC)
VALUE_COUNT, MIN, MAX, SUM, AVG = 0, 1, 2, 3, 4  # tq_terms_metric
METRICS = (VALUE_COUNT, MIN, MAX, SUM, AVG)
RECORD_FIELDS = ("count", "min_value", "max_value", "sum_lo", "sum_hi")


def empty_record():
    return {"count": 0, "min_value": GM.MASK, "max_value": 0, "sum_lo": 0, "sum_hi": 0}


def record_of(values_u64, value_type):
    ints = [int(v) for v in values_u64]
    total = 0 if value_type == GM.F64 else sum(ints)
    return {"count": len(ints), "min_value": min(ints) if ints else GM.MASK, "max_value": max(ints) if ints else 0,
            "sum_lo": total & GM.MASK, "sum_hi": total >> 64}


def typed_sum(rec, value_type):
    """the exact typed sum of a U64 / I64 record"""
    total = rec["sum_lo"] + (rec["sum_hi"] << 64)
    return total - (rec["count"] << 63) if value_type == GM.I64 else total


def f64_image(x):
    """common/src/lib.rs f64_to_u64: the u64 whose order is the f64's"""
    bits = GM._f64_to_bits(float(x))
    return (~bits) & GM.MASK if bits & GM.HIGH else bits ^ GM.HIGH


def metric_rational(rec, value_type, metric):
    """the metric's exact typed value as a Fraction (an F64 min / max: the f64 itself), count == 0: typed 0"""
    if metric == VALUE_COUNT:
        return Fraction(rec["count"])
    if metric in (MIN, MAX):
        if not rec["count"]:
            return Fraction(0)
        return Fraction(GM.typed_from_u64(rec["min_value"] if metric == MIN else rec["max_value"], value_type))
    assert value_type != GM.F64
    if metric == SUM:
        return Fraction(typed_sum(rec, value_type))
    return Fraction(typed_sum(rec, value_type), rec["count"]) if rec["count"] else Fraction(0)


def image(rec, value_type, metric):
    """The order value of a record: Python ints, the quotient rounded by int / int (correctly rounded, half to even)."""
    if metric == VALUE_COUNT:
        return rec["count"]
    if metric in (MIN, MAX):
        if not rec["count"]:
            return 0 if value_type == GM.U64 else GM.HIGH  # typed 0
        return rec["min_value"] if metric == MIN else rec["max_value"]
    assert value_type != GM.F64, "F64 sums are not served"
    if metric == SUM:
        return typed_sum(rec, value_type) + ((1 << 95) if value_type == GM.I64 else 0)
    return f64_image(typed_sum(rec, value_type) / rec["count"] if rec["count"] else 0.0)


def per_key(u64_a, has_a, docs, info, u64_b, has_b, value_type_b):
    """-> (plan, doc counts per key index, records per key index over the docs counted under each key, docs with a value in
    A): what `select` orders and cuts"""
    plan = TM.terms_plan(info)
    docs = np.sort(np.asarray(docs, np.int64))
    docs = docs[np.asarray(has_a, bool)[docs]]
    idx = ((np.asarray(u64_a, np.uint64)[docs] - np.uint64(plan["min_value"])) // np.uint64(plan["gcd"])).astype(np.int64)
    assert idx.size == 0 or (0 <= int(idx.min()) and int(idx.max()) < plan["n_keys"])
    counts = np.bincount(idx, minlength=plan["n_keys"])
    hb = np.asarray(has_b, bool)[docs]
    vals, at = np.asarray(u64_b, np.uint64)[docs][hb], idx[hb]
    order = np.argsort(at, kind="stable")
    vals, at = vals[order], at[order]
    cuts = np.searchsorted(at, np.arange(plan["n_keys"] + 1))
    records = [record_of(vals[cuts[i]: cuts[i + 1]], value_type_b) if cuts[i] != cuts[i + 1] else empty_record()
               for i in range(plan["n_keys"])]
    return plan, counts, records, int(docs.size)


def closed_form(u64_a, has_a, docs, info, u64_b, has_b, value_type_b, order, segment_size, order_metric=AVG):
    """-> (record: dict as tq_agg_terms_t, keys, counts, records: dicts as tq_agg_bucket_stats_t), the rows in the request's
    order and cut at segment_size."""
    if not 1 <= segment_size <= TM.MAX_SIZE:
        raise TM.Refused("invalid", "segment_size")
    if order not in ORDERS:
        raise TM.Refused("invalid", "order")
    table = per_key(u64_a, has_a, docs, info, u64_b, has_b, value_type_b)
    return select(table, int(np.asarray(docs).size), value_type_b, order, segment_size, order_metric)


def select(table, matches, value_type_b, order, segment_size, order_metric=AVG):
    """closed_form's second half over per_key's table (one table serves every order and size)"""
    plan, per, records, valued = table
    nz = np.nonzero(per)[0]
    c = per[nz]
    if order == COUNT_DESC:
        perm = np.lexsort((nz, -c))  # (the last key is the primary one)
    elif order == COUNT_ASC:
        perm = np.lexsort((nz, c))
    elif order == KEY_ASC:
        perm = np.argsort(nz, kind="stable")
    elif order == KEY_DESC:
        perm = np.argsort(-nz, kind="stable")
    else:
        images = [image(records[int(i)], value_type_b, order_metric) for i in nz]
        perm = np.array(sorted(range(nz.size), key=lambda j: (-images[j] if order == METRIC_DESC else images[j], int(nz[j]))), np.int64)
    nz, c = nz[perm], c[perm]
    rec = {"matches": matches, "count": valued, "sum_other_doc_count": int(c[segment_size:].sum()),
           "distinct": int(nz.size), "n_returned": int(min(segment_size, nz.size)),
           "doc_count_error_upper_bound": int(c[segment_size]) if nz.size > segment_size else 0, "out_of_range": 0}
    keys = [plan["min_value"] + plan["gcd"] * int(i) for i in nz[:segment_size]]
    return rec, keys, [int(x) for x in c[:segment_size]], [records[int(i)] for i in nz[:segment_size]]


def compute_metric_value(stats, metric):
    """SegmentStatsCollector::compute_metric_value of one bucket's IntermediateStats -> f64 or None"""
    if metric == VALUE_COUNT:
        return float(stats.count)
    if metric == SUM:
        return stats.sum
    if stats.count > 0:
        return {MIN: stats.min, MAX: stats.max, AVG: stats.sum / float(stats.count)}[metric]
    return None


def reference_segment(u64_a, has_a, docs, u64_b, has_b, value_type_b, order, segment_size, order_metric=AVG, rng=None):
    """SegmentTermCollector::collect over the docs with the stats collector under every bucket, then
    into_intermediate_bucket_result: -> {"entries": [(key, count, IntermediateStats)] kept, in no particular order,
    "metric_values": the f64 of every entry before the cut (key -> value, metric orders), "sum_other_doc_count",
    "doc_count_error_upper_bound", "distinct", "largest_partial_sum"}.  rng: shuffles the map's entries first."""
    buckets = {}
    largest = 0.0
    for d in np.sort(np.asarray(docs, np.int64)).tolist():
        if not has_a[d]:  # (fetch_block without `missing`: a doc without a value enters nothing)
            continue
        b = buckets.setdefault(int(u64_a[d]), [0, GM.IntermediateStats()])
        b[0] += 1
        if has_b[d]:  # (fetch_block_with_missing, missing = None)
            b[1].collect(GM.f64_from_u64(u64_b[d], value_type_b))
            largest = max(largest, abs(b[1].sum))
    entries = [(k, c, st) for k, (c, st) in buckets.items() if c > 0]  # into_vec
    if rng is not None:
        entries = [entries[i] for i in rng.permutation(len(entries))]
    distinct = len(entries)
    total = None
    values = {}
    if order in (KEY_ASC, KEY_DESC):
        if len(entries) > segment_size:
            entries.sort(key=lambda e: e[0], reverse=order == KEY_DESC)
    elif order in (METRIC_DESC, METRIC_ASC):
        keyed = []
        for e in entries:
            v = compute_metric_value(e[2], order_metric)
            keyed.append((0.0 if v is None else v, e))  # unwrap_or(0.0)
            values[e[0]] = keyed[-1][0]
        if len(keyed) > segment_size:
            keyed.sort(key=lambda t: t[0], reverse=order == METRIC_DESC)  # (select_nth_unstable_by(partial_cmp))
        entries = [e for _, e in keyed]
    elif len(entries) > segment_size:
        total = sum(c for _, c, _ in entries)
        entries.sort(key=lambda e: -e[1] if order == COUNT_DESC else e[1])
    kept, before_cutoff, sum_other = TM.cut_off_buckets([(e[0], e[1]) for e in entries], segment_size, total)
    return {"entries": entries[:len(kept)], "metric_values": values, "sum_other_doc_count": sum_other,
            "doc_count_error_upper_bound": before_cutoff, "distinct": distinct, "largest_partial_sum": largest}
