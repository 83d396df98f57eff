"""Model of a histogram with ONE stats sub-aggregation on one segment, on top of tests/agg_model.py, written from the
reference's sources (read, not copied):

* the nested path of SegmentHistogramCollector::collect (src/aggregation/bucket/histogram/histogram.rs:489-505): per doc
  with a value in the bucket column, val = f64_from_fastfield_u64; if bounds.contains(val) the doc's bucket gets
  doc_count += 1 and the doc is pushed to the sub-aggregation under that bucket's id;
* SegmentStatsCollector::collect with a parent_bucket_id (src/aggregation/metric/stats.rs:282-306): the docs of a bucket
  through fetch_block_with_missing(missing = None) — a doc without a value in the metric column yields nothing — into
  IntermediateStats::collect (:164) in doc order.

`expected_sub` is the closed form tests/test_gpu_agg_sub.py holds the device to: agg_model.expected for the bucket column
and, per bucket, exact integers in the metric column's u64 space.  `reference_sub` is the transliteration;
tests/test_agg_sub_model_cpu.py shows where the two agree."""
import numpy as np

from tests import agg_model as GM

RECORD_FIELDS = ("count", "min_value", "max_value", "sum_lo", "sum_hi")


def bucket_of_docs(match_docs, col_a, vt_a, plan):
    """-> (docs, idx): the matching docs that are bucketed — a value in A inside the effective bounds — in doc order, and
    every one's entry of the dense row."""
    docs = np.sort(np.asarray(match_docs, np.int64))
    docs = docs[col_a.has[docs]]
    f = GM.f64_array(col_a.u64[docs], vt_a)
    keep = (plan["bounds_min"] <= f) & (f <= plan["bounds_max"])
    docs, f = docs[keep], f[keep]
    idx = np.array([GM.bucket_pos(float(x), plan["interval"], plan["offset"]) - plan["base_pos"] for x in f], np.int64)
    assert idx.size == 0 or (0 <= int(idx.min()) and int(idx.max()) < plan["n_buckets"])  # (the dense range holds them)
    return docs, idx


def empty_record():
    return {"count": 0, "min_value": GM.MASK, "max_value": 0, "sum_lo": 0, "sum_hi": 0}


def expected_sub(match_docs, col_a, vt_a, plan, col_b, vt_b):
    """-> (record, counts, bucket_records): agg_model.expected's two for column A, and per entry of the row a dict of
    Python ints as tq_agg_bucket_stats_t over the docs counted in that bucket."""
    rec, counts = GM.expected(match_docs, col_a, vt_a, plan)
    docs, idx = bucket_of_docs(match_docs, col_a, vt_a, plan) if plan["n_buckets"] else (np.zeros(0, np.int64),) * 2
    assert np.bincount(idx, minlength=plan["n_buckets"]).tolist() == counts
    has_b = col_b.has[docs]
    vals, at = col_b.u64[docs][has_b], idx[has_b]
    order = np.argsort(at, kind="stable")
    vals, at = vals[order], at[order]
    cuts = np.searchsorted(at, np.arange(plan["n_buckets"] + 1))
    records = []
    for i in range(plan["n_buckets"]):
        ints = vals[cuts[i]: cuts[i + 1]].tolist()
        total = 0 if vt_b == GM.F64 else sum(ints)
        records.append({"count": len(ints), "min_value": min(ints) if ints else GM.MASK, "max_value": max(ints) if ints else 0,
                        "sum_lo": total & GM.MASK, "sum_hi": total >> 64})
    return rec, counts, records


def reference_sub(match_docs, col_a, vt_a, plan, col_b, vt_b):
    """The nested path, doc by doc in doc order -> (doc counts, [IntermediateStats per bucket], partial sums' largest
    magnitude): a dict per bucket as the reference's sparse store, laid out over the plan's dense row."""
    buckets = {}
    largest = 0.0
    for doc in np.sort(np.asarray(match_docs, np.int64)).tolist():
        if not col_a.has[doc]:
            continue
        val = GM.f64_from_u64(col_a.u64[doc], vt_a)
        if not GM.contains((plan["bounds_min"], plan["bounds_max"]), val):
            continue
        b = buckets.setdefault(GM.bucket_pos(val, plan["interval"], plan["offset"]), [0, GM.IntermediateStats()])
        b[0] += 1
        if col_b.has[doc]:  # (fetch_block_with_missing, missing = None)
            b[1].collect(GM.f64_from_u64(col_b.u64[doc], vt_b))
            largest = max(largest, abs(b[1].sum))
    counts, stats = [0] * plan["n_buckets"], [GM.IntermediateStats() for _ in range(plan["n_buckets"])]
    for pos, (c, st) in buckets.items():
        counts[pos - plan["base_pos"]], stats[pos - plan["base_pos"]] = c, st
    return counts, stats, largest
