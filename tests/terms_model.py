"""Models of a terms bucket aggregation on one segment (tq_agg_terms_batch*), written from the reference's sources (read,
not copied): src/aggregation/bucket/term_agg/mod.rs — SegmentTermCollector::collect (836-899), into_intermediate_bucket_result
(1000-1111), cut_off_buckets (1328-1353) — over numpy arrays: the u64-space value of every doc, whether the doc has one,
and the docs that match.

* `closed_form` is what tests/test_gpu_agg_terms.py holds the device to: np.bincount over the key indices
  (value - min) / gcd, np.lexsort under the request's order with ascending key as the tie-break, the cut at segment_size.
* `reference_segment` is the transliteration: a map from value to count filled doc by doc, the entries with a count, the
  order's sort (Python's sort where the reference uses select_nth_unstable / sort_unstable — which of several equal-count
  entries survive the cut is unspecified there, so the two models are compared on what IS specified), cut_off_buckets.

Every figure is an exact integer."""
import functools
import math

import numpy as np

COUNT_DESC, COUNT_ASC, KEY_ASC, KEY_DESC = 0, 1, 2, 3  # tq_terms_order
ORDERS = (COUNT_DESC, COUNT_ASC, KEY_ASC, KEY_DESC)
MAX_KEYS = 65536  # TQ_AGG_MAX_BUCKETS
MAX_SIZE = 1024   # TQ_AGG_TERMS_MAX_SIZE
FIELDS = ("matches", "count", "sum_other_doc_count", "distinct", "n_returned", "doc_count_error_upper_bound", "out_of_range")


class Refused(Exception):
    """what tq_agg_terms_plan refuses: kind = "invalid" (TQ_ERR_INVALID) or "unsupported" (TQ_ERR_UNSUPPORTED)"""

    def __init__(self, kind, why):
        Exception.__init__(self, why)
        self.kind = kind


def column_info(values):
    """min, max, gcd and rows of a column's values as the reference's stats collector leaves them (no rows: 0, 0, 1, 0; all
    equal: gcd 1)."""
    vals = [int(v) for v in np.asarray(values, np.uint64)]
    if not vals:
        return {"min_value": 0, "max_value": 0, "gcd": 1, "num_rows": 0}
    lo = min(vals)
    g = functools.reduce(math.gcd, (v - lo for v in vals), 0)
    return {"min_value": lo, "max_value": max(vals), "gcd": g or 1, "num_rows": len(vals)}


def terms_plan(info, order=COUNT_DESC, segment_size=10):
    """tq_agg_terms_plan: info = {"min_value", "max_value", "gcd", "num_rows"} -> the plan dict of the binding, or Refused."""
    if not 1 <= segment_size <= MAX_SIZE:
        raise Refused("invalid", "segment_size")
    if order not in ORDERS:
        raise Refused("invalid", "order")
    n_keys = (info["max_value"] - info["min_value"]) // info["gcd"] + 1 if info["num_rows"] else 0
    if n_keys > MAX_KEYS:
        raise Refused("unsupported", "n_keys = %d" % n_keys)
    return {"n_keys": n_keys, "min_value": info["min_value"], "gcd": info["gcd"]}


def closed_form(u64, has, docs, info, order, segment_size):
    """-> (record: dict of Python ints as tq_agg_terms_t, keys: list of ints, counts: list of ints), the rows in the request's
    order and cut at segment_size.  u64 / has: per doc; docs: the alive matching docs."""
    plan = terms_plan(info, order, segment_size)
    docs = np.asarray(docs, np.int64)
    vals = np.asarray(u64, np.uint64)[docs][np.asarray(has, bool)[docs]]
    idx = ((vals - np.uint64(plan["min_value"])) // np.uint64(plan["gcd"])).astype(np.int64)
    assert idx.size == 0 or (0 <= int(idx.min()) and int(idx.max()) < plan["n_keys"])
    per_key = np.bincount(idx, minlength=plan["n_keys"])
    nz = np.nonzero(per_key)[0]
    c = per_key[nz]
    if order == COUNT_DESC:
        perm = np.lexsort((nz, -c))  # (the last key is the primary one)
    elif order == COUNT_ASC:
        perm = np.lexsort((nz, c))
    elif order == KEY_ASC:
        perm = np.argsort(nz, kind="stable")
    else:
        perm = np.argsort(-nz, kind="stable")
    nz, c = nz[perm], c[perm]
    rec = {"matches": int(docs.size), "count": int(vals.size), "sum_other_doc_count": int(c[segment_size:].sum()),
           "distinct": int(nz.size), "n_returned": int(min(segment_size, nz.size)),
           "doc_count_error_upper_bound": int(c[segment_size]) if nz.size > segment_size else 0, "out_of_range": 0}
    keys = [plan["min_value"] + plan["gcd"] * int(i) for i in nz[:segment_size]]
    return rec, keys, [int(x) for x in c[:segment_size]]


def cut_off_buckets(entries, num_elem, total_doc_count):
    """cut_off_buckets over [(key, count)]: -> (kept entries, term_doc_count_before_cutoff, sum_other_doc_count)"""
    before_cutoff = entries[num_elem][1] if len(entries) > num_elem else 0
    if total_doc_count is not None:
        sum_other = total_doc_count - sum(c for _, c in entries[:num_elem]) if len(entries) >= num_elem else 0
    else:
        sum_other = sum(c for _, c in entries[num_elem:])
    return entries[:num_elem], before_cutoff, sum_other


def reference_segment(u64, has, docs, order, segment_size, rng=None):
    """SegmentTermCollector::collect over the docs, then into_intermediate_bucket_result: -> {"entries": [(key, count)]
    kept, in no particular order, "sum_other_doc_count", "doc_count_error_upper_bound", "distinct"}.  rng: shuffles the
    map's entries first, as a hash map's iteration order would."""
    buckets = {}
    for d in np.asarray(docs, np.int64).tolist():
        if has[d]:  # (fetch_block without `missing`: a doc without a value enters nothing)
            v = int(u64[d])
            buckets[v] = buckets.get(v, 0) + 1
    entries = [(k, c) for k, c in buckets.items() if c > 0]  # into_vec
    if rng is not None:
        entries = [entries[i] for i in rng.permutation(len(entries))]
    distinct = len(entries)
    total = None
    if order in (KEY_ASC, KEY_DESC):
        if len(entries) > segment_size:
            entries.sort(key=lambda e: e[0], reverse=order == KEY_DESC)
    elif len(entries) > segment_size:
        total = sum(c for _, c in entries)
        entries.sort(key=lambda e: -e[1] if order == COUNT_DESC else e[1])
    kept, before_cutoff, sum_other = cut_off_buckets(entries, segment_size, total)
    return {"entries": kept, "sum_other_doc_count": sum_other, "doc_count_error_upper_bound": before_cutoff, "distinct": distinct}
