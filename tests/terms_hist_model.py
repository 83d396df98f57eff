"""Models of a terms aggregation with one histogram leaf on one segment (tq_agg_terms_hist_batch*), written from the
reference's sources (read, not copied): src/aggregation/bucket/term_agg/term_histogram.rs — the fused collector's collect
(a flat grid counts[term * num_time_buckets + bucket] and per term the docs outside hard_bounds) and its
add_intermediate_aggregation_result (a term's count = its row sum + its remainder, then
SegmentTermCollector::into_intermediate_bucket_result) — and the general buffered path of term_agg/mod.rs for what the
fused collector leaves out: a doc without a value in the key column enters nothing, a doc without a value in the histogram
column counts under its key and in no bucket.

* `closed_form` is what tests/test_gpu_agg_terms_hist.py holds the device to: np.add.at over the (key index, bucket) pairs,
  terms_model's ordering and cut over the keys' totals, the survivors' rows.
* `reference_segment` is the literal per-doc loop, with tests/agg_model.py's bucket arithmetic and terms_model's
  cut_off_buckets.

Every figure is an exact integer."""
import numpy as np

from tests import agg_model as AM
from tests import terms_model as TM

MAX_CELLS = 65536  # TQ_AGG_MAX_BUCKETS


class Refused(Exception):
    """what tq_agg_terms_hist_plan refuses: kind = "invalid" (TQ_ERR_INVALID) or "unsupported" (TQ_ERR_UNSUPPORTED)"""

    def __init__(self, kind, why):
        Exception.__init__(self, why)
        self.kind = kind


def plan(info_t, info_h, value_type, histogram, order=TM.COUNT_DESC, segment_size=10, reserved=(0, 0), histogram_flag=1):
    """tq_agg_terms_hist_plan: the columns' infos ({"min_value", "max_value", "gcd", "num_rows"}) and the request -> the plan
    dict of the binding, or Refused.  histogram: {"interval", optionally "offset", "hard_bounds"}."""
    if reserved[0] or reserved[1]:
        raise Refused("invalid", "reserved")
    if histogram_flag != 1:
        raise Refused("invalid", "histogram")
    try:
        terms = TM.terms_plan(info_t, order, segment_size)
        hist = AM.histogram_plan(info_h, value_type, histogram["interval"], histogram.get("offset", 0.0), histogram.get("hard_bounds"))
    except (TM.Refused, AM.Refused) as e:
        raise Refused(e.kind, str(e))
    n_cells = terms["n_keys"] * (hist["n_buckets"] + 1)
    if n_cells > MAX_CELLS:
        raise Refused("unsupported", "n_keys = %d, n_buckets = %d" % (terms["n_keys"], hist["n_buckets"]))
    return {"terms": terms, "hist": hist, "n_cells": n_cells}


def grid(t_u64, t_has, h_col, value_type, docs, p):
    """The query's grid: [n_keys, n_buckets + 1] int64, the last column the keys' outside entries.  t_u64 / t_has: the key
    column per doc; h_col: an agg_model.Column; docs: the alive matching docs; p: plan()'s dict."""
    n_keys, nb = p["terms"]["n_keys"], p["hist"]["n_buckets"]
    g = np.zeros((n_keys, nb + 1), np.int64)
    docs = np.asarray(docs, np.int64)
    docs = docs[np.asarray(t_has, bool)[docs]]
    if docs.size == 0:
        return g
    idx = ((np.asarray(t_u64, np.uint64)[docs] - np.uint64(p["terms"]["min_value"])) // np.uint64(p["terms"]["gcd"])).astype(np.int64)
    assert 0 <= int(idx.min()) and int(idx.max()) < n_keys
    f = AM.f64_array(h_col.u64[docs], value_type)
    inb = h_col.has[docs] & (p["hist"]["bounds_min"] <= f) & (f <= p["hist"]["bounds_max"])
    b = np.full(docs.size, nb, np.int64)
    # (one bucket_pos per distinct value: Python floats, the arithmetic of the host plan and the kernel)
    uniq, inv = np.unique(f[inb], return_inverse=True)
    pos = np.array([AM.bucket_pos(float(v), p["hist"]["interval"], p["hist"]["offset"]) - p["hist"]["base_pos"] for v in uniq], np.int64)
    if uniq.size:
        b[inb] = pos[inv]
        assert 0 <= int(pos.min()) and int(pos.max()) < nb  # (the dense range holds every in-bounds value)
    np.add.at(g, (idx, b), 1)
    return g


def closed_form(t_u64, t_has, h_col, value_type, docs, p, order, segment_size, g=None):
    """-> (record: dict as tq_agg_terms_t, keys, counts, rows: [n_returned][n_buckets] lists of ints), in the request's order
    and cut at segment_size.  g: grid() of the same arguments, when the caller has it."""
    g = grid(t_u64, t_has, h_col, value_type, docs, p) if g is None else g
    total = g.sum(axis=1)
    nz = np.nonzero(total)[0]
    c = total[nz]
    if order == TM.COUNT_DESC:
        perm = np.lexsort((nz, -c))
    elif order == TM.COUNT_ASC:
        perm = np.lexsort((nz, c))
    elif order == TM.KEY_ASC:
        perm = np.argsort(nz, kind="stable")
    else:
        perm = np.argsort(-nz, kind="stable")
    nz, c = nz[perm], c[perm]
    docs = np.asarray(docs, np.int64)
    rec = {"matches": int(docs.size), "count": int(total.sum()), "sum_other_doc_count": int(c[segment_size:].sum()),
           "distinct": int(nz.size), "n_returned": int(min(segment_size, nz.size)),
           "doc_count_error_upper_bound": int(c[segment_size]) if nz.size > segment_size else 0, "out_of_range": 0}
    keys = [p["terms"]["min_value"] + p["terms"]["gcd"] * int(i) for i in nz[:segment_size]]
    nb = p["hist"]["n_buckets"]
    return rec, keys, [int(x) for x in c[:segment_size]], [[int(x) for x in g[i, :nb]] for i in nz[:segment_size]]


def reference_segment(t_u64, t_has, h_col, value_type, docs, p, order, segment_size):
    """collect doc by doc, then add_intermediate_aggregation_result: -> {"entries": {key: (doc_count, row)} kept,
    "sum_other_doc_count", "doc_count_error_upper_bound", "distinct"}.  The grid is keyed by the VALUE, as the buffered path's
    map is; nothing here uses the key index."""
    nb, hp = p["hist"]["n_buckets"], p["hist"]
    counts, outside = {}, {}  # value -> row of nb cells; value -> the remainder
    for d in np.asarray(docs, np.int64).tolist():
        if not t_has[d]:
            continue  # (fetch_block without `missing`: a doc without a key enters nothing)
        v = int(t_u64[d])
        row = counts.setdefault(v, [0] * nb)
        outside.setdefault(v, 0)
        if h_col.has[d]:
            val = AM.f64_from_u64(h_col.u64[d], value_type)
            if AM.contains((hp["bounds_min"], hp["bounds_max"]), val):
                row[AM.bucket_pos(val, hp["interval"], hp["offset"]) - hp["base_pos"]] += 1
                continue
        outside[v] += 1
    entries = [(v, sum(row) + outside[v]) for v, row in counts.items()]  # in_bounds + out_of_bounds
    entries = [(k, c) for k, c in entries if c > 0]
    distinct = len(entries)
    total = None
    if order in (TM.KEY_ASC, TM.KEY_DESC):
        entries.sort(key=lambda e: e[0], reverse=order == TM.KEY_DESC)
    else:
        total = sum(c for _, c in entries) if len(entries) > segment_size else None
        # (the reference's unstable selection leaves ties open; the ascending key decides them here as on the device)
        entries.sort(key=lambda e: (-e[1], e[0]) if order == TM.COUNT_DESC else (e[1], e[0]))
    kept, before_cutoff, sum_other = TM.cut_off_buckets(entries, segment_size, total)
    return {"entries": {k: (c, counts[k]) for k, c in kept}, "order": [k for k, _ in kept], "sum_other_doc_count": sum_other,
            "doc_count_error_upper_bound": before_cutoff, "distinct": distinct}
