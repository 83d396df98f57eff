"""CPU checks of the terms aggregation with a metric (tq_agg_terms_sub_batch*; tests/terms_sub_model.py): the closed form
that tests/test_gpu_agg_terms_sub.py holds the device to agrees with the transliteration of the reference's nested segment
collector — Kahan f64 sums, compute_metric_value(..).unwrap_or(0.0), the select, cut_off_buckets — on everything the
reference specifies, for the six orders x five metrics and segment_size at, one below and one above the number of entries.
The inputs keep every partial sum below 2^53 (so the reference's f64 sums are the exact ones) and the metric values on
either side of the cut apart in f64 (so the reference's cut is determined); the test asserts both, it cannot pass vacuously.
No device, no tolerance: every comparison is ==."""
import numpy as np
import pytest

from tests import agg_model as GM
from tests import terms_model as TM
from tests import terms_sub_model as SM


def _columns():
    """name -> (u64 of A per doc, has A, match docs, info of A, u64 of B per doc, has B, value type of B)"""
    rng = np.random.default_rng(20261201)
    out = {}
    n_keys = 12
    key_of = np.repeat(np.arange(n_keys), np.arange(n_keys) + 3)  # key k holds k + 3 docs
    md = key_of.size + 40
    perm = rng.permutation(md)
    a = np.zeros(md, np.uint64)
    has_a = np.zeros(md, bool)
    a[perm[:key_of.size]] = np.uint64(500) + np.uint64(7) * key_of.astype(np.uint64)
    has_a[perm[:key_of.size]] = True  # (the other 40 docs have no value in A: they enter nothing)
    k_of_doc = np.full(md, -1)
    k_of_doc[perm[:key_of.size]] = key_of
    info = TM.column_info(a[has_a])
    match = np.nonzero(has_a | (rng.random(md) < 0.5))[0]  # (every doc with a key, so that key k counts k + 3 docs)
    every = np.ones(md, bool)
    noise = rng.integers(0, 100, size=md)
    # U64, full: every metric grows with the key
    out["u64 full"] = (a, has_a, match, info, (np.maximum(k_of_doc, 0) * 1000 + noise).astype(np.uint64), every, GM.U64)
    # I64 straddling zero, Optional: key 6 has docs but no value in B — it orders as typed 0, inside the range
    typed = (k_of_doc - 6) * 1000 + noise - 50
    has_b = k_of_doc != 6
    for k in range(n_keys):  # (every other key loses k // 4 of its k + 3 values: the value counts stay apart at both ends)
        has_b[np.nonzero(k_of_doc == k)[0][:k // 4]] = False
    out["i64 optional, one key without a value"] = (a, has_a, match, info, np.array([GM.to_u64(int(x), GM.I64) for x in typed], np.uint64),
                                                     has_b, GM.I64)
    # B = A
    out["b is a"] = (a, has_a, match, info, a, has_a, GM.U64)
    # F64 metric (min / max / value_count alone)
    f = (k_of_doc - 6) * 0.75 + noise / 1024.0
    out["f64 full"] = (a, has_a, match, info, np.array([GM.to_u64(float(x), GM.F64) for x in f], np.uint64), every, GM.F64)
    return out


COLUMNS = _columns()


@pytest.mark.parametrize("metric", SM.METRICS)
@pytest.mark.parametrize("order", SM.ORDERS)
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_the_two_models_agree_on_what_the_reference_specifies(name, order, metric):
    a, has_a, match, info, b, has_b, vt = COLUMNS[name]
    if vt == GM.F64 and metric in (SM.SUM, SM.AVG):
        if order >= SM.METRIC_DESC:
            with pytest.raises(AssertionError):  # (F64 sums are not served: the closed form has no image for them)
                SM.closed_form(a, has_a, match, info, b, has_b, vt, order, 3, metric)
        return
    plan, per, records, _ = SM.per_key(a, has_a, match, info, b, has_b, vt)
    distinct = int(np.count_nonzero(per))
    assert distinct == 12
    rng = np.random.default_rng(3)
    for size in (distinct - 1, distinct, distinct + 1):
        rec, keys, counts, recs = SM.closed_form(a, has_a, match, info, b, has_b, vt, order, size, metric)
        ref = SM.reference_segment(a, has_a, match, b, has_b, vt, order, size, metric, rng)
        where = (name, order, metric, size)
        # precondition 1: the reference's f64 sums are exact
        assert ref["largest_partial_sum"] < float(1 << 53), where
        # precondition 2: the values on either side of the cut differ in f64
        if order >= SM.METRIC_DESC and distinct > size:
            vals = sorted(ref["metric_values"].values(), reverse=order == SM.METRIC_DESC)
            assert vals[size - 1] != vals[size], (where, vals)
        assert sorted(counts) == sorted(c for _, c, _ in ref["entries"]), where
        assert rec["sum_other_doc_count"] == ref["sum_other_doc_count"], where
        assert rec["doc_count_error_upper_bound"] == ref["doc_count_error_upper_bound"], where
        assert rec["distinct"] == ref["distinct"] == distinct and rec["n_returned"] == len(keys) == len(recs) == min(size, distinct), where
        assert rec["count"] == sum(counts) + rec["sum_other_doc_count"] == int(has_a[match].sum()) and rec["matches"] == match.size
        if order >= SM.KEY_ASC:  # nothing ties at the cut: the kept entries are determined
            assert sorted(zip(keys, counts)) == sorted((k, c) for k, c, _ in ref["entries"]), where
        # per entry the reference kept: the record is the reference's stats
        by_key = dict(zip(keys, recs))
        for k, c, st in ref["entries"]:
            r = records[(k - plan["min_value"]) // plan["gcd"]]
            assert by_key.get(k, r) == r and per[(k - plan["min_value"]) // plan["gcd"]] == c, (where, k)
            assert r["count"] == st.count, (where, k)
            if st.count:
                assert GM.f64_from_u64(r["min_value"], vt) == st.min and GM.f64_from_u64(r["max_value"], vt) == st.max, (where, k)
                if vt != GM.F64:
                    assert float(SM.typed_sum(r, vt)) == st.sum and abs(SM.typed_sum(r, vt)) < 1 << 53, (where, k)
            else:
                assert r == SM.empty_record()
        # the exact order refines the reference's f64 order: along the kept rows the reference's values never go back
        if order >= SM.METRIC_DESC:
            seq = [ref["metric_values"][k] for k in keys]
            assert seq == sorted(seq, reverse=order == SM.METRIC_DESC), (where, seq)
            images = [SM.image(r, vt, metric) for r in recs]
            assert images == sorted(images, reverse=order == SM.METRIC_DESC), where
    if name.startswith("i64") and order >= SM.METRIC_DESC and metric in (SM.MIN, SM.MAX, SM.AVG):
        # the key without a value orders as typed 0: neither first nor last of an I64 metric that straddles zero
        rec, keys, counts, recs = SM.closed_form(a, has_a, match, info, b, has_b, vt, order, distinct, metric)
        at = [i for i, r in enumerate(recs) if r["count"] == 0]
        assert len(at) == 1 and 0 < at[0] < distinct - 1 and keys[at[0]] == 500 + 7 * 6, at


def test_ties_go_to_the_ascending_key_under_both_metric_orders():
    """Every key has the same docs' values: every metric ties across the cut, the smallest keys survive."""
    md = 60
    a = (np.arange(md) % 6).astype(np.uint64) * np.uint64(4) + np.uint64(9)
    b = (np.arange(md) // 6).astype(np.uint64)  # key k holds the values 0..9, whatever k
    every = np.ones(md, bool)
    info = TM.column_info(a)
    for order in (SM.METRIC_DESC, SM.METRIC_ASC):
        for metric in SM.METRICS:
            rec, keys, counts, recs = SM.closed_form(a, every, np.arange(md), info, b, every, GM.U64, order, 4, metric)
            assert keys == [9, 13, 17, 21] and counts == [10] * 4 and rec["doc_count_error_upper_bound"] == 10
            assert rec["sum_other_doc_count"] == 20 and all(r == recs[0] for r in recs)


def test_the_request_is_checked():
    a, has_a, match, info, b, has_b, vt = COLUMNS["u64 full"]
    for bad in ({"segment_size": 0}, {"segment_size": 1025}, {"order": 6}):
        kw = {"order": SM.COUNT_DESC, "segment_size": 3}
        kw.update(bad)
        with pytest.raises(TM.Refused):
            SM.closed_form(a, has_a, match, info, b, has_b, vt, kw["order"], kw["segment_size"])
