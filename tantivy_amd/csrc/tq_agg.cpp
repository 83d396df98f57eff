// tq_agg.cpp — tq_agg_histogram_plan / tq_agg_batch / tq_agg_batch_device: a stats metric and a histogram bucket aggregation
// over a resident u64 column, per query of a batch, on the device (the reference: src/aggregation/metric/stats.rs:86-176;
// src/aggregation/bucket/histogram/histogram.rs:468-518, 672-699, 738-769; src/aggregation/mod.rs:351-383).  The plan —
// validation of the request, normalize_histogram_req's bounds and compute_dense_range — is host arithmetic and lives
// here; everything in front of the aggregation launch — validation of the queries, the doc-set expression, tree and slop
// planning, sub-batches, scatter — is docset_batch's (tq_docset.cpp) under an AggSpec, the kernels tq_agg.hip's.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

#include <cfloat>
#include <cmath>

static_assert(sizeof(tq_agg_stats_t) == 64 && sizeof(TqkAggStats) == sizeof(tq_agg_stats_t), "the 64-byte record");
static_assert(sizeof(tq_agg_request) == 40 && sizeof(tq_agg_hist_plan_t) == 32, "the ABI of the aggregation calls");

namespace tqi {

namespace {

// f64_from_fastfield_u64 (src/aggregation/mod.rs:351-383): the same three conversions as agg_f64 of tq_agg.hip
double agg_f64(uint64_t v, uint32_t value_type) {
  const uint64_t high = 1ull << 63;
  if (value_type == TQ_VALUE_I64) return (double)(int64_t)(v ^ high);
  if (value_type == TQ_VALUE_F64) {
    const uint64_t bits = (v & high) ? v ^ high : ~v;
    double d;
    memcpy(&d, &bits, sizeof d);
    return d;
  }
  return (double)v;
}

// Rust's `f64 as i64`: saturating, NaN is 0 (a plain C++ cast is undefined out of range)
int64_t sat_i64(double x) {
  if (x != x) return 0;
  if (x >= 9223372036854775808.0) return INT64_MAX;
  if (x <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)x;
}

int64_t bucket_pos(double val, double interval, double offset) { return sat_i64(std::floor((val - offset) / interval)); }

int histogram_plan(const char *fn, const tq_column_info_t &info, const tq_agg_request &req, tq_agg_hist_plan_t *out) {
  *out = tq_agg_hist_plan_t{};
  if (req.value_type > TQ_VALUE_F64) return fail(TQ_ERR_INVALID, "%s: value_type %u", fn, req.value_type);
  if (!req.histogram) return TQ_OK;
  if (!std::isfinite(req.interval) || req.interval <= 0.0) return fail(TQ_ERR_INVALID, "%s: interval %g (finite, > 0)", fn, req.interval);
  if (!std::isfinite(req.offset)) return fail(TQ_ERR_INVALID, "%s: offset %g is not finite", fn, req.offset);
  double bmin = -DBL_MAX, bmax = DBL_MAX;
  const double col_min = agg_f64(info.min_value, req.value_type), col_max = agg_f64(info.max_value, req.value_type);
  if (req.has_hard_bounds) {
    if (!std::isfinite(req.hard_min) || !std::isfinite(req.hard_max))
      return fail(TQ_ERR_INVALID, "%s: hard bounds [%g, %g] are not finite", fn, req.hard_min, req.hard_max);
    if (req.hard_min > req.hard_max) return fail(TQ_ERR_INVALID, "%s: hard_min %g above hard_max %g", fn, req.hard_min, req.hard_max);
    // normalize_histogram_req: bounds that cannot exclude a value of the column collapse to the sentinel
    if (!(col_min >= req.hard_min && col_max <= req.hard_max)) {
      bmin = req.hard_min;
      bmax = req.hard_max;
    }
  }
  out->bounds_min = bmin;
  out->bounds_max = bmax;
  if (info.num_rows == 0u) return TQ_OK;  // (no value at all)
  // compute_dense_range; f64::max / f64::min return the other operand for a NaN, as fmax / fmin do
  const double lo = std::fmax(col_min, bmin), hi = std::fmin(col_max, bmax);
  if (lo > hi) return TQ_OK;
  const int64_t base = bucket_pos(lo, req.interval, req.offset), top = bucket_pos(hi, req.interval, req.offset);
  if (top < base) return TQ_OK;  // (not reached: pos is monotonic)
  const uint64_t span = (uint64_t)top - (uint64_t)base;  // buckets - 1; exact in 64 bits
  if (span >= (uint64_t)TQ_AGG_MAX_BUCKETS)
    return fail(TQ_ERR_UNSUPPORTED, "%s: the histogram has %.0f buckets, more than %u (TQ_AGG_MAX_BUCKETS)", fn, (double)span + 1.0,
                TQ_AGG_MAX_BUCKETS);
  out->base_pos = base;
  out->n_buckets = (uint32_t)span + 1u;
  return TQ_OK;
}

// the checks of an aggregation call itself, and its plan
int check_agg_call(tq_segment *s, const char *fn, const tq_agg_request *req, const void *buckets, uint32_t bucket_stride,
                   tq_agg_hist_plan_t *plan) {
  if (req->column >= TQ_MAX_COLUMNS || !s->columns[req->column].live)
    return fail(TQ_ERR_INVALID, "%s: column %u is not a live column of the segment", fn, req->column);
  const int rc = histogram_plan(fn, s->columns[req->column].info, *req, plan);
  if (rc != TQ_OK) return rc;
  if (bucket_stride < plan->n_buckets)
    return fail(TQ_ERR_INVALID, "%s: bucket_stride %u below the histogram's %u buckets", fn, bucket_stride, plan->n_buckets);
  if (plan->n_buckets && !buckets) return fail(TQ_ERR_INVALID, "%s: null bucket rows for a histogram of %u buckets", fn, plan->n_buckets);
  return TQ_OK;
}

}  // namespace

}  // namespace tqi

extern "C" {

int tq_agg_histogram_plan(const tq_column_info_t *info, const tq_agg_request *req, tq_agg_hist_plan_t *out) {
  const char *fn = "tq_agg_histogram_plan";
  if (!info || !req || !out) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  return histogram_plan(fn, *info, *req, out);
}

int tq_agg_batch_device(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_request *req,
                        tq_agg_stats_t *d_out_stats, uint32_t *d_out_buckets, uint32_t bucket_stride, void *hip_stream) {
  const char *fn = "tq_agg_batch_device";
  if (!s || !req || (!queries && n_queries) || (!d_out_stats && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    tq_agg_hist_plan_t plan;
    const int rc = check_agg_call(s, fn, req, d_out_buckets, bucket_stride, &plan);
    if (rc != TQ_OK || n_queries == 0) return rc;
    AggSpec spec{fn, req->column, req->value_type, plan, req->interval, req->offset, bucket_stride, d_out_stats, d_out_buckets};
    return docset_batch(s, queries, n_queries, nullptr, nullptr, 0, nullptr, false, true, hip_stream, false, nullptr, 0, nullptr, &spec);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

int tq_agg_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_request *req, tq_agg_stats_t *out_stats,
                 uint32_t *out_buckets, uint32_t bucket_stride) {
  const char *fn = "tq_agg_batch";
  if (!s || !req || (!queries && n_queries) || (!out_stats && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    tq_agg_hist_plan_t plan;
    int rc = check_agg_call(s, fn, req, out_buckets, bucket_stride, &plan);
    if (rc != TQ_OK || n_queries == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    {
      const int wrc = wait_segment_idle(s);  // (the buffer below may be a batch in flight's)
      if (wrc != TQ_OK) return wrc;
    }
    // on the device: [records | rows of n_buckets entries], copied back row by row into the caller's stride
    const size_t stats_bytes = (size_t)n_queries * sizeof(tq_agg_stats_t);
    const size_t row_bytes = (size_t)plan.n_buckets * sizeof(uint32_t);
    rc = s->d_agg_rows.ensure(stats_bytes + (size_t)n_queries * row_bytes + 64u);
    if (rc != TQ_OK) return rc;
    uint8_t *const base = (uint8_t *)s->d_agg_rows.p;
    AggSpec spec{fn, req->column, req->value_type, plan, req->interval, req->offset, plan.n_buckets, (tq_agg_stats_t *)base,
                 plan.n_buckets ? (uint32_t *)(base + stats_bytes) : nullptr};
    rc = docset_batch(s, queries, n_queries, nullptr, nullptr, 0, nullptr, false, true, nullptr, false, nullptr, 0, nullptr, &spec);
    if (rc != TQ_OK) return rc;
    hipStream_t st = s->stream;
    HIP_TRY(hipMemcpyAsync(out_stats, base, stats_bytes, hipMemcpyDeviceToHost, st));
    if (plan.n_buckets && bucket_stride == plan.n_buckets)
      HIP_TRY(hipMemcpyAsync(out_buckets, base + stats_bytes, (size_t)n_queries * row_bytes, hipMemcpyDeviceToHost, st));
    else if (plan.n_buckets)
      HIP_TRY(hipMemcpy2DAsync(out_buckets, (size_t)bucket_stride * sizeof(uint32_t), base + stats_bytes, row_bytes, row_bytes, n_queries,
                               hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (s->d_agg_rows.cap > ((size_t)256 << 20)) s->d_agg_rows.release();  // (a large result is not kept as scratch)
    if (s->last_batch_slop) {  // a sloppy phrase whose carried list went over the cap is reported; the other rows are valid
      std::vector<uint32_t> over(s->slop_over_words);
      HIP_TRY(hipMemcpy(over.data(), s->d_slop_over.p, over.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
      return slop_overflow_verdict(fn, over.data(), (uint32_t)over.size());
    }
    return TQ_OK;
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

}  // extern "C"
