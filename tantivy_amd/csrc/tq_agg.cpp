// tq_agg.cpp — tq_agg_histogram_plan / tq_agg_batch / tq_agg_batch_device: a stats metric and a histogram bucket aggregation
// over a resident u64 column, per query of a batch, on the device; tq_agg_sub_batch / tq_agg_sub_batch_device: the same with a
// stats record of a second (metric) column per bucket, kernels in tq_agg_sub.hip (the reference: src/aggregation/metric/stats.rs:86-176;
// src/aggregation/bucket/histogram/histogram.rs:468-518, 672-699, 738-769; src/aggregation/mod.rs:351-383).  The plan —
// validation of the request, normalize_histogram_req's bounds and compute_dense_range — is host arithmetic and lives
// here, as do the launch geometry and the launches (kernels: tq_agg.hip); the match words the aggregation reads —
// validation of the queries, the doc-set expression, tree and slop planning, sub-batches, scatter — come from
// docset_batch (tq_docset.cpp), which calls agg_prepare once and agg_launch per sub-batch.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_agg_value.hpp"
#include "tq_internal.hpp"

#include <cfloat>
#include <cmath>

static_assert(sizeof(tq_agg_stats_t) == 64 && sizeof(TqkAggStats) == sizeof(tq_agg_stats_t), "the 64-byte record");
static_assert(TQ_AGGV_U64 == TQ_VALUE_U64 && TQ_AGGV_I64 == TQ_VALUE_I64 && TQ_AGGV_F64 == TQ_VALUE_F64, "tq_agg_value.hpp's value types");
static_assert(sizeof(tq_agg_request) == 40 && sizeof(tq_agg_hist_plan_t) == 32, "the ABI of the aggregation calls");
static_assert(sizeof(tq_agg_metric_request) == 8 && sizeof(tq_agg_bucket_stats_t) == 40 && sizeof(TqkAggBucketStats) == sizeof(tq_agg_bucket_stats_t),
              "the ABI of the sub-aggregation calls");

namespace tqi {

namespace {

int64_t bucket_pos(double val, double interval, double offset) { return tq_agg_sat_i64(std::floor((val - offset) / interval)); }

int histogram_plan(const char *fn, const tq_column_info_t &info, const tq_agg_request &req, tq_agg_hist_plan_t *out) {
  *out = tq_agg_hist_plan_t{};
  if (req.value_type > TQ_VALUE_F64) return fail(TQ_ERR_INVALID, "%s: value_type %u", fn, req.value_type);
  if (!req.histogram) return TQ_OK;
  if (!std::isfinite(req.interval) || req.interval <= 0.0) return fail(TQ_ERR_INVALID, "%s: interval %g (finite, > 0)", fn, req.interval);
  if (!std::isfinite(req.offset)) return fail(TQ_ERR_INVALID, "%s: offset %g is not finite", fn, req.offset);
  double bmin = -DBL_MAX, bmax = DBL_MAX;
  const double col_min = tq_agg_f64(info.min_value, req.value_type), col_max = tq_agg_f64(info.max_value, req.value_type);
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

// a sub-aggregation's own checks, behind check_agg_call (the plan is made)
int check_metric(tq_segment *s, const char *fn, const tq_agg_request *req, const tq_agg_metric_request *metric, const void *bucket_stats,
                 const tq_agg_hist_plan_t &plan) {
  if (!req->histogram) return fail(TQ_ERR_INVALID, "%s: a metric needs the histogram (histogram == 0)", fn);
  if (metric->column >= TQ_MAX_COLUMNS || !s->columns[metric->column].live)
    return fail(TQ_ERR_INVALID, "%s: metric column %u is not a live column of the segment", fn, metric->column);
  if (metric->value_type > TQ_VALUE_F64) return fail(TQ_ERR_INVALID, "%s: metric value_type %u", fn, metric->value_type);
  if (plan.n_buckets && !bucket_stats)
    return fail(TQ_ERR_INVALID, "%s: null bucket records for a histogram of %u buckets", fn, plan.n_buckets);
  return TQ_OK;
}

// tq_agg_batch_device / tq_agg_sub_batch_device (metric: null / the metric column)
int agg_device_call(tq_segment *s, const char *fn, const tq_query *queries, uint32_t n_queries, const tq_agg_request *req,
                    const tq_agg_metric_request *metric, tq_agg_stats_t *d_out_stats, uint32_t *d_out_buckets,
                    tq_agg_bucket_stats_t *d_out_bucket_stats, uint32_t bucket_stride, void *hip_stream) {
  try {
    TQ_SEGMENT_LOCK(s);
    tq_agg_hist_plan_t plan;
    int rc = check_agg_call(s, fn, req, d_out_buckets, bucket_stride, &plan);
    if (rc == TQ_OK && metric) rc = check_metric(s, fn, req, metric, d_out_bucket_stats, plan);
    if (rc != TQ_OK || n_queries == 0) return rc;
    AggSpec spec{req->column, req->value_type, plan, req->interval, req->offset, bucket_stride, d_out_stats, d_out_buckets};
    spec.metric = metric;
    spec.d_bucket_stats = d_out_bucket_stats;
    DocsetCall call(fn, DocsetConsumer::kAgg);
    call.hip_stream = hip_stream;
    call.agg = &spec;
    return docset_batch(s, queries, n_queries, call);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

// tq_agg_batch / tq_agg_sub_batch
int agg_host_call(tq_segment *s, const char *fn, const tq_query *queries, uint32_t n_queries, const tq_agg_request *req,
                  const tq_agg_metric_request *metric, tq_agg_stats_t *out_stats, uint32_t *out_buckets,
                  tq_agg_bucket_stats_t *out_bucket_stats, uint32_t bucket_stride) {
  try {
    TQ_SEGMENT_LOCK(s);
    tq_agg_hist_plan_t plan;
    int rc = check_agg_call(s, fn, req, out_buckets, bucket_stride, &plan);
    if (rc == TQ_OK && metric) rc = check_metric(s, fn, req, metric, out_bucket_stats, plan);
    if (rc != TQ_OK || n_queries == 0) return rc;
    AggSpec spec{req->column, req->value_type, plan, req->interval, req->offset, 0u, nullptr, nullptr};
    spec.metric = metric;
    return agg_host_run(s, fn, queries, n_queries, spec, out_stats, out_buckets, out_bucket_stats, bucket_stride);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

}  // namespace

int agg_histogram_plan_checked(const char *fn, const tq_column_info_t &info, const tq_agg_request &req, tq_agg_hist_plan_t *out) {
  return histogram_plan(fn, info, req, out);
}

// The host-output variant of a checked call whose rows are plan.n_buckets entries per query (the histogram's, the range
// aggregation's): the segment is locked, spec holds everything but the outputs.
int agg_host_run(tq_segment *s, const char *fn, const tq_query *queries, uint32_t n_queries, AggSpec &spec, tq_agg_stats_t *out_stats,
                 uint32_t *out_buckets, tq_agg_bucket_stats_t *out_bucket_stats, uint32_t bucket_stride) {
  const tq_agg_hist_plan_t &plan = spec.plan;
  const tq_agg_metric_request *const metric = spec.metric;
  HIP_TRY(hipSetDevice(s->device));
  int rc = wait_segment_idle(s);  // (the buffer below may be a batch in flight's)
  if (rc != TQ_OK) return rc;
  // on the device: [records | rows of n_buckets entries | with a metric: bucket records, n_buckets per query], copied
  // back row by row into the caller's stride
  const size_t stats_bytes = (size_t)n_queries * sizeof(tq_agg_stats_t);
  const size_t row_bytes = (size_t)plan.n_buckets * sizeof(uint32_t);
  const size_t rec_at = (stats_bytes + (size_t)n_queries * row_bytes + 7u) & ~(size_t)7u;
  const size_t rec_row_bytes = metric ? (size_t)plan.n_buckets * sizeof(tq_agg_bucket_stats_t) : 0u;
  rc = s->d_agg_rows.ensure(rec_at + (size_t)n_queries * rec_row_bytes + 64u);
  if (rc != TQ_OK) return rc;
  uint8_t *const base = (uint8_t *)s->d_agg_rows.p;
  spec.bucket_stride = plan.n_buckets;
  spec.d_stats = (tq_agg_stats_t *)base;
  spec.d_buckets = plan.n_buckets ? (uint32_t *)(base + stats_bytes) : nullptr;
  spec.d_bucket_stats = rec_row_bytes ? (tq_agg_bucket_stats_t *)(base + rec_at) : nullptr;
  DocsetCall call(fn, DocsetConsumer::kAgg);
  call.agg = &spec;
  rc = docset_batch(s, queries, n_queries, call);
  if (rc != TQ_OK) return rc;
  hipStream_t st = s->stream;
  HIP_TRY(hipMemcpyAsync(out_stats, base, stats_bytes, hipMemcpyDeviceToHost, st));
  if (plan.n_buckets && bucket_stride == plan.n_buckets)
    HIP_TRY(hipMemcpyAsync(out_buckets, base + stats_bytes, (size_t)n_queries * row_bytes, hipMemcpyDeviceToHost, st));
  else if (plan.n_buckets)
    HIP_TRY(hipMemcpy2DAsync(out_buckets, (size_t)bucket_stride * sizeof(uint32_t), base + stats_bytes, row_bytes, row_bytes, n_queries,
                             hipMemcpyDeviceToHost, st));
  if (rec_row_bytes)
    HIP_TRY(hipMemcpy2DAsync(out_bucket_stats, (size_t)bucket_stride * sizeof(tq_agg_bucket_stats_t), base + rec_at, rec_row_bytes,
                             rec_row_bytes, n_queries, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (s->d_agg_rows.cap > ((size_t)256 << 20)) s->d_agg_rows.release();  // (a large result is not kept as scratch)
  return slop_overflow_readback(s, fn);  // a sloppy phrase whose carried list went over the cap is reported; the other rows are valid
}

// what the aggregation launches add to: the totals, every query's match count, the records and bucket rows (and, with a
// metric, the bucket records)
int agg_prepare(tq_segment *s, AggSpec &spec, uint32_t n_queries, uint32_t max_sub_n, uint32_t n_words, hipStream_t st) {
  spec.n_slices = pick_slices(s, s->opt.agg_slices, tqk_agg_step_words(), max_sub_n, n_words);
  spec.words_per_slice = (n_words + spec.n_slices - 1u) / spec.n_slices;
  spec.optional = s->columns[spec.column].dev.present != nullptr;
  if (spec.terms) return agg_terms_prepare(s, spec, n_queries, st);
  if (spec.range) {  // (its starts; the records and rows below are a histogram's of plan.n_buckets buckets)
    const int rc = agg_range_prepare(s, spec, st);
    if (rc != TQ_OK) return rc;
  }
  s->stats.algorithmic_bytes += (uint64_t)n_queries * (sizeof(tq_agg_stats_t) + 4u * (uint64_t)spec.plan.n_buckets);
  HIP_TRY(hipMemsetAsync(s->d_match_counter, 0, (spec.metric ? 5u : 3u) * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(s->d_qmatches.p, 0, (size_t)n_queries * sizeof(uint32_t), st));
  const int rc = launched(tqk_launch_agg_init((TqkAggStats *)spec.d_stats, spec.d_buckets, n_queries, spec.plan.n_buckets, spec.bucket_stride, st), "aggregation init");
  if (rc != TQ_OK || !spec.metric) return rc;
  spec.metric_optional = s->columns[spec.metric->column].dev.present != nullptr;
  s->stats.algorithmic_bytes += (uint64_t)n_queries * sizeof(tq_agg_bucket_stats_t) * (uint64_t)spec.plan.n_buckets;
  return launched(tqk_launch_agg_sub_init((TqkAggBucketStats *)spec.d_bucket_stats, n_queries, spec.plan.n_buckets, spec.bucket_stride, st),
                  "sub-aggregation init");
}

// the aggregation in place of the count / scan / write passes: records and rows under the caller's query index
int agg_launch(tq_segment *s, const AggSpec &spec, const TqkDocsetParams &p, uint32_t q0, hipStream_t st) {
  if (spec.terms) return agg_terms_launch(s, spec, p, q0, st);
  const tq_segment::ColumnHost &col = s->columns[spec.column];
  TqkAggParams ap{};
  ap.ds = p;
  ap.col = col.dev;
  ap.min_value = col.info.min_value;
  ap.gcd = col.info.gcd;
  ap.stats = (TqkAggStats *)spec.d_stats + q0;
  ap.buckets = spec.d_buckets ? spec.d_buckets + (size_t)q0 * spec.bucket_stride : nullptr;
  ap.query_sizes = p.query_sizes;
  ap.totals = s->d_match_counter;
  ap.interval = spec.interval;
  ap.offset = spec.offset;
  ap.bounds_min = spec.plan.bounds_min;
  ap.bounds_max = spec.plan.bounds_max;
  ap.base_pos = spec.plan.base_pos;
  ap.n_buckets = spec.plan.n_buckets;
  ap.bucket_stride = spec.bucket_stride;
  ap.lds_buckets = s->opt.agg_lds_buckets < 0 ? tqk_agg_lds_buckets() : (uint32_t)s->opt.agg_lds_buckets;
  ap.value_type = spec.value_type;
  ap.n_slices = spec.n_slices;
  ap.words_per_slice = spec.words_per_slice;
  if (spec.range) return agg_range_launch(s, spec, ap, q0, st);  // (ap's histogram fields are not read)
  if (!spec.metric || !spec.plan.n_buckets)  // (no bucket: no bucket record either; the record alone)
    return launched(tqk_launch_agg(ap, st), "aggregation kernel");
  const tq_segment::ColumnHost &mcol = s->columns[spec.metric->column];
  uint32_t caps[2];
  tqk_agg_sub_lds_capacities(caps);
  TqkAggSubParams sp{};
  sp.a = ap;
  sp.a.lds_buckets = std::min(ap.lds_buckets, caps[1]);
  sp.col_b = mcol.dev;
  sp.min_value_b = mcol.info.min_value;
  sp.gcd_b = mcol.info.gcd;
  sp.bucket_stats = (TqkAggBucketStats *)spec.d_bucket_stats + (size_t)q0 * spec.bucket_stride;
  sp.value_type_b = spec.metric->value_type;
  return launched(tqk_launch_agg_sub(sp, st), "sub-aggregation kernel");
}

int agg_finish(tq_segment *s, const AggSpec &spec, uint32_t n_queries, hipStream_t st) {
  return spec.terms ? agg_terms_finish(s, spec, n_queries, st) : TQ_OK;
}

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
  return agg_device_call(s, fn, queries, n_queries, req, nullptr, d_out_stats, d_out_buckets, nullptr, bucket_stride, hip_stream);
}

int tq_agg_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_request *req, tq_agg_stats_t *out_stats,
                 uint32_t *out_buckets, uint32_t bucket_stride) {
  const char *fn = "tq_agg_batch";
  if (!s || !req || (!queries && n_queries) || (!out_stats && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  return agg_host_call(s, fn, queries, n_queries, req, nullptr, out_stats, out_buckets, nullptr, bucket_stride);
}

int tq_agg_sub_batch_device(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_request *req,
                            const tq_agg_metric_request *metric, tq_agg_stats_t *d_out_stats, uint32_t *d_out_buckets,
                            tq_agg_bucket_stats_t *d_out_bucket_stats, uint32_t bucket_stride, void *hip_stream) {
  const char *fn = "tq_agg_sub_batch_device";
  if (!s || !req || !metric || (!queries && n_queries) || (!d_out_stats && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  return agg_device_call(s, fn, queries, n_queries, req, metric, d_out_stats, d_out_buckets, d_out_bucket_stats, bucket_stride, hip_stream);
}

int tq_agg_sub_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_request *req,
                     const tq_agg_metric_request *metric, tq_agg_stats_t *out_stats, uint32_t *out_buckets,
                     tq_agg_bucket_stats_t *out_bucket_stats, uint32_t bucket_stride) {
  const char *fn = "tq_agg_sub_batch";
  if (!s || !req || !metric || (!queries && n_queries) || (!out_stats && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  return agg_host_call(s, fn, queries, n_queries, req, metric, out_stats, out_buckets, out_bucket_stats, bucket_stride);
}

void tq_agg_sub_lds_capacities(uint32_t out[2]) { tqk_agg_sub_lds_capacities(out); }

}  // extern "C"
