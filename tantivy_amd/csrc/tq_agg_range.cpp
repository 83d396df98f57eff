// tq_agg_range.cpp — tq_agg_range_plan / tq_agg_range_bucket_of / tq_agg_range_batch / tq_agg_range_batch_device: a range
// bucket aggregation over a resident u64 column — doc counts per range and, with a metric, a stats record of a second
// column per range — per query of a batch, on the device (the reference: src/aggregation/bucket/range.rs:276-305, 431-437,
// 451-519; src/aggregation/mod.rs:394-402).  The plan — the bounds' conversion into the column's u64 space, the sort, the
// inserted buckets, the refusals — is host arithmetic and lives here, as do the upload of the buckets' starts and the
// launch (kernel: tq_agg_range.hip; the search both sides run: tq_agg_range_search.hpp).  Everything else is the
// histogram's: agg_prepare / agg_launch of tq_agg.cpp initialise the records and rows and fill the launch parameters for a
// spec that carries `range`, and the match words come from docset_batch (tq_docset.cpp) with the consumer kAgg.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_agg_range_search.hpp"
#include "tq_agg_value.hpp"
#include "tq_internal.hpp"

#include <cmath>

static_assert(sizeof(tq_agg_range_t) == 24 && sizeof(tq_agg_range_request) == 24 && sizeof(tq_agg_range_bucket_t) == 24,
              "the ABI of the range aggregation calls");

namespace tqi {

namespace {

// f64_to_fastfield_u64 with Rust's saturating `as` casts written out (a C++ cast of an out-of-range double is undefined);
// val is not a NaN
uint64_t bound_to_u64(double val, uint32_t value_type) {
  if (value_type == TQ_VALUE_I64) return (uint64_t)tq_agg_sat_i64(val) ^ (1ull << 63);
  if (value_type == TQ_VALUE_F64) {
    uint64_t bits;
    __builtin_memcpy(&bits, &val, sizeof bits);
    return (bits >> 63) ? ~bits : bits ^ (1ull << 63);
  }
  if (!(val > 0.0)) return 0ull;  // (negatives, -0.0)
  if (val >= 18446744073709551616.0) return UINT64_MAX;
  return (uint64_t)val;
}

// the plan under `fn`; out is left empty by a refusal
int range_plan(const char *fn, const tq_agg_range_request &req, std::vector<tq_agg_range_bucket_t> &out) {
  out.clear();
  if (!req.ranges) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  if (req.n_ranges == 0u) return fail(TQ_ERR_INVALID, "%s: n_ranges == 0: a range aggregation needs a range", fn);
  if (req.value_type > TQ_VALUE_F64) return fail(TQ_ERR_INVALID, "%s: value_type %u", fn, req.value_type);
  if (req.reserved[0] | req.reserved[1] | req.reserved[2] | req.reserved2) return fail(TQ_ERR_INVALID, "%s: non-zero reserved bytes of the request", fn);
  std::vector<tq_agg_range_bucket_t> b;
  b.reserve((size_t)req.n_ranges * 2u + 1u);
  for (uint32_t i = 0; i < req.n_ranges; ++i) {
    const tq_agg_range_t &r = req.ranges[i];
    uint8_t rsv = 0;
    for (uint8_t x : r.reserved) rsv |= x;
    if (rsv || r.has_from > 1u || r.has_to > 1u) return fail(TQ_ERR_INVALID, "%s: range %u: non-zero reserved bytes, or has_from / has_to above 1", fn, i);
    if ((r.has_from && std::isnan(r.from)) || (r.has_to && std::isnan(r.to))) return fail(TQ_ERR_INVALID, "%s: range %u has a NaN bound", fn, i);
  }
  for (uint32_t i = 0; i < req.n_ranges; ++i) {
    const tq_agg_range_t &r = req.ranges[i];
    const uint64_t start = r.has_from ? bound_to_u64(r.from, req.value_type) : 0ull;
    const uint64_t end = r.has_to ? bound_to_u64(r.to, req.value_type) : UINT64_MAX;
    if (start > end)
      return fail(TQ_ERR_INVALID, "%s: range %u starts above its end (%llu > %llu in the column's u64 space)", fn, i,
                  (unsigned long long)start, (unsigned long long)end);
    b.push_back(tq_agg_range_bucket_t{start, end, i, 0u});
  }
  // extend_validate_ranges: sort_by_key is stable
  std::stable_sort(b.begin(), b.end(), [](const tq_agg_range_bucket_t &x, const tq_agg_range_bucket_t &y) { return x.start < y.start; });
  for (size_t i = 0; i + 1 < b.size(); ++i)
    if (b[i].end > b[i + 1].start)
      return fail(TQ_ERR_INVALID, "%s: overlapping ranges %u and %u (end %llu > start %llu in the column's u64 space)", fn, b[i].source,
                  b[i + 1].source, (unsigned long long)b[i].end, (unsigned long long)b[i + 1].start);
  if (b.front().start != 0ull) out.push_back(tq_agg_range_bucket_t{0ull, b.front().start, UINT32_MAX, 0u});
  for (size_t i = 0; i < b.size(); ++i) {
    out.push_back(b[i]);
    if (i + 1 < b.size() && b[i].end != b[i + 1].start) out.push_back(tq_agg_range_bucket_t{b[i].end, b[i + 1].start, UINT32_MAX, 0u});
  }
  if (b.back().end != UINT64_MAX) out.push_back(tq_agg_range_bucket_t{b.back().end, UINT64_MAX, UINT32_MAX, 0u});
  if (out.size() > (size_t)TQ_AGG_RANGE_MAX_BUCKETS) {
    const size_t n = out.size();
    out.clear();
    return fail(TQ_ERR_UNSUPPORTED, "%s: the ranges make %zu buckets, more than %u (TQ_AGG_RANGE_MAX_BUCKETS)", fn, n, TQ_AGG_RANGE_MAX_BUCKETS);
  }
  return TQ_OK;
}

// the checks of a call behind the null checks, and its spec without the outputs
int range_spec(tq_segment *s, const char *fn, const tq_agg_range_request *req, const tq_agg_metric_request *metric, const void *counts,
               const void *bucket_stats, uint32_t bucket_stride, AggSpec &spec) {
  int rc = range_plan(fn, *req, spec.range_plan);
  if (rc != TQ_OK) return rc;
  if (req->column >= TQ_MAX_COLUMNS || !s->columns[req->column].live)
    return fail(TQ_ERR_INVALID, "%s: column %u is not a live column of the segment", fn, req->column);
  if (metric) {
    if (metric->column >= TQ_MAX_COLUMNS || !s->columns[metric->column].live)
      return fail(TQ_ERR_INVALID, "%s: metric column %u is not a live column of the segment", fn, metric->column);
    if (metric->value_type > TQ_VALUE_F64) return fail(TQ_ERR_INVALID, "%s: metric value_type %u", fn, metric->value_type);
    if (metric->reserved[0] | metric->reserved[1] | metric->reserved[2]) return fail(TQ_ERR_INVALID, "%s: non-zero reserved bytes of the metric request", fn);
  }
  const uint32_t n_buckets = (uint32_t)spec.range_plan.size();
  if (bucket_stride < n_buckets) return fail(TQ_ERR_INVALID, "%s: bucket_stride %u below the plan's %u buckets", fn, bucket_stride, n_buckets);
  if (!counts) return fail(TQ_ERR_INVALID, "%s: null count rows for %u buckets", fn, n_buckets);
  if (metric && !bucket_stats) return fail(TQ_ERR_INVALID, "%s: null bucket records for %u buckets", fn, n_buckets);
  spec.column = req->column;
  spec.value_type = req->value_type;
  spec.plan.n_buckets = n_buckets;
  spec.metric = metric;
  spec.range = req;
  return TQ_OK;
}

}  // namespace

// the starts on their way up: pinned staging, one copy on st, no synchronisation (the scratch is idle: agg_prepare's stage)
int agg_range_prepare(tq_segment *s, AggSpec &spec, hipStream_t st) {
  const size_t bytes = spec.range_plan.size() * sizeof(uint64_t);
  int rc = s->h_agg_range_starts.ensure(bytes);
  if (rc == TQ_OK) rc = s->d_agg_range_starts.ensure(bytes);
  if (rc != TQ_OK) return rc;
  uint64_t *const h = (uint64_t *)s->h_agg_range_starts.p;
  for (size_t i = 0; i < spec.range_plan.size(); ++i) h[i] = spec.range_plan[i].start;
  HIP_TRY(hipMemcpyAsync(s->d_agg_range_starts.p, h, bytes, hipMemcpyHostToDevice, st));
  spec.d_range_starts = (const uint64_t *)s->d_agg_range_starts.p;
  s->stats.algorithmic_bytes += bytes;
  return TQ_OK;
}

// the range launch in place of the histogram's: a is agg_launch's, filled for the sub-batch
int agg_range_launch(tq_segment *s, const AggSpec &spec, const TqkAggParams &a, uint32_t q0, hipStream_t st) {
  TqkAggRangeParams rp{};
  rp.s.a = a;
  rp.starts = spec.d_range_starts;
  if (spec.metric) {
    const tq_segment::ColumnHost &mcol = s->columns[spec.metric->column];
    uint32_t caps[2];
    tqk_agg_range_lds_capacities(caps);
    rp.s.a.lds_buckets = std::min(a.lds_buckets, caps[1]);
    rp.s.col_b = mcol.dev;
    rp.s.min_value_b = mcol.info.min_value;
    rp.s.gcd_b = mcol.info.gcd;
    rp.s.bucket_stats = (TqkAggBucketStats *)spec.d_bucket_stats + (size_t)q0 * spec.bucket_stride;
    rp.s.value_type_b = spec.metric->value_type;
  }
  return launched(tqk_launch_agg_range(rp, spec.metric != nullptr, st), "range aggregation kernel");
}

}  // namespace tqi

extern "C" {

int tq_agg_range_plan(const tq_agg_range_request *req, tq_agg_range_bucket_t *out_buckets, uint32_t cap, uint32_t *out_n_buckets) {
  const char *fn = "tq_agg_range_plan";
  if (!req || !out_n_buckets || (!out_buckets && cap)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  *out_n_buckets = 0u;
  try {
    std::vector<tq_agg_range_bucket_t> plan;
    const int rc = range_plan(fn, *req, plan);
    if (rc != TQ_OK) return rc;
    *out_n_buckets = (uint32_t)plan.size();
    if (cap < plan.size()) return fail(TQ_ERR_INVALID, "%s: cap %u below the plan's %zu buckets", fn, cap, plan.size());
    std::copy(plan.begin(), plan.end(), out_buckets);
    return TQ_OK;
  } catch (const std::exception &e) {
    return fail(TQ_ERR_INVALID, "%s: %s", fn, e.what());
  }
}

uint32_t tq_agg_range_bucket_of(const uint64_t *starts, uint32_t n, uint64_t value) {
  return starts ? tq_range_bucket_of(starts, n, value) : 0u;
}

int tq_agg_range_batch_device(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_range_request *req,
                              const tq_agg_metric_request *metric, tq_agg_stats_t *d_out_stats, uint32_t *d_out_counts,
                              tq_agg_bucket_stats_t *d_out_bucket_stats, uint32_t bucket_stride, void *hip_stream) {
  const char *fn = "tq_agg_range_batch_device";
  if (!s || !req || (!queries && n_queries) || (!d_out_stats && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    AggSpec spec{0u, 0u, tq_agg_hist_plan_t{}, 0.0, 0.0, bucket_stride, d_out_stats, d_out_counts};
    const int rc = range_spec(s, fn, req, metric, d_out_counts, d_out_bucket_stats, bucket_stride, spec);
    if (rc != TQ_OK || n_queries == 0) return rc;
    spec.d_bucket_stats = d_out_bucket_stats;
    DocsetCall call(fn, DocsetConsumer::kAgg);
    call.hip_stream = hip_stream;
    call.agg = &spec;
    return docset_batch(s, queries, n_queries, call);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

int tq_agg_range_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_range_request *req,
                       const tq_agg_metric_request *metric, tq_agg_stats_t *out_stats, uint32_t *out_counts,
                       tq_agg_bucket_stats_t *out_bucket_stats, uint32_t bucket_stride) {
  const char *fn = "tq_agg_range_batch";
  if (!s || !req || (!queries && n_queries) || (!out_stats && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    AggSpec spec{0u, 0u, tq_agg_hist_plan_t{}, 0.0, 0.0, 0u, nullptr, nullptr};
    const int rc = range_spec(s, fn, req, metric, out_counts, out_bucket_stats, bucket_stride, spec);
    if (rc != TQ_OK || n_queries == 0) return rc;
    return agg_host_run(s, fn, queries, n_queries, spec, out_stats, out_counts, out_bucket_stats, bucket_stride);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

void tq_agg_range_lds_capacities(uint32_t out[2]) { tqk_agg_range_lds_capacities(out); }

}  // extern "C"
