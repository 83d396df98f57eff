// tq_agg_terms_sub.cpp — tq_agg_terms_sub_batch / tq_agg_terms_sub_batch_device: a terms bucket aggregation with a stats
// record of a metric column per key, ordered by doc count, by key or by one metric of the record, per query of a batch, on
// the device (the reference: src/aggregation/bucket/term_agg/mod.rs:836-899, 1040-1111; metric/stats.rs:282-306, 325-357);
// tq_agg_terms_metric_image: the order value of one record, on the host.  The plan and the checks of the terms part are
// tq_agg_terms.cpp's; the scratch rows, the launch geometry and the launches live here (kernels: tq_agg_terms_sub.hip); the
// match words come from docset_batch (tq_docset.cpp) with the consumer kAgg: agg_prepare / agg_launch / agg_finish hand a
// spec that carries `terms_sub` to the three functions below.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

#include "tq_agg_metric_image.hpp"

static_assert(sizeof(tq_agg_terms_sub_request) == 20, "the ABI of the terms-with-a-metric calls");
static_assert(offsetof(tq_agg_terms_sub_request, metric_value_type) == 16 && offsetof(tq_agg_terms_sub_request, reserved) == 18, "the request's bytes");
static_assert(TQ_METRIC_VALUE_COUNT == TQ_IMG_VALUE_COUNT && TQ_METRIC_MIN == TQ_IMG_MIN && TQ_METRIC_MAX == TQ_IMG_MAX &&
                  TQ_METRIC_SUM == TQ_IMG_SUM && TQ_METRIC_AVG == TQ_IMG_AVG,
              "tq_terms_metric is what tq_agg_metric_image.hpp numbers");
static_assert(TQ_VALUE_U64 == TQ_IMG_U64 && TQ_VALUE_I64 == TQ_IMG_I64 && TQ_VALUE_F64 == TQ_IMG_F64, "tq_value_type likewise");

namespace tqi {

namespace {

const char *const kMetricNames[] = {"VALUE_COUNT", "MIN", "MAX", "SUM", "AVG"};

// where the record rows start in the scratch: behind the count rows, on an 8-byte boundary
size_t record_rows_at(uint32_t n_queries, uint32_t n_keys) { return ((size_t)n_queries * n_keys * sizeof(uint32_t) + 7u) & ~(size_t)7u; }

// the checks of a call, and its plan; *terms: the request's terms part
int check_sub_call(tq_segment *s, const char *fn, const tq_agg_terms_sub_request *req, const void *keys, const void *counts,
                   const void *entry_stats, uint32_t out_stride, tq_agg_terms_request *terms, tq_agg_terms_plan_t *plan) {
  *terms = tq_agg_terms_request{req->column, req->order, req->segment_size};
  const int rc = agg_terms_check_call(s, fn, terms, TQ_TERMS_METRIC_ASC, keys, counts, out_stride, plan);
  if (rc != TQ_OK) return rc;
  const bool by_metric = req->order >= TQ_TERMS_METRIC_DESC;
  if (by_metric && req->order_metric > TQ_METRIC_AVG) return fail(TQ_ERR_INVALID, "%s: order_metric %u", fn, req->order_metric);
  if (req->reserved[0] || req->reserved[1]) return fail(TQ_ERR_INVALID, "%s: reserved bytes of the request are not zero", fn);
  if (req->metric_column >= TQ_MAX_COLUMNS || !s->columns[req->metric_column].live)
    return fail(TQ_ERR_INVALID, "%s: metric column %u is not a live column of the segment", fn, req->metric_column);
  if (req->metric_value_type > TQ_VALUE_F64) return fail(TQ_ERR_INVALID, "%s: metric value_type %u", fn, req->metric_value_type);
  if (std::min(req->segment_size, plan->n_keys) && !entry_stats)
    return fail(TQ_ERR_INVALID, "%s: null entry records for %u keys", fn, plan->n_keys);
  if (by_metric && req->metric_value_type == TQ_VALUE_F64 && req->order_metric >= TQ_METRIC_SUM)
    return fail(TQ_ERR_UNSUPPORTED, "%s: an order by %s of a TQ_VALUE_F64 metric column (F64 sums are not served)", fn,
                kMetricNames[req->order_metric]);
  return TQ_OK;
}

AggSpec sub_spec(const tq_agg_terms_sub_request *req, const tq_agg_terms_request *terms, const tq_agg_terms_plan_t &plan,
                 tq_agg_terms_t *d_terms, uint64_t *d_keys, uint32_t *d_counts, tq_agg_bucket_stats_t *d_entry_stats, uint32_t stride) {
  AggSpec spec{req->column, TQ_VALUE_U64, tq_agg_hist_plan_t{}, 0.0, 0.0, 0u, nullptr, nullptr};
  spec.terms = terms;
  spec.terms_sub = req;
  spec.terms_plan = plan;
  spec.d_terms = d_terms;
  spec.d_term_keys = d_keys;
  spec.d_term_counts = d_counts;
  spec.d_term_stats = d_entry_stats;
  spec.terms_stride = stride;
  return spec;
}

}  // namespace

// what the count launches add to: the totals, every query's match count, the records and the scratch rows
int agg_terms_sub_prepare(tq_segment *s, AggSpec &spec, uint32_t n_queries, hipStream_t st) {
  const uint32_t n_keys = spec.terms_plan.n_keys;
  const size_t rec_at = record_rows_at(n_queries, n_keys);
  spec.terms_n_queries = n_queries;  // (where the record rows start: agg_terms_sub_launch)
  const int rc = s->d_agg_term_rows.ensure(rec_at + (size_t)n_queries * n_keys * sizeof(tq_agg_bucket_stats_t) + 64u);
  if (rc != TQ_OK) return rc;
  spec.metric_optional = s->columns[spec.terms_sub->metric_column].dev.present != nullptr;
  s->stats.algorithmic_bytes += (uint64_t)n_queries * (sizeof(tq_agg_terms_t) + (4u + sizeof(tq_agg_bucket_stats_t)) * (uint64_t)n_keys);
  HIP_TRY(hipMemsetAsync(s->d_match_counter, 0, 6u * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(s->d_qmatches.p, 0, (size_t)n_queries * sizeof(uint32_t), st));
  uint8_t *const base = (uint8_t *)s->d_agg_term_rows.p;
  return launched(tqk_launch_agg_terms_sub_init((TqkAggTerms *)spec.d_terms, (uint32_t *)base, (TqkAggBucketStats *)(base + rec_at), n_queries,
                                                n_keys, st),
                  "terms sub-aggregation init");
}

// the count launch in place of a sub-batch's count / scan / write passes: records and rows under the caller's query index
int agg_terms_sub_launch(tq_segment *s, const AggSpec &spec, const TqkDocsetParams &p, uint32_t q0, hipStream_t st) {
  const tq_segment::ColumnHost &col = s->columns[spec.column];
  const tq_segment::ColumnHost &mcol = s->columns[spec.terms_sub->metric_column];
  const uint32_t n_keys = spec.terms_plan.n_keys;
  uint8_t *const base = (uint8_t *)s->d_agg_term_rows.p;
  uint32_t caps[2];
  tqk_agg_terms_sub_lds_capacities(caps);
  TqkAggTermsSubParams tp{};
  tp.t.ds = p;
  tp.t.col = col.dev;
  tp.t.min_value = col.info.min_value;
  tp.t.gcd = col.info.gcd;
  tp.t.records = (TqkAggTerms *)spec.d_terms + q0;
  tp.t.rows = (uint32_t *)base + (size_t)q0 * n_keys;
  tp.t.query_sizes = p.query_sizes;
  tp.t.totals = s->d_match_counter;
  tp.t.n_keys = n_keys;
  tp.t.lds_buckets = s->opt.agg_lds_buckets < 0 ? caps[1] : std::min((uint32_t)s->opt.agg_lds_buckets, caps[1]);
  tp.t.n_slices = spec.n_slices;
  tp.t.words_per_slice = spec.words_per_slice;
  tp.col_b = mcol.dev;
  tp.min_value_b = mcol.info.min_value;
  tp.gcd_b = mcol.info.gcd;
  tp.stats = (TqkAggBucketStats *)(base + record_rows_at(spec.terms_n_queries, n_keys)) + (size_t)q0 * n_keys;
  tp.value_type_b = spec.terms_sub->metric_value_type;
  return launched(tqk_launch_agg_terms_sub_count(tp, st), "terms sub-aggregation count kernel");
}

// the selection, once, behind the last sub-batch's count launch on the same stream
int agg_terms_sub_finish(tq_segment *s, const AggSpec &spec, uint32_t n_queries, hipStream_t st) {
  const uint32_t n_keys = spec.terms_plan.n_keys;
  uint8_t *const base = (uint8_t *)s->d_agg_term_rows.p;
  TqkAggTermsSubSelectParams sp{};
  sp.s.records = (TqkAggTerms *)spec.d_terms;
  sp.s.rows = (const uint32_t *)base;
  sp.s.out_keys = spec.d_term_keys;
  sp.s.out_counts = spec.d_term_counts;
  sp.s.totals = s->d_match_counter;
  sp.s.min_value = spec.terms_plan.min_value;
  sp.s.gcd = spec.terms_plan.gcd;
  sp.s.n_queries = n_queries;
  sp.s.n_keys = n_keys;
  sp.s.out_stride = spec.terms_stride;
  sp.s.segment_size = spec.terms_sub->segment_size;
  sp.s.order = spec.terms_sub->order;
  sp.stats = (const TqkAggBucketStats *)(base + record_rows_at(n_queries, n_keys));
  sp.out_stats = (TqkAggBucketStats *)spec.d_term_stats;
  sp.value_type_b = spec.terms_sub->metric_value_type;
  sp.metric = spec.terms_sub->order_metric;
  return launched(tqk_launch_agg_terms_sub_select(sp, st), "terms sub-aggregation select kernel");
}

}  // namespace tqi

extern "C" {

int tq_agg_terms_sub_batch_device(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_terms_sub_request *req,
                                  tq_agg_terms_t *d_out_terms, uint64_t *d_out_keys, uint32_t *d_out_counts,
                                  tq_agg_bucket_stats_t *d_out_entry_stats, uint32_t out_stride, void *hip_stream) {
  const char *fn = "tq_agg_terms_sub_batch_device";
  if (!s || !req || (!queries && n_queries) || (!d_out_terms && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    tq_agg_terms_request terms;
    tq_agg_terms_plan_t plan;
    const int rc = check_sub_call(s, fn, req, d_out_keys, d_out_counts, d_out_entry_stats, out_stride, &terms, &plan);
    if (rc != TQ_OK || n_queries == 0) return rc;
    AggSpec spec = sub_spec(req, &terms, plan, d_out_terms, d_out_keys, d_out_counts, d_out_entry_stats, out_stride);
    DocsetCall call(fn, DocsetConsumer::kAgg);
    call.hip_stream = hip_stream;
    call.agg = &spec;
    return docset_batch(s, queries, n_queries, call);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

int tq_agg_terms_sub_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_terms_sub_request *req,
                           tq_agg_terms_t *out_terms, uint64_t *out_keys, uint32_t *out_counts, tq_agg_bucket_stats_t *out_entry_stats,
                           uint32_t out_stride) {
  const char *fn = "tq_agg_terms_sub_batch";
  if (!s || !req || (!queries && n_queries) || (!out_terms && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    tq_agg_terms_request terms;
    tq_agg_terms_plan_t plan;
    int rc = check_sub_call(s, fn, req, out_keys, out_counts, out_entry_stats, out_stride, &terms, &plan);
    if (rc != TQ_OK || n_queries == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    rc = wait_segment_idle(s);  // (the buffer below may be a batch in flight's)
    if (rc != TQ_OK) return rc;
    // on the device: [keys, `width` per query | records | entry records, `width` per query | counts, `width` per query] —
    // zeroed, so that what the selection leaves alone past n_returned reads as 0 — copied back row by row into the
    // caller's stride
    const uint32_t width = std::min(req->segment_size, plan.n_keys);
    const size_t key_bytes = (size_t)n_queries * width * sizeof(uint64_t), rec_bytes = (size_t)n_queries * sizeof(tq_agg_terms_t);
    const size_t ent_bytes = (size_t)n_queries * width * sizeof(tq_agg_bucket_stats_t);
    const size_t cnt_bytes = (size_t)n_queries * width * sizeof(uint32_t);
    rc = s->d_agg_rows.ensure(key_bytes + rec_bytes + ent_bytes + cnt_bytes + 64u);
    if (rc != TQ_OK) return rc;
    uint8_t *const base = (uint8_t *)s->d_agg_rows.p;
    uint8_t *const d_ent = base + key_bytes + rec_bytes, *const d_cnt = d_ent + ent_bytes;
    hipStream_t st = s->stream;
    HIP_TRY(hipMemsetAsync(base, 0, key_bytes + rec_bytes + ent_bytes + cnt_bytes, st));
    AggSpec spec = sub_spec(req, &terms, plan, (tq_agg_terms_t *)(base + key_bytes), (uint64_t *)base, (uint32_t *)d_cnt,
                            (tq_agg_bucket_stats_t *)d_ent, width);
    DocsetCall call(fn, DocsetConsumer::kAgg);
    call.agg = &spec;
    rc = docset_batch(s, queries, n_queries, call);
    if (rc != TQ_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out_terms, base + key_bytes, rec_bytes, hipMemcpyDeviceToHost, st));
    if (width) {
      HIP_TRY(hipMemcpy2DAsync(out_keys, (size_t)out_stride * sizeof(uint64_t), base, (size_t)width * sizeof(uint64_t),
                               (size_t)width * sizeof(uint64_t), n_queries, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpy2DAsync(out_counts, (size_t)out_stride * sizeof(uint32_t), d_cnt, (size_t)width * sizeof(uint32_t),
                               (size_t)width * sizeof(uint32_t), n_queries, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpy2DAsync(out_entry_stats, (size_t)out_stride * sizeof(tq_agg_bucket_stats_t), d_ent,
                               (size_t)width * sizeof(tq_agg_bucket_stats_t), (size_t)width * sizeof(tq_agg_bucket_stats_t), n_queries,
                               hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (s->d_agg_rows.cap > ((size_t)256 << 20)) s->d_agg_rows.release();  // (a large result is not kept as scratch)
    if (s->d_agg_term_rows.cap > ((size_t)256 << 20)) s->d_agg_term_rows.release();
    return slop_overflow_readback(s, fn);  // a sloppy phrase whose carried list went over the cap is reported; the other rows are valid
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

void tq_agg_terms_sub_lds_capacities(uint32_t out[2]) { tqk_agg_terms_sub_lds_capacities(out); }

int tq_agg_terms_metric_image(const tq_agg_bucket_stats_t *rec, uint32_t value_type, uint32_t metric, uint64_t out[2]) {
  const char *fn = "tq_agg_terms_metric_image";
  if (!rec || !out) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  if (value_type > TQ_VALUE_F64) return fail(TQ_ERR_INVALID, "%s: value_type %u", fn, value_type);
  if (metric > TQ_METRIC_AVG) return fail(TQ_ERR_INVALID, "%s: metric %u", fn, metric);
  if ((rec->count >> 32) || (rec->sum_hi >> 32))
    return fail(TQ_ERR_INVALID, "%s: a count of %llu, a sum above 2^96 (count below 2^32, sum below 2^96)", fn, (unsigned long long)rec->count);
  if (value_type == TQ_VALUE_F64 && metric >= TQ_METRIC_SUM)
    return fail(TQ_ERR_UNSUPPORTED, "%s: %s of a TQ_VALUE_F64 metric column (F64 sums are not served)", fn, kMetricNames[metric]);
  const TqImage im = tq_metric_image(rec->count, rec->min_value, rec->max_value, rec->sum_lo, rec->sum_hi, value_type, metric);
  out[0] = im.lo;
  out[1] = im.hi;
  return TQ_OK;
}

}  // extern "C"
