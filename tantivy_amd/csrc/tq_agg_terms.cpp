// tq_agg_terms.cpp — tq_agg_terms_plan / tq_agg_terms_batch / tq_agg_terms_batch_device: a terms bucket aggregation — the
// top segment_size values of a resident u64 column by doc count or by key — per query of a batch, on the device (the
// reference: src/aggregation/bucket/term_agg/mod.rs:836-899, 1000-1111, 1328-1353).  The plan — the number of keys and
// the validation of the request — is host arithmetic and lives here, as do the scratch rows, the launch geometry and the
// launches (kernels: tq_agg_terms.hip); the match words come from docset_batch (tq_docset.cpp) with the consumer kAgg:
// agg_prepare / agg_launch / agg_finish of tq_agg.cpp hand a spec that carries `terms` to the three functions below.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

static_assert(sizeof(tq_agg_terms_request) == 12 && sizeof(tq_agg_terms_plan_t) == 24, "the ABI of the terms aggregation calls");
static_assert(sizeof(tq_agg_terms_t) == 40 && sizeof(TqkAggTerms) == sizeof(tq_agg_terms_t), "the 40-byte record");
static_assert(offsetof(tq_agg_terms_t, out_of_range) == offsetof(TqkAggTerms, out_of_range), "the record's last word");

namespace tqi {

int agg_terms_plan_checked(const char *fn, const tq_column_info_t &info, const tq_agg_terms_request &req, uint32_t max_order,
                           tq_agg_terms_plan_t *out) {
  *out = tq_agg_terms_plan_t{};
  if (req.segment_size == 0u || req.segment_size > TQ_AGG_TERMS_MAX_SIZE)
    return fail(TQ_ERR_INVALID, "%s: segment_size %u (1..%u, TQ_AGG_TERMS_MAX_SIZE)", fn, req.segment_size, TQ_AGG_TERMS_MAX_SIZE);
  if (req.order > max_order) return fail(TQ_ERR_INVALID, "%s: order %u", fn, req.order);
  if (info.gcd == 0u || info.max_value < info.min_value)
    return fail(TQ_ERR_INVALID, "%s: a column with gcd %llu, min %llu, max %llu", fn, (unsigned long long)info.gcd,
                (unsigned long long)info.min_value, (unsigned long long)info.max_value);
  out->min_value = info.min_value;
  out->gcd = info.gcd;
  if (info.num_rows == 0u) return TQ_OK;  // (no value at all: no key)
  const uint64_t span = (info.max_value - info.min_value) / info.gcd;  // n_keys - 1; exact, no overflow up to max = u64::MAX
  if (span >= (uint64_t)TQ_AGG_MAX_BUCKETS)
    return fail(TQ_ERR_UNSUPPORTED, "%s: the column has n_keys = %.0f, more than %u (TQ_AGG_MAX_BUCKETS); high-cardinality columns are not served",
                fn, (double)span + 1.0, TQ_AGG_MAX_BUCKETS);
  out->n_keys = (uint32_t)span + 1u;
  return TQ_OK;
}

// the checks of a call, and its plan
int agg_terms_check_call(tq_segment *s, const char *fn, const tq_agg_terms_request *req, uint32_t max_order, const void *keys,
                         const void *counts, uint32_t out_stride, tq_agg_terms_plan_t *plan) {
  if (req->column >= TQ_MAX_COLUMNS || !s->columns[req->column].live)
    return fail(TQ_ERR_INVALID, "%s: column %u is not a live column of the segment", fn, req->column);
  const int rc = agg_terms_plan_checked(fn, s->columns[req->column].info, *req, max_order, plan);
  if (rc != TQ_OK) return rc;
  const uint32_t need = std::min(req->segment_size, plan->n_keys);
  if (out_stride < need)
    return fail(TQ_ERR_INVALID, "%s: out_stride %u below min(segment_size, n_keys) = %u", fn, out_stride, need);
  if (need && (!keys || !counts)) return fail(TQ_ERR_INVALID, "%s: null output rows for %u keys", fn, plan->n_keys);
  return TQ_OK;
}

namespace {

AggSpec terms_spec(const tq_agg_terms_request *req, const tq_agg_terms_plan_t &plan, tq_agg_terms_t *d_terms, uint64_t *d_keys,
                   uint32_t *d_counts, uint32_t stride) {
  AggSpec spec{req->column, TQ_VALUE_U64, tq_agg_hist_plan_t{}, 0.0, 0.0, 0u, nullptr, nullptr};
  spec.terms = req;
  spec.terms_plan = plan;
  spec.d_terms = d_terms;
  spec.d_term_keys = d_keys;
  spec.d_term_counts = d_counts;
  spec.terms_stride = stride;
  return spec;
}

}  // namespace

// what the count launches add to: the totals, every query's match count, the records and the scratch rows
int agg_terms_prepare(tq_segment *s, AggSpec &spec, uint32_t n_queries, hipStream_t st) {
  if (spec.terms_hist) return agg_terms_hist_prepare(s, spec, n_queries, st);
  if (spec.terms_sub) return agg_terms_sub_prepare(s, spec, n_queries, st);
  const uint32_t n_keys = spec.terms_plan.n_keys;
  const int rc = s->d_agg_term_rows.ensure((size_t)n_queries * n_keys * sizeof(uint32_t) + 64u);
  if (rc != TQ_OK) return rc;
  s->stats.algorithmic_bytes += (uint64_t)n_queries * (sizeof(tq_agg_terms_t) + 4u * (uint64_t)n_keys);
  HIP_TRY(hipMemsetAsync(s->d_match_counter, 0, 5u * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(s->d_qmatches.p, 0, (size_t)n_queries * sizeof(uint32_t), st));
  return launched(tqk_launch_agg_terms_init((TqkAggTerms *)spec.d_terms, (uint32_t *)s->d_agg_term_rows.p, n_queries, n_keys, st),
                  "terms aggregation init");
}

// the count launch in place of a sub-batch's count / scan / write passes: records and rows under the caller's query index
int agg_terms_launch(tq_segment *s, const AggSpec &spec, const TqkDocsetParams &p, uint32_t q0, hipStream_t st) {
  if (spec.terms_hist) return agg_terms_hist_launch(s, spec, p, q0, st);
  if (spec.terms_sub) return agg_terms_sub_launch(s, spec, p, q0, st);
  const tq_segment::ColumnHost &col = s->columns[spec.column];
  uint32_t caps[2];
  tqk_agg_terms_lds_capacities(caps);
  TqkAggTermsParams tp{};
  tp.ds = p;
  tp.col = col.dev;
  tp.min_value = col.info.min_value;
  tp.gcd = col.info.gcd;
  tp.records = (TqkAggTerms *)spec.d_terms + q0;
  tp.rows = (uint32_t *)s->d_agg_term_rows.p + (size_t)q0 * spec.terms_plan.n_keys;
  tp.query_sizes = p.query_sizes;
  tp.totals = s->d_match_counter;
  tp.n_keys = spec.terms_plan.n_keys;
  tp.lds_buckets = s->opt.agg_lds_buckets < 0 ? caps[1] : std::min((uint32_t)s->opt.agg_lds_buckets, caps[1]);
  tp.n_slices = spec.n_slices;
  tp.words_per_slice = spec.words_per_slice;
  return launched(tqk_launch_agg_terms_count(tp, st), "terms aggregation count kernel");
}

// the selection, once, behind the last sub-batch's count launch on the same stream
int agg_terms_finish(tq_segment *s, const AggSpec &spec, uint32_t n_queries, hipStream_t st) {
  if (spec.terms_hist) return agg_terms_hist_finish(s, spec, n_queries, st);
  if (spec.terms_sub) return agg_terms_sub_finish(s, spec, n_queries, st);
  TqkAggTermsSelectParams sp{};
  sp.records = (TqkAggTerms *)spec.d_terms;
  sp.rows = (const uint32_t *)s->d_agg_term_rows.p;
  sp.out_keys = spec.d_term_keys;
  sp.out_counts = spec.d_term_counts;
  sp.totals = s->d_match_counter;
  sp.min_value = spec.terms_plan.min_value;
  sp.gcd = spec.terms_plan.gcd;
  sp.n_queries = n_queries;
  sp.n_keys = spec.terms_plan.n_keys;
  sp.out_stride = spec.terms_stride;
  sp.segment_size = spec.terms->segment_size;
  sp.order = spec.terms->order;
  return launched(tqk_launch_agg_terms_select(sp, st), "terms aggregation select kernel");
}

}  // namespace tqi

extern "C" {

int tq_agg_terms_plan(const tq_column_info_t *info, const tq_agg_terms_request *req, tq_agg_terms_plan_t *out) {
  const char *fn = "tq_agg_terms_plan";
  if (!info || !req || !out) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  return agg_terms_plan_checked(fn, *info, *req, TQ_TERMS_KEY_DESC, out);
}

int tq_agg_terms_batch_device(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_terms_request *req,
                              tq_agg_terms_t *d_out_terms, uint64_t *d_out_keys, uint32_t *d_out_counts, uint32_t out_stride,
                              void *hip_stream) {
  const char *fn = "tq_agg_terms_batch_device";
  if (!s || !req || (!queries && n_queries) || (!d_out_terms && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    tq_agg_terms_plan_t plan;
    const int rc = agg_terms_check_call(s, fn, req, TQ_TERMS_KEY_DESC, d_out_keys, d_out_counts, out_stride, &plan);
    if (rc != TQ_OK || n_queries == 0) return rc;
    AggSpec spec = terms_spec(req, plan, d_out_terms, d_out_keys, d_out_counts, out_stride);
    DocsetCall call(fn, DocsetConsumer::kAgg);
    call.hip_stream = hip_stream;
    call.agg = &spec;
    return docset_batch(s, queries, n_queries, call);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

int tq_agg_terms_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_terms_request *req,
                       tq_agg_terms_t *out_terms, uint64_t *out_keys, uint32_t *out_counts, uint32_t out_stride) {
  const char *fn = "tq_agg_terms_batch";
  if (!s || !req || (!queries && n_queries) || (!out_terms && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    tq_agg_terms_plan_t plan;
    int rc = agg_terms_check_call(s, fn, req, TQ_TERMS_KEY_DESC, out_keys, out_counts, out_stride, &plan);
    if (rc != TQ_OK || n_queries == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    rc = wait_segment_idle(s);  // (the buffer below may be a batch in flight's)
    if (rc != TQ_OK) return rc;
    // on the device: [keys, `width` per query | records | counts, `width` per query] — zeroed, so that what the selection
    // leaves alone past n_returned reads as 0 — copied back row by row into the caller's stride
    const uint32_t width = std::min(req->segment_size, plan.n_keys);
    const size_t key_bytes = (size_t)n_queries * width * sizeof(uint64_t), rec_bytes = (size_t)n_queries * sizeof(tq_agg_terms_t);
    const size_t cnt_bytes = (size_t)n_queries * width * sizeof(uint32_t);
    rc = s->d_agg_rows.ensure(key_bytes + rec_bytes + cnt_bytes + 64u);
    if (rc != TQ_OK) return rc;
    uint8_t *const base = (uint8_t *)s->d_agg_rows.p;
    hipStream_t st = s->stream;
    HIP_TRY(hipMemsetAsync(base, 0, key_bytes + rec_bytes + cnt_bytes, st));
    AggSpec spec = terms_spec(req, plan, (tq_agg_terms_t *)(base + key_bytes), (uint64_t *)base, (uint32_t *)(base + key_bytes + rec_bytes), width);
    DocsetCall call(fn, DocsetConsumer::kAgg);
    call.agg = &spec;
    rc = docset_batch(s, queries, n_queries, call);
    if (rc != TQ_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out_terms, base + key_bytes, rec_bytes, hipMemcpyDeviceToHost, st));
    if (width) {
      HIP_TRY(hipMemcpy2DAsync(out_keys, (size_t)out_stride * sizeof(uint64_t), base, (size_t)width * sizeof(uint64_t),
                               (size_t)width * sizeof(uint64_t), n_queries, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpy2DAsync(out_counts, (size_t)out_stride * sizeof(uint32_t), base + key_bytes + rec_bytes, (size_t)width * sizeof(uint32_t),
                               (size_t)width * sizeof(uint32_t), n_queries, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (s->d_agg_rows.cap > ((size_t)256 << 20)) s->d_agg_rows.release();  // (a large result is not kept as scratch)
    if (s->d_agg_term_rows.cap > ((size_t)256 << 20)) s->d_agg_term_rows.release();
    return slop_overflow_readback(s, fn);  // a sloppy phrase whose carried list went over the cap is reported; the other rows are valid
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

void tq_agg_terms_lds_capacities(uint32_t out[2]) { tqk_agg_terms_lds_capacities(out); }

uint32_t tq_agg_terms_max_size(void) { return tqk_agg_terms_max_size(); }

}  // extern "C"
