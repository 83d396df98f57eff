// tq_agg_terms_hist.cpp — tq_agg_terms_hist_plan / tq_agg_terms_hist_batch / tq_agg_terms_hist_batch_device: a terms bucket
// aggregation over a column T with a dense histogram of a column H per key, per query of a batch, on the device (the
// reference: src/aggregation/bucket/term_agg/term_histogram.rs, the fused collector; the buffered path of term_agg/mod.rs
// for what it leaves out).  The plan is the terms plan of T (tq_agg_terms.cpp), the histogram plan of H (tq_agg.cpp) and the
// grid's size; the scratch rows, the launch geometry and the launches live here (kernels: tq_agg_terms_hist.hip, the
// selection: tq_agg_terms.hip); the match words come from docset_batch (tq_docset.cpp) with the consumer kAgg: agg_prepare
// / agg_launch / agg_finish hand a spec that carries `terms_hist` to the three functions below.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

static_assert(sizeof(tq_agg_terms_hist_request) == 56 && sizeof(tq_agg_terms_hist_plan_t) == 64, "the ABI of the terms x histogram calls");
static_assert(offsetof(tq_agg_terms_hist_request, hist) == 16 && offsetof(tq_agg_terms_hist_plan_t, hist) == 24 &&
                  offsetof(tq_agg_terms_hist_plan_t, n_cells) == 56,
              "the request's and the plan's bytes");

namespace tqi {

namespace {

int terms_hist_plan_checked(const char *fn, const tq_column_info_t &info_t, const tq_column_info_t &info_h,
                            const tq_agg_terms_hist_request &req, tq_agg_terms_hist_plan_t *out) {
  *out = tq_agg_terms_hist_plan_t{};
  if (req.reserved || req.hist.reserved) return fail(TQ_ERR_INVALID, "%s: reserved fields of the request are not zero", fn);
  if (req.hist.histogram != 1u)
    return fail(TQ_ERR_INVALID, "%s: the histogram half needs histogram == 1 (histogram == %u)", fn, req.hist.histogram);
  int rc = agg_terms_plan_checked(fn, info_t, req.terms, TQ_TERMS_KEY_DESC, &out->terms);
  if (rc == TQ_OK) rc = agg_histogram_plan_checked(fn, info_h, req.hist, &out->hist);
  if (rc != TQ_OK) {
    *out = tq_agg_terms_hist_plan_t{};
    return rc;
  }
  const uint64_t n_cells = (uint64_t)out->terms.n_keys * ((uint64_t)out->hist.n_buckets + 1u);
  if (n_cells > (uint64_t)TQ_AGG_MAX_BUCKETS) {
    const uint32_t n_keys = out->terms.n_keys, n_buckets = out->hist.n_buckets;
    *out = tq_agg_terms_hist_plan_t{};
    return fail(TQ_ERR_UNSUPPORTED, "%s: n_keys = %u keys x (n_buckets = %u buckets + 1) is a grid of %llu cells, more than %u (TQ_AGG_MAX_BUCKETS)",
                fn, n_keys, n_buckets, (unsigned long long)n_cells, TQ_AGG_MAX_BUCKETS);
  }
  out->n_cells = (uint32_t)n_cells;
  return TQ_OK;
}

// the checks of a call, and its plan
int check_hist_call(tq_segment *s, const char *fn, const tq_agg_terms_hist_request *req, const void *keys, const void *counts,
                    const void *hist, uint32_t out_stride, uint32_t hist_stride, tq_agg_terms_hist_plan_t *plan) {
  if (req->terms.column >= TQ_MAX_COLUMNS || !s->columns[req->terms.column].live)
    return fail(TQ_ERR_INVALID, "%s: column %u is not a live column of the segment", fn, req->terms.column);
  if (req->hist.column >= TQ_MAX_COLUMNS || !s->columns[req->hist.column].live)
    return fail(TQ_ERR_INVALID, "%s: histogram column %u is not a live column of the segment", fn, req->hist.column);
  const int rc = terms_hist_plan_checked(fn, s->columns[req->terms.column].info, s->columns[req->hist.column].info, *req, plan);
  if (rc != TQ_OK) return rc;
  const uint32_t need = std::min(req->terms.segment_size, plan->terms.n_keys);
  if (out_stride < need)
    return fail(TQ_ERR_INVALID, "%s: out_stride %u below min(segment_size, n_keys) = %u", fn, out_stride, need);
  if (hist_stride < plan->hist.n_buckets)
    return fail(TQ_ERR_INVALID, "%s: hist_stride %u below the histogram's %u buckets", fn, hist_stride, plan->hist.n_buckets);
  if (need && (!keys || !counts)) return fail(TQ_ERR_INVALID, "%s: null output rows for %u keys", fn, plan->terms.n_keys);
  if (need && plan->hist.n_buckets && !hist)
    return fail(TQ_ERR_INVALID, "%s: null histogram rows for %u keys x %u buckets", fn, plan->terms.n_keys, plan->hist.n_buckets);
  return TQ_OK;
}

AggSpec hist_spec(const tq_agg_terms_hist_request *req, const tq_agg_terms_hist_plan_t &plan, tq_agg_terms_t *d_terms, uint64_t *d_keys,
                  uint32_t *d_counts, uint32_t *d_hist, uint32_t out_stride, uint32_t hist_stride) {
  AggSpec spec{req->terms.column, req->hist.value_type, plan.hist, req->hist.interval, req->hist.offset, hist_stride, nullptr, d_hist};
  spec.terms = &req->terms;
  spec.terms_hist = req;
  spec.terms_plan = plan.terms;
  spec.terms_hist_cells = plan.n_cells;
  spec.d_terms = d_terms;
  spec.d_term_keys = d_keys;
  spec.d_term_counts = d_counts;
  spec.terms_stride = out_stride;
  return spec;
}

// the scratch: [grid rows, n_cells per query | totals rows, n_keys per query]
uint32_t *totals_rows_at(tq_segment *s, uint32_t n_queries, uint32_t n_cells) {
  return (uint32_t *)s->d_agg_term_rows.p + (size_t)n_queries * n_cells;
}

TqkAggTermsHistFinishParams finish_params(tq_segment *s, const AggSpec &spec, uint32_t n_queries) {
  TqkAggTermsHistFinishParams fp{};
  fp.records = (const TqkAggTerms *)spec.d_terms;
  fp.grid = (const uint32_t *)s->d_agg_term_rows.p;
  fp.totals_rows = totals_rows_at(s, n_queries, spec.terms_hist_cells);
  fp.out_keys = spec.d_term_keys;
  fp.out_hist = spec.d_buckets;
  fp.min_value = spec.terms_plan.min_value;
  fp.gcd = spec.terms_plan.gcd;
  fp.n_queries = n_queries;
  fp.n_keys = spec.terms_plan.n_keys;
  fp.n_buckets = spec.plan.n_buckets;
  fp.out_stride = spec.terms_stride;
  fp.hist_stride = spec.bucket_stride;
  fp.width = std::min(spec.terms->segment_size, spec.terms_plan.n_keys);
  return fp;
}

}  // namespace

// what the count launches add to: the totals, every query's match count, the records and the scratch rows
int agg_terms_hist_prepare(tq_segment *s, AggSpec &spec, uint32_t n_queries, hipStream_t st) {
  const uint32_t n_keys = spec.terms_plan.n_keys, n_cells = spec.terms_hist_cells;
  spec.terms_n_queries = n_queries;  // (where the totals rows start)
  const int rc = s->d_agg_term_rows.ensure((size_t)n_queries * ((size_t)n_cells + n_keys) * sizeof(uint32_t) + 64u);
  if (rc != TQ_OK) return rc;
  spec.metric_optional = s->columns[spec.terms_hist->hist.column].dev.present != nullptr;
  s->stats.algorithmic_bytes += (uint64_t)n_queries * (sizeof(tq_agg_terms_t) + 4u * ((uint64_t)n_keys + n_cells));
  HIP_TRY(hipMemsetAsync(s->d_match_counter, 0, 6u * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(s->d_qmatches.p, 0, (size_t)n_queries * sizeof(uint32_t), st));
  return launched(tqk_launch_agg_terms_hist_init((TqkAggTerms *)spec.d_terms, (uint32_t *)s->d_agg_term_rows.p,
                                                 totals_rows_at(s, n_queries, n_cells), n_queries, n_cells, n_keys, st),
                  "terms x histogram init");
}

// the count launch in place of a sub-batch's count / scan / write passes: records and grid rows under the caller's query index
int agg_terms_hist_launch(tq_segment *s, const AggSpec &spec, const TqkDocsetParams &p, uint32_t q0, hipStream_t st) {
  const tq_segment::ColumnHost &col = s->columns[spec.column];
  const tq_segment::ColumnHost &hcol = s->columns[spec.terms_hist->hist.column];
  uint32_t caps[2];
  tqk_agg_terms_hist_lds_capacities(caps);
  TqkAggTermsHistParams hp{};
  hp.t.ds = p;
  hp.t.col = col.dev;
  hp.t.min_value = col.info.min_value;
  hp.t.gcd = col.info.gcd;
  hp.t.records = (TqkAggTerms *)spec.d_terms + q0;
  hp.t.rows = (uint32_t *)s->d_agg_term_rows.p + (size_t)q0 * spec.terms_hist_cells;
  hp.t.query_sizes = p.query_sizes;
  hp.t.totals = s->d_match_counter;
  hp.t.n_keys = spec.terms_plan.n_keys;
  hp.t.lds_buckets = s->opt.agg_lds_buckets < 0 ? caps[1] : std::min((uint32_t)s->opt.agg_lds_buckets, caps[1]);
  hp.t.n_slices = spec.n_slices;
  hp.t.words_per_slice = spec.words_per_slice;
  hp.col_h = hcol.dev;
  hp.min_value_h = hcol.info.min_value;
  hp.gcd_h = hcol.info.gcd;
  hp.interval = spec.interval;
  hp.offset = spec.offset;
  hp.bounds_min = spec.plan.bounds_min;
  hp.bounds_max = spec.plan.bounds_max;
  hp.base_pos = spec.plan.base_pos;
  hp.n_buckets = spec.plan.n_buckets;
  hp.value_type_h = spec.value_type;
  return launched(tqk_launch_agg_terms_hist_count(hp, st), "terms x histogram count kernel");
}

// once, behind the last sub-batch's count launch on the same stream: the keys' totals, the terms call's selection over
// them, the survivors' rows
int agg_terms_hist_finish(tq_segment *s, const AggSpec &spec, uint32_t n_queries, hipStream_t st) {
  const TqkAggTermsHistFinishParams fp = finish_params(s, spec, n_queries);
  int rc = launched(tqk_launch_agg_terms_hist_rowsum(fp, st), "terms x histogram row-sum kernel");
  if (rc != TQ_OK) return rc;
  TqkAggTermsSelectParams sp{};
  sp.records = (TqkAggTerms *)spec.d_terms;
  sp.rows = fp.totals_rows;
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
  rc = launched(tqk_launch_agg_terms_select(sp, st), "terms x histogram select kernel");
  if (rc != TQ_OK) return rc;
  return launched(tqk_launch_agg_terms_hist_gather(fp, st), "terms x histogram gather kernel");
}

}  // namespace tqi

extern "C" {

int tq_agg_terms_hist_plan(const tq_column_info_t *info_t, const tq_column_info_t *info_h, const tq_agg_terms_hist_request *req,
                           tq_agg_terms_hist_plan_t *out) {
  const char *fn = "tq_agg_terms_hist_plan";
  if (!info_t || !info_h || !req || !out) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  return terms_hist_plan_checked(fn, *info_t, *info_h, *req, out);
}

int tq_agg_terms_hist_batch_device(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_terms_hist_request *req,
                                   tq_agg_terms_t *d_out_terms, uint64_t *d_out_keys, uint32_t *d_out_counts, uint32_t *d_out_hist,
                                   uint32_t out_stride, uint32_t hist_stride, void *hip_stream) {
  const char *fn = "tq_agg_terms_hist_batch_device";
  if (!s || !req || (!queries && n_queries) || (!d_out_terms && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    tq_agg_terms_hist_plan_t plan;
    const int rc = check_hist_call(s, fn, req, d_out_keys, d_out_counts, d_out_hist, out_stride, hist_stride, &plan);
    if (rc != TQ_OK || n_queries == 0) return rc;
    AggSpec spec = hist_spec(req, plan, d_out_terms, d_out_keys, d_out_counts, d_out_hist, out_stride, hist_stride);
    DocsetCall call(fn, DocsetConsumer::kAgg);
    call.hip_stream = hip_stream;
    call.agg = &spec;
    return docset_batch(s, queries, n_queries, call);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

int tq_agg_terms_hist_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, const tq_agg_terms_hist_request *req,
                            tq_agg_terms_t *out_terms, uint64_t *out_keys, uint32_t *out_counts, uint32_t *out_hist, uint32_t out_stride,
                            uint32_t hist_stride) {
  const char *fn = "tq_agg_terms_hist_batch";
  if (!s || !req || (!queries && n_queries) || (!out_terms && n_queries)) return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    tq_agg_terms_hist_plan_t plan;
    int rc = check_hist_call(s, fn, req, out_keys, out_counts, out_hist, out_stride, hist_stride, &plan);
    if (rc != TQ_OK || n_queries == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    rc = wait_segment_idle(s);  // (the buffer below may be a batch in flight's)
    if (rc != TQ_OK) return rc;
    // on the device: [keys, `width` per query | records | counts, `width` per query | histogram rows, `width` x n_buckets per
    // query] — zeroed, so that what the selection and the gather leave alone past n_returned reads as 0 — copied back row
    // by row into the caller's strides
    const uint32_t width = std::min(req->terms.segment_size, plan.terms.n_keys), n_buckets = plan.hist.n_buckets;
    const size_t key_bytes = (size_t)n_queries * width * sizeof(uint64_t), rec_bytes = (size_t)n_queries * sizeof(tq_agg_terms_t);
    const size_t cnt_bytes = (size_t)n_queries * width * sizeof(uint32_t);
    const size_t hist_row_bytes = (size_t)n_buckets * sizeof(uint32_t), hist_bytes = (size_t)n_queries * width * hist_row_bytes;
    rc = s->d_agg_rows.ensure(key_bytes + rec_bytes + cnt_bytes + hist_bytes + 64u);
    if (rc != TQ_OK) return rc;
    uint8_t *const base = (uint8_t *)s->d_agg_rows.p;
    uint8_t *const d_cnt = base + key_bytes + rec_bytes, *const d_hist = d_cnt + cnt_bytes;
    hipStream_t st = s->stream;
    HIP_TRY(hipMemsetAsync(base, 0, key_bytes + rec_bytes + cnt_bytes + hist_bytes, st));
    AggSpec spec = hist_spec(req, plan, (tq_agg_terms_t *)(base + key_bytes), (uint64_t *)base, (uint32_t *)d_cnt,
                             hist_bytes ? (uint32_t *)d_hist : nullptr, width, n_buckets);
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
    }
    if (hist_bytes && out_stride == width)  // (every query's row set follows the one before it: one copy)
      HIP_TRY(hipMemcpy2DAsync(out_hist, (size_t)hist_stride * sizeof(uint32_t), d_hist, hist_row_bytes, hist_row_bytes,
                               (size_t)n_queries * width, hipMemcpyDeviceToHost, st));
    else if (hist_bytes)
      for (uint32_t q = 0; q < n_queries; ++q)
        HIP_TRY(hipMemcpy2DAsync(out_hist + (size_t)q * out_stride * hist_stride, (size_t)hist_stride * sizeof(uint32_t),
                                 d_hist + (size_t)q * width * hist_row_bytes, hist_row_bytes, hist_row_bytes, width, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (s->d_agg_rows.cap > ((size_t)256 << 20)) s->d_agg_rows.release();  // (a large result is not kept as scratch)
    if (s->d_agg_term_rows.cap > ((size_t)256 << 20)) s->d_agg_term_rows.release();
    return slop_overflow_readback(s, fn);  // a sloppy phrase whose carried list went over the cap is reported; the other rows are valid
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

void tq_agg_terms_hist_lds_capacities(uint32_t out[2]) { tqk_agg_terms_hist_lds_capacities(out); }

}  // extern "C"
