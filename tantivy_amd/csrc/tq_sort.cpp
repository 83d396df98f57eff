// tq_sort.cpp — tq_search_sorted_batch / tq_search_sorted_batch_device: TopDocs::order_by_fast_field on the device.  The
// segment's first min(k, matches) alive matching docs of every query under a u64 column's order (the reference's
// collect_segment_top_k over SortByStaticFastValue, src/collector/sort_key/sort_key_computer.rs:118-135): the checks of the
// sort itself live here, everything in front of the selection — validation of the queries, the doc-set expression, tree
// and slop planning, sub-batches, scatter — is docset_batch's (tq_docset.cpp) under a SortSpec, the kernels tq_sort.hip's.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

namespace tqi {

namespace {

int check_sort_call(tq_segment *s, const char *fn, const tq_query *queries, uint32_t n_queries, uint32_t column, uint8_t order,
                    uint8_t nulls, uint32_t out_stride) {
  if (column >= TQ_MAX_COLUMNS || !s->columns[column].live)
    return fail(TQ_ERR_INVALID, "%s: column %u is not a live column of the segment", fn, column);
  if (order > TQ_SORT_ASC) return fail(TQ_ERR_INVALID, "%s: order %u", fn, order);
  if (nulls > TQ_NULLS_FIRST) return fail(TQ_ERR_INVALID, "%s: nulls %u", fn, nulls);
  uint32_t max_k = 0;
  for (uint32_t qi = 0; qi < n_queries; ++qi) {
    if (queries[qi].k == 0u || queries[qi].k > TQ_MAX_K)
      return fail(TQ_ERR_INVALID, "%s: query %u: k %u (1..%u)", fn, qi, queries[qi].k, TQ_MAX_K);
    max_k = std::max(max_k, queries[qi].k);
  }
  if (out_stride < max_k) return fail(TQ_ERR_INVALID, "%s: out_stride %u below the largest k %u", fn, out_stride, max_k);
  return TQ_OK;
}

}  // namespace

}  // namespace tqi

extern "C" {

int tq_search_sorted_batch_device(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t column, uint8_t order,
                                  uint8_t nulls, uint32_t out_stride, uint32_t *d_out_docs, uint64_t *d_out_values,
                                  uint8_t *d_out_has_value, uint32_t *d_out_counts, void *hip_stream) {
  const char *fn = "tq_search_sorted_batch_device";
  if (!s || (!queries && n_queries) || ((!d_out_docs || !d_out_values || !d_out_has_value || !d_out_counts) && n_queries))
    return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    const int rc = check_sort_call(s, fn, queries, n_queries, column, order, nulls, out_stride);
    if (rc != TQ_OK || n_queries == 0) return rc;
    SortSpec spec{fn, column, order, nulls, out_stride, d_out_docs, d_out_values, d_out_has_value, d_out_counts};
    return docset_batch(s, queries, n_queries, nullptr, nullptr, 0, nullptr, false, true, hip_stream, false, nullptr, 0, &spec);
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

int tq_search_sorted_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t column, uint8_t order, uint8_t nulls,
                           uint32_t out_stride, uint32_t *out_docs, uint64_t *out_values, uint8_t *out_has_value,
                           uint32_t *out_counts) {
  const char *fn = "tq_search_sorted_batch";
  if (!s || (!queries && n_queries) || ((!out_docs || !out_values || !out_has_value || !out_counts) && n_queries))
    return fail(TQ_ERR_INVALID, "%s: null argument", fn);
  try {
    TQ_SEGMENT_LOCK(s);
    int rc = check_sort_call(s, fn, queries, n_queries, column, order, nulls, out_stride);
    if (rc != TQ_OK || n_queries == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    {
      const int wrc = wait_segment_idle(s);  // (the row buffer below may be a batch in flight's)
      if (wrc != TQ_OK) return wrc;
    }
    // the rows on the device: [values | docs | counts | flags], each part aligned for its type
    const size_t n_ent = (size_t)n_queries * out_stride;
    const size_t docs_at = n_ent * sizeof(uint64_t), counts_at = docs_at + n_ent * sizeof(uint32_t);
    const size_t has_at = counts_at + (size_t)n_queries * sizeof(uint32_t);
    rc = s->d_sort_rows.ensure(has_at + n_ent);
    if (rc != TQ_OK) return rc;
    uint8_t *const base = (uint8_t *)s->d_sort_rows.p;
    SortSpec spec{fn, column, order, nulls, out_stride, (uint32_t *)(base + docs_at), (uint64_t *)base, base + has_at,
                  (uint32_t *)(base + counts_at)};
    rc = docset_batch(s, queries, n_queries, nullptr, nullptr, 0, nullptr, false, true, nullptr, false, nullptr, 0, &spec);
    if (rc != TQ_OK) return rc;
    hipStream_t st = s->stream;
    HIP_TRY(hipMemcpyAsync(out_values, base, n_ent * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_docs, base + docs_at, n_ent * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_counts, base + counts_at, (size_t)n_queries * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_has_value, base + has_at, n_ent, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (s->d_sort_rows.cap > ((size_t)256 << 20)) s->d_sort_rows.release();  // (a large result is not kept as scratch)
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
