// tq_sort.cpp — tq_search_sorted_batch / tq_search_sorted_batch_device: TopDocs::order_by_fast_field on the device.  The
// segment's first min(k, matches) alive matching docs of every query under a u64 column's order (the reference's
// collect_segment_top_k over SortByStaticFastValue, src/collector/sort_key/sort_key_computer.rs:118-135).  The checks of
// the sort itself, its launch geometry, buffers and launches (kernels: tq_sort.hip) live here; the match words the
// selection reads — validation of the queries, the doc-set expression, tree and slop planning, sub-batches, scatter — come
// from docset_batch (tq_docset.cpp), which calls sort_prepare once and sort_launch per sub-batch.
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

// The slices per query of a sorted or an aggregation call: enough workgroups for the machine, no slice below four steps of
// the walk (1024 words), or what "sort_slices" / "agg_slices" forces.
uint32_t pick_slices(const tq_segment *s, int forced, uint32_t step_words, uint32_t max_sub_n, uint32_t n_words) {
  if (forced > 0) return (uint32_t)forced;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || cus <= 0) cus = 256;
  const uint32_t want = ((uint32_t)cus * 4u + max_sub_n - 1u) / std::max(1u, max_sub_n);
  return std::max(1u, std::min({want, 256u, n_words / (4u * step_words)}));
}

int sort_prepare(tq_segment *s, SortSpec &spec, const tq_query *queries, uint32_t n_queries, uint32_t max_sub_n, uint32_t n_words, hipStream_t st) {
  uint32_t max_k = 1;
  for (uint32_t qi = 0; qi < n_queries; ++qi) max_k = std::max(max_k, queries[qi].k);
  spec.kpl = max_k <= 64u ? 1 : max_k <= 256u ? 4 : 16;
  spec.n_slices = pick_slices(s, s->opt.sort_slices, tqk_sort_step_words(), max_sub_n, n_words);
  spec.words_per_slice = (n_words + spec.n_slices - 1u) / spec.n_slices;
  spec.optional = s->columns[spec.column].dev.present != nullptr;
  const size_t ks_bytes = (size_t)n_queries * sizeof(uint32_t);
  const size_t part_bytes = spec.n_slices > 1u ? (size_t)max_sub_n * spec.n_slices * (size_t)spec.kpl * 64u * 2u * sizeof(uint64_t) : 0u;
  int rc = s->h_sort_ks.ensure(ks_bytes);
  if (rc == TQ_OK) rc = s->d_sort_ks.ensure(ks_bytes);
  if (rc == TQ_OK && part_bytes) rc = s->d_sort_partials.ensure(part_bytes);
  if (rc == TQ_OK && part_bytes) rc = s->d_sort_slice_counts.ensure((size_t)max_sub_n * spec.n_slices * sizeof(uint2));
  if (rc != TQ_OK) return rc;
  uint32_t *const h_ks = (uint32_t *)s->h_sort_ks.p;  // every query's k, and the three totals the selection adds to
  for (uint32_t qi = 0; qi < n_queries; ++qi) h_ks[qi] = queries[qi].k;
  HIP_TRY(hipMemcpyAsync(s->d_sort_ks.p, h_ks, ks_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(s->d_match_counter, 0, 3u * sizeof(unsigned long long), st));
  return TQ_OK;
}

// the selection in place of the count / scan / write passes: rows under the caller's query index
int sort_launch(tq_segment *s, const SortSpec &spec, const TqkDocsetParams &p, uint32_t q0, hipStream_t st) {
  const tq_segment::ColumnHost &col = s->columns[spec.column];
  TqkSortParams sp{};
  sp.ds = p;
  sp.col = col.dev;
  sp.min_value = col.info.min_value;
  sp.gcd = col.info.gcd;
  sp.ks = (const uint32_t *)s->d_sort_ks.p + q0;
  sp.partials = (uint64_t *)s->d_sort_partials.p;
  sp.slice_counts = (uint2 *)s->d_sort_slice_counts.p;
  sp.out_docs = spec.d_docs + (size_t)q0 * spec.out_stride;
  sp.out_values = spec.d_values + (size_t)q0 * spec.out_stride;
  sp.out_has_value = spec.d_has_value + (size_t)q0 * spec.out_stride;
  sp.out_counts = spec.d_counts + q0;
  sp.query_sizes = p.query_sizes;
  sp.totals = s->d_match_counter;
  sp.n_slices = spec.n_slices;
  sp.words_per_slice = spec.words_per_slice;
  sp.out_stride = spec.out_stride;
  sp.ascending = spec.ascending;
  sp.nulls_first = spec.nulls_first;
  hipError_t e = tqk_launch_sort_select(sp, (int)spec.kpl, st);
  if (e == hipSuccess) e = tqk_launch_sort_merge(sp, (int)spec.kpl, st);
  return launched(e, "sort kernel");
}

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
    SortSpec spec{column, order, nulls, out_stride, d_out_docs, d_out_values, d_out_has_value, d_out_counts};
    DocsetCall call(fn, DocsetConsumer::kSort);
    call.hip_stream = hip_stream;
    call.sort = &spec;
    return docset_batch(s, queries, n_queries, call);
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
    rc = wait_segment_idle(s);  // (the row buffer below may be a batch in flight's)
    if (rc != TQ_OK) return rc;
    // the rows on the device: [values | docs | counts | flags], each part aligned for its type
    const size_t n_ent = (size_t)n_queries * out_stride;
    const size_t docs_at = n_ent * sizeof(uint64_t), counts_at = docs_at + n_ent * sizeof(uint32_t);
    const size_t has_at = counts_at + (size_t)n_queries * sizeof(uint32_t);
    rc = s->d_sort_rows.ensure(has_at + n_ent);
    if (rc != TQ_OK) return rc;
    uint8_t *const base = (uint8_t *)s->d_sort_rows.p;
    SortSpec spec{column, order, nulls, out_stride, (uint32_t *)(base + docs_at), (uint64_t *)base, base + has_at, (uint32_t *)(base + counts_at)};
    DocsetCall call(fn, DocsetConsumer::kSort);
    call.sort = &spec;
    rc = docset_batch(s, queries, n_queries, call);
    if (rc != TQ_OK) return rc;
    hipStream_t st = s->stream;
    HIP_TRY(hipMemcpyAsync(out_values, base, n_ent * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_docs, base + docs_at, n_ent * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_counts, base + counts_at, (size_t)n_queries * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_has_value, base + has_at, n_ent, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (s->d_sort_rows.cap > ((size_t)256 << 20)) s->d_sort_rows.release();  // (a large result is not kept as scratch)
    return slop_overflow_readback(s, fn);  // a sloppy phrase whose carried list went over the cap is reported; the other rows are valid
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "%s: %s", fn, e.what());
  }
}

}  // extern "C"
