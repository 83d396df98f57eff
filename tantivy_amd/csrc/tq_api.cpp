// tq_api.cpp — the C ABI of include/tantivy_amd.h: contexts, segment residency, options, statistics,
// deletes and counting, codec access, the cross-segment merge.  Compiled with hipcc.  The other entry
// points: tq_terms.cpp (tq_term_prepare*), tq_search.cpp (tq_search_batch*), tq_submit.cpp (tq_submit /
// tq_wait / tq_search_one), tq_encode.hip, tq_comm.cpp.
#include "tq_internal.hpp"
#include "../host/bm25.hpp"

namespace tqi {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}
}  // namespace tqi

int tq_internal_fail(int code, const char *where, const char *what) {
  return fail(code, "%s: %s", where, what);
}
bool tq_internal_ctx_has_device(const tq_ctx *ctx, int device) {
  return std::find(ctx->devices.begin(), ctx->devices.end(), device) != ctx->devices.end();
}

extern "C" {

const char *tq_last_error(void) { return g_last_error.c_str(); }

int tq_init(const int *device_ids, int n_devices, tq_ctx **out) {
  if (!out) return fail(TQ_ERR_INVALID, "tq_init: out is null");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0)
    return fail(TQ_ERR_NO_DEVICE, "tq_init: no HIP device visible (%s)",
                e == hipSuccess ? "count=0" : hipGetErrorString(e));
  tq_ctx *ctx = new tq_ctx();
  if (!device_ids || n_devices <= 0) {
    ctx->devices.push_back(0);
  } else {
    for (int i = 0; i < n_devices; ++i) {
      if (device_ids[i] < 0 || device_ids[i] >= count) {
        delete ctx;
        return fail(TQ_ERR_INVALID, "tq_init: device %d out of range (%d visible)", device_ids[i],
                    count);
      }
      ctx->devices.push_back(device_ids[i]);
    }
  }
  *out = ctx;
  return TQ_OK;
}

void tq_shutdown(tq_ctx *ctx) { delete ctx; }

static int segment_upload_common(tq_ctx *ctx, int device, uint32_t max_doc, const uint8_t *idx,
                                 size_t idx_len, const uint8_t *pos, size_t pos_len,
                                 const uint8_t *fieldnorm, size_t fn_len, uint8_t record_option,
                                 bool from_device, tq_segment **out) {
  if (!ctx || !out || !idx) return fail(TQ_ERR_INVALID, "tq_segment_upload: null argument");
  if (idx_len < 8) return fail(TQ_ERR_FORMAT, "idx sub-file shorter than its 8-byte header");
  if (record_option > TQ_WITH_FREQS_AND_POSITIONS)
    return fail(TQ_ERR_INVALID, "bad record_option %u", record_option);
  if (fieldnorm && fn_len < max_doc)
    return fail(TQ_ERR_FORMAT, "fieldnorm file has %zu bytes for max_doc %u", fn_len, max_doc);
  if (std::find(ctx->devices.begin(), ctx->devices.end(), device) == ctx->devices.end())
    return fail(TQ_ERR_INVALID, "device %d not part of this context", device);
  HIP_TRY(hipSetDevice(device));
  tq_segment *s = new tq_segment();
  s->submit = tq_new_submit_queue();  // (exists for the segment's whole life: tq_submit takes no creation lock)
  if (!s->submit) {
    delete s;
    return fail(TQ_ERR_INVALID, "tq_segment_upload: out of memory");
  }
  s->ctx = ctx;
  s->device = device;
  s->dscratch = ctx->scratch_for(device);
  s->max_doc = max_doc;
  s->record_option = record_option;
  s->idx_len = idx_len;
  s->pos_len = (pos && pos_len) ? pos_len : 0;
  if (!from_device) {
    s->h_idx.assign(idx, idx + idx_len);
    if (pos && pos_len) s->h_pos.assign(pos, pos + pos_len);
  }
  const hipMemcpyKind kind = from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  auto up = [&](uint8_t **dst, const uint8_t *src, size_t n) -> int {
    HIP_TRY(hipMalloc((void **)dst, n + PAD));
    HIP_TRY(hipMemset(*dst + n, 0, PAD));
    HIP_TRY(hipMemcpy(*dst, src, n, kind));
    return TQ_OK;
  };
  int rc = up(&s->d_idx, idx, idx_len);
  if (rc == TQ_OK && pos && pos_len) rc = up(&s->d_pos, pos, pos_len);
  if (rc == TQ_OK && fieldnorm) rc = up(&s->d_fn, fieldnorm, max_doc);
  if (rc == TQ_OK) {
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_stage_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_batch_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->side_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
      e = hipEventCreateWithFlags(&s->ev_copy_done[i], hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_buf_free[i], hipEventDisableTiming);
    }
    for (int i = 0; i < tq_segment::kTimingRing; ++i) {
      if (e == hipSuccess) e = hipEventCreate(&s->ev_t0[i]);
      if (e == hipSuccess) e = hipEventCreate(&s->ev_t1[i]);
      if (e == hipSuccess) e = hipEventCreate(&s->ev_k0[i]);
      if (e == hipSuccess) e = hipEventCreate(&s->ev_k1[i]);
    }
    // (word 0: the batch's matches; words 1 and 2: a sorted batch's valued matches and row entries, tq_sort.hip; words 3
    // and 4: a sub-aggregation's bucketed docs with a metric value and bucketed docs, tq_agg_sub.hip; word 3 of a terms
    // aggregation: the entries returned, tq_agg_terms.hip; words 4 and 5 of one with a metric: counted docs with a metric
    // value and counted docs, tq_agg_terms_sub.hip)
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_match_counter, 6u * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_tp_info, 2 * sizeof(TqpInfo));
    if (e != hipSuccess) rc = fail(TQ_ERR_HIP, "segment setup: %s", hipGetErrorString(e));
  }
  if (rc != TQ_OK) {
    tq_segment_free(s);
    return rc;
  }
  s->dseg.idx = s->d_idx;
  s->dseg.pos = s->d_pos;
  s->dseg.fieldnorm = s->d_fn;
  s->dseg.max_doc = max_doc;
  s->dseg.const_fieldnorm_id = 1;  // FieldNormReader::constant(max_doc, 1)
  s->dseg.min_fieldnorm_id = 1;
  if (fieldnorm && !from_device) {
    uint8_t mn = 255;
    for (uint32_t d = 0; d < max_doc; ++d) mn = fieldnorm[d] < mn ? fieldnorm[d] : mn;
    s->dseg.min_fieldnorm_id = max_doc ? mn : 0;
  } else if (fieldnorm) {  // smallest fieldnorm id present: a device reduction, 4 bytes back
    uint32_t *slot = (uint32_t *)s->d_tp_info;
    uint32_t mn = 255;
    hipError_t e = hipMemcpy(slot, &mn, 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = tqp_launch_min_fieldnorm(s->d_fn, max_doc, slot, s->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&mn, slot, 4, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) {
      tq_segment_free(s);
      return fail(TQ_ERR_HIP, "fieldnorm scan: %s", hipGetErrorString(e));
    }
    s->dseg.min_fieldnorm_id = max_doc ? mn : 0;
  }
  // Bm25Weight.cache under the segment's own average fieldnorm (bm25.rs:62-69 with avg = total_num_tokens /
  // max_doc, the 8-byte header of the .idx sub-file): the range maxima of lists with bitmaps are built under it
  {
    uint64_t total_tokens = 0;
    hipError_t e = hipSuccess;
    if (!from_device)
      memcpy(&total_tokens, idx, 8);
    else
      e = hipMemcpy(&total_tokens, s->d_idx, 8, hipMemcpyDeviceToHost);
    const float avg = max_doc ? (float)total_tokens / (float)max_doc : 0.0f;
    if (e == hipSuccess && total_tokens && std::isfinite(avg) && avg > 0.0f) {
      const tantivy_amd::Bm25Weight w = tantivy_amd::Bm25Weight::from_idf(1.0f, avg);
      e = hipMalloc((void **)&s->d_local_cache, 256 * sizeof(float));
      if (e == hipSuccess) e = hipMemcpy(s->d_local_cache, w.cache, 256 * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
      tq_segment_free(s);
      return fail(TQ_ERR_HIP, "segment cache: %s", hipGetErrorString(e));
    }
  }
  *out = s;
  return TQ_OK;
}

int tq_segment_upload(tq_ctx *ctx, int device, uint32_t max_doc, const uint8_t *idx,
                      size_t idx_len, const uint8_t *pos, size_t pos_len, const uint8_t *fieldnorm,
                      size_t fn_len, uint8_t record_option, tq_segment **out) {
  return segment_upload_common(ctx, device, max_doc, idx, idx_len, pos, pos_len, fieldnorm, fn_len,
                               record_option, false, out);
}

int tq_segment_upload_device(tq_ctx *ctx, int device, uint32_t max_doc, const uint8_t *d_idx,
                             size_t idx_len, const uint8_t *d_pos, size_t pos_len,
                             const uint8_t *d_fieldnorm, size_t fn_len, uint8_t record_option,
                             tq_segment **out) {
  return segment_upload_common(ctx, device, max_doc, d_idx, idx_len, d_pos, pos_len, d_fieldnorm,
                               fn_len, record_option, true, out);
}

// F fields over one doc-id space: the sub-files laid end to end (each keeps its header and gets its own padding, the
// next one starts 16-byte aligned), uploaded as ONE .idx and ONE .pos buffer; the per-field bases shift a term's offsets
// when it is prepared (tq_fields.cpp), so every decode path works on the concatenation unchanged.
int tq_segment_upload_fields(tq_ctx *ctx, int device, uint32_t max_doc, uint32_t n_fields, const tq_field_files *fields,
                             uint8_t record_option, tq_segment **out) {
  if (!ctx || !out || !fields) return fail(TQ_ERR_INVALID, "tq_segment_upload_fields: null argument");
  if (n_fields == 0 || n_fields > TQ_MAX_FIELDS)
    return fail(TQ_ERR_INVALID, "tq_segment_upload_fields: n_fields %u not in 1..%u", n_fields, TQ_MAX_FIELDS);
  if (n_fields == 1)
    return tq_segment_upload(ctx, device, max_doc, fields[0].idx, fields[0].idx_len, fields[0].pos, fields[0].pos_len,
                             fields[0].fieldnorm, fields[0].fn_len, record_option, out);
  uint64_t idx_base[TQ_MAX_FIELDS], pos_base[TQ_MAX_FIELDS], pos_len[TQ_MAX_FIELDS];
  size_t idx_total = 0, pos_total = 0;
  for (uint32_t f = 0; f < n_fields; ++f) {
    const tq_field_files &ff = fields[f];
    if (!ff.idx) return fail(TQ_ERR_INVALID, "tq_segment_upload_fields: field %u: null idx", f);
    if (ff.idx_len < 8) return fail(TQ_ERR_FORMAT, "field %u: idx sub-file shorter than its 8-byte header", f);
    if (ff.fieldnorm && ff.fn_len < max_doc)
      return fail(TQ_ERR_FORMAT, "field %u: fieldnorm file has %zu bytes for max_doc %u", f, ff.fn_len, max_doc);
    pos_len[f] = ff.pos && ff.pos_len ? ff.pos_len : 0;
    idx_base[f] = idx_total;
    pos_base[f] = pos_total;
    // (the last field's padding is the buffer's own)
    idx_total += f + 1 < n_fields ? (ff.idx_len + PAD + 15) & ~(size_t)15 : ff.idx_len;
    pos_total += f + 1 < n_fields && pos_len[f] ? (pos_len[f] + PAD + 15) & ~(size_t)15 : pos_len[f];
  }
  std::vector<uint8_t> idx(idx_total, 0), pos(pos_total, 0);
  for (uint32_t f = 0; f < n_fields; ++f) {
    memcpy(idx.data() + idx_base[f], fields[f].idx, fields[f].idx_len);
    if (pos_len[f]) memcpy(pos.data() + pos_base[f], fields[f].pos, pos_len[f]);
  }
  tq_segment *s = nullptr;
  int rc = segment_upload_common(ctx, device, max_doc, idx.data(), idx_total, pos_total ? pos.data() : nullptr, pos_total,
                                 fields[0].fieldnorm, fields[0].fn_len, record_option, false, &s);
  if (rc != TQ_OK) return rc;
  s->n_fields = n_fields;
  for (uint32_t f = 0; f < n_fields; ++f) {
    s->field_idx_base[f] = idx_base[f];
    s->field_idx_len[f] = fields[f].idx_len;
    s->field_pos_base[f] = pos_base[f];
    s->field_pos_len[f] = pos_len[f];
    if (f == 0 || !fields[f].fieldnorm) continue;
    hipError_t e = hipMalloc((void **)&s->d_fn_field[f], (size_t)max_doc + PAD);
    if (e == hipSuccess) e = hipMemset(s->d_fn_field[f] + max_doc, 0, PAD);
    if (e == hipSuccess) e = hipMemcpy(s->d_fn_field[f], fields[f].fieldnorm, max_doc, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      tq_segment_free(s);
      return fail(TQ_ERR_HIP, "field %u fieldnorms: %s", f, hipGetErrorString(e));
    }
  }
  *out = s;
  return TQ_OK;
}

void tq_segment_free(tq_segment *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  if (s->batch_in_flight && s->ev_batch_done) (void)hipEventSynchronize(s->ev_batch_done);
  for (void *slab : s->term_slabs) (void)hipFree(slab);  // (the terms' table blobs: tq_term_arena.cpp term_alloc)
  // (bitmaps, byte-wide tfs, position directories, plain lists: the arena and its overflow)
  dense_arena_free(s);
  for (void *ptr : s->dense_extra) (void)hipFree(ptr);
  if (s->d_terms) (void)hipFree(s->d_terms);
  if (s->d_idx) (void)hipFree(s->d_idx);
  if (s->d_pos) (void)hipFree(s->d_pos);
  if (s->d_fn) (void)hipFree(s->d_fn);
  for (uint8_t *fn : s->d_fn_field)
    if (fn) (void)hipFree(fn);
  if (s->d_alive) (void)hipFree(s->d_alive);
  if (s->d_docmat) (void)hipFree(s->d_docmat);
  if (s->d_doccls) (void)hipFree(s->d_doccls);
  if (s->d_tp_info) (void)hipFree(s->d_tp_info);
  if (s->d_local_cache) (void)hipFree(s->d_local_cache);
  if (s->d_match_counter) (void)hipFree(s->d_match_counter);
  s->d_stage.release();
  s->d_misc.release();
  for (int i = 0; i < 2; ++i) {
    s->h_prep_stage[i].release();
    if (s->ev_prep[i]) (void)hipEventDestroy(s->ev_prep[i]);
  }
  if (s->ev_prep_order) (void)hipEventDestroy(s->ev_prep_order);
  s->d_thr.release();
  tq_free_plan_scratch(s->plan);
  s->plan = nullptr;
  tq_free_submit_queue(s->submit);
  s->submit = nullptr;
  s->d_qmatches.release();
  s->d_share_words.release();
  s->d_ashare_words.release();
  s->d_bshare_words.release();
  s->d_count_queries.release();
  s->d_count_out.release();
  s->d_count_bits.release();
  s->d_count_wgs.release();
  s->d_set_work.release();
  free_columns(s);
  s->d_docset_queries.release();
  s->d_docset_counts.release();
  s->d_docset_offs.release();
  s->d_docset_partials.release();
  s->d_docset_starts.release();
  s->d_docset_docs.release();
  s->d_docset_squeries.release();
  s->d_docset_caches.release();
  s->d_docset_scores.release();
  s->d_docset_trees.release();
  s->d_sort_ks.release();
  s->d_sort_partials.release();
  s->d_sort_slice_counts.release();
  s->d_sort_rows.release();
  s->h_sort_ks.release();
  s->d_agg_rows.release();
  s->d_agg_term_rows.release();
  s->d_agg_range_starts.release();
  s->h_agg_range_starts.release();
  s->h_docset.release();
  s->h_stage.release();
  s->h_out.release();
  if (s->side_stream) (void)hipStreamSynchronize(s->side_stream);
  if (s->copy_stream) (void)hipStreamSynchronize(s->copy_stream);
  for (hipEvent_t ev : {s->ev_stage_done, s->ev_fork, s->ev_join, s->ev_batch_done, s->ev_copy_done[0],
                        s->ev_copy_done[1], s->ev_buf_free[0], s->ev_buf_free[1]})
    if (ev) (void)hipEventDestroy(ev);
  if (s->side_stream) (void)hipStreamDestroy(s->side_stream);
  if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
  s->d_stage_alt.release();
  for (int i = 0; i < tq_segment::kTimingRing; ++i)
    for (hipEvent_t ev : {s->ev_t0[i], s->ev_t1[i], s->ev_k0[i], s->ev_k1[i]})
      if (ev) (void)hipEventDestroy(ev);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

}  // extern "C"

namespace tqi {
// Orders work about to be enqueued on `st` after the segment's previous batch, whatever stream
// that batch ran on (no-op when it is the same stream: stream order already holds).
int order_after_last_batch(tq_segment *s, hipStream_t st) {
  if (s->batch_in_flight && s->last_stream != st)
    HIP_TRY(hipStreamWaitEvent(st, s->ev_batch_done, 0));
  return TQ_OK;
}
// Host-side wait for everything the segment has in flight (its own stream and the last batch).
int wait_segment_idle(tq_segment *s) {
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (s->batch_in_flight) {
    HIP_TRY(hipEventSynchronize(s->ev_batch_done));
    s->batch_in_flight = false;
  }
  return TQ_OK;
}
}  // namespace tqi

extern "C" {

int tq_segment_set_alive_bitset(tq_segment *s, const uint8_t *bytes, size_t len) {
  if (!s) return fail(TQ_ERR_INVALID, "tq_segment_set_alive_bitset: null segment");
  TQ_SEGMENT_LOCK(s);
  HIP_TRY(hipSetDevice(s->device));
  {
    const int wrc = wait_segment_idle(s);  // batches may run on a caller's stream
    if (wrc != TQ_OK) return wrc;
  }
  if (s->d_alive) (void)hipFree(s->d_alive);
  s->d_alive = nullptr;
  s->bytes_alive = 0;
  s->dseg.alive = nullptr;
  if (!bytes) return TQ_OK;  // no deletes
  // BitSet::serialize (common/src/bitset.rs:215-223): u32 LE max_value, then 64-bit tiny sets
  if (len < 4) return fail(TQ_ERR_FORMAT, "alive bitset shorter than its header");
  const uint32_t max_value = rd32(bytes);
  const size_t need = ((size_t)s->max_doc + 63) / 64 * 8;
  if (max_value != s->max_doc || len - 4 < need || (len - 4) % 8 != 0)
    return fail(TQ_ERR_FORMAT, "alive bitset for %u docs / %zu bytes does not fit max_doc %u",
                max_value, len - 4, s->max_doc);
  HIP_TRY(hipMalloc((void **)&s->d_alive, len - 4 + PAD));
  HIP_TRY(hipMemset(s->d_alive + (len - 4), 0, PAD));
  HIP_TRY(hipMemcpy(s->d_alive, bytes + 4, len - 4, hipMemcpyHostToDevice));
  s->bytes_alive = len - 4;
  s->dseg.alive = s->d_alive;
  s->alive_docs = 0;  // (what a query that matches every doc counts: tq_count_batch needs no kernel for it)
  for (uint32_t d = 0; d + 8u <= s->max_doc; d += 8u) s->alive_docs += (uint32_t)__builtin_popcount(bytes[4 + (d >> 3)]);
  if (s->max_doc & 7u) s->alive_docs += (uint32_t)__builtin_popcount(bytes[4 + (s->max_doc >> 3)] & ((1u << (s->max_doc & 7u)) - 1u));
  return TQ_OK;
}

int tq_last_batch_match_counts(tq_segment *s, uint32_t *out, uint32_t n) {
  if (!s || !out) return fail(TQ_ERR_INVALID, "tq_last_batch_match_counts: null argument");
  TQ_SEGMENT_LOCK(s);
  if (n > s->last_batch_queries) return fail(TQ_ERR_INVALID, "the last batch had %u queries", s->last_batch_queries);
  HIP_TRY(hipSetDevice(s->device));
  {
    const int wrc = wait_segment_idle(s);
    if (wrc != TQ_OK) return wrc;
  }
  HIP_TRY(hipMemcpy(out, s->d_qmatches.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return TQ_OK;
}

int tq_last_batch_query_kernels(tq_segment *s, uint32_t *out, uint32_t n) {
  if (!s || !out) return fail(TQ_ERR_INVALID, "tq_last_batch_query_kernels: null argument");
  TQ_SEGMENT_LOCK(s);
  if (!s->opt.record_query_kernels || s->last_query_kernel.size() < n)
    return fail(TQ_ERR_INVALID, "the last batch recorded %zu queries (option \"record_query_kernels\")", s->last_query_kernel.size());
  memcpy(out, s->last_query_kernel.data(), (size_t)n * sizeof(uint32_t));
  return TQ_OK;
}

int tq_count_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries,
                   uint32_t *out_counts) {
  if (!s || (!queries && n_queries) || !out_counts)
    return fail(TQ_ERR_INVALID, "tq_count_batch: null argument");
  TQ_SEGMENT_LOCK(s);
  if (n_queries == 0) return TQ_OK;
  return count_batch(s, queries, n_queries, out_counts);
}

// a doc-set call whose consumer is its rows, into host buffers
static DocsetCall rows_call(const char *fn, uint32_t *out_docs, float *out_scores, uint64_t out_cap, uint64_t *out_starts) {
  DocsetCall call(fn);
  call.out_docs = out_docs;
  call.out_scores = out_scores;
  call.out_cap = out_cap;
  call.out_starts = out_starts;
  return call;
}

int tq_docset_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t *out_docs, uint64_t out_cap,
                    uint64_t *out_starts) {
  if (!s || (!queries && n_queries) || (!out_docs && out_cap) || !out_starts)
    return fail(TQ_ERR_INVALID, "tq_docset_batch: null argument");
  TQ_SEGMENT_LOCK(s);
  return docset_batch(s, queries, n_queries, rows_call("tq_docset_batch", out_docs, nullptr, out_cap, out_starts));
}

int tq_docset_batch_device(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t *d_out_docs,
                           uint64_t out_cap, uint64_t *d_out_starts, void *hip_stream) {
  if (!s || (!queries && n_queries) || (!d_out_docs && out_cap) || !d_out_starts)
    return fail(TQ_ERR_INVALID, "tq_docset_batch_device: null argument");
  TQ_SEGMENT_LOCK(s);
  DocsetCall call = rows_call("tq_docset_batch_device", d_out_docs, nullptr, out_cap, d_out_starts);
  call.device_out = true;
  call.hip_stream = hip_stream;
  return docset_batch(s, queries, n_queries, call);
}

int tq_docset_scored_batch(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t *out_docs, float *out_scores,
                           uint64_t out_cap, uint64_t *out_starts) {
  if (!s || (!queries && n_queries) || ((!out_docs || !out_scores) && out_cap) || !out_starts)
    return fail(TQ_ERR_INVALID, "tq_docset_scored_batch: null argument");
  TQ_SEGMENT_LOCK(s);
  DocsetCall call = rows_call("tq_docset_scored_batch", out_docs, out_scores, out_cap, out_starts);
  call.scored = true;
  return docset_batch(s, queries, n_queries, call);
}

int tq_docset_scored_batch_device(tq_segment *s, const tq_query *queries, uint32_t n_queries, uint32_t *d_out_docs,
                                  float *d_out_scores, uint64_t out_cap, uint64_t *d_out_starts, void *hip_stream) {
  if (!s || (!queries && n_queries) || ((!d_out_docs || !d_out_scores) && out_cap) || !d_out_starts)
    return fail(TQ_ERR_INVALID, "tq_docset_scored_batch_device: null argument");
  TQ_SEGMENT_LOCK(s);
  DocsetCall call = rows_call("tq_docset_scored_batch_device", d_out_docs, d_out_scores, out_cap, d_out_starts);
  call.scored = call.device_out = true;
  call.hip_stream = hip_stream;
  return docset_batch(s, queries, n_queries, call);
}

int tq_last_batch_stats(tq_segment *s, tq_batch_stats *out) {
  if (!s || !out) return fail(TQ_ERR_INVALID, "tq_last_batch_stats: null argument");
  TQ_SEGMENT_LOCK(s);
  HIP_TRY(hipSetDevice(s->device));
  if (s->stats_pending) {
    {
      const int wrc = wait_segment_idle(s);  // batches may run on a caller's stream
      if (wrc != TQ_OK) return wrc;
    }
    unsigned long long m = 0;
    if (s->stats_sorted) {  // a sorted batch: matches, matches with a value, row entries written (an aggregation: none)
      unsigned long long t[3] = {0, 0, 0};
      HIP_TRY(hipMemcpy(t, s->d_match_counter, sizeof t, hipMemcpyDeviceToHost));
      m = t[0];
      s->stats.matches = m;
      // a value per valued match, a presence word per match of an Optional column, 13 per entry (doc, value, flag)
      s->stats.algorithmic_bytes += 8u * t[1] + (s->stats_sorted_optional ? 8u * t[0] : 0u) + 13u * t[2];
      if (s->stats_agg_metric) {
        unsigned long long b[2] = {0, 0};
        HIP_TRY(hipMemcpy(b, s->d_match_counter + 3, sizeof b, hipMemcpyDeviceToHost));
        s->stats.algorithmic_bytes += 8u * b[0] + (s->stats_agg_metric_optional ? 8u * b[1] : 0u);
      }
      if (s->stats_agg_terms) {  // 12 per entry returned (key, doc count)
        unsigned long long e = 0;
        HIP_TRY(hipMemcpy(&e, s->d_match_counter + 3, sizeof e, hipMemcpyDeviceToHost));
        s->stats.algorithmic_bytes += 12u * e;
        if (s->stats_agg_terms_sub) {  // 40 more per entry returned (its record); the metric column's reads
          unsigned long long b[2] = {0, 0};
          HIP_TRY(hipMemcpy(b, s->d_match_counter + 4, sizeof b, hipMemcpyDeviceToHost));
          s->stats.algorithmic_bytes += 40u * e + 8u * b[0] + (s->stats_agg_metric_optional ? 8u * b[1] : 0u);
        }
        if (s->stats_agg_terms_hist_row) {  // 4 x n_buckets more per entry returned (its row); the histogram column's reads
          unsigned long long b[2] = {0, 0};
          HIP_TRY(hipMemcpy(b, s->d_match_counter + 4, sizeof b, hipMemcpyDeviceToHost));
          s->stats.algorithmic_bytes += 4u * (uint64_t)(s->stats_agg_terms_hist_row - 1u) * e + 8u * b[0] + (s->stats_agg_metric_optional ? 8u * b[1] : 0u);
        }
      }
      s->stats_sorted = false;
    } else {
      HIP_TRY(hipMemcpy(&m, s->d_match_counter, sizeof m, hipMemcpyDeviceToHost));
      s->stats.matches = m;
      s->stats.algorithmic_bytes += m * s->stats_match_bytes;  // 1 fieldnorm byte per scored doc; 4 per doc of a doc set
    }
    if (s->opt.timing) {
      uint64_t first = s->batches_reported;
      if (s->batches_timed - first > (uint64_t)tq_segment::kTimingRing)
        first = s->batches_timed - tq_segment::kTimingRing;
      double k_sum = 0, t_sum = 0;
      uint32_t n = 0;
      for (uint64_t b = first; b < s->batches_timed; ++b) {
        const int i = (int)(b % tq_segment::kTimingRing);
        float km = 0, tm = 0;
        if (hipEventElapsedTime(&km, s->ev_k0[i], s->ev_k1[i]) == hipSuccess &&
            hipEventElapsedTime(&tm, s->ev_t0[i], s->ev_t1[i]) == hipSuccess) {
          k_sum += km;
          t_sum += tm;
          ++n;
        }
      }
      s->batches_reported = s->batches_timed;
      if (n) {
        s->stats.kernel_ms = (float)(k_sum / n);
        s->stats.total_ms = (float)(t_sum / n);
      }
      s->stats.batches_averaged = n;
    }
    s->stats.host_plan_ms = s->host_ms_n ? (float)(s->host_ms_sum / s->host_ms_n) : 0.0f;
    s->host_ms_sum = 0;
    s->host_ms_n = 0;
    s->stats_pending = false;
  }
  *out = s->stats;
  return TQ_OK;
}

int tq_segment_reserve_columns(tq_segment *s, const uint64_t *postings_offs, uint32_t n) {
  if (!s || (!postings_offs && n)) return fail(TQ_ERR_INVALID, "tq_segment_reserve_columns: null argument");
  TQ_SEGMENT_LOCK(s);
  if (!s->terms.empty())
    return fail(TQ_ERR_INVALID, "tq_segment_reserve_columns: call it before the first tq_term_prepare");
  s->reserved_cols.clear();
  for (uint32_t i = 0; i < n && i < TQD_MAT_SLOTS; ++i) s->reserved_cols[postings_offs[i]] = true;
  s->cols_reserved = true;
  return TQ_OK;
}

int tq_segment_get_stats(tq_segment *s, tq_segment_stats *out) {
  if (!s || !out) return fail(TQ_ERR_INVALID, "tq_segment_get_stats: null argument");
  TQ_SEGMENT_LOCK(s);
  tq_segment_stats r{};
  r.index_bytes = s->idx_len;
  r.positions_bytes = s->pos_len;
  r.fieldnorm_bytes = s->d_fn ? s->max_doc : 0;
  r.alive_bytes = s->bytes_alive;
  r.term_table_bytes = s->bytes_term_tables + s->d_terms_cap * sizeof(TqdTerm);
  r.bitmap_bytes = s->bytes_bitmaps;
  r.docmat_bytes = s->bytes_docmat;
  r.posdir_bytes = s->bytes_posdir;
  r.scratch_bytes = s->d_stage.cap + s->d_stage_alt.cap + s->d_misc.cap + s->d_thr.cap + s->d_qmatches.cap + s->d_share_words.cap +
                    s->d_ashare_words.cap + s->d_bshare_words.cap + s->d_count_queries.cap + s->d_count_out.cap +
                    s->d_count_bits.cap + s->d_count_wgs.cap + s->d_set_work.cap + s->docset_scratch_bytes();
  {
    std::lock_guard<std::mutex> lk(s->dscratch->m);
    r.device_scratch_bytes = s->dscratch->partials.cap + s->dscratch->share_stage.cap + s->dscratch->ashare_stage.cap +
                             s->dscratch->bshare_stage.cap;
  }
  r.n_terms = (uint32_t)s->terms.size();
  r.n_dense_lists = s->n_dense_lists;
  r.n_docmat_columns = s->n_mat_slots;
  r.probe_evictions = (uint32_t)std::min<uint64_t>(s->probe_evictions, 0xFFFFFFFFull);
  r.dense_budget_bytes = s->dense_budget();
  r.lead_mat_bytes = s->lmat_bytes_total;
  r.lead_mat_stale = s->lmat_stale_skips;
  *out = r;
  return TQ_OK;
}

int tq_set_option(tq_segment *s, const char *name, int64_t value) {
  if (!s || !name) return fail(TQ_ERR_INVALID, "tq_set_option: null argument");
  TQ_SEGMENT_LOCK(s);
  if (!strcmp(name, "exhaustive"))  // (the two words tq_submit reads without the segment lock: atomic stores)
    __atomic_store_n(&s->opt.exhaustive, value != 0 ? 1 : 0, __ATOMIC_RELAXED);
  else if (!strcmp(name, "timing"))
    s->opt.timing = value != 0;
  else if (!strcmp(name, "use_dpp"))
    s->opt.use_dpp = value != 0;
  else if (!strcmp(name, "use_dense"))
    s->opt.use_dense = value != 0;
  else if (!strcmp(name, "or_windows"))
    s->opt.or_windows = value < 0 ? -1 : (value != 0);
  else if (!strcmp(name, "dense_ratio") && value >= 1)  // affects terms prepared afterwards
    s->opt.dense_ratio = (int)value;
  else if (!strcmp(name, "rdir_budget_x") && value >= 0 && value <= 0x7FFFFFFF)
    s->opt.rdir_budget_x = (int)value;
  else if (!strcmp(name, "lead_mat_budget_x") && value >= 0 && value <= 0x7FFFFFFF)  // (0: the tables that exist are not used)
    s->opt.lead_mat_budget_x = (int)value;
  else if (!strcmp(name, "lead_mat_cut") && value >= 1 && value <= 0x7FFFFFFF)  // affects tables built afterwards
    s->opt.lead_mat_cut = (int)value;
  else if (!strcmp(name, "probe_budget_x") && value >= 0 && value <= 0x7FFFFFFF)
    s->opt.probe_budget_x = (int)value, s->probe_full = false;
  else if (!strcmp(name, "dense_budget_x") && value >= 0)
    s->opt.dense_budget_x = (int)value;
  else if (!strcmp(name, "bound_slack_ppm") && value >= 0 && value <= 1000000000)
    __atomic_store_n(&s->opt.bound_slack_ppm, (int)value, __ATOMIC_RELAXED);
  else if (!strcmp(name, "dense"))  // affects terms prepared afterwards
    s->opt.dense = value != 0;
  else if (!strcmp(name, "docmat"))  // affects terms prepared afterwards
    s->opt.docmat = value != 0;
  else if (!strcmp(name, "docsig"))  // affects terms prepared afterwards
    s->opt.docsig = value != 0;
  else if (!strcmp(name, "device_prepare"))  // affects terms prepared afterwards
    s->opt.device_prepare = value != 0;
  else if (!strcmp(name, "xunion_ratio") && value >= 0 && value <= 0x7FFFFFFF)
    s->opt.xunion_ratio = (int)value;
  else if (!strcmp(name, "count_bitmap_ratio") && value >= 0 && value <= 0x7FFFFFFF)
    s->opt.count_bitmap_ratio = (int)value;
  else if (!strcmp(name, "docset_temp_lists") && value >= 0 && value <= 0x7FFFFFFF)
    s->opt.docset_temp_lists = (int)value;
  else if (!strcmp(name, "docset_trees") && (value == 0 || value == 1))
    s->opt.docset_trees = (int)value;
  else if (!strcmp(name, "docset_score_trees") && (value == 0 || value == 1))
    s->opt.docset_score_trees = (int)value;
  else if (!strcmp(name, "sort_slices") && value >= 0 && value <= 256)
    s->opt.sort_slices = (int)value;
  else if (!strcmp(name, "agg_slices") && value >= 0 && value <= 256)
    s->opt.agg_slices = (int)value;
  else if (!strcmp(name, "agg_lds_buckets") && value >= 0 && value <= (int64_t)tqk_agg_lds_buckets())
    s->opt.agg_lds_buckets = (int)value;
  else if (!strcmp(name, "ashare_inline_warm") && value >= 0 && value <= 2)
    s->opt.ashare_inline_warm = (int)value;
  else if (!strcmp(name, "ashare_min_batch") && value >= 0 && value <= 0x7FFFFFFF)
    s->opt.ashare_min_batch = (int)value;
  else if (!strcmp(name, "xunion_min_queries") && value >= 1 && value <= 0x7FFFFFFF)
    s->opt.xunion_min_queries = (int)value;
  else if (!strcmp(name, "record_query_kernels"))
    s->opt.record_query_kernels = value != 0;
  else if (!strcmp(name, "debug") && value >= -1 && value <= 0x7FFFFFFF)  // (diagnosis: the kernels' TQ_DEBUG word)
    s->opt.debug = (int)value;
  else if (!strcmp(name, "submit_window_us") && value >= 0 && value <= 1000000)
    s->opt.submit_window_us = (int)value;
  else
    return fail(TQ_ERR_INVALID, "unknown option '%s'", name);
  return TQ_OK;
}

int tq_decode_postings(tq_segment *s, tq_term_handle term, uint32_t *docs, uint32_t *tfs) {
  if (!s || !docs || !tfs) return fail(TQ_ERR_INVALID, "tq_decode_postings: null argument");
  TQ_SEGMENT_LOCK(s);
  if (term >= s->terms.size()) return fail(TQ_ERR_INVALID, "unknown term handle %u", term);
  if (s->terms[term].set_kind != TermHost::kNoSet) return fail(TQ_ERR_INVALID, "tq_decode_postings: handle %u is a term set: it has no postings", term);
  HIP_TRY(hipSetDevice(s->device));
  int rc = sync_terms(s, s->stream);
  if (rc != TQ_OK) return rc;
  const TermHost &t = s->terms[term];
  const size_t bytes = (size_t)t.doc_freq * sizeof(uint32_t);
  rc = s->d_misc.ensure(2 * bytes + 64);
  if (rc != TQ_OK) return rc;
  uint32_t *dd = (uint32_t *)s->d_misc.p, *dt = dd + t.doc_freq;
  hipError_t e = tqk_launch_decode_list(s->dseg, s->d_terms, term, t.n_blocks, dd, dt,
                                        s->opt.use_dpp != 0, s->stream);
  if (e != hipSuccess) return fail(TQ_ERR_HIP, "decode launch: %s", hipGetErrorString(e));
  HIP_TRY(hipMemcpyAsync(docs, dd, bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(tfs, dt, bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return TQ_OK;
}

int tq_decode_position_deltas(tq_segment *s, tq_term_handle term, uint32_t *out, uint64_t cap,
                              uint64_t *n_out) {
  if (!s || !n_out) return fail(TQ_ERR_INVALID, "tq_decode_position_deltas: null argument");
  TQ_SEGMENT_LOCK(s);
  if (term >= s->terms.size()) return fail(TQ_ERR_INVALID, "unknown term handle %u", term);
  const TermHost &t = s->terms[term];
  if (t.set_kind != TermHost::kNoSet) return fail(TQ_ERR_INVALID, "tq_decode_position_deltas: handle %u is a term set: it has no positions", term);
  if (t.positions_len == 0) return fail(TQ_ERR_UNSUPPORTED, "term has no positions on the device");
  *n_out = t.n_positions;
  const uint64_t n = std::min<uint64_t>(cap, t.n_positions);
  if (n == 0 || !out) return TQ_OK;
  HIP_TRY(hipSetDevice(s->device));
  int rc = sync_terms(s, s->stream);
  if (rc != TQ_OK) return rc;
  rc = s->d_misc.ensure(n * sizeof(uint32_t));
  if (rc != TQ_OK) return rc;
  hipError_t e = tqk_launch_decode_positions(s->dseg, s->d_terms, term, (uint32_t *)s->d_misc.p, n,
                                             s->stream);
  if (e != hipSuccess) return fail(TQ_ERR_HIP, "decode launch: %s", hipGetErrorString(e));
  HIP_TRY(hipMemcpyAsync(out, s->d_misc.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return TQ_OK;
}

// ---- derived tables, read back (diagnostic: tests/test_gpu_prepare_tables.py).  Where a table lives and how long it
// is, from the host's records alone; the copies below are the only device work.
namespace {
struct TableSpan {
  const void *p = nullptr;
  size_t bytes = 0;
  bool host = false;  // (a value the host keeps: min_fieldnorm_id)
};
bool table_span(tq_segment *s, uint32_t term, uint32_t which, TableSpan &sp) {
  if (which >= TQ_TABLE_DOCMAT) {
    const size_t per_doc = (size_t)s->max_doc * sizeof(uint64_t);
    switch (which) {
      case TQ_TABLE_DOCMAT: sp = {s->d_docmat, s->d_docmat ? per_doc : 0, false}; return true;
      case TQ_TABLE_DOCCLS: sp = {s->d_doccls, s->d_doccls ? per_doc : 0, false}; return true;
      case TQ_TABLE_LOCAL_CACHE: sp = {s->d_local_cache, s->d_local_cache ? 256 * sizeof(float) : 0, false}; return true;
      case TQ_TABLE_MIN_FIELDNORM_ID: sp = {&s->dseg.min_fieldnorm_id, sizeof(uint32_t), true}; return true;
      default: return false;
    }
  }
  const TermHost &t = s->terms[term];
  const TqdTerm &d = s->h_dterms[term];
  const size_t n_words = bitmap_words(s);
  const size_t n_dir = ((size_t)t.doc_freq + 3) / 4 + 1;
  const bool list = t.set_kind == TermHost::kNoSet;  // (a term set has a bitmap and nothing else)
  uint32_t n_buckets = 0;
  if (list && t.n_blocks) (void)coarse_shift(s->max_doc, t.n_blocks, &n_buckets);
  auto span = [&](const void *p, size_t bytes) { sp = {p, p ? bytes : 0, false}; };
  switch (which) {
    case TQ_TABLE_REC: span(list ? d.rec : nullptr, 16 * ((size_t)t.n_blocks + 1)); return true;
    case TQ_TABLE_COARSE: span(list ? d.coarse : nullptr, 4 * ((size_t)n_buckets + 1)); return true;
    case TQ_TABLE_TAIL_DOCS: span(list && t.n_tail ? d.tail_docs : nullptr, 4 * (size_t)t.n_tail); return true;
    case TQ_TABLE_TAIL_TFS: span(list && t.n_tail ? d.tail_tfs : nullptr, 4 * (size_t)t.n_tail); return true;
    case TQ_TABLE_POS_BLK: span(list && d.n_pos_blocks ? d.pos_blk : nullptr, 8 * (size_t)d.n_pos_blocks); return true;
    case TQ_TABLE_POS_TAIL: span(list && d.n_pos_tail ? d.pos_tail : nullptr, 4 * (size_t)d.n_pos_tail); return true;
    case TQ_TABLE_DENSE: span(t.dense_blob, n_words * sizeof(uint2)); return true;
    case TQ_TABLE_BITS: span(list ? d.bits : nullptr, ((n_words + 255) & ~(size_t)255) * sizeof(uint32_t)); return true;
    case TQ_TABLE_POS_DIR: span(list ? t.posdir_blob : nullptr, n_dir * sizeof(uint32_t)); return true;
    case TQ_TABLE_TF8: span(list ? t.tf8_blob : nullptr, t.doc_freq); return true;
    case TQ_TABLE_RMAX: span(list ? t.rmax_blob : nullptr, tqd_rm_level_off(s->max_doc, TQD_RM_LEVELS)); return true;
    case TQ_TABLE_RDIR: span(list ? t.rdir_blob : nullptr, t.rdir_shift ? rdir_bytes(s, t.doc_freq, t.rdir_shift) : 0); return true;
    case TQ_TABLE_LNORM: span(list ? t.lnorm_blob : nullptr, (size_t)t.n_blocks * 128u); return true;
    case TQ_TABLE_LMAT: span(list && lmat_valid(s, t) ? t.lmat_blob : nullptr, (size_t)t.n_blocks * 1024u); return true;
    case TQ_TABLE_FLAT:
      span(list ? t.flat_blob : nullptr, (((size_t)t.doc_freq * sizeof(uint32_t) + 15) & ~(size_t)15) + t.doc_freq);
      return true;
    case TQ_TABLE_PROBE_DENSE: span(t.probe_dense_blob, n_words * sizeof(uint2)); return true;
    case TQ_TABLE_PROBE_TF8: span(t.probe_tf8_blob, t.doc_freq); return true;
    case TQ_TABLE_PROBE_POS_DIR: span(t.probe_posdir_blob, n_dir * sizeof(uint32_t)); return true;
    default: return false;
  }
}
int table_handle_ok(tq_segment *s, tq_term_handle term, const char *who) {
  if (term >= s->terms.size()) return fail(TQ_ERR_INVALID, "%s: unknown term handle %u", who, term);
  if (s->terms[term].set_kind == TermHost::kSetReleased) return fail(TQ_ERR_INVALID, "%s: handle %u is a released term set", who, term);
  return TQ_OK;
}
// every producer of a table has finished: the segment's stream (the batch path's copy stream is ordered before it by
// an event), the batches in flight, and the list maxima a tq_term_prepare_batch call left on their way
int table_quiesce(tq_segment *s) {
  HIP_TRY(hipSetDevice(s->device));
  const int rc = wait_segment_idle(s);
  if (rc != TQ_OK) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  prep_apply_lmax(s, true);
  return TQ_OK;
}
}  // namespace

int tq_term_table_read(tq_segment *s, tq_term_handle term, uint32_t which, void *out, uint64_t cap_bytes, uint64_t *n_bytes) {
  if (!s || !n_bytes) return fail(TQ_ERR_INVALID, "tq_term_table_read: null argument");
  *n_bytes = 0;
  TQ_SEGMENT_LOCK(s);
  if (which < TQ_TABLE_DOCMAT) {
    const int hrc = table_handle_ok(s, term, "tq_term_table_read");
    if (hrc != TQ_OK) return hrc;
  }
  int rc = table_quiesce(s);
  if (rc != TQ_OK) return rc;
  TableSpan sp;
  if (!table_span(s, term, which, sp)) return fail(TQ_ERR_INVALID, "tq_term_table_read: unknown table %u", which);
  *n_bytes = sp.bytes;
  if (!sp.bytes || !out || !cap_bytes) return TQ_OK;
  if (cap_bytes < sp.bytes)
    return fail(TQ_ERR_INVALID, "tq_term_table_read: table %u holds %zu bytes, room for %llu", which, sp.bytes, (unsigned long long)cap_bytes);
  if (sp.host) {
    memcpy(out, sp.p, sp.bytes);
    return TQ_OK;
  }
  HIP_TRY(hipMemcpyAsync(out, sp.p, sp.bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return TQ_OK;
}

int tq_term_table_info(tq_segment *s, tq_term_handle term, tq_term_table_info_t *info) {
  if (!s || !info) return fail(TQ_ERR_INVALID, "tq_term_table_info: null argument");
  TQ_SEGMENT_LOCK(s);
  int rc = table_handle_ok(s, term, "tq_term_table_info");
  if (rc != TQ_OK) return rc;
  rc = table_quiesce(s);
  if (rc != TQ_OK) return rc;
  const TermHost &t = s->terms[term];
  const TqdTerm &d = s->h_dterms[term];
  *info = tq_term_table_info_t{};
  info->n_blocks = t.n_blocks;
  info->n_full = t.n_full;
  info->n_tail = t.n_tail;
  info->coarse_shift = d.coarse_shift;
  info->payload_base = d.payload_base;
  info->has_freq = d.has_freq;
  info->rdir_shift = t.rdir_blob ? t.rdir_shift : 0u;
  info->rmax_list = t.rmax_list;
  info->n_pos_blocks = d.n_pos_blocks;
  info->n_pos_tail = d.n_pos_tail;
  info->field = t.field;
  info->n_positions = t.n_positions;
  info->doc_freq = t.doc_freq;
  info->probe_slot = t.probe_slot < 0 ? 0xFFFFFFFFu : (uint32_t)t.probe_slot;
  return TQ_OK;
}

}  // extern "C"

extern "C" {
// ---- cross-segment merge (merge_top_k)
int tq_merge_topk(const float *scores, const uint32_t *docs, const uint32_t *counts,
                  uint32_t n_segments, uint32_t n_queries, uint32_t stride, uint32_t offset,
                  uint32_t limit, float *out_scores, uint32_t *out_segment_ords,
                  uint32_t *out_docs, uint32_t *out_counts) {
  if (!scores || !docs || !counts || !out_scores || !out_segment_ords || !out_docs || !out_counts)
    return fail(TQ_ERR_INVALID, "tq_merge_topk: null argument");
  struct H {
    float s;
    uint32_t o, d;
  };
  std::vector<H> all;
  for (uint32_t q = 0; q < n_queries; ++q) {
    all.clear();
    for (uint32_t sg = 0; sg < n_segments; ++sg) {
      const uint32_t c = std::min(counts[(size_t)sg * n_queries + q], stride);
      const size_t b = ((size_t)sg * n_queries + q) * stride;
      for (uint32_t i = 0; i < c; ++i) all.push_back({scores[b + i], sg, docs[b + i]});
    }
    // top_score_collector.rs:590-600: sort key desc, then DocAddress asc.  Scores are compared
    // through the order-preserving u32 transform the device keys use (a strict weak order even
    // for NaN inputs, which partial_cmp().unwrap_or(Equal) in the reference is not)
    auto sortable = [](float x) {
      uint32_t u;
      memcpy(&u, &x, 4);
      if ((u & 0x7FFFFFFFu) == 0u) u = 0u;  // -0.0 == +0.0
      return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
    };
    std::sort(all.begin(), all.end(), [&](const H &a, const H &b) {
      const uint32_t ka = sortable(a.s), kb = sortable(b.s);
      if (ka != kb) return ka > kb;
      if (a.o != b.o) return a.o < b.o;
      return a.d < b.d;
    });
    uint32_t w = 0;
    for (size_t i = offset; i < all.size() && w < limit; ++i, ++w) {
      out_scores[(size_t)q * limit + w] = all[i].s;
      out_segment_ords[(size_t)q * limit + w] = all[i].o;
      out_docs[(size_t)q * limit + w] = all[i].d;
    }
    out_counts[q] = w;
    for (; w < limit; ++w) {
      out_scores[(size_t)q * limit + w] = 0.0f;
      out_segment_ords[(size_t)q * limit + w] = 0xFFFFFFFFu;
      out_docs[(size_t)q * limit + w] = TQ_TERMINATED;
    }
  }
  return TQ_OK;
}

int tq_merge_topk_device(tq_ctx *ctx, int device, const float *d_scores, const uint32_t *d_docs,
                         const uint32_t *d_counts, const uint32_t *segment_ords,
                         uint32_t n_segments, uint32_t n_queries, uint32_t stride,
                         uint32_t offset, uint32_t limit, float *d_out_scores,
                         uint32_t *d_out_segment_ords, uint32_t *d_out_docs,
                         uint32_t *d_out_counts, void *hip_stream) {
  if (!ctx || !d_scores || !d_docs || !d_counts || !d_out_scores || !d_out_segment_ords ||
      !d_out_docs || !d_out_counts)
    return fail(TQ_ERR_INVALID, "tq_merge_topk_device: null argument");
  if (limit == 0) return fail(TQ_ERR_INVALID, "tq_merge_topk_device: limit 0");
  HIP_TRY(hipSetDevice(device));
  TqkSegMergeParams p{};
  p.scores = d_scores;
  p.docs = d_docs;
  p.counts = d_counts;
  p.segment_ords = segment_ords;
  p.out_scores = d_out_scores;
  p.out_segment_ords = d_out_segment_ords;
  p.out_docs = d_out_docs;
  p.out_counts = d_out_counts;
  p.n_segments = n_segments;
  p.n_queries = n_queries;
  p.stride = stride;
  p.offset = offset;
  p.limit = limit;
  hipError_t e = tqk_launch_merge_segments(p, (hipStream_t)hip_stream);
  if (e != hipSuccess) return fail(TQ_ERR_HIP, "merge launch: %s", hipGetErrorString(e));
  return TQ_OK;
}

int tq_copy_to_host_async(tq_ctx *ctx, int device, void *dst_pinned_host, const void *src_device, size_t bytes,
                          void *hip_stream) {
  if (!ctx || !dst_pinned_host || !src_device) return fail(TQ_ERR_INVALID, "tq_copy_to_host_async: null argument");
  if (!bytes) return TQ_OK;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemcpyAsync(dst_pinned_host, src_device, bytes, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  return TQ_OK;
}

}  // extern "C"
