// tq_term_tables.cpp — the side tables of a prepared list, built on the device from one decode of the list: byte-wide
// tfs, range maxima, plain arrays, leader norms, the doc matrix's column or signature bit, the range directory, and
// the dense lists' bitmap + rank directory with its position directory.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

namespace tqi {

// Range directories (TermHost::rdir_blob; rdir_lookup in tq_common.hpp): carved out of 32 MB chunks of the segment's
// arena, kept until the segment is closed.  rdir_plan: the list's shift S — ranges of 2^S docs, the smallest S in 2..16 that leaves at most
// df ranges (one to two postings per range; entries keep 16 bits of the doc id) — or 0: no directory (the option is
// off, the segment or the list is tiny, or the directories have reached "rdir_budget_x").  rdir_bytes: entries (one
// u32 per posting) behind (max_doc >> S) + 2 directory slots (padded to four).
size_t rdir_dir_words(const tq_segment *s, uint32_t S) { return (((size_t)(s->max_doc >> S) + 2u) + 3u) & ~(size_t)3u; }
size_t rdir_bytes(const tq_segment *s, uint32_t doc_freq, uint32_t S) {
  return (rdir_dir_words(s, S) + (size_t)doc_freq) * sizeof(uint32_t);
}
uint32_t rdir_plan(tq_segment *s, uint32_t doc_freq) {
  static const uint32_t kRatio = tune_u32("TQ_RDIR_RATIO", 0);  // (experiments: only lists below max_doc / ratio)
  static const uint32_t kMinDf = std::max<uint32_t>(1u, tune_u32("TQ_RDIR_MIN_DF", 256));  // (below: the directory would outweigh the list)
  if (!s->opt.dense || s->opt.rdir_budget_x <= 0 || s->max_doc < 4096u || doc_freq < kMinDf) return 0u;
  if (kRatio && (uint64_t)doc_freq * kRatio >= s->max_doc) return 0u;
  static const uint32_t kPerRange = std::max<uint32_t>(1u, tune_u32("TQ_RDIR_PER_RANGE", 1));  // (postings per range, at least: 1 / 2 / 4 / 8 — and2_distinct 1.32 / 1.36 / 1.42 / 1.54 ms)
  uint32_t S = 2;
  while (S < 16u && (s->max_doc >> S) + 1u > doc_freq / kPerRange) ++S;
  if (s->rdir_bytes_total + rdir_bytes(s, doc_freq, S) > s->rdir_budget()) return 0u;
  return S;
}
int attach_rdir(tq_segment *s, uint32_t handle, uint32_t S, void **tab) {
  TermHost &t = s->terms[handle];
  const int rc = rdir_alloc(s, rdir_bytes(s, t.doc_freq, S), tab);
  if (rc != TQ_OK) return rc;
  t.rdir_blob = *tab;
  t.rdir_ent = (uint32_t *)*tab + rdir_dir_words(s, S);
  t.rdir_shift = S;
  return TQ_OK;
}
// rmax_list (the list's largest tf/(tf + norm), what the shared intersection launch bounds a probed list with) of the
// lists whose directories an earlier tq_term_prepare_batch call built, once that call's launch has finished
void prep_apply_lmax(tq_segment *s, bool wait) {
  for (int bx = 0; bx < 2; ++bx) {
    std::vector<uint32_t> &hs = s->prep_lmax_handles[bx];
    if (hs.empty() || !s->ev_prep[bx]) continue;
    if (wait) {
      if (hipEventSynchronize(s->ev_prep[bx]) != hipSuccess) continue;
    } else if (hipEventQuery(s->ev_prep[bx]) != hipSuccess) {
      (void)hipGetLastError();
      continue;
    }
    for (size_t i = 0; i < hs.size(); ++i) {
      TermHost &t = s->terms[hs[i]];
      const uint32_t lmax = s->prep_lmax_host[bx][i];
      if (t.field) continue;  // (a non-primary list: the maximum was taken under field 0's norms)
      if (t.rdir_blob && !t.rmax_blob && lmax) t.rmax_list = std::min<uint32_t>(lmax, 255u);
    }
    hs.clear();
  }
}

// One decode of the list into d_misc: doc ids | term freqs | 16 words | scan_words of scan scratch (tile sums) | the
// range maxima's accumulators (want_rm: one u32 per TQD_RM_SHIFT docs + the list's maximum, else 8 spare words).
int decode_list(tq_segment *s, const TermHost &t, size_t scan_words, bool want_rm, DecodedList &dl) {
  const size_t rm_words = want_rm ? ((size_t)s->max_doc >> TQD_RM_SHIFT) + 8 : 8;
  const int rc = s->d_misc.ensure(2 * (size_t)t.doc_freq * sizeof(uint32_t) +
                                  std::max<size_t>(128, 64 + (scan_words + rm_words) * sizeof(uint32_t)));
  if (rc != TQ_OK) return rc;
  dl.dd = (uint32_t *)s->d_misc.p;
  dl.dt = dl.dd + t.doc_freq;
  dl.scan_scratch = dl.dt + t.doc_freq + 16;
  dl.rm_acc = want_rm ? dl.scan_scratch + scan_words : nullptr;
  const hipError_t e = tqk_launch_decode_list(s->dseg, t.d_self, 0u, t.n_blocks, dl.dd, dl.dt, s->opt.use_dpp != 0, s->stream);
  if (e != hipSuccess) return fail(TQ_ERR_HIP, "decode launch: %s", hipGetErrorString(e));
  return TQ_OK;
}

// What a list's own tables (build_dense_device) and a probe slot's (build_probe_tables) are built by alike.
hipError_t enqueue_bitmap(tq_segment *s, const DecodedList &dl, uint32_t doc_freq, void *blob) {
  const size_t n_words = bitmap_words(s);
  uint32_t *bad = (uint32_t *)s->d_tp_info;
  hipError_t e = hipMemsetAsync(blob, 0, n_words * sizeof(uint2), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0, 4, s->stream);
  if (e == hipSuccess)
    e = tqp_launch_dense(dl.dd, doc_freq, s->max_doc, (uint2 *)blob, (uint32_t)n_words, bad, dl.scan_scratch, s->stream);
  return e;
}
hipError_t enqueue_rmax(tq_segment *s, const DecodedList &dl, uint32_t doc_freq, uint8_t *out) {
  const uint32_t n_ranges = (s->max_doc >> TQD_RM_SHIFT) + 1u;
  hipError_t e = hipMemsetAsync(dl.rm_acc, 0, ((size_t)n_ranges + 1u) * sizeof(uint32_t), s->stream);
  if (e == hipSuccess)
    e = tqp_launch_rmax(dl.dd, dl.dt, doc_freq, s->d_fn, s->dseg.const_fieldnorm_id, s->d_local_cache, dl.rm_acc, s->max_doc,
                        out, dl.rm_acc + n_ranges, s->stream);
  return e;
}
hipError_t finish_tables(tq_segment *s, const DecodedList &dl, uint32_t *bad, uint32_t *lmax) {
  hipError_t e = hipSuccess;
  if (bad) e = hipMemcpyAsync(bad, s->d_tp_info, 4, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess && lmax)
    e = hipMemcpyAsync(lmax, dl.rm_acc + (s->max_doc >> TQD_RM_SHIFT) + 1u, 4, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  return e;
}

// Dense lists also get their term freqs as one byte per posting (255 = "255 or more: read the
// packed value"): with the posting index from the bitmap's rank the tf of a candidate is ONE load,
// where block record -> packed tf bits are two dependent ones (the shared-union kernel's scoring
// stage is a chain of dependent gathers, 1.6 us each under load).  d_tfs = the decoded tfs.
static int build_tf8(tq_segment *s, uint32_t handle, const uint32_t *d_tfs) {
  TermHost &t = s->terms[handle];
  const size_t bytes = ((size_t)t.doc_freq + 7) & ~(size_t)7;
  if (s->dense_bytes_total + bytes > s->dense_budget()) return TQ_OK;
  void *blob = nullptr;
  {
    const int arc = dense_alloc(s, bytes + PAD, &blob);
    if (arc != TQ_OK) return arc;
  }
  hipError_t e = tqk_launch_tf8_pack(d_tfs, t.doc_freq, (uint8_t *)blob, s->stream);
  if (e != hipSuccess) {
    dense_release(s, blob);
    return fail(TQ_ERR_HIP, "tf8 pack: %s", hipGetErrorString(e));
  }
  t.tf8_blob = blob;
  s->h_dterms[handle].tf8 = (const uint8_t *)blob;
  s->dense_bytes_total += bytes;
  s->bytes_bitmaps += bytes;
  mark_term_dirty(s, handle);
  return TQ_OK;
}

// Range maxima of a list that gets a bitmap (its own or the probe tables'): tq_ashare.hip bounds the non-leader
// lists of an intersection per TQD_RM_SHIFT-doc range instead of by their weight (block_wand_intersection.rs:59-85
// uses the block-max of the secondaries' current blocks).  dd / dt = the decoded list; acc = n_ranges + 1 u32 of
// scratch.  13 KB per list of a 10M-doc segment (five levels, one byte per 1024 docs at the finest).
static int build_rmax(tq_segment *s, uint32_t handle, const DecodedList &dl) {
  TermHost &t = s->terms[handle];
  if (t.rmax_blob || !s->d_local_cache || !t.doc_freq || t.field) return TQ_OK;  // (norm-derived: field-0 lists only)
  const uint32_t n_out = tqd_rm_level_off(s->max_doc, TQD_RM_LEVELS);  // every level (tq_device.h)
  void *blob = nullptr;
  const int arc = dense_alloc(s, n_out, &blob);
  if (arc != TQ_OK) return arc;
  uint32_t lmax = 0;
  hipError_t e = enqueue_rmax(s, dl, t.doc_freq, (uint8_t *)blob);
  if (e == hipSuccess) e = finish_tables(s, dl, nullptr, &lmax);
  if (e != hipSuccess) {
    dense_release(s, blob);
    return fail(TQ_ERR_HIP, "range maxima: %s", hipGetErrorString(e));
  }
  t.rmax_blob = blob;
  t.rmax_list = rmax_list_of(lmax);
  s->bytes_bitmaps += n_out;
  return TQ_OK;
}

// A list WITHOUT a bitmap as plain arrays — doc ids, then min(tf, 255) per posting — for the
// doc-major union launch (tq_xunion.hip), which scatters such a list into its tile row with a
// cursor instead of decoding blocks.  Built on the batch's stream the first time an unpruned
// union needs the list; counts against the side tables' budget (false = over it: *ok stays false).
int build_flat(tq_segment *s, uint32_t handle, hipStream_t st, bool *ok) {
  TermHost &t = s->terms[handle];
  *ok = t.flat_blob != nullptr;
  if (*ok || t.doc_freq == 0) return TQ_OK;
  const size_t doc_bytes = ((size_t)t.doc_freq * sizeof(uint32_t) + 15) & ~(size_t)15;
  const size_t bytes = doc_bytes + (((size_t)t.doc_freq + 15) & ~(size_t)15);
  if (s->dense_bytes_total + bytes > s->dense_budget()) return TQ_OK;
  void *blob = nullptr;
  {
    const int arc = dense_alloc(s, bytes + PAD, &blob);
    if (arc != TQ_OK) return arc;
  }
  const hipError_t e = tqk_launch_flat_list(s->dseg, t.d_self, 0u, t.n_blocks, (uint32_t *)blob,
                                            (uint8_t *)blob + doc_bytes, st);
  if (e != hipSuccess) {
    dense_release(s, blob);
    return fail(TQ_ERR_HIP, "flat list: %s", hipGetErrorString(e));
  }
  t.flat_blob = blob;
  s->dense_bytes_total += bytes;
  s->bytes_bitmaps += bytes;
  *ok = true;
  return TQ_OK;
}

// A leader's fieldnorm ids in posting order (TermHost::lnorm_blob) — 128 bytes per block, the tail block included, so
// that lane l of block j reads its two docs' bytes at 128 j + 2 l.  Built like the plain arrays above: one launch on the
// batch's stream the first time the list leads queries of a shared-intersection launch, no host synchronisation (this
// batch's kernels follow on the same stream, later batches on other streams wait for this batch's end), counted
// against the side tables' budget.  Over the budget, or no memory: the list stays without (stage A gathers as before).
void build_lnorm(tq_segment *s, uint32_t handle, hipStream_t st) {
  TermHost &t = s->terms[handle];
  if (t.lnorm_blob || s->lnorm_off || !t.n_blocks || !t.d_self || !s->dseg.fieldnorm || t.field) return;
  const size_t bytes = (size_t)t.n_blocks * 128u;
  if (s->dense_bytes_total + bytes > s->dense_budget()) return;
  void *blob = nullptr;
  if (dense_alloc(s, bytes + PAD, &blob) != TQ_OK) {
    (void)hipGetLastError();
    return;
  }
  // (the batch has been admitted to the shared launch with the span as it is: a table outside it — an allocation of
  // its own, far from the arena — cannot be named by a 32-bit offset)
  if ((uint64_t)blob < s->share_table_lo + 8u || (uint64_t)blob + bytes - s->share_table_lo >= (8ull << 32)) {
    dense_release(s, blob);
    s->lnorm_off = true;
    return;
  }
  if (tqk_launch_lead_norms(s->dseg, t.d_self, 0u, t.n_blocks, (uint8_t *)blob, st) != hipSuccess) {
    (void)hipGetLastError();
    dense_release(s, blob);
    return;
  }
  t.lnorm_blob = blob;
  s->dense_bytes_total += bytes;
  s->bytes_bitmaps += bytes;
  s->share_span_terms = ~(size_t)0;  // (the tables' address span is taken again: tq_search.cpp)
}

// A leader's doc-matrix words in posting order (TermHost::lmat_blob) — 1 KB per block, the tail block included, so that
// lane l of block j reads its two docs' words as one 16-byte load at 1024 j + 16 l.  Planned here, filled by fill_lmat
// on the batch's stream BEHIND order_batch: a first fill needs no ordering (no earlier batch names the blob), a refill
// of a stale table rewrites it in place and must follow every batch that may read it — order_batch puts this batch's
// stream behind the segment's previous batch, which followed the one before it.  Field-0 lists only (like lnorm; it
// needs no fieldnorm file), under "lead_mat_cut", inside "lead_mat_budget_x" — a budget of its own — and inside the
// address span the launch's 32-bit offsets reach.  A stale table is refilled only when the doc matrix did not change
// since the previous batch was planned; until then the lead carries offset 0 and stage A gathers.
bool plan_lmat(tq_segment *s, uint32_t handle, bool *fill) {
  TermHost &t = s->terms[handle];
  *fill = false;
  if (lead_mat_budget_x(s) <= 0 || !s->d_docmat) return false;
  if (t.lmat_blob) {
    if (t.lmat_epoch == s->docmat_epoch) return true;
    if (s->docmat_epoch != s->docmat_epoch_planned) {  // (still moving: not this batch)
      ++s->lmat_stale_skips;
      return false;
    }
    t.lmat_epoch = s->docmat_epoch;
    *fill = true;
    return true;
  }
  if (s->lmat_off || !t.n_blocks || !t.d_self || t.field || t.set_kind != TermHost::kNoSet) return false;
  if ((uint64_t)t.doc_freq * lead_mat_cut(s) > s->max_doc) return false;  // (several of its docs share a 128-byte line of the matrix)
  const size_t bytes = (size_t)t.n_blocks * 1024u;
  if (s->lmat_bytes_total + bytes > (size_t)lead_mat_budget_x(s) * (s->idx_len + s->pos_len + s->max_doc)) return false;
  void *blob = nullptr;
  if (dense_alloc(s, bytes + PAD, &blob) != TQ_OK) {
    (void)hipGetLastError();
    return false;
  }
  if ((uint64_t)blob & 15u) {  // (the lanes' 16-byte loads; dense_alloc hands out 256-byte multiples: this list only, not the segment)
    dense_release(s, blob);
    return false;
  }
  if ((uint64_t)blob < s->share_table_lo + 8u || (uint64_t)blob + bytes - s->share_table_lo >= (8ull << 32)) {  // outside the span
    dense_release(s, blob);
    s->lmat_off = true;
    return false;
  }
  t.lmat_blob = blob;
  t.lmat_epoch = s->docmat_epoch;
  s->lmat_bytes_total += bytes;
  s->share_span_terms = ~(size_t)0;  // (the tables' address span is taken again: tq_search.cpp)
  *fill = true;
  return true;
}
hipError_t fill_lmat(tq_segment *s, uint32_t handle, hipStream_t st) {
  TermHost &t = s->terms[handle];
  const hipError_t e = tqk_launch_lead_mat(s->dseg, t.d_self, 0u, t.n_blocks, (uint64_t *)t.lmat_blob, st);
  if (e != hipSuccess) t.lmat_epoch = 0;  // (never a live epoch: the table is refilled before it is used again)
  return e;
}

// The doc matrix (TqdSegment::docmat): allocated with the first list that needs it.
int ensure_docmat(tq_segment *s) {
  if (s->d_docmat) return TQ_OK;
  const size_t mat_bytes = (size_t)s->max_doc * sizeof(uint64_t);
  if (s->dense_bytes_total + mat_bytes > s->dense_budget()) return TQ_OK;  // (stays null: over budget)
  HIP_TRY(hipMalloc((void **)&s->d_docmat, mat_bytes + PAD));
  HIP_TRY(hipMemsetAsync((uint8_t *)s->d_docmat + mat_bytes, 0, PAD, s->stream));
  docmat_written(s);
  const hipError_t e = tqk_launch_docmat_init(s->d_docmat, s->d_fn, s->dseg.const_fieldnorm_id, s->max_doc, s->stream);
  if (e != hipSuccess) return fail(TQ_ERR_HIP, "docmat init: %s", hipGetErrorString(e));
  s->dense_bytes_total += mat_bytes;
  s->bytes_docmat = mat_bytes;
  s->dseg.docmat = s->d_docmat;
  return TQ_OK;
}

// Lists WITHOUT a column in the doc matrix (the sparse, high-weight lists; dense lists beyond the
// 40 columns) share the top 16 bits of the doc-matrix words: every such list sets bit
// 48 + hash(handle) of the docs it holds.  A clear bit proves "not in the list"; a set bit means
// "maybe" (another list with the same bit, or this one).  The union kernels test it where they
// used to assume the list holds every candidate — a rare list holds a fraction of a percent of
// them, and each wrong guess cost a seek and a block search.  The same gather that brings a
// candidate's fieldnorm id and column bits brings its signature.  Only prepared (queried) lists
// set bits; built by one decode of the list.
int add_to_doc_signatures(tq_segment *s, uint32_t handle) {
  TermHost &t = s->terms[handle];
  if (t.doc_freq == 0) return TQ_OK;
  const bool has_col = ((s->h_dterms[handle].has_freq >> 8) & 0xFFu) != 0u;
  bool want_sig = s->opt.docsig && s->opt.docmat && s->opt.dense && s->max_doc >= 4096u && !has_col;
  // (a list without tables of its own also gets its range directory from the same decode)
  const uint32_t rd_shift = !(t.dense_blob && t.tf8_blob) && !t.rdir_blob ? rdir_plan(s, t.doc_freq) : 0u;
  if (want_sig) {
    const int rc = ensure_docmat(s);
    if (rc != TQ_OK) return rc;
    want_sig = s->d_docmat != nullptr;
  }
  if (!want_sig && !rd_shift) return TQ_OK;
  DecodedList dl;
  int rc = decode_list(s, t, 0, false, dl);
  if (rc != TQ_OK) return rc;
  hipError_t e = hipSuccess;
  if (want_sig) {
    const uint32_t bit = sig_bit(handle);
    docmat_written(s);
    e = tqk_launch_docmat_set(s->d_docmat, dl.dd, t.doc_freq, (TQD_SIG_SHIFT - 8u) + bit, s->max_doc, s->stream);
    if (e != hipSuccess) return fail(TQ_ERR_HIP, "docmat signature: %s", hipGetErrorString(e));
    s->h_dterms[handle].has_freq |= (bit + 1u) << 16;
    mark_term_dirty(s, handle);
  }
  if (rd_shift) {
    void *tab = nullptr;
    rc = attach_rdir(s, handle, rd_shift, &tab);
    if (rc != TQ_OK) return rc;
    e = tqk_launch_rdir_fill(dl.dd, dl.dt, t.doc_freq, s->max_doc, (uint32_t *)tab, rd_shift, s->stream);
    if (e != hipSuccess) {
      t.rdir_blob = t.rdir_ent = nullptr, t.rdir_shift = 0;  // (not filled: the list does without)
      return fail(TQ_ERR_HIP, "range directory: %s", hipGetErrorString(e));
    }
    if (s->d_local_cache && !t.field) {  // the list's largest tf/(tf + norm): td_rmax_scatter_kernel's value, one range
      uint32_t *acc = dl.dt + t.doc_freq + 8u, lmax = 0;
      e = hipMemsetAsync(acc, 0, sizeof(uint32_t), s->stream);
      if (e == hipSuccess) e = tqp_launch_list_max(dl.dd, dl.dt, t.doc_freq, s->d_fn, s->dseg.const_fieldnorm_id, s->d_local_cache, acc, s->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(&lmax, acc, 4, hipMemcpyDeviceToHost, s->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
      if (e != hipSuccess) return fail(TQ_ERR_HIP, "list maximum: %s", hipGetErrorString(e));
      if (lmax) t.rmax_list = std::min<uint32_t>(lmax, 255u);
    }
  }
  return TQ_OK;
}

// Dense lists (doc_freq >= max_doc/TQD_DENSE_RATIO) also get a membership bitmap with a rank directory,
// {32 doc bits, number of postings before them} per 32 docs: a probe of doc d costs one 8-byte load instead
// of a block decode; the posting index (=> block, slot, tf) falls out of the rank.  Derived data like the
// unrolled skip table; the index bytes stay untouched.  The list is decoded once on the device (the kernel of
// tq_decode_postings), bitmap bits set by atomic OR, rank directory and position directory by grid-wide
// scans (tq_prepare.hip); 4 bytes (the validity flag) come back.
int build_dense_device(tq_segment *s, uint32_t handle) {
  TermHost &t = s->terms[handle];
  const size_t n_words = bitmap_words(s);
  DecodedList dl;
  int rc = decode_list(s, t, tqp_scan_scratch_words((uint32_t)std::max<size_t>(n_words, (size_t)t.doc_freq / 4 + 2)), true, dl);
  if (rc != TQ_OK) return rc;
  uint32_t *const dd = dl.dd, *const dt = dl.dt;
  rc = build_tf8(s, handle, dt);
  if (rc != TQ_OK) return rc;
  if (t.tf8_blob) {  // (the shared launches probe a list through bitmap + tf bytes: only then is it bounded by ranges)
    rc = build_rmax(s, handle, dl);
    if (rc != TQ_OK) return rc;
  }
  void *blob = nullptr;
  {
    const int arc = dense_alloc(s, n_words * sizeof(uint2), &blob);
    if (arc != TQ_OK) return arc;
  }
  s->bytes_bitmaps += n_words * sizeof(uint2);
  ++s->n_dense_lists;
  uint32_t h_bad = 0;
  hipError_t e = enqueue_bitmap(s, dl, t.doc_freq, blob);
  if (e == hipSuccess) e = finish_tables(s, dl, &h_bad, nullptr);
  if (e != hipSuccess || h_bad) {
    dense_release(s, blob);
    return e != hipSuccess ? fail(TQ_ERR_HIP, "dense tables: %s", hipGetErrorString(e))
                           : fail(TQ_ERR_FORMAT, "posting list not strictly increasing below max_doc");
  }
  t.dense_blob = blob;
  s->h_dterms[handle].dense = (const uint2 *)blob;
  mark_term_dirty(s, handle);
  if (s->n_mat_slots < TQD_MAT_SLOTS && s->opt.docmat && t.wants_col) {  // the list's column of the doc matrix
    {
      const int mrc = ensure_docmat(s);
      if (mrc != TQ_OK) return mrc;
    }
    if (s->d_docmat) {
      const uint32_t slot = s->n_mat_slots++;
      docmat_written(s);
      e = tqk_launch_docmat_set(s->d_docmat, dd, t.doc_freq, slot, s->max_doc, s->stream);
      if (e != hipSuccess) return fail(TQ_ERR_HIP, "docmat set: %s", hipGetErrorString(e));
      // the list's tf classes (the first TQD_CLS_SLOTS columns; 8 B per doc once, inside the dense budget)
      static const bool kDocCls = tune_u32("TQ_DOCCLS", 1) != 0;
      if (kDocCls && slot < TQD_CLS_SLOTS && t.tf8_blob) {
        const size_t cls_bytes = (size_t)s->max_doc * sizeof(uint64_t);
        if (!s->d_doccls && s->dense_bytes_total + cls_bytes <= s->dense_budget()) {
          HIP_TRY(hipMalloc((void **)&s->d_doccls, cls_bytes + PAD));
          HIP_TRY(hipMemsetAsync(s->d_doccls, 0, cls_bytes + PAD, s->stream));
          s->dense_bytes_total += cls_bytes;
          s->bytes_docmat += cls_bytes;
          s->dseg.doccls = s->d_doccls;
        }
        if (s->d_doccls) {
          e = tqk_launch_doccls_set(s->d_doccls, dd, dt, t.doc_freq, slot, s->max_doc, s->stream);
          if (e != hipSuccess) return fail(TQ_ERR_HIP, "doccls set: %s", hipGetErrorString(e));
          s->h_dterms[handle].has_freq |= 1u << 24;  // (TqdTermHead::has_freq bit 24: the list's classes are in doccls)
        }
      }
      s->h_dterms[handle].has_freq |= (slot + 1u) << 8;
    }
  }
  if (t.positions_len > 0) {  // position directory: positions before every fourth posting
    const size_t n_dir = ((size_t)t.doc_freq + 3) / 4 + 1;
    // ... followed by the bitmap's doc bits alone (TqdTerm::bits: the phrase sweep's stream), 16-byte aligned
    const size_t dir_bytes = (n_dir * sizeof(uint32_t) + PAD + 15) & ~(size_t)15;
    const size_t n_bits = (n_words + 255) & ~(size_t)255;
    void *db = nullptr;
    {
      const int arc = dense_alloc(s, dir_bytes + n_bits * sizeof(uint32_t) + PAD, &db);
      if (arc != TQ_OK) return arc;
    }
    e = tqp_launch_posdir(dt, t.doc_freq, (uint32_t *)db, (uint32_t)n_dir, dl.scan_scratch, s->stream);
    if (e == hipSuccess)
      e = tqp_launch_bits((const uint2 *)blob, (uint32_t)n_words, (uint32_t *)((uint8_t *)db + dir_bytes), (uint32_t)n_bits, s->stream);
    uint32_t total = 0;
    if (e == hipSuccess)
      e = hipMemcpyAsync(&total, (uint32_t *)db + (n_dir - 1), 4, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess || total != (uint32_t)t.n_positions) {
      dense_release(s, db);
      return e != hipSuccess ? fail(TQ_ERR_HIP, "position directory: %s", hipGetErrorString(e))
                             : fail(TQ_ERR_FORMAT, "term freqs sum to %u positions, the stream holds %llu",
                                    total, (unsigned long long)t.n_positions);
    }
    t.posdir_blob = db;
    s->h_dterms[handle].pos_dir = (const uint32_t *)db;
    s->h_dterms[handle].bits = (const uint32_t *)((uint8_t *)db + dir_bytes);
    s->dense_bytes_total += n_dir * sizeof(uint32_t) + n_bits * sizeof(uint32_t);
    s->bytes_posdir += n_dir * sizeof(uint32_t) + n_bits * sizeof(uint32_t);
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  return TQ_OK;
}

}  // namespace tqi
