// tq_term_probe.cpp — the probe pool: bitmap + rank directory, tf bytes, position directory and range maxima of lists
// BELOW "dense_ratio", in equal slots with least-recently-used eviction (tq_segment::ProbeSlot), built the first time a
// boolean query names the list.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

namespace tqi {

// Bitmap + rank directory and byte-wide tfs of a list BELOW "dense_ratio", for the boolean leads of the
// shared launch only (tq_ashare.hip probes every list but the leader through them): built the first time a
// boolean query names the list, inside "probe_budget_x"; no doc-matrix column, no position directory, and
// TermHost::dense_blob stays null — the other kernels and planners keep treating the list as sparse.
// *ok = the list can be probed (it has its own tables, or these).
void probe_begin_batch(tq_segment *s) {
  ++s->probe_batch;
  s->probe_waited = false;
}
void probe_touch(tq_segment *s, uint32_t handle) {
  const int32_t sl = s->terms[handle].probe_slot;
  if (sl >= 0) s->probe_slots[(size_t)sl].last_batch = s->probe_batch;
}
namespace {
// a slot for `handle`: a free one, a new one while the pool is below its budget, else the least recently used one
// (its owner loses its tables: the batches in flight are waited for first), else — every slot belongs to the batch
// being planned — one more.  *slot = -1: the list does not fit a slot (more postings than max_doc / 32: such a list
// gets tables of its own long before the budget of the dense lists is used up).
int probe_slot_acquire(tq_segment *s, uint32_t handle, bool must, int32_t *slot, bool *no_room) {
  *no_room = false;
  *slot = -1;
  TermHost &t = s->terms[handle];
  if (!s->probe_slot_bytes) {
    const size_t n_words = bitmap_words(s);
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    s->probe_bm_bytes = up(n_words * sizeof(uint2));
    // (lists below "dense_ratio" are the ones that need probe tables: max_doc / dense_ratio postings at most; a longer
    // list that did not get tables of its own takes the oversize road of build_probe_tables)
    s->probe_tf_cap = up(std::max<size_t>((size_t)s->max_doc / (size_t)std::max(1, std::min(s->opt.dense_ratio, 1 << 20)), 4096u) + PAD);
    s->probe_dir_cap = up(s->probe_tf_cap + 16 + PAD);  // ((df + 3) / 4 + 1) * 4 bytes
    s->probe_rm_bytes = up(tqd_rm_level_off(s->max_doc, TQD_RM_LEVELS));
    s->probe_slot_bytes = s->probe_bm_bytes + s->probe_tf_cap + s->probe_dir_cap + s->probe_rm_bytes;
  }
  if ((size_t)t.doc_freq + 8 > s->probe_tf_cap - PAD) return TQ_OK;
  const size_t budget_slots = std::max<size_t>(TQ_MAX_TERMS, s->probe_budget() / s->probe_slot_bytes);
  int32_t pick = -1;
  for (size_t i = 0; i < s->probe_slots.size() && pick < 0; ++i)
    if (s->probe_slots[i].owner == 0xFFFFFFFFu) pick = (int32_t)i;
  if (pick < 0 && s->probe_slots.size() >= budget_slots) {  // least recently used, not by this batch
    // (a query that can run without the tables — a shared-launch candidate — only takes a slot nobody has used for
    // kIdle batches: with a working set above the budget plain LRU rebuilt hundreds of tables per batch, 47 ms of
    // host time at 4 096 terms; a nested query MUST have its bitmaps and takes the least recently used slot)
    static const uint64_t kIdle = std::max<uint32_t>(1u, tune_u32("TQ_PROBE_IDLE_BATCHES", 64));
    uint64_t oldest = must ? s->probe_batch : (s->probe_batch > kIdle ? s->probe_batch - kIdle : 0);
    for (size_t i = 0; i < s->probe_slots.size(); ++i)
      if (s->probe_slots[i].last_batch < oldest) {
        oldest = s->probe_slots[i].last_batch;
        pick = (int32_t)i;
      }
    if (pick < 0 && !must) {
      *no_room = true;
      s->probe_no_room_batch = s->probe_batch;  // (the rest of this batch does not scan the slots again)
      return TQ_OK;
    }
    if (pick >= 0 && !must) {  // (a full pool takes few new lists per batch from callers that can do without)
      static const uint32_t kPerBatch = tune_u32("TQ_PROBE_REPLACE_PER_BATCH", 1);
      if (s->probe_replaced_batch != s->probe_batch) {
        s->probe_replaced_batch = s->probe_batch;
        s->probe_replaced_n = 0;
      }
      if (s->probe_replaced_n++ >= kPerBatch) {
        *no_room = true;
        s->probe_no_room_batch = s->probe_batch;
        return TQ_OK;
      }
    }
    if (pick >= 0) {
      // a batch in flight may still read the slot — unless nobody has used it for three batches (two are in flight at most)
      if (!s->probe_waited && s->probe_slots[(size_t)pick].last_batch + 3 > s->probe_batch) {
        const int wrc = wait_segment_idle(s);
        if (wrc != TQ_OK) return wrc;
        s->probe_waited = true;
      }
      TermHost &old = s->terms[s->probe_slots[(size_t)pick].owner];
      old.probe_dense_blob = old.probe_tf8_blob = old.probe_posdir_blob = nullptr;
      if (old.rmax_blob && !old.dense_blob) {  // (the range maxima lived in the slot)
        old.rmax_blob = nullptr;
        if (!old.rdir_blob) old.rmax_list = 255;  // (a list with a range directory keeps its maximum)
      }
      old.probe_slot = -1;
      s->probe_slots[(size_t)pick].owner = 0xFFFFFFFFu;
      ++s->probe_evictions;
      s->share_span_terms = ~(size_t)0;
    }
  }
  if (pick < 0) {  // a new slot (below the budget, or every slot is this batch's)
    void *base = nullptr;
    const int arc = dense_alloc(s, s->probe_slot_bytes, &base);
    if (arc != TQ_OK) return arc;
    tq_segment::ProbeSlot ps;
    ps.base = (uint8_t *)base;
    s->probe_slots.push_back(ps);
    s->probe_bytes_total += s->probe_slot_bytes;
    s->bytes_bitmaps += s->probe_slot_bytes;
    pick = (int32_t)s->probe_slots.size() - 1;
  }
  s->probe_slots[(size_t)pick].owner = handle;
  s->probe_slots[(size_t)pick].last_batch = s->probe_batch;
  t.probe_slot = pick;
  *slot = pick;
  return TQ_OK;
}
void probe_slot_release(tq_segment *s, uint32_t handle) {  // (a failed build)
  TermHost &t = s->terms[handle];
  if (t.probe_slot < 0) return;
  s->probe_slots[(size_t)t.probe_slot].owner = 0xFFFFFFFFu;
  t.probe_slot = -1;
}
}  // namespace

int build_probe_tables(tq_segment *s, uint32_t handle, bool *ok, bool must) {
  const bool any_size = must;
  TermHost &t = s->terms[handle];
  *ok = (t.dense_blob && t.tf8_blob) || (t.probe_dense_blob && t.probe_tf8_blob);
  if (*ok) {
    probe_touch(s, handle);
    return TQ_OK;
  }
  if (t.set_kind != TermHost::kNoSet) return TQ_OK;  // (a term set is its bitmap: there is no list to build tables from)
  if (!s->opt.dense || !s->opt.use_dense || !t.doc_freq || s->opt.probe_budget_x <= 0) return TQ_OK;
  if (!must && s->probe_no_room_batch == s->probe_batch) return TQ_OK;
  // (segments below 4096 docs: the shared launches are not used there — only nested boolean queries, which reach every
  // list through a bitmap whatever the segment's size, ask with any_size)
  if (s->max_doc < 4096u && !any_size) return TQ_OK;
  HIP_TRY(hipSetDevice(s->device));
  int32_t slot = -1;
  bool no_room = false;
  int rc = probe_slot_acquire(s, handle, must, &slot, &no_room);
  if (rc != TQ_OK || no_room) return rc;
  uint8_t *base = nullptr;
  if (slot >= 0) {
    base = s->probe_slots[(size_t)slot].base;
  } else {
    // a list of more postings than a slot holds ("dense_ratio" below 32 leaves such lists without tables of their
    // own): tables of its own size, kept for good — there are at most 32 of them
    const size_t tf_room = (((size_t)t.doc_freq + 8 + PAD) + 255) & ~(size_t)255;
    void *own = nullptr;
    rc = dense_alloc(s, s->probe_bm_bytes + 2 * tf_room + 256 + s->probe_rm_bytes, &own);
    if (rc != TQ_OK) return rc;
    base = (uint8_t *)own;
    s->probe_bytes_total += s->probe_bm_bytes + 2 * tf_room + 256 + s->probe_rm_bytes;
    s->bytes_bitmaps += s->probe_bm_bytes + 2 * tf_room + 256 + s->probe_rm_bytes;
  }
  // (layout of a slot: bitmap | tf bytes | position directory | range maxima; an oversize list: the same, its own sizes)
  const size_t tf_cap = slot >= 0 ? s->probe_tf_cap : ((((size_t)t.doc_freq + 8 + PAD) + 255) & ~(size_t)255);
  const size_t dir_cap = slot >= 0 ? s->probe_dir_cap : tf_cap + 256;
  DecodedList dl;
  rc = decode_list(s, t, tqp_scan_scratch_words((uint32_t)bitmap_words(s)), true, dl);
  if (rc != TQ_OK) {
    probe_slot_release(s, handle);
    return rc;
  }
  void *blob = base, *tfb = base + s->probe_bm_bytes;
  hipError_t e = tqk_launch_tf8_pack(dl.dt, t.doc_freq, (uint8_t *)tfb, s->stream);
  if (e == hipSuccess) e = enqueue_bitmap(s, dl, t.doc_freq, blob);
  // range maxima of the list (tq_ashare.hip's bound on a probed list), into the slot
  uint8_t *rmb = base + s->probe_bm_bytes + tf_cap + dir_cap;
  const bool want_rm = !t.rmax_blob && s->d_local_cache && !t.field;  // (norm-derived: field-0 lists only)
  if (e == hipSuccess && want_rm) e = enqueue_rmax(s, dl, t.doc_freq, rmb);
  uint32_t h_bad = 0, lmax = 0;
  if (e == hipSuccess) e = finish_tables(s, dl, &h_bad, want_rm ? &lmax : nullptr);
  if (e != hipSuccess || h_bad) {
    probe_slot_release(s, handle);
    return e != hipSuccess ? fail(TQ_ERR_HIP, "probe tables: %s", hipGetErrorString(e))
                           : fail(TQ_ERR_FORMAT, "posting list not strictly increasing below max_doc");
  }
  t.probe_dense_blob = blob;
  t.probe_tf8_blob = tfb;
  if (slot < 0) t.probe_own_dir = base + s->probe_bm_bytes + tf_cap;  // (where its position directory goes)
  if (want_rm) {
    t.rmax_blob = rmb;
    t.rmax_list = rmax_list_of(lmax);
  }
  *ok = true;
  return TQ_OK;
}

// The position directory of a list whose tables came from build_probe_tables: entry j = positions before posting
// 4 j, what a phrase inside a boolean query needs to find a doc's positions from the bitmap's rank (tq_tree.hip).
// Lives in the list's slot of the probe pool.
int build_probe_posdir(tq_segment *s, uint32_t handle, bool *ok) {
  TermHost &t = s->terms[handle];
  *ok = t.posdir_blob || t.probe_posdir_blob;
  if (*ok || !t.doc_freq || t.positions_len == 0) return TQ_OK;
  const bool own = t.dense_blob && t.tf8_blob;  // (a dense list whose directory did not fit when its tables were built)
  if (!own && !(t.probe_dense_blob && t.probe_tf8_blob)) return TQ_OK;
  if (!own && t.probe_slot < 0 && !t.probe_own_dir) return TQ_OK;
  const size_t n_dir = ((size_t)t.doc_freq + 3) / 4 + 1;
  const size_t need = n_dir * sizeof(uint32_t);
  if (!own && t.probe_slot >= 0 && need + PAD > s->probe_dir_cap) return TQ_OK;
  HIP_TRY(hipSetDevice(s->device));
  DecodedList dl;
  int rc = decode_list(s, t, tqp_scan_scratch_words((uint32_t)n_dir), false, dl);
  if (rc != TQ_OK) return rc;
  void *db = nullptr;
  if (own) {
    rc = dense_alloc(s, need + PAD, &db);
    if (rc != TQ_OK) return rc;
    s->bytes_posdir += need;
  } else if (t.probe_slot >= 0) {
    db = s->probe_slots[(size_t)t.probe_slot].base + s->probe_bm_bytes + s->probe_tf_cap;
  } else {
    db = t.probe_own_dir;
  }
  hipError_t e = tqp_launch_posdir(dl.dt, t.doc_freq, (uint32_t *)db, (uint32_t)n_dir, dl.scan_scratch, s->stream);
  uint32_t total = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&total, (uint32_t *)db + (n_dir - 1), 4, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess || total != (uint32_t)t.n_positions)
    return e != hipSuccess ? fail(TQ_ERR_HIP, "position directory: %s", hipGetErrorString(e))
                           : fail(TQ_ERR_FORMAT, "term freqs sum to %u positions, the stream holds %llu", total,
                                  (unsigned long long)t.n_positions);
  t.probe_posdir_blob = db;
  *ok = true;
  return TQ_OK;
}

}  // namespace tqi
