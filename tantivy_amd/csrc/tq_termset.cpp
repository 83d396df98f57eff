// tq_termset.cpp — term sets: tq_term_set_prepare / tq_term_set_info / tq_term_set_release, and the check every entry
// point makes of a query that names one.  A set is what AutomatonWeight::scorer (src/query/automaton_weight.rs:87-111)
// leaves for FuzzyTermQuery, RegexQuery and TermSetQuery: the docs of N posting lists OR-ed into a bitset under a
// ConstScorer (src/query/const_score_query.rs:95-148).  Here: a slot of the segment's term table without blocks whose
// `dense` table is that bitset with a rank directory (built by tq_termset.hip), whose doc_freq is the bitset's length
// (the reference's size_hint / cost) and whose score is the caller's weight as given.
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

namespace tqi {

namespace {
constexpr uint32_t kMaxMembers = 1u << 20;
constexpr uint32_t kConstScoreFlag = 1u << 25;  // TqdTermHead::has_freq bit 25
inline size_t set_words(const tq_segment *s) { return ((size_t)s->max_doc + 31u) / 32u; }
inline size_t set_bytes(const tq_segment *s) { return set_words(s) * sizeof(uint2); }

}  // namespace

// a released table goes back to the allocator when it had an allocation of its own; a piece of the arena waits for the next set
void set_table_release(tq_segment *s, void *tab) {
  if (!tab) return;
  const bool own = std::find(s->dense_extra.begin(), s->dense_extra.end(), tab) != s->dense_extra.end();
  dense_release(s, tab);
  if (!own) s->set_free_tables.push_back(tab);
}

int set_table_acquire(tq_segment *s, void **tab) {
  if (!s->set_free_tables.empty()) {
    *tab = s->set_free_tables.back();
    s->set_free_tables.pop_back();
    return TQ_OK;
  }
  return dense_alloc(s, (set_words(s) + 1u) * sizeof(uint2), tab);  // (+ the sentinel entry of every dense table)
}

uint32_t set_slot_commit(tq_segment *s, void *tab, uint32_t n_docs) {
  TqdTerm dt{};
  dt.dense = (const uint2 *)tab;
  dt.doc_freq = n_docs;
  dt.has_freq = kConstScoreFlag;
  TermHost th;
  th.dense_blob = tab;
  th.doc_freq = n_docs;
  th.postings_len = set_words(s) * sizeof(uint32_t);  // what a set adds to algorithmic_bytes / unique_bytes: its bits
  th.wants_col = false;
  th.set_kind = TermHost::kSet;
  uint32_t handle;
  if (!s->set_free_slots.empty()) {
    handle = s->set_free_slots.back();
    s->set_free_slots.pop_back();
    s->terms[handle] = th;
    s->h_dterms[handle] = dt;
  } else {
    handle = (uint32_t)s->terms.size();
    s->terms.push_back(th);
    s->h_dterms.push_back(dt);
    ++s->n_set_slots;
  }
  mark_term_dirty(s, handle);
  s->bytes_bitmaps += set_bytes(s);  // (not dense_bytes_total: which ordinary lists get bitmaps does not depend on sets)
  s->share_span_terms = ~(size_t)0;  // (the tables' address span is taken again: tq_search.cpp)
  return handle;
}

int check_set_query(const tq_segment *s, const tq_query &q, uint32_t qi, const char *fn, bool *has) {
  *has = false;
  if (!s->n_set_slots || !q.terms || q.n_terms > TQ_MAX_TERMS) return TQ_OK;
  for (uint32_t i = 0; i < q.n_terms; ++i) {
    const uint32_t h = q.terms[i];
    if (h >= s->terms.size() || s->terms[h].set_kind == TermHost::kNoSet) continue;
    if (s->terms[h].set_kind == TermHost::kSetReleased)
      return fail(TQ_ERR_INVALID, "%s: query %u: term handle %u is a released term set", fn, qi, h);
    if (q.mode == TQ_MODE_PHRASE || (q.nested_occurs && q.nested_occurs[i] != 255u && (q.nested_occurs[i] & TQ_NESTED_PHRASE)))
      return fail(TQ_ERR_INVALID, "%s: query %u: a term set (handle %u) has no positions: it cannot be a term of a phrase", fn, qi, h);
    *has = true;
  }
  if (*has && q.mode == TQ_MODE_BOOL && bool_query_is_tree(q))
    return fail(TQ_ERR_UNSUPPORTED, "%s: query %u: a term set inside a nested boolean query (nested_occurs / atom_of) stays on the CPU", fn, qi);
  return TQ_OK;
}

}  // namespace tqi

extern "C" {

int tq_term_set_prepare(tq_segment *s, const tq_term_handle *members, uint32_t n, tq_term_handle *out) {
  if (!s || !out || (!members && n)) return fail(TQ_ERR_INVALID, "tq_term_set_prepare: null argument");
  if (n > kMaxMembers) return fail(TQ_ERR_INVALID, "tq_term_set_prepare: %u members, at most %u", n, kMaxMembers);
  try {
    TQ_SEGMENT_LOCK(s);
    std::vector<uint32_t> hs;
    hs.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t h = members[i];
      if (h == TQ_TERM_ABSENT) continue;
      if (h == TQ_TERM_ALL) return fail(TQ_ERR_INVALID, "tq_term_set_prepare: member %u is TQ_TERM_ALL", i);
      if (h >= s->terms.size()) return fail(TQ_ERR_INVALID, "tq_term_set_prepare: member %u: term handle %u out of range", i, h);
      if (s->terms[h].set_kind != TermHost::kNoSet)
        return fail(TQ_ERR_INVALID, "tq_term_set_prepare: member %u: handle %u is %s", i, h,
                    s->terms[h].set_kind == TermHost::kSet ? "a term set" : "a released term set");
      hs.push_back(h);
    }
    std::sort(hs.begin(), hs.end());
    hs.erase(std::unique(hs.begin(), hs.end()), hs.end());
    HIP_TRY(hipSetDevice(s->device));
    // the members with a bitmap of their own are OR-ed, the others scattered block by block (four blocks per work item)
    std::vector<const uint2 *> bm;
    std::vector<uint2> items;
    for (const uint32_t h : hs) {
      const TermHost &t = s->terms[h];
      if (t.dense_blob) {
        bm.push_back((const uint2 *)t.dense_blob);
      } else {
        for (uint32_t j = 0; j < t.n_blocks; j += 4u) items.push_back(make_uint2(h, j));
      }
    }
    if (!items.empty()) {  // (the scatter reads the members' records)
      const int src = sync_terms(s, s->stream);
      if (src != TQ_OK) return src;
    }
    const size_t n_words = set_words(s);
    void *tab = nullptr;
    {
      const int arc = set_table_acquire(s, &tab);
      if (arc != TQ_OK) return arc;
    }
    const size_t bm_bytes = (bm.size() * sizeof(const uint2 *) + 255) & ~(size_t)255;
    const size_t item_bytes = (items.size() * sizeof(uint2) + 255) & ~(size_t)255;
    const size_t scratch_words = tqk_termset_scratch_words((uint32_t)n_words);
    int rc = s->d_set_work.ensure(bm_bytes + item_bytes + scratch_words * sizeof(uint32_t));
    if (rc != TQ_OK) {
      set_table_release(s, tab);
      return rc;
    }
    uint8_t *const work = (uint8_t *)s->d_set_work.p;
    uint32_t *const scratch = (uint32_t *)(work + bm_bytes + item_bytes);
    const uint32_t total_at = std::max<uint32_t>(1u, (uint32_t)((n_words + tqk_termset_scan_tile() - 1u) / tqk_termset_scan_tile()));
    uint32_t n_docs = 0;
    // everything on the segment's stream (bm / items live until the synchronise below); option "timing": two events
    // around the zeroing and the three stages, their distance left in tq_batch_stats.kernel_ms for tq_last_batch_stats
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t e = hipSuccess;
    if (s->opt.timing) {
      e = hipEventCreate(&ev0);
      if (e == hipSuccess) e = hipEventCreate(&ev1);
    }
    if (e == hipSuccess && !bm.empty())
      e = hipMemcpyAsync(work, bm.data(), bm.size() * sizeof(const uint2 *), hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess && !items.empty())
      e = hipMemcpyAsync(work + bm_bytes, items.data(), items.size() * sizeof(uint2), hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess && ev0) e = hipEventRecord(ev0, s->stream);
    if (e == hipSuccess) e = hipMemsetAsync(tab, 0, (n_words + 1u) * sizeof(uint2), s->stream);
    if (e == hipSuccess)
      e = tqk_launch_termset_build(s->dseg, s->d_terms, (const uint2 *const *)work, (uint32_t)bm.size(), (const uint2 *)(work + bm_bytes),
                                   (uint32_t)items.size(), (uint2 *)tab, (uint32_t)n_words, scratch, s->stream);
    if (e == hipSuccess && ev1) e = hipEventRecord(ev1, s->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&n_docs, scratch + total_at, sizeof n_docs, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    float build_ms = 0.0f;
    if (e == hipSuccess && ev0 && ev1) e = hipEventElapsedTime(&build_ms, ev0, ev1);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(s->stream);
      set_table_release(s, tab);
      return fail(TQ_ERR_HIP, "tq_term_set_prepare: %s", hipGetErrorString(e));
    }
    if (s->opt.timing) {  // (the last call's figures, as after a count or doc-set batch)
      s->stats = tq_batch_stats{};
      s->stats_pending = false;
      s->stats.kernel_ms = s->stats.total_ms = build_ms;
      s->stats.batches_averaged = 1;
      // the HBM model of the build: the scattered members' posting bytes + 4 B per 32 docs per bitmap member + 8 B per 32
      // docs written and read once by the scan
      uint64_t model = 2ull * n_words * sizeof(uint2) + (uint64_t)bm.size() * n_words * sizeof(uint32_t);
      for (const uint32_t h : hs)
        if (!s->terms[h].dense_blob) model += s->terms[h].postings_len;
      s->stats.algorithmic_bytes = model;
      s->stats.chunks = (uint32_t)bm.size();  // the members that were OR-ed word-wise (the others were scattered)
    }
    const uint32_t handle = set_slot_commit(s, tab, n_docs);
    *out = handle;
    return TQ_OK;
  } catch (const std::exception &e) {
    return fail(TQ_ERR_HIP, "tq_term_set_prepare: %s", e.what());
  }
}

int tq_term_set_info(tq_segment *s, tq_term_handle set, uint32_t *n_docs, uint64_t *bytes) {
  if (!s || !n_docs || !bytes) return fail(TQ_ERR_INVALID, "tq_term_set_info: null argument");
  TQ_SEGMENT_LOCK(s);
  if (!is_term_set(s, set)) return fail(TQ_ERR_INVALID, "tq_term_set_info: handle %u is not a live term set", set);
  *n_docs = s->terms[set].doc_freq;
  *bytes = set_bytes(s);
  return TQ_OK;
}

int tq_term_set_release(tq_segment *s, tq_term_handle set) {
  if (!s) return fail(TQ_ERR_INVALID, "tq_term_set_release: null segment");
  TQ_SEGMENT_LOCK(s);
  if (!is_term_set(s, set)) return fail(TQ_ERR_INVALID, "tq_term_set_release: handle %u is not a live term set", set);
  HIP_TRY(hipSetDevice(s->device));
  {
    const int wrc = wait_segment_idle(s);  // batches may run on a caller's stream
    if (wrc != TQ_OK) return wrc;
  }
  set_table_release(s, s->terms[set].dense_blob);
  s->bytes_bitmaps -= std::min(s->bytes_bitmaps, set_bytes(s));
  s->terms[set] = TermHost{};
  s->terms[set].wants_col = false;
  s->terms[set].set_kind = TermHost::kSetReleased;
  s->h_dterms[set] = TqdTerm{};
  mark_term_dirty(s, set);
  s->set_free_slots.push_back(set);
  s->share_span_terms = ~(size_t)0;
  return TQ_OK;
}

}  // extern "C"
