// tq_terms.cpp — term preparation's entry points: tq_term_prepare (one list: host walk or device walk, one blocking
// upload) and tq_term_prepare_batch (a batch's new lists together, as named stages over one PrepareBatch), the
// registration both share, and the device copy of the term table.
//   tq_term_walk.cpp    the host walker and the blob's layout     tq_term_arena.cpp  where the blobs and tables live
//   tq_term_tables.cpp  the side tables built at registration     tq_term_probe.cpp  the probe pool
// Part of the C ABI library of include/tantivy_amd.h (internal declarations: tq_internal.hpp).
#include "tq_internal.hpp"

namespace tqi {

uint32_t add_term(tq_segment *s, const TqdTerm &dt, const TermHost &th, uint64_t postings_off) {
  const uint32_t handle = (uint32_t)s->terms.size();
  s->terms.push_back(th);
  s->terms.back().wants_col = !s->cols_reserved || s->reserved_cols.count(postings_off) != 0;
  s->h_dterms.push_back(dt);
  if (s->prep_field) {  // a list of a non-primary field (tq_term_prepare_field): TqdTermHead::has_freq bits 26..28
    s->terms.back().field = s->prep_field;
    s->terms.back().wants_col = !s->cols_reserved;  // (reserved columns name field-0 lists)
    s->h_dterms.back().has_freq |= (uint32_t)s->prep_field << 26;
    ++s->n_field_terms;
  }
  mark_term_dirty(s, handle);
  s->term_by_off.emplace(postings_off, handle);
  return handle;
}

// the part of tq_term_prepare both walks share: the handle, and the dense-list structures (only while the bitmaps
// together stay within a fixed multiple of the segment's own size)
int register_term(tq_segment *s, const TqdTerm &dt, const TermHost &th, uint64_t postings_off, tq_term_handle *out) {
  const uint32_t handle = add_term(s, dt, th, postings_off);
  *out = handle;
  if (dense_candidate(s, th.doc_freq) && dense_fits(s)) {
    s->dense_bytes_total += dense_table_bytes(s);
    // (device scans whether or not a host copy of the index exists: round 4's host builder pulled the decoded
    // list back, built bitmap and rank directory in a loop and uploaded 2.5 MB per list)
    const int rc = build_dense_device(s, handle);
    if (rc != TQ_OK) return rc;
  }
  return add_to_doc_signatures(s, handle);
}

// tq_term_prepare without a host copy of the index: two small kernels walk the list's skip data
// and positions header where they lie in HBM (tq_prepare.hip); the host sizes the tables from
// TermInfo, and reads back 48 bytes of facts in between (no index bytes).
static int term_prepare_device(tq_segment *s, uint64_t postings_off, uint32_t postings_len,
                        uint64_t positions_off, uint32_t positions_len, uint32_t doc_freq,
                        tq_term_handle *out) {
  const uint32_t n_full = doc_freq / 128u, n_tail = doc_freq % 128u;
  const uint32_t n_blocks = n_full + (n_tail ? 1u : 0u);
  uint32_t n_buckets = 0;
  const uint32_t shift = coarse_shift(s->max_doc, n_blocks, &n_buckets);
  const bool maybe_pos = s->record_option == TQ_WITH_FREQS_AND_POSITIONS && s->d_pos != nullptr;
  if (maybe_pos && (positions_off > s->pos_len || (uint64_t)positions_len > s->pos_len - positions_off))
    return fail(TQ_ERR_FORMAT, "positions_range outside the pos file");
  // (no positions part: the positions tables get a blob of their own, sized after the walk)
  const TermBlobLayout lay = term_blob_layout(n_blocks, n_buckets, n_tail, 0, 0);
  const size_t total = lay.total;
  uint8_t *blob = nullptr;
  {
    const int arc = term_alloc(s, total, &blob);
    if (arc != TQ_OK) return arc;
  }
  s->bytes_term_tables += total;
  uint8_t *pblob = nullptr;
  size_t ptotal_alloc = 0;
  // a failed preparation hands its blobs back (positions blob first: the slab's last allocation), once the stream is idle
  auto bail = [&](int rc) {
    (void)hipStreamSynchronize(s->stream);
    term_release(s, pblob, ptotal_alloc);
    term_release(s, blob, total);
    return rc;
  };
  hipError_t e = hipMemsetAsync(blob, 0, total, s->stream);
  TqpPostingsParams pp{};
  pp.idx = s->d_idx;
  pp.pos = s->d_pos;
  pp.postings_off = postings_off;
  pp.positions_off = positions_off;
  pp.postings_len = postings_len;
  pp.positions_len = positions_len;
  pp.doc_freq = doc_freq;
  pp.record_option = s->record_option;
  pp.max_doc = s->max_doc;
  pp.want_pos = maybe_pos ? 1u : 0u;
  pp.rec = (uint4 *)(blob + lay.o_rec);
  pp.tail_docs = (uint32_t *)(blob + lay.o_tdocs);
  pp.tail_tfs = (uint32_t *)(blob + lay.o_ttfs);
  pp.info = s->d_tp_info;
  if (e == hipSuccess) e = tqp_launch_postings(pp, s->stream);
  TqpInfo info{};
  if (e == hipSuccess) e = hipMemcpyAsync(&info, s->d_tp_info, sizeof info, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return bail(fail(TQ_ERR_HIP, "device term prepare: %s", hipGetErrorString(e)));
  if (info.status != TQP_OK)
    return bail(fail(info.status == TQP_TOO_MANY_POSITIONS ? TQ_ERR_UNSUPPORTED : TQ_ERR_FORMAT,
                     "term at %llu: %s", (unsigned long long)postings_off, tqp_message(info.status)));
  e = tqp_launch_coarse((const uint4 *)(blob + lay.o_rec), n_blocks, shift, n_buckets,
                        (uint32_t *)(blob + lay.o_coarse), s->stream);
  if (e != hipSuccess) return bail(fail(TQ_ERR_HIP, "coarse table: %s", hipGetErrorString(e)));
  // positions tables, sized from the walk
  const bool want_pos = maybe_pos && info.record == TQ_WITH_FREQS_AND_POSITIONS;
  uint32_t n_pos_tail = 0;
  size_t o_pboff = 0, o_ptail = 0;
  if (want_pos) {
    const uint64_t tail_cap = info.n_positions - info.n_pos_blocks * 128ull;
    if (tail_cap > 127ull)
      return bail(fail(TQ_ERR_FORMAT, "positions stream and postings disagree on the number of positions"));
    size_t ptotal = 0;
    o_pboff = 0;
    ptotal = align16(8 * (size_t)info.n_pos_blocks);
    o_ptail = ptotal;
    ptotal = align16(ptotal + 4 * (size_t)tail_cap) + PAD;
    if (term_alloc(s, ptotal, &pblob) != TQ_OK) return bail(TQ_ERR_HIP);
    ptotal_alloc = ptotal;
    s->bytes_term_tables += ptotal;
    if (e == hipSuccess) e = hipMemsetAsync(pblob, 0, ptotal, s->stream);
    TqpPositionsParams qp{};
    qp.pos = s->d_pos;
    qp.positions_off = positions_off;
    qp.pos_hdr = info.pos_hdr;
    qp.n_pos_blocks = info.n_pos_blocks;
    qp.n_positions = info.n_positions;
    qp.positions_len = positions_len;
    qp.pos_tail_cap = (uint32_t)tail_cap;
    qp.pos_blk = (uint64_t *)(pblob + o_pboff);
    qp.pos_tail = (uint32_t *)(pblob + o_ptail);
    qp.result = (uint32_t *)(s->d_tp_info + 1);
    uint32_t res[2] = {0, 0};
    if (e == hipSuccess) e = tqp_launch_positions(qp, s->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(res, s->d_tp_info + 1, sizeof res, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess || res[0] != TQP_OK) {
      return bail(e != hipSuccess ? fail(TQ_ERR_HIP, "device positions prepare: %s", hipGetErrorString(e))
                                  : fail(TQ_ERR_FORMAT, "term at %llu: %s", (unsigned long long)postings_off,
                                         tqp_message(res[0])));
    }
    n_pos_tail = res[1];
  } else {
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  TqdTerm dt{};
  dt.rec = (const uint4 *)(blob + lay.o_rec);
  dt.coarse = (const uint32_t *)(blob + lay.o_coarse);
  dt.tail_docs = (const uint32_t *)(blob + lay.o_tdocs);
  dt.tail_tfs = (const uint32_t *)(blob + lay.o_ttfs);
  dt.pos_blk = (const uint64_t *)(pblob ? pblob + o_pboff : blob + lay.o_rec);
  dt.pos_tail = (const uint32_t *)(pblob ? pblob + o_ptail : blob + lay.o_rec);
  dt.payload_base = 8 + postings_off + info.payload;
  dt.n_full = n_full;
  dt.n_tail = n_tail;
  dt.n_blocks = n_blocks;
  dt.doc_freq = doc_freq;
  dt.n_pos_blocks = want_pos ? (uint32_t)info.n_pos_blocks : 0u;
  dt.n_pos_tail = n_pos_tail;
  dt.has_freq = info.record != TQ_BASIC ? 1u : 0u;
  dt.coarse_shift = shift;
  {
    const hipError_t se = hipMemcpy(blob + lay.o_self, &dt, sizeof dt, hipMemcpyHostToDevice);
    if (se != hipSuccess) return bail(fail(TQ_ERR_HIP, "term record upload: %s", hipGetErrorString(se)));
  }
  TermHost th;
  th.blob = blob;
  th.d_self = (const TqdTerm *)(blob + lay.o_self);
  th.pos_blob = pblob;
  th.doc_freq = doc_freq;
  th.n_blocks = n_blocks;
  th.n_full = n_full;
  th.n_tail = n_tail;
  th.last_doc = info.last_doc;
  th.postings_len = postings_len;
  th.positions_len = want_pos ? positions_len : 0;
  th.n_positions = want_pos ? info.n_positions : 0;
  return register_term(s, dt, th, postings_off, out);
}

void mark_term_dirty(tq_segment *s, uint32_t handle) {
  s->d_terms_dirty = true;
  s->d_terms_dirty_from = std::min<size_t>(s->d_terms_dirty_from, handle);
}

// The device copy of the term table, brought up to date (blocking form: codec access, Count, a grown table).
// tq_search_batch* takes the cheap road when it can: the records of the terms prepared since the last batch are
// appended through the batch's own staging blob (terms_pending_sync / tq_search.cpp) — no wait for the batches in
// flight, which never read beyond the entries they were planned with.
int sync_terms(tq_segment *s, hipStream_t st) {
  if (!s->d_terms_dirty) return TQ_OK;
  const size_t n = s->h_dterms.size();
  // nothing in flight may still read the table while it is rewritten
  {
    const int wrc = wait_segment_idle(s);
    if (wrc != TQ_OK) return wrc;
  }
  if (n > s->d_terms_cap) {
    HIP_TRY(hipStreamSynchronize(st));
    if (s->d_terms) (void)hipFree(s->d_terms);
    s->d_terms = nullptr;
    s->d_terms_cap = 0;
    size_t cap = std::max<size_t>(1024, n * 2);
    HIP_TRY(hipMalloc((void **)&s->d_terms, cap * sizeof(TqdTerm)));
    s->d_terms_cap = cap;
    s->d_terms_dirty_from = 0;
  }
  const size_t from = std::min(s->d_terms_dirty_from, n);
  if (n > from)
    HIP_TRY(hipMemcpy(s->d_terms + from, s->h_dterms.data() + from, (n - from) * sizeof(TqdTerm), hipMemcpyHostToDevice));
  s->d_terms_dirty = false;
  s->d_terms_dirty_from = ~(size_t)0;
  s->d_terms_synced = n;
  return TQ_OK;
}

}  // namespace tqi

namespace tqi {
// tq_term_prepare with offsets already shifted by the field's bases (field 0: as given); s->prep_field names the field
int term_prepare_shifted(tq_segment *s, uint64_t postings_off, uint32_t postings_len,
                    uint64_t positions_off, uint32_t positions_len, uint32_t doc_freq,
                    tq_term_handle *out) {
  TQ_SEGMENT_LOCK(s);
  auto it = s->term_by_off.find(postings_off);
  if (it != s->term_by_off.end()) {
    *out = it->second;
    return TQ_OK;
  }
  if (doc_freq == 0) return fail(TQ_ERR_INVALID, "tq_term_prepare: doc_freq 0 (term absent)");
  if (!postings_range_ok(s->idx_len, postings_off, postings_len)) return bad_postings_range(s->idx_len, postings_off, postings_len);
  HIP_TRY(hipSetDevice(s->device));
  if (s->device_prepare())
    return term_prepare_device(s, postings_off, postings_len, positions_off, positions_len, doc_freq,
                               out);
  WalkedTerm w;
  {
    const int wrc = host_walk_term(walk_source(s), postings_off, postings_len, positions_off, positions_len, doc_freq, w);
    if (wrc != TQ_OK) return wrc;
  }
  uint8_t *blob = nullptr;
  {
    const int arc = term_alloc(s, w.lay.total, &blob);
    if (arc != TQ_OK) return arc;
  }
  s->bytes_term_tables += w.lay.total;
  place_walked_term(w, blob);
  hipError_t ce = hipMemcpy(blob, w.hb.data(), w.lay.total, hipMemcpyHostToDevice);
  if (ce != hipSuccess) {
    term_release(s, blob, w.lay.total);
    return fail(TQ_ERR_HIP, "term upload: %s", hipGetErrorString(ce));
  }
  return register_term(s, w.dt, w.th, postings_off, out);
}
}  // namespace tqi

extern "C" int tq_term_prepare(tq_segment *s, uint64_t postings_off, uint32_t postings_len,
                               uint64_t positions_off, uint32_t positions_len, uint32_t doc_freq,
                               tq_term_handle *out) {
  if (!s || !out) return fail(TQ_ERR_INVALID, "tq_term_prepare: null argument");
  if (s->n_fields > 1)  // (field 0's ranges, checked against field 0's sub-files)
    return tq_term_prepare_field(s, 0, postings_off, postings_len, positions_off, positions_len, doc_freq, out);
  return term_prepare_shifted(s, postings_off, postings_len, positions_off, positions_len, doc_freq, out);
}

// The new terms of a batch together: every list is walked on the host as tq_term_prepare walks
// it, the blobs go up from ONE pinned staging buffer with asynchronous copies and one wait, and the signature bits of
// all the lists without a column are set by ONE launch (tq_term_prepare costs a blocking copy and two launches per
// term: two thousand new terms per 10 000-query batch while a 65 536-term vocabulary is being discovered).  Lists
// dense enough for tables of their own are prepared one by one as before (there are at most a few hundred per
// segment).  out[i] = the handle of infos[i] (known terms: the one they have).
namespace {
using Clock = std::chrono::steady_clock;
struct PrepareBatch {
  tq_segment *s;
  const tq_term_info *infos;
  uint32_t n;
  tq_term_handle *out;
  std::vector<uint32_t> fresh;  // indices of infos that need preparing
  std::vector<WalkedTerm> prewalked;  // per fresh index: walked without the lock (prewalked_ok: and well-formed)
  std::vector<char> prewalked_ok;
  std::vector<WalkedTerm> walked;  // the lists this call uploads together, and the index of infos each belongs to
  std::vector<uint32_t> walked_of;
  size_t stage_bytes = 0, ptr_bytes = 0;  // the blobs (256-byte aligned each); the arrays of the signature launch behind them
  uint32_t bx = 0;                        // which of the two pinned buffers / events
  uint8_t *hs = nullptr, *region = nullptr;  // the pinned buffer; the ONE device region of the lot
  // per list that gets a signature bit or a range directory: record pointer (in hs, behind the blobs), range directory,
  // signature bit, shift, doc freq, (out) list maximum — six arrays behind the blobs
  std::vector<uint32_t *> tabs;
  std::vector<uint32_t> bits, shifts, dfs;
  uint32_t n_sig = 0;
  bool any_tab = false;
  bool trace = false;
  Clock::time_point t0, t1, t2, t3, t4;
  ~PrepareBatch() {
    if (!trace) return;
    auto us = [](auto x, auto y) { return (long)std::chrono::duration_cast<std::chrono::microseconds>(y - x).count(); };
    fprintf(stderr, "[tq] prepare_batch %zu new terms: walk %ld us, lock %ld us, place %ld us, register + tables %ld us, copy + launch %ld us\n",
            fresh.size(), us(t0, t1), us(t1, t2), us(t2, t3), us(t3, t4), us(t4, Clock::now()));
  }
};

int prepare_one(PrepareBatch &b, uint32_t i) {
  const tq_term_info &ti = b.infos[i];
  return term_prepare_shifted(b.s, ti.postings_off, ti.postings_len, ti.positions_off, ti.positions_len, ti.doc_freq, &b.out[i]);
}

// under the lock: out[] of the terms the segment knows, the others collected
void resolve_known(PrepareBatch &b) {
  for (uint32_t i = 0; i < b.n; ++i) {
    auto it = b.s->term_by_off.find(b.infos[i].postings_off);
    b.out[i] = it != b.s->term_by_off.end() ? it->second : TQ_TERM_ABSENT;
    if (it == b.s->term_by_off.end()) b.fresh.push_back(i);
  }
}

// The host walk of the new lists runs WITHOUT the segment's lock (it reads the host copy of the index and a few
// options): a second host thread can walk the next batch's terms while the first plans and enqueues this one.
void prewalk(PrepareBatch &b) {
  const tq_segment *s = b.s;
  const WalkSource src = walk_source(s);
  b.prewalked.resize(b.fresh.size());
  b.prewalked_ok.assign(b.fresh.size(), 0);
  auto walk_some = [&](size_t k0, size_t step) {
    for (size_t k = k0; k < b.fresh.size(); k += step) {
      const tq_term_info &ti = b.infos[b.fresh[k]];
      if (ti.doc_freq == 0 || !postings_range_ok(s->idx_len, ti.postings_off, ti.postings_len)) continue;  // (reported under the lock)
      if (dense_candidate(s, ti.doc_freq)) continue;  // (whatever the budget says then: not walked here)
      if (host_walk_term(src, ti.postings_off, ti.postings_len, ti.positions_off, ti.positions_len, ti.doc_freq, b.prewalked[k]) == TQ_OK)
        b.prewalked_ok[k] = 1;  // (a malformed list: walked again under the lock, where its error is reported)
    }
  };
  // (a batch that discovers a large vocabulary names a couple of thousand new lists, 0.8 us of walking each: a few
  // short-lived helper threads take their share — TQ_PREP_THREADS, default 4 walkers from 512 lists on)
  static const uint32_t kWalkers = std::max<uint32_t>(1u, tune_u32("TQ_PREP_THREADS", 4));
  const size_t n_walk = std::min<size_t>(kWalkers, b.fresh.size() / 256u);
  std::vector<std::thread> helpers;
  for (size_t w = 1; w < n_walk; ++w) {
    try {
      helpers.emplace_back(walk_some, w, n_walk);
    } catch (...) {  // (a thread limit: the caller walks that share too)
      walk_some(w, n_walk);
    }
  }
  walk_some(0, std::max<size_t>(1, n_walk));
  for (std::thread &h : helpers) h.join();
}

// under the lock: every fresh term is known by now, invalid, dense (prepared one by one, here), a repeat, or walked
int classify_and_walk(PrepareBatch &b) {
  tq_segment *s = b.s;
  std::unordered_set<uint64_t> walked_offs;  // (postings offsets seen in this call: a term named twice is prepared once)
  b.walked.reserve(b.fresh.size());
  walked_offs.reserve(b.fresh.size() * 2);
  for (size_t fk = 0; fk < b.fresh.size(); ++fk) {
    const uint32_t i = b.fresh[fk];
    const tq_term_info &ti = b.infos[i];
    auto it = s->term_by_off.find(ti.postings_off);
    if (it != s->term_by_off.end()) {  // (named twice in this call, or prepared by another thread meanwhile)
      b.out[i] = it->second;
      continue;
    }
    if (ti.doc_freq == 0) return fail(TQ_ERR_INVALID, "tq_term_prepare_batch: doc_freq 0 (term absent)");
    if (!postings_range_ok(s->idx_len, ti.postings_off, ti.postings_len)) return bad_postings_range(s->idx_len, ti.postings_off, ti.postings_len);
    const bool dense = dense_candidate(s, ti.doc_freq) && dense_fits(s);
    const bool dup = !walked_offs.insert(ti.postings_off).second;
    if (dense || dup) {
      if (!dup) {
        const int rc = prepare_one(b, i);
        if (rc != TQ_OK) return rc;
      }
      continue;
    }
    if (fk < b.prewalked_ok.size() && b.prewalked_ok[fk]) {
      b.walked.push_back(std::move(b.prewalked[fk]));
    } else {
      b.walked.emplace_back();
      const int wrc = host_walk_term(walk_source(s), ti.postings_off, ti.postings_len, ti.positions_off, ti.positions_len, ti.doc_freq, b.walked.back());
      if (wrc != TQ_OK) return wrc;
    }
    b.walked_of.push_back(i);
    b.stage_bytes += (b.walked.back().lay.total + 255) & ~(size_t)255;
  }
  return TQ_OK;
}

// blobs: ONE device region for the lot, the bytes through one of two pinned buffers, one asynchronous copy on the
// segment's copy stream — and no wait: an event orders every later reader (the next batch's kernels, table
// builders on the segment's stream) behind the copy and the signature launch.  (A copy per term was 3 us of host
// time each; a wait for the segment's stream stalled the batches in flight for a millisecond per call.)
int stage_blobs(PrepareBatch &b) {
  tq_segment *s = b.s;
  b.ptr_bytes = (b.walked.size() * (2 * sizeof(const TqdTerm *) + 4 * sizeof(uint32_t)) + 255) & ~(size_t)255;
  prep_apply_lmax(s, false);
  const uint32_t bx = b.bx = s->prep_calls++ & 1u;
  if (!s->ev_prep[bx]) HIP_TRY(hipEventCreateWithFlags(&s->ev_prep[bx], hipEventDisableTiming));
  if (s->prep_used[bx]) HIP_TRY(hipEventSynchronize(s->ev_prep[bx]));  // (the copy of two calls ago: long done)
  prep_apply_lmax(s, false);  // (what that call left in the buffer, before it is written again)
  s->prep_lmax_handles[bx].clear();
  int rc = s->h_prep_stage[bx].ensure(b.stage_bytes + 2 * b.ptr_bytes);
  if (rc != TQ_OK) return rc;
  b.hs = (uint8_t *)s->h_prep_stage[bx].p;
  rc = term_alloc(s, b.stage_bytes + b.ptr_bytes, &b.region);
  if (rc != TQ_OK) return rc;
  s->bytes_term_tables += b.stage_bytes + b.ptr_bytes;
  size_t at = 0;
  for (WalkedTerm &w : b.walked) {
    place_walked_term(w, b.region + at);
    memcpy(b.hs + at, w.hb.data(), w.lay.total);
    at += (w.lay.total + 255) & ~(size_t)255;
  }
  return TQ_OK;
}

// handles; which of them get signature bits and range directories (their record pointers and bits ride behind the blobs)
int register_walked(PrepareBatch &b) {
  tq_segment *s = b.s;
  const bool sigs = s->opt.docsig && s->opt.docmat && s->opt.dense && s->max_doc >= 4096u;
  if (sigs) {
    const int rc = ensure_docmat(s);
    if (rc != TQ_OK) return rc;
  }
  b.t3 = b.t4 = Clock::now();
  const TqdTerm **h_selfs = (const TqdTerm **)(b.hs + b.stage_bytes);
  for (size_t k = 0; k < b.walked.size(); ++k) {
    WalkedTerm &w = b.walked[k];
    const uint32_t handle = add_term(s, w.dt, w.th, w.postings_off);
    b.out[b.walked_of[k]] = handle;
    if (!w.th.doc_freq) continue;
    const bool sig = sigs && s->d_docmat;
    const uint32_t S = rdir_plan(s, w.th.doc_freq);
    void *tab = nullptr;
    if (S && attach_rdir(s, handle, S, &tab) != TQ_OK) {  // (no memory for it: the list does without)
      (void)hipGetLastError();
      tab = nullptr;
    }
    if (tab) b.any_tab = true;
    if (!sig && !tab) continue;
    const uint32_t bit = sig_bit(handle);
    h_selfs[b.n_sig++] = w.th.d_self;
    b.tabs.push_back((uint32_t *)tab);
    b.bits.push_back(sig ? bit : 0xFFFFFFFFu);
    b.shifts.push_back(tab ? S : 0u);
    b.dfs.push_back(w.th.doc_freq);
    s->prep_lmax_handles[b.bx].push_back(handle);
    if (sig) s->h_dterms[handle].has_freq |= (bit + 1u) << 16;
  }
  if (b.n_sig) {
    const size_t n_sig = b.n_sig;
    uint8_t *at = (uint8_t *)(h_selfs + n_sig);
    memcpy(at, b.tabs.data(), n_sig * sizeof(uint32_t *));
    at += n_sig * sizeof(uint32_t *);
    for (const std::vector<uint32_t> *arr : {&b.bits, &b.shifts, &b.dfs}) {
      memcpy(at, arr->data(), n_sig * sizeof(uint32_t));
      at += n_sig * sizeof(uint32_t);
    }
    memset(at, 0, n_sig * sizeof(uint32_t));  // (the lists' maxima: written by the launch)
  }
  b.t4 = Clock::now();
  return TQ_OK;
}

// the one copy, the one launch, the maxima's copy back, and the event every later reader waits for
int enqueue_upload(PrepareBatch &b) {
  tq_segment *s = b.s;
  const uint32_t bx = b.bx, n_sig = b.n_sig;
  hipStream_t cs = s->copy_stream ? s->copy_stream : s->stream;
  // (the doc matrix may just have been created on the segment's stream: the copy stream follows it)
  hipError_t e = hipSuccess;
  if (cs != s->stream) {
    if (!s->ev_prep_order) e = hipEventCreateWithFlags(&s->ev_prep_order, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(s->ev_prep_order, s->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(cs, s->ev_prep_order, 0);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(b.region, b.hs, b.stage_bytes + b.ptr_bytes, hipMemcpyHostToDevice, cs);
  bool lmax_pending = false;
  if (e == hipSuccess && n_sig) {
    const TqdTerm **d_selfs = (const TqdTerm **)(b.region + b.stage_bytes);
    uint32_t *const *d_tabs = (uint32_t *const *)(d_selfs + n_sig);
    const uint32_t *d_bits = (const uint32_t *)(d_tabs + n_sig);
    uint32_t *d_lmax = (uint32_t *)(d_bits + 3 * n_sig);
    if (s->d_docmat) docmat_written(s);  // (signature bits; with a null matrix the launch only fills range directories)
    e = tqk_launch_docsig_batch(s->dseg, d_selfs, d_bits, n_sig, s->d_docmat, b.any_tab ? d_tabs : nullptr, d_bits + n_sig,
                                d_bits + 2 * n_sig, s->d_local_cache, d_lmax, s->opt.use_dpp != 0, cs);
    if (e == hipSuccess && b.any_tab && s->d_local_cache) {
      uint32_t *h_lmax = (uint32_t *)(b.hs + b.stage_bytes + b.ptr_bytes);
      e = hipMemcpyAsync(h_lmax, d_lmax, (size_t)n_sig * sizeof(uint32_t), hipMemcpyDeviceToHost, cs);
      s->prep_lmax_host[bx] = h_lmax;
      lmax_pending = true;
    }
  }
  if (!lmax_pending) s->prep_lmax_handles[bx].clear();
  if (e == hipSuccess) e = hipEventRecord(s->ev_prep[bx], cs);
  if (e == hipSuccess && cs != s->stream) e = hipStreamWaitEvent(s->stream, s->ev_prep[bx], 0);
  if (e != hipSuccess) return fail(TQ_ERR_HIP, "term upload: %s", hipGetErrorString(e));
  s->prep_used[bx] = true;
  s->prep_pending = (int)bx;  // (the next batch on a stream of the caller's waits for the event too: tq_search.cpp)
  return TQ_OK;
}

void resolve_repeats(PrepareBatch &b) {  // (a term named twice in one call)
  for (uint32_t i : b.fresh)
    if (b.out[i] == TQ_TERM_ABSENT) {
      auto it = b.s->term_by_off.find(b.infos[i].postings_off);
      if (it != b.s->term_by_off.end()) b.out[i] = it->second;
    }
}
}  // namespace

// (infos: offsets already shifted by the field's bases; the terms registered under the second lock are tagged `field`)
int tqi::term_prepare_batch_shifted(tq_segment *s, const tq_term_info *infos, uint32_t n, tq_term_handle *out, uint8_t field) {
  PrepareBatch b{s, infos, n, out};
  {
    TQ_SEGMENT_LOCK(s);
    resolve_known(b);
  }
  if (b.fresh.empty()) return TQ_OK;
  static const bool trace = getenv("TQ_TRACE") != nullptr;
  b.trace = trace;
  b.t0 = b.t1 = b.t2 = b.t3 = b.t4 = Clock::now();
  if (!s->device_prepare()) prewalk(b);
  b.t1 = Clock::now();
  TQ_SEGMENT_LOCK(s);
  FieldScope field_scope(s, field);  // (add_term tags what is registered while the lock is held)
  b.t2 = b.t3 = b.t4 = Clock::now();
  HIP_TRY(hipSetDevice(s->device));
  if (s->device_prepare()) {  // (no host copy of the index: the device walk, term by term)
    for (uint32_t i : b.fresh) {
      const int rc = prepare_one(b, i);
      if (rc != TQ_OK) return rc;
    }
    return TQ_OK;
  }
  int rc = classify_and_walk(b);
  if (rc == TQ_OK && !b.walked.empty()) {
    rc = stage_blobs(b);
    if (rc == TQ_OK) rc = register_walked(b);
    if (rc == TQ_OK) rc = enqueue_upload(b);
  }
  if (rc != TQ_OK) return rc;
  resolve_repeats(b);
  return TQ_OK;
}

extern "C" int tq_term_prepare_batch(tq_segment *s, const tq_term_info *infos, uint32_t n, tq_term_handle *out) {
  if (!s || (!infos && n) || (!out && n)) return fail(TQ_ERR_INVALID, "tq_term_prepare_batch: null argument");
  if (s->n_fields > 1) return tq_term_prepare_batch_fields(s, infos, nullptr, n, out);
  return term_prepare_batch_shifted(s, infos, n, out, 0);
}
